"""SD 2.x on the MI355X: the LCM step kernel of every prediction type against float64, the OpenCLIP-H text encoder, the
synthetic SD 2.1-768 pipeline (v-prediction) against the CPU oracle, an fp64 audit of every launch of an SD2 pass, and the
worker with MODEL=synthetic-sd2."""
import ctypes as C
import os
from dataclasses import dataclass, field
from typing import Optional

import numpy as np
import pytest
import torch

import sd2_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# North_star: |delta| < 1e-2 per pixel on the decoded [0,1] image.
# The final latents: fp16-operand kernels against the fp32 oracle, bound relative to the scale of the data as for SD1.5
# (tests/test_configs_gpu.py): max |delta| < 5e-3 x std(oracle latents) -- a few fp16 roundings per step at the scale of the
# data, four steps -- times the guidance scale under classifier-free guidance, since eps_u + g (eps_t - eps_u) carries g times
# the rounding of its two inputs.  A wrong prediction type, a skipped step or a mis-scaled sigma shows up at >= 5e-2 x std.
LATENT_REL_TOL = 5e-3
IMG_TOL = 1e-2


# ---- 1. the step kernel ------------------------------------------------------------------------------------------------
def _coef(i, steps=4):
    from sdlcm_amd.scheduler import LCMSchedule, SD21_768_SCHEDULE
    s = LCMSchedule(**SD21_768_SCHEDULE)
    ts = s.timesteps(steps)
    coef, last = s.step_coefficients(ts, i)
    return [float(np.float32(c)) for c in coef], last          # the values the kernel receives (fp32)


@pytest.mark.parametrize("pred", R.PREDS)
@pytest.mark.parametrize("B,h,w", [(1, 5, 7), (3, 9, 3)])
@pytest.mark.parametrize("cfg", [False, True])
def test_step_kernel_vs_fp64(pred, B, h, w, cfg):
    from sdlcm_amd import ops
    g = torch.Generator().manual_seed(B * 100 + h)
    for i in (0, 3):                                            # a middle step and the last one
        coef, last = _coef(i)
        m, mu = torch.randn(B, h, w, 4, generator=g), torch.randn(B, h, w, 4, generator=g)      # NHWC model outputs
        x, n = torch.randn(B, 4, h, w, generator=g), torch.randn(B, 4, h, w, generator=g)
        lat = x.to(DEV)
        ops.scheduler_step(m.to(DEV), lat, n.to(DEV), coef, last, B, h, w, eps_uncond=mu.to(DEV) if cfg else None,
                           guidance=7.5 if cfg else 1.0, pred=pred)
        torch.cuda.synchronize()
        nchw = lambda t: t.permute(0, 3, 1, 2).double().numpy()
        want, bound = R.lcm_step_coef_fp64(coef, last, nchw(m), x.double().numpy(), n.double().numpy(), pred,
                                           nchw(mu) if cfg else None, 7.5 if cfg else 1.0)
        err = np.abs(lat.cpu().double().numpy() - want)
        assert (err <= bound).all(), f"{pred} step {i}: worst err/bound {float((err / bound).max()):.3g}"


def test_step_ex_epsilon_is_bit_identical_and_bad_type_is_refused():
    from sdlcm_amd import lib, ops
    L = lib.load()
    B, h, w = 3, 9, 7
    g = torch.Generator().manual_seed(2)
    eps, eu = (torch.randn(B, h, w, 4, generator=g).to(DEV) for _ in range(2))
    x, n = (torch.randn(B, 4, h, w, generator=g).to(DEV) for _ in range(2))
    coef, _ = _coef(1)
    arr = (C.c_float * 6)(*coef)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    for uncond in (None, eu):
        for last in (0, 1):
            a, b = x.clone(), x.clone()
            pu = p(uncond) if uncond is not None else None
            lib.check(L.lcm_scheduler_step(p(eps), pu, 4.0, p(a), p(n), arr, last, B, h, w, st))
            lib.check(L.lcm_scheduler_step_ex(p(eps), pu, 4.0, p(b), p(n), arr, last, lib.LCM_PRED_EPSILON, B, h, w, st))
            torch.cuda.synchronize()
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    c = x.clone()
    ops.scheduler_step(eps, c, n, coef, False, B, h, w)                  # the default: the old entry point
    d = x.clone()
    ops.scheduler_step(eps, d, n, coef, False, B, h, w, pred="epsilon")
    torch.cuda.synchronize()
    assert torch.equal(c.view(torch.int32), d.view(torch.int32))
    before = x.clone()
    for bad in (3, -1, 7):
        rc = L.lcm_scheduler_step_ex(p(eps), None, 1.0, p(x), p(n), arr, 0, bad, B, h, w, st)
        assert rc == -1, rc                                                 # LCM_EINVAL
        assert b"prediction type" in L.lcm_last_error()
    torch.cuda.synchronize()
    assert torch.equal(x, before)                                           # nothing was enqueued
    with pytest.raises(ValueError, match="x_start"):
        ops.scheduler_step(eps, x, n, coef, False, B, h, w, pred="x_start")


# ---- 2. the text encoder -----------------------------------------------------------------------------------------------
def test_clip_h_text_encoder_parity():
    from sdlcm_amd.clip import CLIP_H, ClipTextHip, HashTokenizer, synthetic_clip_h
    from oracle.clip import clip_text_oracle
    sd = synthetic_clip_h()
    ids = HashTokenizer()(["a photo of an astronaut riding a horse on mars", ""])
    ref = clip_text_oracle(sd, CLIP_H, ids).numpy()
    got = ClipTextHip(sd, CLIP_H, device=DEV).forward(ids).float().cpu().numpy()
    e = np.abs(got - ref)
    print(f"[sd2] clip-h last_hidden_state: max|d|={e.max():.4g} max|ref|={np.abs(ref).max():.4g}")
    assert e.max() < 2e-2 * max(1.0, np.abs(ref).max())


# ---- 3. the pipeline ---------------------------------------------------------------------------------------------------
def _oracle_scheduler():
    from oracle.scheduler import LCMSchedulerOracle

    class VPredLCMSchedulerOracle(LCMSchedulerOracle):
        """LCMScheduler.step with prediction_type="v_prediction", on SD 2.1-768's beta schedule (scaled_linear 0.00085 -
        0.012: the parent's defaults).  set_alpha_to_one=false changes final_alpha_cumprod only, which LCM never reads: its
        last step uses its own t as the previous timestep."""

        def step(self, v, i, sample, noise=None):
            sa, sb, c_skip, c_out, sap, sbp, last = self.coefficients(i)
            x0 = sa * sample - sb * v
            den = c_out * x0 + c_skip * sample
            if last:
                return den, den
            return sap * den + sbp * noise, den
    return VPredLCMSchedulerOracle()


@pytest.fixture(scope="module")
def sd2():
    from sdlcm_amd import weights
    from sdlcm_amd.config import SD2_UNET, unet_config
    from sdlcm_amd.pipeline import LcmHipPipeline
    from sdlcm_amd.scheduler import LCMSchedule, SD21_768_SCHEDULE
    from oracle.pipeline import LCMPipelineOracle
    ucfg = unet_config(SD2_UNET)
    usd, vsd = weights.synthetic_sd2_unet(), weights.synthetic_vae()
    hip = LcmHipPipeline(usd, vsd, ucfg, device=DEV, schedule=LCMSchedule(**SD21_768_SCHEDULE))
    ora = LCMPipelineOracle(usd, vsd, ucfg)
    ora.sched = _oracle_scheduler()
    yield dict(hip=hip, ora=ora)
    hip.close()


def _embeds(seed, D=1024):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(1, 77, D, generator=g).half(), torch.randn(1, 77, D, generator=g).half()


def _img01(x_nchw):
    return np.clip(x_nchw / 2 + 0.5, 0, 1)


@pytest.mark.parametrize("size,steps,guidance", [(64, 2, 1.0), (512, 4, 1.0), (64, 2, 7.5)])
def test_sd2_pipeline_parity(sd2, size, steps, guidance):
    from sdlcm_amd.scheduler import LCMSchedule, SD21_768_SCHEDULE
    hip, ora = sd2["hip"], sd2["ora"]
    pe, ne = _embeds(size + steps)
    kw = dict(negative_embeds=ne) if guidance > 1 else {}
    ref = ora(pe.float(), size, size, steps, guidance, 77, negative_embeds=ne.float() if guidance > 1 else None)
    out = hip.generate(pe, [77], size, size, steps, guidance, want_float=True, **kw)
    a, b = _img01(out["image"].transpose(0, 3, 1, 2)), _img01(ref["image"])
    e = np.abs(a - b)
    gl = ref["latents"][0].astype(np.float32)
    lat = np.abs(out["latents"][0] - gl)
    print(f"[sd2] {size}px {steps}-step g={guidance}: image max|d|={e.max():.4g}; latents max|d|={lat.max():.4g} "
          f"= {lat.max() / gl.std():.3g} x std ({gl.std():.3g})")
    assert e.max() < IMG_TOL
    assert lat.max() < LATENT_REL_TOL * max(1.0, guidance) * gl.std()
    # the same run read as epsilon prediction is a different image: the test tells the two apart
    hip.sched = LCMSchedule(**dict(SD21_768_SCHEDULE, prediction_type="epsilon"))
    try:
        wrong = hip.generate(pe, [77], size, size, steps, guidance, want_float=True, **kw)
    finally:
        hip.sched = LCMSchedule(**SD21_768_SCHEDULE)
    ew = np.abs(_img01(wrong["image"].transpose(0, 3, 1, 2)) - b)
    lw = np.abs(wrong["latents"][0] - gl)
    print(f"[sd2] epsilon reading: image max|d|={ew.max():.4g}, latents {lw.max() / gl.std():.3g} x std")
    assert ew.max() > 10 * IMG_TOL and lw.max() > 10 * LATENT_REL_TOL * max(1.0, guidance) * gl.std()
    # graph replay gives the eager bits
    rep = hip.generate(pe, [77], size, size, steps, guidance, **kw)
    assert np.array_equal(rep["rgb"], out["rgb"]) and np.array_equal(rep["latents"], out["latents"])


# ---- 4. launch audit ---------------------------------------------------------------------------------------------------
def _audit(hip, name, pe, guidance=1.0, **kw):
    from launch_audit import Audit
    plans = hip.lanes[0].plans
    before = set(plans)
    with Audit() as au:
        hip.generate(pe, [300], 512, 512, 4, guidance, want_float=True, **kw)
    for k in set(plans) - before:
        plans.pop(k)
    torch.cuda.empty_cache()
    launched = au.record_keys()
    assert au.checked_keys() == launched, f"{name}: hook saw {len(au.checked_keys())} of {len(launched)} plan keys"
    from launch_audit import failures, summary_line
    bad = failures(au.checks)
    print(f"[audit] {name}: {len(au.checks)} launches checked, {len(launched)} plan keys "
          f"({sum(k in au.table for k in launched)} in the table), {summary_line(au.checks)}")
    for c in bad:
        print(f"[audit] {name} FAIL {c}")
    assert not bad, f"{name}: {len(bad)} launches outside their fp64 error bound"
    return au


def test_audit_sd2_512_passes_fp64(sd2):
    """Every contraction / attention launch of a 512^2 SD2 pass (64-wide heads at 4096 tokens, 1024-wide cross-attention
    K/V) and of a CFG pass, within its fp64 bound; the CLIP-H GEMMs of the text encoder likewise."""
    from launch_audit import Audit
    from sdlcm_amd.clip import CLIP_H, ClipTextHip, HashTokenizer, synthetic_clip_h
    hip = sd2["hip"]
    pe, ne = _embeds(11)
    _audit(hip, "sd2 B1 512px", pe)
    _audit(hip, "sd2 B1 512px cfg", pe, 7.5, negative_embeds=ne)
    enc = ClipTextHip(synthetic_clip_h(), CLIP_H, device=DEV)
    with Audit() as au:
        enc.forward(HashTokenizer()(["a castle on a hill at dawn"]))
    from launch_audit import failures, summary_line
    bad = failures(au.checks)
    print(f"[audit] clip-h: {len(au.checks)} launches checked, {summary_line(au.checks)}")
    assert au.checks and not bad, bad
    assert {"embed_tokens", "layernorm"} <= {c["op"] for c in au.checks}


# ---- 5. the worker -----------------------------------------------------------------------------------------------------
@dataclass
class _Style:
    style: Optional[str] = None
    level: int = 0


@dataclass
class _Req:
    prompt: str
    size: str = "512x512"
    num_inference_steps: int = 4
    guidance_scale: float = 1.0
    seed: Optional[int] = None
    style_lora: _Style = field(default_factory=_Style)


@dataclass
class _Job:
    req: _Req


def _make_worker(monkeypatch, model, wid):
    monkeypatch.setenv("MODEL", model)
    monkeypatch.setenv("MODEL_ROOT", "/nonexistent")
    from sdlcm_amd.backends.worker_factory import create_hip_worker
    return create_hip_worker(worker_id=wid)


def test_sd2_worker(monkeypatch):
    import sys
    import threading
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from tools import minipool
    job = lambda s, size="256x256": _Job(_Req(prompt=f"a lighthouse {s}", size=size, seed=s))
    w15 = _make_worker(monkeypatch, "synthetic", 0)
    try:
        sd15_png = w15.run_job(job(5))
        # a synthetic-sd2 worker next to a live synthetic SD1.5 one: an engine of its own
        w = _make_worker(monkeypatch, "synthetic-sd2", 1)
        try:
            eng = w._engine
            assert eng is not w15._engine
            assert eng.pipe.unet.ctx_dim == 1024 and eng.encode.enc.D == 1024 and eng.encode.enc.cfg["hidden_act"] == "gelu"
            assert eng.pipe.sched.prediction_type == "v_prediction"
            png, seed = w.run_job(job(7))
            assert seed == 7 and png[:8] == b"\x89PNG\r\n\x1a\n"
            assert w.run_job(job(7)) == (png, 7)
            png5, _ = w.run_job(job(5))
            assert png5 != sd15_png[0]
            _, s3, lat = w.run_job_with_latents(job(3))
            assert s3 == 3 and isinstance(lat, bytes) and len(lat) == 512
            # a drained batch of four: each request keeps the bytes of its solo run
            solo = {s: w.run_job(job(s)) for s in range(4)}
            pool = minipool.MiniPool(lambda worker_id: w, {"m": "synthetic-sd2"}, "m")
            w.bind_queue(pool.q)
            try:
                gate, inside = threading.Event(), threading.Event()
                hold = pool.submit_job(minipool.CustomJob(handler=lambda: (inside.set(), gate.wait(30))))
                assert inside.wait(30)
                n0 = len(eng.batcher.batches)
                futs = [pool.submit_job(minipool.GenerationJob(req=job(s).req)) for s in range(4)]
                gate.set()
                hold.result(60)
                res = [f.result(600) for f in futs]
                pool.q.join()
                assert res == [solo[s] for s in range(4)]
                assert eng.batcher.batches[n0:] == [4]
            finally:
                w.bind_queue(None)
                pool._worker = None
                pool.shutdown()
        finally:
            w.close()
        # the SD1.5 worker still gives its previous bytes
        assert w15.run_job(job(5)) == sd15_png
    finally:
        w15.close()
