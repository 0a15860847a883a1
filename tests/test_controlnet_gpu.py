"""ControlNet-conditioned generation on the GPU: the hint-stack kernels against fp64, the injected residuals against the CPU
reference's taps, end-to-end parity with tests/controlnet_reference.py, determinism and isolation of the plain path.

Parity bound: the project's contract, per-pixel |d| < 1e-2 on the decoded [0, 1] image, every pixel."""
import io
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

TOL = 1e-2
# final latents against the fp32 reference: the bound of tests/test_configs_gpu.py (relative to the spread of the data)
LATENT_REL_TOL = 5e-3
COND = (16, 32, 96, 256)


def _u01(img_nchw):
    return np.clip(img_nchw / 2 + 0.5, 0, 1)


@pytest.fixture(scope="module")
def nets():
    from sdlcm_amd import weights
    return dict(unet=weights.synthetic_unet(), vae=weights.synthetic_vae(), cn=weights.synthetic_controlnet(),
                cn_zero=weights.synthetic_controlnet(zero=True))


@pytest.fixture(scope="module")
def pipe(nets):
    from sdlcm_amd.pipeline import LcmHipPipeline
    p = LcmHipPipeline(nets["unet"], nets["vae"], device="cuda:0")
    yield p
    p.close()


@pytest.fixture(scope="module")
def pe():
    return torch.randn(1, 77, 768, generator=torch.Generator().manual_seed(5)).to(torch.float16)


# ---- hint stack: every layer against fp64 on the same fp16-rounded operands ---------------------------------------------
def _layer_check(got, xin64, xerr, w, bias, B, H, W, stride, silu, K_eff):
    """Worst |got - ref| / bound of one hint layer: launch_audit.hint_layer_check (the derivation lives there, with the audit's
    other references: fp32 chain, operand error, bias, SiLU, the fp16 store)."""
    import launch_audit as la
    return la.hint_layer_check(got, xin64, xerr, w, bias, B, H, W, stride, silu, K_eff)


def _hint_images(B, H, W, seed=0):
    import controlnet_reference as cr
    imgs = np.stack([cr.test_hint(W, H, seed + b) for b in range(B)])
    imgs[0, :4, :4] = 0           # the uint8 edge values, also in the image corner (zero padding next to 0 and 255)
    imgs[0, -4:, -4:] = 255
    return imgs


@pytest.mark.parametrize("B,H,W", [(1, 64, 64), (1, 72, 40), (8, 40, 24), (1, 264, 136)])
def test_hint_stack_layers_vs_fp64(nets, B, H, W):
    """Every layer from ITS OWN stored input (the previous layer's fp16 output), and the whole stack end to end, at even and
    odd latent extents (72x40 -> 9x5, 264x136 -> 33x17), batch 1 and 8, hints that contain 0 and 255."""
    import launch_audit as la
    from sdlcm_amd import ops
    from sdlcm_amd.model import ControlNetHip
    dev = torch.device("cuda:0")
    cn = ControlNetHip(nets["cn"], None, None, dev)
    hint = torch.from_numpy(_hint_images(B, H, W)).to(dev)
    out = torch.zeros(B * (H // 8) * (W // 8), 320, dtype=torch.float16, device=dev)
    cn.embed_hint(hint, B, H, W, out)
    torch.cuda.synchronize()
    # layer 0: operand u8 / 255 carried as fp16 hi + lo (~22 bits) plus the fp32 division
    x64, xerr = la.hint_u8_input(hint)
    got = cn.buf.get("hint0", B * H * W, COND[0])
    worst = {0: _layer_check(got, x64, xerr, cn.w["hint.0.w"], cn.w["hint.0.b"], B, H, W, 1, True, la.HINT_U8_K)}
    h, w = H, W
    x = got
    for i in range(6):
        cin, cout, stride = COND[i // 2], COND[i // 2 + (i & 1)], 1 + (i & 1)
        ho, wo = ((h + 1) // 2, (w + 1) // 2) if stride == 2 else (h, w)
        y = cn.buf.get(f"hint{i + 1}", B * ho * wo, cout)
        xin = x.to(torch.float64).reshape(B, h, w, cin)
        worst[i + 1] = _layer_check(y, xin, None, cn.w[f"hint.{i + 1}.w"], cn.w[f"hint.{i + 1}.b"], B, h, w, stride, True, 9 * cin)
        x, h, w = y, ho, wo
    xin = x.to(torch.float64).reshape(B, h, w, COND[-1])
    worst[7] = _layer_check(out, xin, None, cn.w["hint.7.w"], cn.w["hint.7.b"], B, h, w, 1, False, 9 * COND[-1])
    # the whole stack against the fp32 CPU restatement: errors of eight fp16 stores compound, so this one is the loose sanity
    # check (relative to the embedding's scale); the per-layer bounds above are the sharp ones
    import controlnet_reference as cr
    ref = cr.ControlNetOracle(nets["cn"]).embed_hint(hint.cpu().numpy())
    g = out.reshape(B, h, w, 320).permute(0, 3, 1, 2).float().cpu()
    rel = float((g - ref).abs().max() / ref.abs().max())
    print(f"hint stack B={B} {H}x{W}: worst error/bound per layer {worst}, whole stack max|d|/max|ref| = {rel:.3g}")
    assert all(v <= 1.0 for v in worst.values()), worst
    assert rel < 2e-2, rel


# ---- end to end ---------------------------------------------------------------------------------------------------------
def _run_pair(pipe, nets, pe, width, height, steps=4, guidance=1.0, scale=1.0, seed=42, cn_key="cn", taps=None, negative=None,
              unet_cfg=None, unet_key="unet"):
    import controlnet_reference as cr
    hint = cr.test_hint(width, height)
    ora = cr.ControlNetPipelineOracle(nets[unet_key], nets["vae"], nets[cn_key], unet_cfg)
    ref = ora(pe.float(), width, height, steps, guidance, seed, hint, scale, negative_embeds=None if negative is None else negative.float())
    out = pipe.generate(pe, [seed], width, height, steps, guidance, want_float=True, control=(hint[None], scale), taps=taps,
                        negative_embeds=negative)
    a, b = _u01(out["image"].transpose(0, 3, 1, 2)), _u01(ref["image"])
    lat = float(np.abs(out["latents"] - ref["latents"]).max() / (max(1.0, guidance) * ref["latents"].std()))
    return float(np.abs(a - b).max()), lat, out, ref


@pytest.mark.parametrize("width,height", [(64, 64), (128, 128), (256, 256), (520, 392)])
def test_controlnet_parity(pipe, nets, pe, width, height):
    pipe.set_controlnet(nets["cn"])
    err, lat_err, out, ref = _run_pair(pipe, nets, pe, width, height)
    print(f"controlnet parity {width}x{height} 4 steps: max|d| image = {err:.3g} (tol {TOL}), max|d| latents / std = {lat_err:.3g}")
    assert err < TOL, err
    assert lat_err < LATENT_REL_TOL, lat_err


def test_controlnet_parity_512_fixture(pipe, nets, pe):
    from sdlcm_amd import weights  # noqa: F401
    import controlnet_reference as cr
    fx = np.load(os.path.join(os.path.dirname(__file__), "golden", "oracle_controlnet_512_4step.npz"))
    pipe.set_controlnet(nets["cn"])
    hint = cr.test_hint(512, 512)
    out = pipe.generate(pe, [int(fx["seed"])], 512, 512, 4, 1.0, want_float=True, control=(hint[None], float(fx["scale"])))
    a = _u01(out["image"].transpose(0, 3, 1, 2))[0]
    lo = fx["image_lo"]
    lo = np.stack([lo & 3, (lo >> 2) & 3, (lo >> 4) & 3, (lo >> 6) & 3], 1).reshape(3, 512, 512)
    hi = np.cumsum(fx["image_hi_dx"], axis=2, dtype=np.uint8)            # differences along x modulo 256
    b = (hi.astype(np.float32) * 4 + lo) / 1023.0                         # every pixel, 10 bits (make_controlnet_golden.py)
    err = float(np.abs(a - b).max())
    fl = fx["latents"].astype(np.float32)                                # stored as fp16: 2^-11 relative on top of the bound
    lat_err = float(np.abs(out["latents"][0] - fl).max())
    print(f"controlnet parity 512x512 4 steps vs fixture: max|d| image = {err:.3g} (tol {TOL}), latents = {lat_err:.3g} "
          f"(std {fl.std():.3g})")
    assert err < TOL, err
    assert lat_err < LATENT_REL_TOL * fl.std() + 2.0 ** -11 * np.abs(fl).max(), lat_err


def test_controlnet_cfg_parity(nets, pe):
    """Classifier-free guidance on a checkpoint without a guidance embedding: the ControlNet runs on both halves."""
    from sdlcm_amd.pipeline import LcmHipPipeline
    from sdlcm_amd import weights
    cfg = dict(time_cond_proj_dim=None)
    usd = weights.synthetic_unet(cfg)
    p = LcmHipPipeline(usd, nets["vae"], unet_cfg=cfg, device="cuda:0")
    try:
        p.set_controlnet(nets["cn"])
        neg = torch.randn(1, 77, 768, generator=torch.Generator().manual_seed(6)).to(torch.float16)
        n2 = dict(nets, unet_nc=usd)
        from oracle.unet import SD15_UNET
        err, lat_err, _, _ = _run_pair(p, n2, pe, 64, 64, guidance=3.0, negative=neg, unet_cfg=dict(SD15_UNET, **cfg), unet_key="unet_nc")
        print(f"controlnet CFG parity 64x64 guidance 3: max|d| = {err:.3g}, latents {lat_err:.3g}")
        assert err < TOL, err
        assert lat_err < LATENT_REL_TOL, lat_err
    finally:
        p.close()


def test_controlnet_sd2_parity(nets):
    from sdlcm_amd.pipeline import LcmHipPipeline
    from sdlcm_amd.scheduler import LCMSchedule
    from sdlcm_amd import weights
    from sdlcm_amd.config import SD2_UNET
    usd = weights.synthetic_sd2_unet()
    csd = weights.synthetic_controlnet(SD2_UNET)
    p = LcmHipPipeline(usd, nets["vae"], unet_cfg=SD2_UNET, device="cuda:0")
    try:
        p.set_controlnet(csd, weights.controlnet_config(SD2_UNET))
        pe2 = torch.randn(1, 77, 1024, generator=torch.Generator().manual_seed(5)).to(torch.float16)
        n2 = dict(unet=usd, vae=nets["vae"], cn=csd)
        from oracle.unet import SD15_UNET
        ocfg = dict(SD15_UNET, **{k: SD2_UNET[k] for k in ("attention_head_dim", "cross_attention_dim", "time_cond_proj_dim")})
        err, lat_err, _, _ = _run_pair(p, n2, pe2, 64, 64, unet_cfg=ocfg)
        print(f"controlnet SD 2.x parity 64x64: max|d| = {err:.3g}, latents {lat_err:.3g}")
        assert err < TOL, err
        assert lat_err < LATENT_REL_TOL, lat_err
    finally:
        p.close()


def test_injection_taps(pipe, nets, pe):
    """Each of the 13 residuals and each modified skip of the first step of a real pass against the reference's taps."""
    import controlnet_reference as cr
    pipe.set_controlnet(nets["cn"])
    W = H = 64
    hint = cr.test_hint(W, H)
    taps = {}
    pipe.generate(pe, [42], W, H, 1, 1.0, want_float=True, control=(hint[None], 0.75), taps=taps)
    ora = cr.ControlNetPipelineOracle(nets["unet"], nets["vae"], nets["cn"])
    ora.unet.taps, ora.cn.taps = {}, {}
    ora(pe.float(), W, H, 1, 1.0, 42, hint, 0.75)
    worst = {}
    for i in list(range(12)) + ["mid"]:
        r_ref = ora.cn.taps[f"cn.res.{i}"]
        s_ref = ora.unet.taps[f"skip_mod.{i}" if i != "mid" else "mid_mod"]
        r_got, s_got = taps[f"ctl.res.{i}"], taps[f"ctl.skip.{i}" if i != "mid" else "ctl.mid"]
        # a residual is a linear map of a feature map that carries the encoder's accumulated fp16 error; the feature-map tap test of
        # this suite (tests/test_pipeline_gpu.py) allows 5 % of a tensor's scale, the residuals and the modified skips are held
        # to a fifth of that: 1 % of the tensor's own largest value
        worst[i] = (float((r_got - r_ref).abs().max() / r_ref.abs().max()), float((s_got - s_ref).abs().max() / s_ref.abs().max()))
    print("injection taps (residual, modified skip) max|d| / max|ref|:", worst)
    assert all(a < 1e-2 and b < 1e-2 for a, b in worst.values()), worst


def test_all_zero_variant_matches_plain(pipe, nets, pe):
    import controlnet_reference as cr
    plain = pipe.generate(pe, [42], 128, 128, 4, 1.0, want_float=True)["image"].copy()
    pipe.set_controlnet(nets["cn_zero"])
    hint = cr.test_hint(128, 128)
    out = pipe.generate(pe, [42], 128, 128, 4, 1.0, want_float=True, control=(hint[None], 1.0))["image"]
    err = float(np.abs(_u01(out) - _u01(plain)).max())
    print(f"all-zero ControlNet vs plain request 128x128: max|d| = {err:.3g}")
    assert err < TOL, err


def test_determinism_and_isolation(nets, pe):
    """Same request, seed and hint -> identical bytes alone, at positions 0 / 3 / 7 of a batch of 8 with different hints, on lane
    0 and lane 1, and after a plain request in between; a plain request's bytes are the same before a ControlNet is loaded, after
    it is loaded and after a ControlNet request ran."""
    import controlnet_reference as cr
    from sdlcm_amd.pipeline import LcmHipPipeline
    p = LcmHipPipeline(nets["unet"], nets["vae"], device="cuda:0")
    try:
        W = H = 64
        plain0 = p.generate(pe, [7], W, H, 2, 1.0)["rgb"].copy()
        plain0_l1 = p.generate(pe, [7], W, H, 2, 1.0, lane=1)["rgb"].copy()
        p.set_controlnet(nets["cn"])
        plain1 = p.generate(pe, [7], W, H, 2, 1.0)["rgb"].copy()
        hints = np.stack([cr.test_hint(W, H, s) for s in range(8)])
        solo = p.generate(pe, [42], W, H, 2, 1.0, control=(hints[:1], 1.0))["rgb"].copy()
        plain2 = p.generate(pe, [7], W, H, 2, 1.0)["rgb"].copy()
        solo2 = p.generate(pe, [42], W, H, 2, 1.0, control=(hints[:1], 1.0))["rgb"].copy()
        lane1 = p.generate(pe, [42], W, H, 2, 1.0, control=(hints[:1], 1.0), lane=1)["rgb"].copy()
        plain2_l1 = p.generate(pe, [7], W, H, 2, 1.0, lane=1)["rgb"].copy()
        assert np.array_equal(plain0, plain1) and np.array_equal(plain0, plain2), "plain request changed by the ControlNet"
        assert np.array_equal(plain0_l1, plain2_l1) and np.array_equal(plain0, plain0_l1)
        assert np.array_equal(solo, solo2), "ControlNet request not reproducible after a plain request"
        assert np.array_equal(solo, lane1), "lane 1 differs from lane 0"
        assert not np.array_equal(solo[0], plain0[0])
        pe8 = pe.expand(8, -1, -1).contiguous()
        for pos in (0, 3, 7):
            order = list(range(1, 8))
            order.insert(pos, 0)
            seeds = [42 if k == 0 else 100 + k for k in order]
            out = p.generate(pe8, seeds, W, H, 2, 1.0, control=(hints[order], 1.0))["rgb"]
            assert np.array_equal(out[pos], solo[0]), f"element {pos} of a batch of 8 differs from the solo request"
        # a different hint is a different picture
        other = p.generate(pe, [42], W, H, 2, 1.0, control=(hints[1:2], 1.0))["rgb"]
        assert not np.array_equal(other, solo)
    finally:
        p.close()


def test_errors(pipe, nets, pe):
    from sdlcm_amd.lib import LcmHipError
    import controlnet_reference as cr
    hint = cr.test_hint(64, 64)[None]
    pipe.set_controlnet(None)
    with pytest.raises(LcmHipError, match="no ControlNet is loaded"):
        pipe.generate(pe, [1], 64, 64, 2, 1.0, control=(hint, 1.0))
    pipe.set_controlnet(nets["cn"])
    with pytest.raises(LcmHipError, match="outside"):
        pipe.generate(pe, [1], 64, 64, 2, 1.0, control=(hint, 2.5))
    with pytest.raises(LcmHipError, match="refinement"):
        pipe.generate(pe, [1], 64, 64, 2, 1.0, control=(hint, 1.0), passes=1, strength=0.5)
    with pytest.raises(LcmHipError, match="uint8"):
        pipe.generate(pe, [1], 64, 64, 2, 1.0, control=(hint[:, :32], 1.0))


# ---- the worker and the pool ----------------------------------------------------------------------------------------------
from dataclasses import dataclass, field          # noqa: E402
from typing import Any, Optional                  # noqa: E402


@dataclass
class _Style:
    style: Optional[str] = None
    level: int = 0


@dataclass
class _Req:
    prompt: str
    size: str = "64x64"
    num_inference_steps: int = 2
    guidance_scale: float = 1.0
    seed: Optional[int] = None
    style_lora: _Style = field(default_factory=_Style)
    controlnet_image: Any = None
    controlnet_conditioning_scale: Optional[float] = None
    denoise_strength: Optional[float] = None
    pass_number: Optional[int] = None


@dataclass
class _Job:
    req: _Req


def _png(arr):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(arr, "RGB").save(b, "PNG")
    return b.getvalue()


@pytest.fixture(scope="module")
def plain_bytes():
    """A plain request's PNG from a worker created with CONTROLNET unset, in this session."""
    os.environ["MODEL"] = "synthetic"
    os.environ.setdefault("MODEL_ROOT", "/nonexistent")
    os.environ.pop("CONTROLNET", None)
    from sdlcm_amd.backends.worker_factory import create_hip_worker
    w = create_hip_worker(worker_id=0)
    try:
        import controlnet_reference as cr
        out = w.run_job(_Job(_Req(prompt="a lighthouse at dusk", seed=7)))
        with pytest.raises(RuntimeError, match="no ControlNet is loaded"):
            w.run_job(_Job(_Req(prompt="x", seed=1, controlnet_image=cr.test_hint(64, 64))))
        return out
    finally:
        w.close()


@pytest.fixture(scope="module")
def worker(plain_bytes):
    os.environ["MODEL"] = "synthetic"
    os.environ.setdefault("MODEL_ROOT", "/nonexistent")
    os.environ["CONTROLNET"] = "synthetic"
    from sdlcm_amd.backends.worker_factory import create_hip_worker
    w = create_hip_worker(worker_id=0)
    yield w
    w.close()
    os.environ.pop("CONTROLNET", None)


def test_worker_isolation_lazy_load_and_inputs(worker, plain_bytes):
    import controlnet_reference as cr
    from PIL import Image
    eng = worker._engine
    plain = _Job(_Req(prompt="a lighthouse at dusk", seed=7))
    assert eng.pipe.controlnet is None                                     # nothing loaded before a request needs it
    assert worker.run_job(plain) == plain_bytes
    hint = cr.test_hint(64, 64)
    mk = lambda img, **kw: _Job(_Req(prompt="a lighthouse at dusk", seed=7, controlnet_image=img, **kw))
    n0 = dict(eng.stats)
    a = worker.run_job(mk(hint))
    assert eng.pipe.controlnet is not None
    assert eng.stats["controlnet_evals"] - n0["controlnet_evals"] == 2 and eng.stats["unet_evals"] - n0["unet_evals"] == 2
    assert worker.run_job(plain) == plain_bytes                            # after it is loaded and after a ControlNet request ran
    assert a[0][:8] == b"\x89PNG\r\n\x1a\n" and a[1] == 7 and a != plain_bytes
    assert worker.run_job(mk(_png(hint))) == a and worker.run_job(mk(Image.fromarray(hint, "RGB"))) == a
    big = cr.test_hint(128, 128)                                          # another size: resized on the host with LANCZOS
    want = np.asarray(Image.fromarray(big, "RGB").resize((64, 64), Image.LANCZOS))
    assert worker.run_job(mk(big)) == worker.run_job(mk(want))
    assert worker.run_job(mk(hint, controlnet_conditioning_scale=0.5)) != a
    png, seed, lat = worker.run_job_with_latents(mk(hint))
    assert (png, seed) == a and len(lat) == 512
    for bad, word in ((dict(controlnet_image=b"junk"), "controlnet_image"),
                      (dict(controlnet_image=hint, controlnet_conditioning_scale=2.5), "controlnet_conditioning_scale"),
                      (dict(controlnet_image=hint, denoise_strength=0.5), "refinement"),
                      (dict(controlnet_image=hint, pass_number=2), "refinement")):
        with pytest.raises(RuntimeError, match=word):
            worker.run_job(_Job(_Req(prompt="p", seed=1, **bad)))
    assert worker.run_job(plain) == plain_bytes


def test_sdxl_worker_refuses_a_hint(monkeypatch):
    import controlnet_reference as cr
    monkeypatch.setenv("MODEL", "synthetic-sdxl")
    monkeypatch.setenv("MODEL_ROOT", "/nonexistent")
    monkeypatch.setenv("CONTROLNET", "synthetic")
    from sdlcm_amd.backends.worker_factory import create_hip_worker
    w = create_hip_worker(worker_id=1)
    try:
        with pytest.raises(RuntimeError, match="SDXL"):
            w.run_job(_Job(_Req(prompt="p", size="256x256", seed=1, guidance_scale=5.0, controlnet_image=cr.test_hint(256, 256))))
    finally:
        w.close()


def test_pool_mixed_jobs_bad_hint_and_mode_switch(worker):
    """Through the pool-shaped loop (tools/minipool, the pool of tests/pool_scenario.py): mixed plain and ControlNet jobs each
    get their solo bytes, a bad hint fails its own future only, a queued mode switch is not overtaken."""
    import controlnet_reference as cr
    from test_refine_gpu import _held_pool, _minipool, _outcome
    minipool = _minipool()

    def mk(s):
        kind = s % 3
        extra = [dict(), dict(controlnet_image=cr.test_hint(64, 64, s)), dict(controlnet_image=cr.test_hint(64, 64, s),
                                                                              controlnet_conditioning_scale=0.5)][kind]
        return _Req(prompt=f"mixed {s}", seed=s, **extra)
    solo = {s: worker.run_job(_Job(mk(s))) for s in range(12)}
    pool, gate, hold = _held_pool(worker, minipool)
    try:
        n0 = len(worker._engine.batcher.batches)
        futs = [pool.submit_job(minipool.GenerationJob(req=mk(s))) for s in range(12)]
        bad = pool.submit_job(minipool.GenerationJob(req=_Req(prompt="bad", seed=99, controlnet_image=b"not an image")))
        gate.set()
        hold.result(60)
        res = [_outcome(f) for f in futs]
        rb = _outcome(bad)
        pool.q.join()
        assert res == [solo[s] for s in range(12)]
        assert isinstance(rb, RuntimeError) and "controlnet_image" in str(rb)
        assert len(worker._engine.batcher.batches[n0:]) < 12               # they were coalesced, each class among itself
    finally:
        worker.bind_queue(None)
        pool._worker = None
        pool.shutdown()
    # a mode switch queued between ControlNet jobs is a barrier: the jobs behind it are not drained into the pass before it
    pool, gate, hold = _held_pool(worker, minipool)
    try:
        q = pool.q
        running = minipool.GenerationJob(req=mk(1))                       # the job whose run_job call would drain the queue
        behind = minipool.GenerationJob(req=mk(4))                        # same key, but queued BEHIND a job of another kind
        barrier = pool.submit_job(minipool.CustomJob(handler=lambda: "barrier"))
        fb = pool.submit_job(behind)
        assert worker._drain(q, running, worker._job_key(running.req), 7) == []
        gate.set()
        hold.result(60)
        assert _outcome(barrier) == "barrier" and _outcome(fb) == solo[4]
        pool.q.join()
    finally:
        worker.bind_queue(None)
        pool._worker = None
        pool.shutdown()
