"""Hires fix on the GPU (enable_hr and its fields): lcm_latents_upscale_renoise against the float64 reference of
tests/hires_reference.py, the two-size chain against the CPU restatement, the worker's behaviour -- bytes that do not depend on
batch or padding, plain requests untouched, isolation of a bad request -- and the hand-over launch audited inside a real chain."""
import io
import os
import sys
import threading
from dataclasses import dataclass, field
from typing import Optional

import numpy as np
import pytest
import torch

import hires_reference as hr
import launch_audit as la

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


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
    enable_hr: Optional[bool] = None
    hr_scale: Optional[float] = None
    hr_resize_x: Optional[int] = None
    hr_resize_y: Optional[int] = None
    hr_second_pass_steps: Optional[int] = None
    denoising_strength: Optional[float] = None
    hr_upscaler: Optional[str] = None
    denoise_strength: Optional[float] = None
    pass_number: Optional[int] = None
    controlnet_image: Optional[object] = None


@dataclass
class _Job:
    req: _Req


def _png_size(png):
    from PIL import Image
    return Image.open(io.BytesIO(png)).size


# ---------------------------------------------------------------------------------------------------------------------------
# the kernel
# ---------------------------------------------------------------------------------------------------------------------------
def _operands(B, h, w, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    x0 = torch.randn(B, 4, h, w, generator=g)
    x0 = x0 * (4.0 / float(x0.abs().max()))                # max|x0| = 4: the scale of denoised SD latents
    return x0, torch.randn(B, 4, H, W, generator=g)


@pytest.mark.parametrize("B,dup", [(1, False), (2, True)])
@pytest.mark.parametrize("mode", hr.MODES)
@pytest.mark.parametrize("shape", hr.SHAPES, ids=lambda s: f"{s[0][0]}x{s[0][1]}-{s[1][0]}x{s[1][1]}")
def test_upscale_renoise_fp64(shape, mode, B, dup):
    from sdlcm_amd import ops
    from sdlcm_amd.scheduler import LCMSchedule
    (h, w), (H, W) = shape
    s = LCMSchedule()
    sa, sb = s.renoise_coefficients(s.timesteps(4, 0.7)[0])
    x0, noise = _operands(B, h, w, H, W, seed=17 * h + W + mode)
    rows = 2 * B if dup else B
    lat = torch.full((rows + 1, 4, H, W), -7.0, device=DEV)           # one image more: must stay untouched
    x_up = torch.full((B + 1, 4, H, W), -7.0, device=DEV)
    ops.latents_upscale_renoise(x0.to(DEV), h, w, noise.to(DEV), sa, sb, mode, lat, B, H, W, x_up=x_up, dup=dup)
    torch.cuda.synchronize()
    got, gup = lat.cpu().numpy(), x_up.cpu().numpy()
    up, ref = hr.upscale_renoise_fp64(x0.numpy(), noise.numpy(), sa, sb, H, W, mode)
    tol = hr.operator_tolerance(x0.numpy(), noise.numpy())
    e_lat, e_up = np.abs(got[:B] - ref).max(), np.abs(gup[:B] - up).max()
    print(f"[hires] mode {mode} B={B} dup={dup} {h}x{w} -> {H}x{W}: lat err {e_lat:.3g}, x_up err {e_up:.3g}, bound {tol:.3g}")
    assert e_lat <= tol and e_up <= tol
    if dup:
        assert np.array_equal(got[:B], got[B:2 * B])
    assert (got[rows] == -7.0).all() and (gup[B] == -7.0).all()
    # without x_up: the same bits
    lat2 = torch.zeros(rows, 4, H, W, device=DEV)
    ops.latents_upscale_renoise(x0.to(DEV), h, w, noise.to(DEV), sa, sb, mode, lat2, B, H, W, dup=dup)
    torch.cuda.synchronize()
    assert la.same_bits(lat2, lat[:rows])


@pytest.mark.parametrize("mode", hr.MODES)
@pytest.mark.parametrize("B,h,w,dup", [(1, 8, 8, False), (3, 9, 5, True), (2, 64, 64, True)])
def test_identity_size_has_the_bits_of_latents_renoise(mode, B, h, w, dup):
    """H == h, W == w: modes 0 and 2 must equal lcm_latents_renoise bit for bit (the issue); bicubic's weights are exactly
    (0, 1, 0, 0) there, so it does too."""
    from sdlcm_amd import ops
    x0, noise = _operands(B, h, w, h, w, seed=5)
    rows = 2 * B if dup else B
    a, b = torch.zeros(rows, 4, h, w, device=DEV), torch.zeros(rows, 4, h, w, device=DEV)
    x_up = torch.zeros(B, 4, h, w, device=DEV)
    ops.latents_upscale_renoise(x0.to(DEV), h, w, noise.to(DEV), 0.5477, 0.8367, mode, a, B, h, w, x_up=x_up, dup=dup)
    ops.latents_renoise(x0.to(DEV), noise.to(DEV), 0.5477, 0.8367, b, B, h, w, dup=dup)
    torch.cuda.synchronize()
    assert la.same_bits(a, b) and la.same_bits(x_up.cpu(), x0)


def test_bad_arguments_return_an_error_and_launch_nothing():
    from sdlcm_amd import ops
    from sdlcm_amd.lib import LcmHipError
    x0 = torch.ones(1, 4, 4, 4, device=DEV)
    noise = torch.ones(1, 4, 16, 16, device=DEV)
    lat = torch.full((1, 4, 16, 16), -7.0, device=DEV)
    for kw, text in ((dict(mode=3), "unknown mode"), (dict(mode=-1), "unknown mode"), (dict(H=17), "outside"), (dict(W=3), "outside"),
                     (dict(h=0), "bad shape"), (dict(B=0), "bad shape"), (dict(x0=None), "null pointer"), (dict(lat=None), "null pointer")):
        a = dict(x0=x0, h=4, w=4, noise=noise, mode=0, lat=lat, B=1, H=16, W=16)
        a.update(kw)
        with pytest.raises(LcmHipError, match=text):
            ops.latents_upscale_renoise(a["x0"], a["h"], a["w"], a["noise"], 0.6, 0.8, a["mode"], a["lat"], a["B"], a["H"], a["W"])
    torch.cuda.synchronize()
    assert (lat == -7.0).all()


# ---------------------------------------------------------------------------------------------------------------------------
# the chain against the CPU restatement
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def state():
    from sdlcm_amd import weights
    from sdlcm_amd.pipeline import LcmHipPipeline
    usd, vsd = weights.synthetic_unet(), weights.synthetic_vae()
    hip = LcmHipPipeline(usd, vsd, device=DEV)
    yield dict(hip=hip, ora=hr.HiresChainOracle(usd, vsd))
    hip.close()


def _embeds(B, seed=5):
    return torch.randn(B, 77, 768, generator=torch.Generator().manual_seed(seed)).to(torch.float16)


def _image_err(out, b, ref):
    a = np.clip(out["image"][b:b + 1].transpose(0, 3, 1, 2) / 2 + 0.5, 0, 1)
    return float(np.abs(a - np.clip(ref["image"] / 2 + 0.5, 0, 1)).max())


@pytest.mark.parametrize("B,target,mode", [(1, (96, 96), hr.BILINEAR), (2, (128, 128), hr.BICUBIC)])
def test_chain_parity_with_the_cpu_restatement(state, B, target, mode):
    hip, ora = state["hip"], state["ora"]
    seeds = [4100 + b for b in range(B)]
    pe = _embeds(B, seed=40 + B)
    hires = (target[0], target[1], 2, 0.7, mode)
    out = hip.generate(pe, seeds, 64, 64, 2, 1.0, want_float=True, hires=hires)
    assert out["unet_evals"] == 4
    assert out["rgb"].shape == (B, target[1], target[0], 3) and out["latents"].shape == (B, 4, target[1] // 8, target[0] // 8)
    assert out["lowres_latents"].shape == (B, 4, 8, 8) and out["pool8"].shape == (B, 4, 8, 8)
    for b in range(B):
        ref = ora(pe[b:b + 1].float(), 64, 64, 2, 1.0, seeds[b], hires)
        e = _image_err(out, b, ref)
        print(f"[hires] 64x64 -> {target[0]}x{target[1]} mode {mode} request {b} of {B}: image[0,1] max|d| = {e:.4g}, "
              f"upscaled max|d| = {np.abs(out['upscaled_latents'][b] - ref['upscaled'][0]).max():.3g}")
        assert e < 1e-2
        assert np.abs(out["rgb"][b].astype(int) - ref["image_u8"][0].astype(int)).max() <= 3
    # stage 1 is the plain request, bit for bit -- and it did not decode: the plain request's plan is another one
    plain = hip.generate(pe, seeds, 64, 64, 2, 1.0)
    assert np.array_equal(out["lowres_latents"], plain["latents"])
    # the captured graphs give the eager bytes; a request's bytes do not depend on its batch
    rep = hip.generate(pe, seeds, 64, 64, 2, 1.0, hires=hires)
    assert np.array_equal(rep["rgb"], out["rgb"]) and np.array_equal(rep["latents"], out["latents"])
    assert np.array_equal(rep["lowres_latents"], plain["latents"]) and rep["unet_evals"] == 4
    if B > 1:
        solo = hip.generate(pe[1:], seeds[1:], 64, 64, 2, 1.0, hires=hires)
        assert np.array_equal(solo["rgb"][0], rep["rgb"][1]) and np.array_equal(solo["pool8"][0], rep["pool8"][1])
    kinds = [k[-1] for k in hip.lanes[0].plans if isinstance(k[-1], str)]
    assert "latents" in kinds and "from-state" in kinds


def test_chain_under_classifier_free_guidance():
    """A UNet without the guidance embedding: guidance 3.0 with negative embeddings is classifier-free guidance on doubled rows
    (the hand-over writes both halves of the state); nearest-exact."""
    from sdlcm_amd import weights
    from sdlcm_amd.pipeline import LcmHipPipeline
    nocond = dict(time_cond_proj_dim=None)
    usd, vsd = weights.synthetic_unet(nocond), weights.synthetic_vae()
    hip = LcmHipPipeline(usd, vsd, unet_cfg=nocond, device=DEV)
    try:
        from sdlcm_amd.config import unet_config
        ora = hr.HiresChainOracle(usd, vsd, unet_config(nocond))
        pe, ne = _embeds(1, seed=71), _embeds(1, seed=72)
        hires = (96, 96, 2, 0.7, hr.NEAREST_EXACT)
        out = hip.generate(pe, [88], 64, 64, 2, 3.0, negative_embeds=ne, want_float=True, hires=hires)
        ref = ora(pe.float(), 64, 64, 2, 3.0, 88, hires, negative_embeds=ne.float())
        e = _image_err(out, 0, ref)
        print(f"[hires] cfg 3.0, 64x64 -> 96x96 nearest-exact: image[0,1] max|d| = {e:.4g}")
        assert e < 1e-2 and out["unet_evals"] == 8
        plain = hip.generate(pe, [88], 64, 64, 2, 3.0, negative_embeds=ne)
        rep = hip.generate(pe, [88], 64, 64, 2, 3.0, negative_embeds=ne, hires=hires)
        assert np.array_equal(out["lowres_latents"], plain["latents"]) and np.array_equal(rep["rgb"], out["rgb"])
    finally:
        hip.close()


def test_generate_argument_errors(state):
    from sdlcm_amd.lib import LcmHipError
    hip, pe = state["hip"], _embeds(1)
    with pytest.raises(ValueError, match="The combined original_steps x strength"):
        hip.generate(pe, [1], 64, 64, 2, 1.0, hires=(96, 96, 7, 0.1, 0))
    for hires, text in (((96, 96, 2, 0.7, 5), "unknown latent upscaler"), ((320, 96, 2, 0.7, 0), "outside"),
                        ((96, 100, 2, 0.7, 0), "divisible by 8")):
        with pytest.raises(LcmHipError, match=text):
            hip.generate(pe, [1], 64, 64, 2, 1.0, hires=hires)
    with pytest.raises(LcmHipError, match="not combined"):
        hip.generate(pe, [1], 64, 64, 2, 1.0, hires=(96, 96, 2, 0.7, 0), strength=0.5, passes=1)


def test_hand_over_launch_audited_inside_a_real_chain(state, monkeypatch):
    """tests/launch_audit.py's hook, extended by the new entry point: the chain runs eagerly under the audit, and the hand-over
    launch -- fed by the real stage 1, feeding the real stage 2 -- is compared against float64 under the operator bound; what it
    must not write stays unchanged; every other launch of both stages is checked as in any audited pass."""
    hip = state["hip"]
    monkeypatch.setitem(la.CHECKED, "latents_upscale_renoise", ("lat", "x_up"))

    class Audit(la.Audit):
        def _ref_latents_upscale_renoise(self, B, A, r):
            Bn, h, w, H, W, dup, mode = A["B"], A["h"], A["w"], A["H"], A["W"], A["dup"], A["mode"]
            n = Bn * 4 * H * W
            assert la.tail_same(A["lat"], B["lat"], (2 if dup else 1) * n) and la.tail_same(A["x_up"], B["x_up"], n)
            x0 = B["x0"].reshape(-1)[:Bn * 4 * h * w].view(Bn, 4, h, w).cpu().numpy()
            nz = B["noise"].reshape(-1)[:n].view(Bn, 4, H, W).cpu().numpy()
            up, ref = hr.upscale_renoise_fp64(x0, nz, A["sqrt_a"], A["sqrt_b"], H, W, mode)
            tol = hr.operator_tolerance(x0, nz)
            lat = A["lat"].reshape(-1)[:n].view(Bn, 4, H, W).cpu().numpy()
            xu = A["x_up"].reshape(-1)[:n].view(Bn, 4, H, W).cpu().numpy()
            return max(np.abs(lat - ref).max(), np.abs(xu - up).max()) / tol, None

    plans = hip.lanes[0].plans
    before = set(plans)
    with Audit() as au:
        out = hip.generate(_embeds(2, seed=77), [501, 502], 72, 40, 2, 1.0, want_float=True, hires=(136, 104, 2, 0.7, hr.BICUBIC))
    for k in set(plans) - before:
        plans.pop(k)
    bad = la.failures(au.checks)
    per = la.entry_table(au.checks)
    print(f"[audit] hires 72x40 -> 136x104 B2: {len(au.checks)} launches checked, {la.summary_line(au.checks)}")
    assert not bad, bad
    assert per["latents_upscale_renoise"][0] == 1 and per["latents_upscale_renoise"][1] <= 1.0
    assert "latents_renoise" not in per                   # the hand-over IS the re-noise: stage 2 launches none of its own
    assert au.checked_keys() == au.record_keys() and np.isfinite(out["latents"]).all()


# ---------------------------------------------------------------------------------------------------------------------------
# the worker
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def worker():
    os.environ["MODEL"] = "synthetic"
    os.environ.setdefault("MODEL_ROOT", "/nonexistent")
    from sdlcm_amd.backends.worker_factory import create_hip_worker
    w = create_hip_worker(worker_id=0)
    yield w
    w.close()


def _mk(s, **extra):
    kw = dict(enable_hr=True, hr_scale=1.5, denoising_strength=0.7)
    kw.update(extra)
    return _Req(prompt=f"hires {s}", seed=s, **kw)


def test_run_job_serves_enable_hr(worker, state):
    """The test that fails without the feature: the PNG has the target size and is what the CPU restatement gives."""
    eng = worker._engine
    n0 = eng.stats["hires_requests"], eng.stats["unet_evals"]
    plain, _ = worker.run_job(_Job(_Req(prompt="hires 3", seed=3)))
    png, seed = worker.run_job(_Job(_mk(3)))
    assert seed == 3 and _png_size(plain) == (64, 64) and _png_size(png) == (96, 96)
    assert eng.stats["hires_requests"] == n0[0] + 1 and eng.stats["unet_evals"] == n0[1] + 2 + 4
    with torch.cuda.stream(eng.pipe.stream):
        pe = eng.encode(["hires 3"]).float().cpu()
        eng.pipe.stream.synchronize()
    ref = state["ora"](pe, 64, 64, 2, 1.0, 3, (96, 96, 2, 0.7, hr.BILINEAR))
    from PIL import Image
    got = np.asarray(Image.open(io.BytesIO(png)).convert("RGB")).astype(int)
    assert np.abs(got - ref["image_u8"][0].astype(int)).max() <= 3
    # run_job_with_latents: the 8x8 pool of the final target-size latents
    from oracle import glue
    png2, _, blob = worker.run_job_with_latents(_Job(_mk(3)))
    assert png2 == png and len(blob) == 512
    want = np.frombuffer(glue.latents_blob(ref["latents"]), np.float16).astype(np.float32)
    got = np.frombuffer(blob, np.float16).astype(np.float32)
    assert np.abs(got - want).max() < 5e-3 * max(1.0, want.std()) + 2.0 ** -10 * np.abs(want).max()
    # the other fields reach the chain
    assert _png_size(worker.run_job(_Job(_mk(3, hr_resize_x=128, hr_resize_y=72)))[0]) == (128, 72)
    assert worker.run_job(_Job(_mk(3, hr_upscaler="Latent (bicubic)")))[0] != png
    assert worker.run_job(_Job(_mk(3, hr_second_pass_steps=3)))[0] != png


def test_bytes_do_not_depend_on_batch_or_padding_and_plain_requests_are_untouched(worker):
    from sdlcm_amd.backends.hip_worker import encode_png
    eng = worker._engine
    plain_req = _Req(prompt="a quiet harbour", seed=5)
    plain_before = worker.run_job(_Job(plain_req))
    plain_key = worker._job_key(plain_req)
    req = _mk(0)
    key = worker._job_key(req)
    assert key[:6] == plain_key[:6] and len(plain_key) == 6 and key[6:] == ("hires", 96, 96, 2, 0.7, 0)

    def batch(reqs, lane=0):
        return encode_png(eng.run_batch(key, [worker._prepare(r, key) for r in reqs], lane)[0][0])
    pngs = {"alone": worker.run_job(_Job(req))[0],
            "batch of 2": batch([req, _mk(1)]),
            "padded tail": batch([req, _mk(1), _mk(2), _mk(2)]),
            "batch of 8": batch([req] + [_mk(s) for s in range(1, 8)])}
    if eng.n_lanes > 1:
        pngs["lane 1"] = batch([req], lane=1)
    for tag, png in pngs.items():
        assert png == pngs["alone"], tag
    assert _png_size(pngs["alone"]) == (96, 96)
    assert worker.run_job(_Job(plain_req)) == plain_before
    assert worker.run_job(_Job(_Req(prompt="a quiet harbour", seed=5, enable_hr=False, hr_scale=3.0))) == plain_before


def test_a_pass_is_capped_at_what_the_workspace_holds(worker, monkeypatch):
    """The need comes from the plan: with a workspace that holds two images' parts, a batch of 4 runs as 2 + 2 and every request
    keeps its bytes; the cap never goes below one."""
    eng = worker._engine
    pipe = eng.pipe
    key = worker._job_key(_mk(0))
    solo = [eng.run_batch(key, [worker._prepare(_mk(s), key)], 0)[0][0] for s in range(4)]
    P = pipe.plan(1, 12, 12, 2, False, 1.0, lane=0, refine=(0.7, 1, True), kind="from-state")
    need = pipe.splitk_need(P)
    print(f"[hires] split-K workspace a 96x96 second stage needs per image: {need} bytes")
    assert need >= 0 and pipe.hires_batch_cap(96, 96, 2, 0.7, sizes=eng.batch_sizes) == max(eng.batch_sizes)
    calls = []
    real = pipe.generate
    monkeypatch.setattr(pipe, "generate", lambda pe, seeds, *a, **kw: calls.append(len(seeds)) or real(pe, seeds, *a, **kw))
    monkeypatch.setattr(type(pipe), "hires_batch_cap", lambda self, *a, **kw: 2)
    got = eng.run_batch(key, [worker._prepare(_mk(s), key) for s in range(4)], 0)
    assert calls == [2, 2]
    for s in range(4):
        assert np.array_equal(got[s][0], solo[s])
    monkeypatch.undo()
    if need:
        have = pipe.lanes[0].splitk_ws.numel() * 4
        assert pipe.hires_batch_cap(96, 96, 2, 0.7, sizes=(1, 2, 4, have // need * 2 + 8)) == 4


def _minipool():
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from tools import minipool
    return minipool


def _outcome(f):
    try:
        return f.result(600)
    except Exception as e:      # noqa
        return e


def test_errors_reach_the_right_job_inside_a_drained_batch(worker):
    minipool = _minipool()
    bad = {2: (dict(hr_scale=9.0), "hr_scale"), 4: (dict(hr_upscaler="ESRGAN_4x"), "Latent (nearest-exact)"),
           5: (dict(denoise_strength=0.5), "not combined"), 6: (dict(hr_second_pass_steps=40), "The combined original_steps x strength"),
           7: (dict(controlnet_image=np.zeros((64, 64, 3), np.uint8)), "not combined")}
    solo = {s: worker.run_job(_Job(_mk(s))) for s in range(9) if s not in bad}
    pool = minipool.MiniPool(lambda worker_id: worker, {"m": "synthetic"}, "m")
    worker.bind_queue(pool.q)
    gate, inside = threading.Event(), threading.Event()
    hold = pool.submit_job(minipool.CustomJob(handler=lambda: (inside.set(), gate.wait(30))))
    assert inside.wait(30)
    try:
        n0 = len(worker._engine.batcher.batches)
        futs = [pool.submit_job(minipool.GenerationJob(req=_mk(s, **bad.get(s, ({}, ""))[0]))) for s in range(9)]
        gate.set()
        hold.result(60)
        res = [_outcome(f) for f in futs]
        pool.q.join()
        for s in range(9):
            if s in bad:
                assert isinstance(res[s], RuntimeError) and bad[s][1] in str(res[s]), (s, res[s])
            else:
                assert res[s] == solo[s], s
        ran = worker._engine.batcher.batches[n0:]
        assert sum(ran) == 4 and len(ran) < 4                       # the four good jobs shared passes
    finally:
        worker.bind_queue(None)
        pool._worker = None
        pool.shutdown()


def test_the_sdxl_worker_refuses_enable_hr(monkeypatch):
    monkeypatch.setenv("MODEL", "synthetic-sdxl")
    monkeypatch.setenv("MODEL_ROOT", "/nonexistent")
    from sdlcm_amd.backends.hip_worker import HipLcmSDXLWorker
    with pytest.raises(RuntimeError, match="SDXL"):
        HipLcmSDXLWorker._job_key(_mk(1))
