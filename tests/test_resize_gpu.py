"""The HIP Lanczos resampler on the MI355X (csrc/resize.hip) against PIL itself, byte for byte: ``ops.resize_lanczos_u8`` on the
case list (every size as L and RGB, with a noise picture and with a 0/255 picture that drives the overshoot into both clamps),
the output window and the destination stride, ``hip_worker.resize`` for the three ``resize_mode`` values and its PIL fallback,
and whole requests: the same upload fitted under LCM_RESIZE=hip and under LCM_RESIZE=pil gives identical PNG bytes."""
import os
from dataclasses import dataclass, field
from typing import Any, Optional

import numpy as np
import pytest
import torch

import resize_reference as R
from test_resize_cpu import CASES, picture, pil_resize

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _resize(a, w, h, window=None, poison=0xA5):
    """Host uint8 [sh,sw] or [sh,sw,3] -> the device's fit (or its window), host."""
    from sdlcm_amd import ops
    C = 1 if a.ndim == 2 else 3
    sh, sw = a.shape[:2]
    ww, wh = (w, h) if window is None else window[2:]
    need = ops.resize_ws_bytes(sw, sh, C, w, h, window)
    assert need > 0
    ws = torch.full((need,), poison, dtype=torch.uint8, device=DEV)              # poisoned: nothing relies on zeros
    out = torch.full((wh, ww) + a.shape[2:], 77, dtype=torch.uint8, device=DEV)
    ops.resize_lanczos_u8(torch.from_numpy(a).to(DEV), out, ws, w, h, window)
    return out.cpu().numpy()


@pytest.mark.parametrize("src,out", CASES, ids=lambda v: f"{v[0]}x{v[1]}")
def test_resampler_equals_pil(src, out):
    for channels in (1, 3):
        for kind in ("noise", "bw"):
            a = picture(src[0], src[1], channels, kind)
            got = _resize(a, out[0], out[1])
            want = pil_resize(a, out[0], out[1])
            assert got.shape == want.shape
            bad = np.argwhere(got != want)
            assert bad.size == 0, (channels, kind, len(bad), bad[:4].tolist())
            if kind == "bw" and (src, out) in (((7, 5), (64, 64)), ((64, 64), (512, 512))):
                assert want.min() == 0 and want.max() == 255                     # the overshoot met both clamps


def test_window_and_stride_write_one_slot_only():
    from sdlcm_amd import ops
    a = picture(300, 200, 3, "noise", 3)
    full = pil_resize(a, 96, 64)
    win = (16, 0, 64, 64)                                                        # resize_mode 1 of 300x200 for a 64x64 request
    assert R.mode_geometry(1, 300, 200, 64, 64) == (96, 64, 16, 0)
    batch = torch.empty((2, 64, 64, 3), dtype=torch.uint8, device=DEV)
    pattern = torch.arange(64 * 64 * 3, device=DEV).mul(37).add(11).to(torch.uint8).reshape(64, 64, 3)
    batch[0].copy_(pattern)
    batch[1].fill_(99)
    ws = torch.full((ops.resize_ws_bytes(300, 200, 3, 96, 64, win),), 0x5A, dtype=torch.uint8, device=DEV)
    ops.resize_lanczos_u8(torch.from_numpy(a).to(DEV), batch[1], ws, 96, 64, win)
    assert np.array_equal(batch[1].cpu().numpy(), full[:, 16:80])
    assert torch.equal(batch[0], pattern)
    # a gray mask into slot 0 of a [2,H,W] tensor, rows of a wider destination (stride 80 bytes), a window in the middle
    m = picture(129, 67, 1, "bw", 4)
    wide = torch.full((2, 40, 80), 7, dtype=torch.uint8, device=DEV)
    dst = wide[0, 3:33, 10:60]
    assert dst.stride(0) == 80
    w2 = (5, 7, 50, 30)
    ws2 = torch.full((ops.resize_ws_bytes(129, 67, 1, 100, 50, w2),), 0x5A, dtype=torch.uint8, device=DEV)
    ops.resize_lanczos_u8(torch.from_numpy(m).to(DEV), dst, ws2, 100, 50, w2)
    got = wide.cpu().numpy()
    assert np.array_equal(got[0, 3:33, 10:60], pil_resize(m, 100, 50)[7:37, 5:55])
    got[0, 3:33, 10:60] = 7
    assert (got == 7).all()
    # windows that leave the grid replicate its edge (resize_mode 2), on either axis and with a pass that keeps its size
    small = pil_resize(a, 64, 42)
    assert np.array_equal(_resize(a, 64, 42, (0, -11, 64, 64)), np.pad(small, ((11, 11), (0, 0), (0, 0)), mode="edge"))
    tall = pil_resize(a, 30, 64)
    assert np.array_equal(_resize(a, 30, 64, (-17, 0, 64, 64)), np.pad(tall, ((0, 0), (17, 17), (0, 0)), mode="edge"))
    keep = picture(40, 64, 3, "noise", 8)
    assert np.array_equal(_resize(keep, 40, 64, (-12, 0, 64, 64)), np.pad(keep, ((0, 0), (12, 12), (0, 0)), mode="edge"))
    assert np.array_equal(_resize(keep, 64, 64, (0, 0, 64, 64)), pil_resize(keep, 64, 64))
    # a workspace that is too small, a destination of another shape: refused before any launch
    from sdlcm_amd.lib import LcmHipError
    with pytest.raises(LcmHipError, match="workspace"):
        ops.resize_lanczos_u8(torch.from_numpy(a).to(DEV), batch[1], ws[:4096], 96, 64, win)
    with pytest.raises(LcmHipError, match="destination"):
        ops.resize_lanczos_u8(torch.from_numpy(a).to(DEV), batch, ws, 96, 64, win)


def test_public_resize_modes_and_fallback(monkeypatch):
    from sdlcm_amd.backends import fit, hip_worker
    monkeypatch.setenv("LCM_RESIZE", "hip")
    for (sw, sh), (W, H) in (((300, 200), (64, 64)), ((100, 50), (64, 64)), ((50, 100), (72, 40)), ((33, 65), (96, 48))):
        for a in (picture(sw, sh, 3, "noise", 11), picture(sw, sh, 1, "bw", 12)):
            for mode in (0, 1, 2):
                assert fit.is_pending(fit.prepare(a, W, H, mode))
                got = hip_worker.resize(a, W, H, mode)
                assert np.array_equal(got, fit.fit_host(a, W, H, mode)), (sw, sh, W, H, mode)      # PIL + crop / np edge replication
                assert np.array_equal(got, R.fit(a, W, H, mode))
    edge = picture(3, 300, 3, "noise")
    assert fit.is_pending(fit.prepare(edge, 8, 16)) and np.array_equal(hip_worker.resize(edge, 8, 16), pil_resize(edge, 8, 16))
    out = picture(3, 301, 3, "noise")                                            # PIL swaps its passes here: the fallback takes it
    assert not fit.is_pending(fit.prepare(out, 8, 16)) and np.array_equal(hip_worker.resize(out, 8, 16), pil_resize(out, 8, 16))
    same = picture(64, 64, 3, "noise")
    assert hip_worker.resize(same, 64, 64, 1) is same
    monkeypatch.setenv("LCM_RESIZE", "pil")
    a = picture(100, 80, 3, "noise")
    assert np.array_equal(hip_worker.resize(a, 64, 64), pil_resize(a, 64, 64))
    with pytest.raises(ValueError, match="resize"):
        hip_worker.resize(a.astype(np.float32), 64, 64)
    with pytest.raises(ValueError, match="mode"):
        hip_worker.resize(a, 64, 64, 3)


# ---- whole requests ------------------------------------------------------------------------------------------------------------
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
    init_image: Optional[Any] = None
    denoising_strength: Optional[float] = None
    mask: Optional[Any] = None
    resize_mode: Optional[Any] = None
    controlnet_image: Optional[Any] = None
    controlnet_module: Optional[str] = None


@dataclass
class _Job:
    req: _Req


def _photo(w, h, seed):
    """A smooth picture with texture (seeded), uint8 [h, w, 3]."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([128 + 100 * np.sin(x / 7.0 + seed), 128 + 100 * np.cos(y / 5.0), 128 + 90 * np.sin((x + y) / 9.0)], -1)
    return np.clip(base + rng.normal(0, 12, (h, w, 3)), 0, 255).astype(np.uint8)


def _mask(w, h):
    m = np.zeros((h, w), np.uint8)
    m[h // 5:h * 3 // 4, w // 3:w * 4 // 5] = 255
    return m


@pytest.fixture(scope="module")
def worker():
    old = {k: os.environ.get(k) for k in ("MODEL", "MODEL_ROOT", "CONTROLNET", "LCM_RESIZE")}
    os.environ["MODEL"] = "synthetic"
    os.environ.setdefault("MODEL_ROOT", "/nonexistent")
    os.environ["CONTROLNET"] = "synthetic"
    from sdlcm_amd.backends.worker_factory import create_hip_worker
    w = create_hip_worker(worker_id=0)
    yield w
    w.close()
    for k, v in old.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def _both(worker, make):
    """The request under LCM_RESIZE=hip and under LCM_RESIZE=pil -> (png, png, requests the device fitted in each)."""
    eng = worker._engine
    out = []
    for mode in ("hip", "pil"):
        os.environ["LCM_RESIZE"] = mode
        n0 = eng.stats["resized_on_device"]
        out.append((worker.run_job(_Job(make())), eng.stats["resized_on_device"] - n0))
    os.environ["LCM_RESIZE"] = "hip"
    return out[0][0], out[1][0], (out[0][1], out[1][1])


def test_requests_keep_their_bytes_whichever_resampler_fits_them(worker):
    from sdlcm_amd.backends import fit
    eng = worker._engine
    kinds = {
        "img2img": lambda: _Req(prompt="a harbour", seed=5, init_image=_photo(100, 80, 1), denoising_strength=0.5),
        "inpaint": lambda: _Req(prompt="a harbour", seed=6, init_image=_photo(100, 80, 2), denoising_strength=0.5, mask=_mask(90, 70)),
        "canny": lambda: _Req(prompt="a harbour", seed=7, controlnet_image=_photo(100, 80, 3), controlnet_module="canny"),
        "hint": lambda: _Req(prompt="a harbour", seed=8, controlnet_image=_photo(100, 80, 4)),
        "inpaint, mode 2": lambda: _Req(prompt="a harbour", seed=9, init_image=_photo(100, 80, 5), denoising_strength=0.5,
                                        mask=_mask(90, 70), resize_mode=2),
    }
    pngs = {}
    for name, make in kinds.items():
        hip, pil, moved = _both(worker, make)
        assert hip == pil and hip[0][:8] == b"\x89PNG\r\n\x1a\n", name
        assert moved == (1, 0), (name, moved)                                    # one REQUEST, also with a picture and a mask
        pngs[name] = hip
    assert len(set(p[0] for p in pngs.values())) == len(pngs)
    # the upload reaches the chain: the same request with the picture fitted by the caller, and with another picture
    os.environ["LCM_RESIZE"] = "hip"
    fitted = fit.fit_host(_photo(100, 80, 1), 64, 64)
    n0 = eng.stats["resized_on_device"]
    assert worker.run_job(_Job(_Req(prompt="a harbour", seed=5, init_image=fitted, denoising_strength=0.5))) == pngs["img2img"]
    assert eng.stats["resized_on_device"] == n0                                  # an upload of the request's size moves no counter
    assert worker.run_job(_Job(_Req(prompt="a harbour", seed=5, init_image=_photo(100, 80, 11), denoising_strength=0.5))) != pngs["img2img"]
    assert eng.stats["resized_on_device"] == n0 + 1
    # uploads of two sizes and one that fits, in one batched pass: every request keeps its solo bytes
    key = worker._job_key(kinds["img2img"]())
    reqs = [kinds["img2img"](), _Req(prompt="a harbour", seed=5, init_image=fitted, denoising_strength=0.5),
            _Req(prompt="a quay", seed=12, init_image=_photo(33, 65, 6), denoising_strength=0.5)]
    from sdlcm_amd.backends.hip_worker import encode_png
    got = [encode_png(r[0]) for r in eng.run_batch(key, [worker._prepare(r, key) for r in reqs], 0)]
    assert got[0] == pngs["img2img"][0] == got[1] and got[2] == worker.run_job(_Job(reqs[2]))[0]


def test_resize_mode_crops_on_the_device(worker):
    from sdlcm_amd.backends import fit
    os.environ["LCM_RESIZE"] = "hip"
    eng = worker._engine
    pic = _photo(100, 50, 21)
    cropped = pil_resize(pic, 128, 64)[:, 32:96]                                 # mode 1 on the host: cover 64x64, keep the centre
    assert np.array_equal(cropped, fit.fit_host(pic, 64, 64, 1))
    mk = lambda img, **kw: _Job(_Req(prompt="a lighthouse", seed=3, init_image=img, denoising_strength=0.6, **kw))
    n0 = eng.stats["resized_on_device"]
    with_mode = worker.run_job(mk(pic, resize_mode=1))
    assert eng.stats["resized_on_device"] == n0 + 1
    assert with_mode == worker.run_job(mk(cropped))
    assert eng.stats["resized_on_device"] == n0 + 1
    assert with_mode != worker.run_job(mk(pic)) and with_mode != worker.run_job(mk(pic, resize_mode=2))
    assert worker.run_job(mk(pic, resize_mode=2)) == worker.run_job(mk(fit.fit_host(pic, 64, 64, 2)))
    assert worker.run_job(mk(pic, resize_mode=0)) == worker.run_job(mk(pic))
    # a request without a picture does not have the field read
    plain = worker.run_job(_Job(_Req(prompt="a lighthouse", seed=3)))
    assert worker.run_job(_Job(_Req(prompt="a lighthouse", seed=3, resize_mode=3))) == plain


def test_latent_upscale_mode_fails_its_own_job_inside_a_batch(worker):
    from test_refine_gpu import _held_pool, _minipool, _outcome
    os.environ["LCM_RESIZE"] = "hip"
    minipool = _minipool()
    good = lambda: _Req(prompt="a pier", seed=31, init_image=_photo(100, 80, 31), denoising_strength=0.5, resize_mode=1)
    bad = lambda: _Req(prompt="a pier", seed=32, init_image=_photo(100, 80, 32), denoising_strength=0.5, resize_mode=3)
    solo = worker.run_job(_Job(good()))
    with pytest.raises(RuntimeError, match="Invalid resize_mode 3"):
        worker.run_job(_Job(bad()))
    pool, gate, hold = _held_pool(worker, minipool)
    try:
        futs = [pool.submit_job(minipool.GenerationJob(req=r)) for r in (good(), bad())]
        gate.set()
        hold.result(60)
        res = [_outcome(f) for f in futs]
        pool.q.join()
        assert res[0] == solo
        assert isinstance(res[1], RuntimeError) and "Invalid resize_mode 3" in str(res[1]) and "crop and resize" in str(res[1])
    finally:
        worker.bind_queue(None)
        pool._worker = None
        pool.shutdown()
