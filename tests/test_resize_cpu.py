"""The Lanczos resampler's definition and host half, without a GPU: tests/resize_reference.py (the numpy restatement of
include/lcm_hip.h) against PIL's ``Image.resize(..., Image.LANCZOS)`` byte for byte; the library's host tables (csrc/resize.cpp,
through the C ABI) against the restatement's integer tables and bounds exactly; ``backends/fit.py`` -- ``resize_mode`` parsing and
errors, the geometry of modes 1 and 2 against PIL + crop and ``np.pad(mode="edge")``, the domain rule -- and the worker's batch key."""
import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np
import pytest

import resize_reference as R

# source (w, h) -> output (w, h): the case list of tests/test_resize_gpu.py
CASES = [((64, 64), (64, 40)), ((64, 40), (64, 64)), ((7, 5), (64, 64)), ((1, 1), (8, 8)), ((300, 200), (64, 64)),
         ((129, 67), (128, 64)), ((33, 65), (520, 392)), ((1000, 3), (8, 8)), ((2048, 16), (8, 8)), ((16, 1600), (8, 8)),
         ((3, 300), (8, 16)), ((512, 512), (64, 64)), ((64, 64), (512, 512))]


def picture(sw, sh, channels, kind, seed=0):
    """A noise picture, or a 0/255 picture (it drives the Lanczos overshoot into both clamps); uint8 [sh, sw] or [sh, sw, 3]."""
    rng = np.random.default_rng(seed + 1000 * channels + sw * 7 + sh)
    a = rng.integers(0, 256, (sh, sw) if channels == 1 else (sh, sw, 3), dtype=np.uint8)
    return a if kind == "noise" else ((a > 127) * np.uint8(255)).astype(np.uint8)


def pil_resize(a, w, h):
    from PIL import Image
    return np.asarray(Image.fromarray(a, "L" if a.ndim == 2 else "RGB").resize((w, h), Image.LANCZOS))


@pytest.fixture(scope="module")
def L():
    import __graft_entry__
    __graft_entry__.build()
    from sdlcm_amd import lib
    return lib.load()


@pytest.mark.parametrize("src,out", CASES, ids=lambda v: f"{v[0]}x{v[1]}")
def test_restatement_equals_pil(src, out):
    for channels in (1, 3):
        for kind in ("noise", "bw"):
            a = picture(src[0], src[1], channels, kind)
            assert np.array_equal(R.resize(a, out[0], out[1]), pil_resize(a, out[0], out[1])), (channels, kind)


def test_restatement_window_and_fill():
    a = picture(300, 200, 3, "noise")
    full = R.resize(a, 96, 64)
    assert np.array_equal(R.resize(a, 96, 64, (16, 0, 64, 64)), full[:, 16:80])
    assert np.array_equal(R.resize(a, 96, 64, (5, 7, 33, 20)), full[7:27, 5:38])
    small = R.resize(a, 64, 42)
    assert np.array_equal(R.resize(a, 64, 42, (0, -11, 64, 64)), np.pad(small, ((11, 11), (0, 0), (0, 0)), mode="edge"))


@pytest.mark.parametrize("n_in,n_out", [(7, 64), (300, 64), (129, 128), (2048, 8), (1, 8), (64, 64)])
def test_library_tables_equal_the_restatement(L, n_in, n_out):
    for o0, n in ((0, n_out), (-3, n_out + 5), (n_out // 3, max(1, n_out // 2))):
        nb = L.lcm_resize_table_bytes(n_in, n_out, n)
        ks = L.lcm_resize_ksize(n_in, n_out)
        assert ks == R.ksize(n_in, n_out) and nb == (4 * n * (2 + ks) + 15) // 16 * 16
        buf = np.full(nb // 4, -77, np.int32)
        assert L.lcm_resize_tables(n_in, n_out, o0, n, buf.ctypes.data, nb) == 0
        bounds, kk = R.tables(n_in, n_out, o0, n)
        assert np.array_equal(buf[:2 * n].reshape(n, 2), bounds)
        assert np.array_equal(buf[2 * n:2 * n + n * ks].reshape(n, ks), kk)
        first, last = C.c_int(), C.c_int()
        assert L.lcm_resize_span(n_in, n_out, o0, n, C.byref(first), C.byref(last)) == 0
        assert (first.value, last.value) == (bounds[0, 0], bounds[-1, 0] + bounds[-1, 1])
        tile = 5
        spans = [bounds[min(i + tile, n) - 1].sum() - bounds[i, 0] for i in range(0, n, tile)]
        assert L.lcm_resize_max_span(n_in, n_out, o0, n, tile) == max(spans)
    # every row sums to 2^22 within the rounding of its taps, and the accumulator of a pass stays inside int32
    bounds, kk = R.tables(n_in, n_out)
    assert np.abs(kk.sum(1) - (1 << 22)).max() <= bounds[:, 1].max()
    assert (1 << 21) + 255 * np.abs(kk).sum(1).max() < 2 ** 31


def test_library_plans_and_argument_checks(L):
    assert L.lcm_resize_passes(300, 200, 64, 64) == 3 and L.lcm_resize_passes(64, 64, 64, 40) == 2
    assert L.lcm_resize_passes(64, 40, 80, 40) == 1 and L.lcm_resize_passes(64, 40, 64, 40) == 1
    th, tv = L.lcm_resize_table_bytes(300, 96, 64), L.lcm_resize_table_bytes(200, 64, 64)
    assert L.lcm_resize_plan_table_bytes(300, 200, 96, 64, 64, 64) == th + tv
    buf = np.zeros((th + tv) // 4, np.int32)
    assert L.lcm_resize_plan_tables(300, 200, 96, 64, 16, 0, 64, 64, buf.ctypes.data, th + tv) == 0
    bh, kh = R.tables(300, 96, 16, 64)
    bv, kv = R.tables(200, 64, 0, 64)
    assert np.array_equal(buf[:128].reshape(64, 2), bh) and np.array_equal(buf[128:128 + kh.size].reshape(kh.shape), kh)
    v = buf[th // 4:]
    assert np.array_equal(v[:128].reshape(64, 2), bv) and np.array_equal(v[128:128 + kv.size].reshape(kv.shape), kv)
    # the workspace: tables, then only the source rows the vertical pass reads
    first, last = C.c_int(), C.c_int()
    L.lcm_resize_span(200, 64, 0, 64, C.byref(first), C.byref(last))
    assert L.lcm_resize_ws_bytes(3, 300, 200, 96, 64, 16, 0, 64, 64) == th + tv + ((last.value - first.value) * 64 * 3 + 15) // 16 * 16
    # outside the domain: sizes are 0, calls refuse before anything is enqueued
    assert L.lcm_resize_table_bytes(8193, 64, 64) == 0 and L.lcm_resize_table_bytes(64, 4097, 64) == 0
    assert L.lcm_resize_ws_bytes(2, 64, 64, 32, 32, 0, 0, 32, 32) == 0 and L.lcm_resize_ws_bytes(3, 8193, 64, 32, 32, 0, 0, 32, 32) == 0
    assert L.lcm_resize_tables(8193, 64, 0, 64, buf.ctypes.data, 1 << 20) == -1 and b"8192" in L.lcm_last_error()
    assert L.lcm_resize_tables(300, 96, 0, 64, buf.ctypes.data, 16) == -1 and b"needed" in L.lcm_last_error()
    p = C.c_void_p(buf.ctypes.data)
    assert L.lcm_resize_lanczos_u8(None, 0, 3, 8, 8, 4, 4, 0, 0, 4, 4, p, 12, p, 64, None) == -1 and b"null" in L.lcm_last_error()
    assert L.lcm_resize_lanczos_u8(p, 24, 2, 8, 8, 4, 4, 0, 0, 4, 4, p, 12, p, 64, None) == -1 and b"channels" in L.lcm_last_error()
    assert L.lcm_resize_lanczos_u8(p, 23, 3, 8, 8, 4, 4, 0, 0, 4, 4, p, 12, p, 1 << 20, None) == -1 and b"stride" in L.lcm_last_error()
    assert L.lcm_resize_lanczos_u8(p, 24, 3, 8, 8, 4, 4, 0, 0, 4, 4, p, 12, p, 16, None) == -1 and b"workspace" in L.lcm_last_error()


# ---- backends/fit.py -----------------------------------------------------------------------------------------------------------
@dataclass
class _Req:
    prompt: str = "p"
    size: str = "64x64"
    num_inference_steps: int = 2
    guidance_scale: float = 1.0
    seed: Optional[int] = 1
    style_lora: Optional[object] = None
    init_image: Optional[object] = None
    denoising_strength: Optional[float] = None
    mask: Optional[object] = None
    resize_mode: Optional[object] = None


def test_resize_mode_parsing_and_errors():
    from sdlcm_amd.backends import fit

    class _Bare:
        pass
    assert fit.parse_resize_mode(_Bare()) == 0
    for v, want in ((None, 0), (0, 0), (1, 1), (2, 2), (1.0, 1), (np.int64(2), 2)):
        assert fit.parse_resize_mode(_Req(resize_mode=v)) == want
    with pytest.raises(RuntimeError, match=r"Invalid resize_mode 3: the latent upscale is not served; this worker serves 0 \(just resize\), "
                                          r"1 \(crop and resize\), 2 \(resize and fill\)"):
        fit.parse_resize_mode(_Req(resize_mode=3))
    for bad in (4, -1, 1.5, "1", True, b"2", float("nan"), [1]):
        with pytest.raises(RuntimeError, match=r"Invalid resize_mode .*0 \(just resize\), 1 \(crop and resize\), 2 \(resize and fill\)") as e:
            fit.parse_resize_mode(_Req(resize_mode=bad))
        assert repr(bad) in str(e.value)


@pytest.mark.parametrize("src,size", [((300, 200), (64, 64)), ((100, 50), (64, 64)), ((50, 100), (64, 64)), ((200, 300), (96, 48)),
                                      ((77, 31), (40, 72)), ((64, 64), (32, 32)), ((1000, 40), (64, 64))])
def test_mode_geometry_against_pil_crop_and_edge_pad(src, size):
    from sdlcm_amd.backends import fit
    (sw, sh), (W, H) = src, size
    for a in (picture(sw, sh, 3, "noise", 5), picture(sw, sh, 1, "bw", 6)):
        tail = ((0, 0),) * (a.ndim - 2)
        # mode 1, as A1111 writes it: resize so that the request is covered, keep the centred window
        r, rs = W / H, sw / sh
        fw, fh = (W if r > rs else sw * H // sh), (H if r <= rs else sh * W // sw)
        res = pil_resize(a, fw, fh)
        want1 = res[fh // 2 - H // 2:fh // 2 - H // 2 + H, fw // 2 - W // 2:fw // 2 - W // 2 + W]
        assert want1.shape[:2] == (H, W)
        assert fit.geometry(1, sw, sh, W, H) == R.mode_geometry(1, sw, sh, W, H) == (fw, fh, fw // 2 - W // 2, fh // 2 - H // 2)
        assert np.array_equal(fit.fit_host(a, W, H, 1), want1) and np.array_equal(R.fit(a, W, H, 1), want1)
        # mode 2: resize so that the picture fits inside, centre it, replicate its edge rows / columns into the bands
        fw, fh = (W if r < rs else sw * H // sh), (H if r >= rs else sh * W // sw)
        res = pil_resize(a, fw, fh)
        px, py = W // 2 - fw // 2, H // 2 - fh // 2
        want2 = np.pad(res, ((py, H - fh - py), (px, W - fw - px)) + tail, mode="edge")
        assert fit.geometry(2, sw, sh, W, H) == R.mode_geometry(2, sw, sh, W, H) == (fw, fh, -px, -py)
        assert np.array_equal(fit.fit_host(a, W, H, 2), want2) and np.array_equal(R.fit(a, W, H, 2), want2)
        # mode 0 is the stretch the fit_* helpers do
        assert np.array_equal(fit.fit_host(a, W, H, 0), pil_resize(a, W, H)) and np.array_equal(R.fit(a, W, H, 0), pil_resize(a, W, H))
    # a fit that A1111's integer division would round to nothing keeps one row
    assert fit.geometry(2, 1000, 8, 64, 64) == (64, 1, 0, -32) and fit.geometry(1, 8, 1000, 64, 64)[:2] == (64, 8000)
    same = picture(W, H, 3, "noise")
    for mode in (0, 1, 2):
        assert fit.fit_host(same, W, H, mode) is same and fit.prepare(same, W, H, mode) is same


def test_domain_rule_and_backend_switch(monkeypatch):
    from sdlcm_amd.backends import fit, img2img
    assert fit.in_domain(3, 300, 3, 8, 16) and not fit.in_domain(3, 301, 3, 8, 16)
    assert R.in_domain(3, 300, 3, 8, 16) and not R.in_domain(3, 301, 3, 8, 16)
    assert fit.in_domain(8192, 8192, 1, 4096, 4096) and not fit.in_domain(8193, 64, 3, 64, 64) and not fit.in_domain(64, 64, 3, 4097, 64)
    assert not fit.in_domain(64, 64, 4, 32, 32)
    a = picture(100, 80, 3, "noise")
    monkeypatch.setenv("LCM_RESIZE", "hip")
    p = fit.prepare(a, 64, 64, 1)
    assert fit.is_pending(p) and (p.fit_w, p.fit_h, p.x0, p.y0) == (80, 64, 8, 0) and p.shape == (64, 64, 3) and p.dtype == np.uint8
    assert fit.is_pending(fit.prepare(picture(3, 300, 1, "noise"), 8, 16)) and fit.prepare(picture(3, 300, 1, "noise"), 8, 16).shape == (16, 8)
    out = fit.prepare(picture(3, 301, 3, "noise"), 8, 16)                      # outside the domain: the host's fit, silently
    assert isinstance(out, np.ndarray) and np.array_equal(out, pil_resize(picture(3, 301, 3, "noise"), 8, 16))
    assert isinstance(fit.stack([a[:64, :64], p]), list) and fit.stack([a[:64, :64], a[:64, :64]]).shape == (2, 64, 64, 3)
    monkeypatch.setenv("LCM_RESIZE", "pil")
    calls = []
    out = fit.prepare(a, 64, 64, 0, lambda *args: (calls.append(args[1:]), img2img.fit_init(*args))[1])
    assert calls == [(64, 64)] and np.array_equal(out, pil_resize(a, 64, 64))       # today's helper, today's bytes
    assert np.array_equal(fit.prepare(a, 64, 64, 2), fit.fit_host(a, 64, 64, 2))
    monkeypatch.setenv("LCM_RESIZE", "cuda")
    with pytest.raises(RuntimeError, match="LCM_RESIZE"):
        fit.prepare(a, 64, 64)


def test_job_key_ignores_the_mode_and_requests_without_a_picture():
    from sdlcm_amd.backends.hip_worker import HipLcmWorker
    pic = picture(100, 80, 3, "noise")
    plain = HipLcmWorker._job_key(_Req())
    assert HipLcmWorker._job_key(_Req(resize_mode=3)) == plain == HipLcmWorker._job_key(_Req(resize_mode="junk"))   # no picture: not read
    i2i = HipLcmWorker._job_key(_Req(init_image=pic, denoising_strength=0.5))
    for mode in (None, 0, 1, 2):
        assert HipLcmWorker._job_key(_Req(init_image=pic, denoising_strength=0.5, resize_mode=mode)) == i2i
    inp = HipLcmWorker._job_key(_Req(init_image=pic, denoising_strength=0.5, mask=pic[..., 0]))
    assert HipLcmWorker._job_key(_Req(init_image=pic, denoising_strength=0.5, mask=pic[..., 0], resize_mode=2)) == inp != i2i
    with pytest.raises(RuntimeError, match="Invalid resize_mode 3"):
        HipLcmWorker._job_key(_Req(init_image=pic, denoising_strength=0.5, resize_mode=3))
    with pytest.raises(RuntimeError, match="Invalid resize_mode 7"):
        HipLcmWorker._job_key(_Req(init_image=pic, denoising_strength=0.5, mask=pic[..., 0], resize_mode=7))
