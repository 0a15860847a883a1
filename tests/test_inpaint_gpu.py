"""Inpainting on the GPU.  The mask path is integer arithmetic and the step is a select between two existing expressions, so
every kernel test here compares for EQUALITY: the mask launches against the numpy restatement of tests/inpaint_reference.py, the
masked step against lcm_scheduler_step_ex / lcm_latents_renoise themselves, the overlay against numpy.  Then the chain (eager,
captured, replayed, solo, against image-to-image, against the CPU chain), its launch count, one audited eager run, and the worker."""
import base64
import ctypes as C
import io
import os
import sys
import threading
from dataclasses import dataclass, field
from typing import Optional

import numpy as np
import pytest
import torch

import inpaint_reference as ir
import launch_audit as la
import refine_reference as rr
import vae_encoder_reference as ver

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
    init_image: Optional[object] = None
    init_images: Optional[object] = None
    denoising_strength: Optional[float] = None
    mask: Optional[object] = None
    mask_image: Optional[object] = None
    mask_blur: Optional[float] = None
    inpainting_mask_invert: Optional[object] = None
    inpainting_fill: Optional[object] = None
    inpaint_full_res: Optional[object] = None
    enable_hr: Optional[bool] = None
    denoise_strength: Optional[float] = None
    pass_number: Optional[int] = None
    controlnet_image: Optional[object] = None


@dataclass
class _Job:
    req: _Req


def _pic(h=64, w=64, seed=0):
    """A smooth picture with some texture (seeded), uint8 [h, w, 3]."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([128 + 100 * np.sin(x / 7.0 + seed), 128 + 100 * np.cos(y / 5.0), 128 + 90 * np.sin((x + y) / 9.0)], -1)
    return np.clip(base + rng.normal(0, 12, (h, w, 3)), 0, 255).astype(np.uint8)


def _png(arr):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(arr).save(b, "PNG")
    return b.getvalue()


def _png_rgb(png):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(png)).convert("RGB"))


def _weights_dev(sigma):
    from sdlcm_amd.pipeline import mask_blur_weights
    r, w = mask_blur_weights(sigma)
    return r, (torch.from_numpy(w.astype(np.int64)).to(torch.int32).to(DEV) if r > 0 else None)


# ---------------------------------------------------------------------------------------------------------------------------
# the mask on the device
# ---------------------------------------------------------------------------------------------------------------------------
MASK_KINDS = ("binary", "gray", "zeros", "ones", "pixel", "edge", "half-blocks")


def _masks(kind, B, H, W, seed=0):
    rng = np.random.default_rng(seed)
    m = np.zeros((B, H, W), np.uint8)
    if kind == "binary":
        m = (rng.random((B, H, W)) < 0.5).astype(np.uint8) * 255
    elif kind == "gray":
        m = rng.integers(0, 256, (B, H, W), dtype=np.uint8)
    elif kind == "ones":
        m[:] = 255
    elif kind == "pixel":
        for b in range(B):
            m[b, (b * 5) % H, (W - 1 - b * 3) % W] = 255           # b = 0: the last column of the first row
    elif kind == "edge":
        m[:, :, 4:] = 255                                         # a vertical edge at x = 4: not block-aligned
    elif kind == "half-blocks":                                   # every 8 x 8 block has exactly 32 of its 64 pixels white
        y, x = np.mgrid[0:H, 0:W]
        pats = [(y % 8) < 4, (x % 8) >= 4, ((x + y) % 2) == 0]
        for b in range(B):
            m[b] = pats[b % 3].astype(np.uint8) * 255
    return m


def _prepare(m, sigma, want_latmask=True):
    """-> (alpha, latent mask | None, launches) of ops.inpaint_mask_prepare, with one guard image behind every output."""
    from sdlcm_amd import ops
    B, H, W = m.shape
    r, wts = _weights_dev(sigma)
    dm = torch.from_numpy(m).to(DEV)
    alpha = torch.full((B + 1, H, W), 77, dtype=torch.uint8, device=DEV)
    tmp = torch.full((B + 1, H, W), 78, dtype=torch.uint8, device=DEV)
    lm = torch.full((B + 1, H // 8, W // 8), 79, dtype=torch.uint8, device=DEV) if want_latmask else None
    n = ops.inpaint_mask_prepare(dm, wts, r, alpha, tmp, lm, B, H, W)
    torch.cuda.synchronize()
    assert torch.equal(dm.cpu(), torch.from_numpy(m)), "the mask was written"
    assert bool((alpha[B] == 77).all()) and bool((tmp[B] == 78).all()), "a plane was written past its B images"
    if lm is not None:
        assert bool((lm[B] == 79).all()), "the latent mask was written past its B images"
    return alpha[:B].cpu().numpy(), (lm[:B].cpu().numpy() if lm is not None else None), n


@pytest.mark.parametrize("sigma", [0, 1, 4, 12])                   # 12: r = 30 exceeds an 8-pixel side
@pytest.mark.parametrize("H,W", [(8, 8), (16, 24), (72, 88)])
@pytest.mark.parametrize("B", [1, 3])
def test_mask_prepare_bit_exact(B, H, W, sigma):
    assert ir.blur_radius(12) == 30
    for kind in MASK_KINDS:
        m = _masks(kind, B, H, W, seed=H + W + B)
        alpha, M, n = _prepare(m, sigma)
        want = ir.blur(m, sigma)
        assert n == (1 if sigma == 0 else 3)                      # at most three launches; no blur launch without a blur
        assert np.array_equal(alpha, want), (kind, int((alpha != want).sum()))
        assert np.array_equal(M, ir.latent_mask(want)), kind
        if sigma == 0:
            assert np.array_equal(alpha, m)
            if kind == "half-blocks":                             # block sum 8160 = the tie: M = 1
                assert int(m[0, :8, :8].astype(np.int64).sum()) == 8160 and bool((M == 1).all())
            if kind == "edge":                                    # the first block column is half white by columns 4..7: the tie again
                assert bool((M == 1).all())
        if kind == "zeros":
            assert not alpha.any() and not M.any()
        if kind == "ones":
            assert bool((alpha == 255).all()) and bool((M == 1).all())


@pytest.mark.parametrize("sigma", [1, 12, 32])
@pytest.mark.parametrize("H,W", [(1, 1), (9, 11), (37, 301)])      # any size for alpha alone; 301: two tiles of the row pass
def test_alpha_alone_at_any_size(H, W, sigma):
    for kind in ("gray", "pixel"):
        m = _masks(kind, 2, H, W, seed=H)
        alpha, M, n = _prepare(m, sigma, want_latmask=False)
        assert M is None and n == 2
        assert np.array_equal(alpha, ir.blur(m, sigma)), kind


# ---------------------------------------------------------------------------------------------------------------------------
# the masked step against the existing kernels
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("last", [0, 1])
@pytest.mark.parametrize("pred", ["epsilon", "v_prediction", "sample"])
@pytest.mark.parametrize("cfg,dup", [(False, False), (True, True), (True, False)])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("h,w", [(8, 8), (9, 11)])
def test_step_bit_exact_against_the_existing_kernels(h, w, B, cfg, dup, pred, last):
    from sdlcm_amd import ops
    from sdlcm_amd.scheduler import LCMSchedule
    s = LCMSchedule()
    ts = s.timesteps(2, 0.5)
    coef, is_last = s.step_coefficients(ts, 1 if last else 0)
    assert bool(is_last) == bool(last)
    ksa, ksb = s.renoise_coefficients(ts[1])
    g = torch.Generator().manual_seed(100 * h + 10 * B + int(cfg) + 2 * last)
    UB = 2 * B if cfg else B
    eps = torch.randn(UB, h, w, 4, generator=g).to(DEV)
    lat0 = torch.randn(UB + 1, 4, h, w, generator=g).to(DEV)       # one image more: must stay untouched
    noise, z, e1 = (torch.randn(B, 4, h, w, generator=g).to(DEV) for _ in range(3))
    kw = dict(eps_uncond=eps[:B], guidance=7.5) if cfg else {}
    e, off = (eps[B:], B) if cfg else (eps, 0)
    # the two sides of the select, from the kernels that define them
    stepped = lat0.clone()
    ops.scheduler_step(e, stepped[off:], noise, coef, last, B, h, w, pred=pred, **kw)
    kept = z.clone()
    if not last:
        ops.latents_renoise(z, e1, ksa, ksb, kept, B, h, w)
    rnd = (torch.rand(B, h, w, generator=g) < 0.5).to(torch.uint8)
    rnd[0, 0, 0], rnd[0, 0, 1] = 1, 0
    for tag, M in (("ones", torch.ones(B, h, w, dtype=torch.uint8)), ("zeros", torch.zeros(B, h, w, dtype=torch.uint8)), ("random", rnd)):
        lat = lat0.clone()
        ops.scheduler_step_inpaint(e, lat[off:], None if last else noise, z, None if last else e1, M.to(DEV), coef, last, ksa, ksb,
                                   B, h, w, pred=pred, dup=dup, **kw)
        torch.cuda.synchronize()
        sel = M.to(DEV).bool()[:, None].expand(B, 4, h, w)
        want = torch.where(sel, stepped[off:off + B], kept)
        assert la.same_bits(lat[off:off + B], want), tag
        if tag == "ones":
            assert la.same_bits(lat[off:off + B], stepped[off:off + B])
        if tag == "zeros":
            assert la.same_bits(lat[off:off + B], kept) and (not last or la.same_bits(kept, z))
        assert la.same_bits(lat[UB], lat0[UB]), "the image behind the state was written"
        if cfg:                                                   # dup: the other half gets the same values; else it is left alone
            assert la.same_bits(lat[:B], want if dup else lat0[:B]), tag


# ---------------------------------------------------------------------------------------------------------------------------
# the overlay
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,W", [(8, 8), (9, 11), (64, 64)])
def test_composite_exact(H, W, B):
    from sdlcm_amd import ops
    rng = np.random.default_rng(H * W + B)
    gen = rng.integers(0, 256, (B + 1, H, W, 3), dtype=np.uint8)
    init = rng.integers(0, 256, (B + 1, H, W, 3), dtype=np.uint8)
    alpha = rng.integers(0, 256, (B + 1, H, W), dtype=np.uint8)
    alpha[:, 0], alpha[:, H - 1] = 0, 255                          # a row of 0 and a row of 255
    alpha[:, H // 2, : W // 2] = 1
    alpha[:, H // 2, W // 2:] = 254
    d_gen, d_init, d_alpha = (torch.from_numpy(a).to(DEV) for a in (gen, init, alpha))
    ops.inpaint_composite_rgb8(d_gen, d_init, d_alpha, B, H, W)
    torch.cuda.synchronize()
    got = d_gen.cpu().numpy()
    assert np.array_equal(got[:B], ir.composite(gen[:B], init[:B], alpha[:B]))
    assert np.array_equal(got[:B, 0], init[:B, 0]) and np.array_equal(got[:B, H - 1], gen[:B, H - 1])
    assert np.array_equal(got[B], gen[B]), "the image behind the batch was written"
    assert np.array_equal(d_init.cpu().numpy(), init) and np.array_equal(d_alpha.cpu().numpy(), alpha)


def test_bad_arguments_return_an_error_and_enqueue_nothing():
    from sdlcm_amd import lib, ops
    from sdlcm_amd.lib import LcmHipError
    from sdlcm_amd.scheduler import LCMSchedule
    L = lib.load()
    H = W = 16
    m = torch.full((1, H, W), 200, dtype=torch.uint8, device=DEV)
    alpha, tmp = torch.full_like(m, 1), torch.full_like(m, 2)
    lm = torch.full((1, 2, 2), 3, dtype=torch.uint8, device=DEV)
    r, wts = _weights_dev(4)
    big = torch.zeros(200, dtype=torch.int32, device=DEV)
    for args, text in (((m, big, 81, alpha, tmp, lm, 1, H, W), "radius"), ((m, wts, -1, alpha, tmp, lm, 1, H, W), "radius"),
                       ((m, None, r, alpha, tmp, lm, 1, H, W), "weights"), ((m, wts, r, alpha, None, lm, 1, H, W), "scratch"),
                       ((m, wts, r, alpha, alpha, lm, 1, H, W), "aliases"), ((m, wts, r, alpha, m, lm, 1, H, W), "aliases"),
                       ((m, wts, r, alpha, tmp, lm, 1, 12, W), "divisible by 8"), ((m, wts, r, alpha, tmp, lm, 1, H, 20), "divisible by 8"),
                       ((m, wts, r, alpha, tmp, lm, 0, H, W), "bad shape"), ((m, wts, r, alpha, tmp, lm, 1, H, 0), "bad shape"),
                       ((None, wts, r, alpha, tmp, lm, 1, H, W), "null"), ((m, wts, r, None, tmp, lm, 1, H, W), "null"),
                       ((m.reshape(-1)[1:], wts, r, alpha, tmp, None, 1, 3, 5), "aligned")):
        with pytest.raises(LcmHipError, match=text):
            ops.inpaint_mask_prepare(*args)
    # the masked step
    s = LCMSchedule()
    coef, _ = s.step_coefficients(s.timesteps(2, 0.5), 0)
    h = w = 4
    eps, lat, noise, z, e1 = (torch.full((1, 4, h, w), float(i), device=DEV) for i in range(5))
    M = torch.ones(1, h, w, dtype=torch.uint8, device=DEV)
    for kwargs, text in ((dict(B=0), "bad shape"), (dict(w=0), "bad shape"), (dict(noise=None), "null"), (dict(e1=None), "null"),
                         (dict(z=None), "null"), (dict(latmask=None), "null"), (dict(eps=eps.reshape(-1)[1:]), "16-byte")):
        a = dict(eps=eps, lat=lat, noise=noise, z=z, e1=e1, latmask=M, coef6=coef, last=0, next_sqrt_a=0.5, next_sqrt_b=0.5, B=1, h=h, w=w)
        a.update(kwargs)
        with pytest.raises(LcmHipError, match=text):
            ops.scheduler_step_inpaint(**a)
    with pytest.raises(ValueError, match="unknown prediction type"):
        ops.scheduler_step_inpaint(eps, lat, noise, z, e1, M, coef, 0, 0.5, 0.5, 1, h, w, pred="flow")
    arr = (C.c_float * 6)(*coef)
    p = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.lcm_scheduler_step_inpaint(p(eps), None, 1.0, p(lat), p(noise), p(z), p(e1), p(M), arr, 0, 0.5, 0.5, 7, 1, h, w, 0, st) != 0
    assert b"unknown prediction type 7" in L.lcm_last_error()
    # the overlay
    rgb, init = torch.full((1, H, W, 3), 9, dtype=torch.uint8, device=DEV), torch.full((1, H, W, 3), 10, dtype=torch.uint8, device=DEV)
    a8 = torch.full((1, H, W), 128, dtype=torch.uint8, device=DEV)
    for args, text in (((rgb, init, a8, 0, H, W), "bad shape"), ((rgb, init, a8, 1, H, -1), "bad shape"), ((rgb, None, a8, 1, H, W), "null"),
                       ((rgb, rgb, a8, 1, H, W), "aliases"), ((rgb.reshape(-1)[1:], init, a8, 1, 4, 4), "aligned"),
                       ((rgb, init, a8.reshape(-1)[8:], 1, 4, 4), "aligned")):
        with pytest.raises(LcmHipError, match=text):
            ops.inpaint_composite_rgb8(*args)
    torch.cuda.synchronize()
    # nothing was enqueued: every buffer a call could have written is as it was
    assert bool((alpha == 1).all()) and bool((tmp == 2).all()) and bool((lm == 3).all()) and bool((m == 200).all())
    assert bool((lat == 1.0).all()) and bool((rgb == 9).all())


# ---------------------------------------------------------------------------------------------------------------------------
# the chain
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def enc_sd():
    from sdlcm_amd import weights
    return weights.synthetic_vae_encoder()


@pytest.fixture(scope="module")
def state(enc_sd):
    from sdlcm_amd import weights
    from sdlcm_amd.pipeline import LcmHipPipeline
    usd, vsd = weights.synthetic_unet(), weights.synthetic_vae()
    hip = LcmHipPipeline(usd, vsd, device=DEV)
    hip.set_vae_encoder_source(enc_sd)
    yield dict(hip=hip, ora=rr.RefineChainOracle(usd, vsd))
    hip.close()


def _embeds(B, seed=5):
    return torch.randn(B, 77, 768, generator=torch.Generator().manual_seed(seed)).to(torch.float16)


SEEDS = [9300, 9301]


def _inputs():
    pics = np.stack([_pic(64, 64, 51), _pic(64, 64, 52)])
    half = np.zeros((2, 64, 64), np.uint8)
    half[0, :, 28:] = 255                                          # the right part, the edge inside a latent cell
    half[1, 36:, :] = 255                                          # the lower part
    return _embeds(2, seed=43), pics, half


@pytest.fixture(scope="module")
def half_plane(state):
    """The half-plane masks with blur 4 at 64 x 64, 2 steps, strength 0.5, B = 2: one eager run, shared."""
    pe, pics, half = _inputs()
    return state["hip"].generate_inpaint(pe, SEEDS, pics, half, 64, 64, 2, 0.5, mask_blur=4, want_float=True)


def test_chain_eager_captured_replayed_and_solo(state, half_plane):
    hip = state["hip"]
    pe, pics, half = _inputs()
    eager = half_plane
    assert eager["unet_evals"] == 2 and eager["rgb"].shape == (2, 64, 64, 3) and eager["init_latents"].shape == (2, 4, 8, 8)
    assert eager["alpha"].shape == (2, 64, 64) and eager["latent_mask"].shape == (2, 8, 8)
    cap = hip.generate_inpaint(pe, SEEDS, pics, half, 64, 64, 2, 0.5, mask_blur=4)
    rep = hip.generate_inpaint(pe, SEEDS, pics, half, 64, 64, 2, 0.5, mask_blur=4)        # replays both graphs
    for o in (cap, rep):
        for k in ("rgb", "latents", "pool8", "init_latents", "alpha", "latent_mask"):
            assert np.array_equal(o[k], eager[k]), k
    kinds = {P.kind for P in hip.lanes[0].plans.values() if P.graph is not None}
    assert "inpaint" in kinds
    solo = hip.generate_inpaint(pe[1:], SEEDS[1:], pics[1:], half[1:], 64, 64, 2, 0.5, mask_blur=4)
    for k in ("rgb", "latents", "pool8", "init_latents", "alpha", "latent_mask"):
        assert np.array_equal(solo[k][0], rep[k][1]), k


def test_half_plane_mask_keeps_what_it_must(half_plane):
    _, pics, half = _inputs()
    out = half_plane
    alpha = ir.blur(half, 4)
    M = ir.latent_mask(alpha)
    assert np.array_equal(out["alpha"], alpha) and np.array_equal(out["latent_mask"], M)
    assert 0 < M.sum() < M.size and (alpha == 0).any() and (alpha == 255).any()
    keep4 = np.broadcast_to((M == 0)[:, None], out["latents"].shape)
    assert np.array_equal(out["latents"][keep4].view(np.int32), out["init_latents"][keep4].view(np.int32))
    assert (out["latents"][~keep4] != out["init_latents"][~keep4]).any()
    assert np.array_equal(out["rgb"][alpha == 0], pics[alpha == 0])
    assert (out["rgb"][alpha == 255] != pics[alpha == 255]).any()


def test_all_white_is_image_to_image_and_all_black_is_the_picture(state):
    hip = state["hip"]
    pe, pics, _ = _inputs()
    white, black = np.full((2, 64, 64), 255, np.uint8), np.zeros((2, 64, 64), np.uint8)
    i2i = hip.generate_img2img(pe, SEEDS, pics, 64, 64, 2, 0.5)
    w = hip.generate_inpaint(pe, SEEDS, pics, white, 64, 64, 2, 0.5, mask_blur=0)
    for k in ("latents", "pool8", "rgb", "init_latents"):
        assert np.array_equal(w[k], i2i[k]), k
    assert bool((w["alpha"] == 255).all()) and bool((w["latent_mask"] == 1).all())
    for blur in (0, 4):
        b = hip.generate_inpaint(pe, SEEDS, pics, black, 64, 64, 2, 0.5, mask_blur=blur)
        assert np.array_equal(b["rgb"], pics)
        assert np.array_equal(b["latents"].view(np.int32), b["init_latents"].view(np.int32))
        assert np.array_equal(b["init_latents"], i2i["init_latents"])
    # image-to-image itself is as it was before any inpaint request ran
    again = hip.generate_img2img(pe, SEEDS, pics, 64, 64, 2, 0.5)
    for k in ("latents", "pool8", "rgb"):
        assert np.array_equal(again[k], i2i[k]), k


def test_chain_against_the_cpu_chain(state, enc_sd, half_plane):
    ora = state["ora"]
    pe, pics, half = _inputs()
    M = ir.latent_mask(ir.blur(half, 4))
    assert np.array_equal(half_plane["latent_mask"], M)              # integer path: both sides select the same cells
    for b in range(2):
        ref = ir.cpu_chain(ora, enc_sd, pe[b:b + 1].float(), pics[b], M[b], 2, 0.5, SEEDS[b])
        a = np.clip(half_plane["image"][b:b + 1].transpose(0, 3, 1, 2) / 2 + 0.5, 0, 1)
        e = float(np.abs(a - np.clip(ref["image"] / 2 + 0.5, 0, 1)).max())
        dl = float(np.abs(half_plane["latents"][b] - ref["latents"][0]).max())
        print(f"[inpaint] 64x64 steps 2 strength 0.5 blur 4 request {b}: pre-overlay image[0,1] max|d| = {e:.4g}, latents max|d| = {dl:.3g}")
        assert e < 1e-2


def test_launch_count_is_image_to_images_plus_at_most_four(state, monkeypatch):
    """The masked step replaces the step launch one for one; the request adds the mask launches (at most three) and the overlay."""
    from sdlcm_amd import ops
    hip = state["hip"]
    pe, pics, half = _inputs()
    calls = {}

    def count(name):
        real = getattr(ops, name)

        def f(*a, **kw):
            r = real(*a, **kw)
            calls[name] = calls.get(name, 0) + (r if name == "inpaint_mask_prepare" else 1)
            return r
        monkeypatch.setattr(ops, name, f)
    for name in ("scheduler_step", "scheduler_step_inpaint", "inpaint_mask_prepare", "inpaint_composite_rgb8", "latents_renoise",
                 "vae_posterior_renoise", "scheduler_step_handover"):
        count(name)
    with ops.recording() as r_i2i:
        hip.generate_img2img(pe, SEEDS, pics, 64, 64, 2, 0.5, want_float=True)
    c_i2i, calls = calls, {}
    with ops.recording() as r_inp:
        hip.generate_inpaint(pe, SEEDS, pics, half, 64, 64, 2, 0.5, mask_blur=4, want_float=True)
    c_inp = calls
    assert c_i2i == dict(scheduler_step=2, vae_posterior_renoise=1)
    assert c_inp == dict(scheduler_step_inpaint=2, vae_posterior_renoise=1, inpaint_mask_prepare=3, inpaint_composite_rgb8=1)
    # everything else the two requests launch is recorded launch for launch: the new wrappers account for the whole difference
    new = c_inp["scheduler_step_inpaint"] + c_inp["inpaint_mask_prepare"] + c_inp["inpaint_composite_rgb8"]
    assert len(r_inp) - len(r_i2i) == new
    assert new - c_i2i["scheduler_step"] <= 4


def test_new_launches_audited_inside_a_real_chain(state, monkeypatch):
    """tests/launch_audit.py's hook, extended by the three new entry points (and the three of image-to-image's front stage): one
    eager chain at an odd latent size runs under the audit; the mask launches and the overlay are compared with numpy for
    equality, the masked step with the existing step and re-noise kernels for equality; what a launch must not write stays
    unchanged; every other launch passes as in any audited pass."""
    hip = state["hip"]
    monkeypatch.setitem(la.CHECKED, "vae_posterior_renoise", ("z_out", "lat", "moments"))
    monkeypatch.setitem(la.CHECKED, "vae_enc_conv_in_u8", ("out",))
    monkeypatch.setitem(la.CHECKED, "conv3x3_down", ("out",))
    monkeypatch.setitem(la.CHECKED, "inpaint_mask_prepare", ("alpha_out", "scratch", "latmask_out"))
    monkeypatch.setitem(la.CHECKED, "scheduler_step_inpaint", ("lat",))
    monkeypatch.setitem(la.CHECKED, "inpaint_composite_rgb8", ("rgb",))
    exact = lambda ok: (0.0 if ok else float("inf"), None)

    class Audit(la.Audit):
        def _ref_vae_posterior_renoise(self, B, A, r):
            n, h, w, dup = A["B"], A["h"], A["w"], A["dup"]
            assert la.tail_same(A["lat"], B["lat"], (2 if dup else 1) * n * 4 * h * w) and la.tail_same(A["z_out"], B["z_out"], n * 4 * h * w)
            ref = ver.posterior_reference(B["pre_mean"][:n].cpu(), B["pre_logvar"][:n].cpu(), B["quant_w"].cpu(), B["quant_b"].cpu(),
                                          B["e0"][:n].cpu(), B["e1"][:n].cpu(), A["scaling"], A["sqrt_a"], A["sqrt_b"])
            return ver.posterior_check(A["z_out"], A["lat"], ref, n, dup, got_moments=A["moments"]), None

        def _ref_vae_enc_conv_in_u8(self, B, A, r):
            return ver.conv_in_check(A["out"], B["img_u8"], B["w"], B["bias"], A["B"], A["H"], A["W"]), None

        def _ref_conv3x3_down(self, B, A, r):
            n, H, W = A["B"], A["H"], A["W"]
            rows = n * ver.down_size(H) * ver.down_size(W)
            assert la.tail_same(A["out"], B["out"], rows * A["Cout"])
            ref, bnd = ver.down_reference(B["x"], B["w"], B["bias"], n, H, W)
            return la.worst_ratio(A["out"][:rows], ref, bnd), None

        def _ref_inpaint_mask_prepare(self, B, A, r):
            m = B["mask_u8"].cpu().numpy()
            w = B["weights_u32"].cpu().numpy().astype(np.int64)
            assert len(w) == 2 * A["radius"] + 1 and w.sum() == 65536 and r == 3
            t = ir.blur_pass(m, w, axis=2)
            alpha = ir.blur_pass(t, w, axis=1)
            return exact(np.array_equal(A["scratch"].cpu().numpy(), t) and np.array_equal(A["alpha_out"].cpu().numpy(), alpha)
                         and np.array_equal(A["latmask_out"].cpu().numpy(), ir.latent_mask(alpha)))

        def _ref_scheduler_step_inpaint(self, B, A, r):
            n, h, w, last = A["B"], A["h"], A["w"], A["last"]
            stepped = B["lat"].clone()
            self._saved["scheduler_step"](B["eps"], stepped, B["noise"], A["coef6"], last, n, h, w, pred=A["pred"])
            kept = B["z"].clone()
            if not last:
                self._saved["latents_renoise"](B["z"], B["e1"], A["next_sqrt_a"], A["next_sqrt_b"], kept, n, h, w)
            torch.cuda.current_stream().synchronize()
            sel = B["latmask"].bool()[:, None].expand(n, 4, h, w)
            return exact(la.same_bits(A["lat"], torch.where(sel, stepped, kept)))

        def _ref_inpaint_composite_rgb8(self, B, A, r):
            want = ir.composite(B["rgb"].cpu().numpy(), B["init_u8"].cpu().numpy(), B["alpha_u8"].cpu().numpy())
            return exact(np.array_equal(A["rgb"].cpu().numpy(), want))

    plans = hip.lanes[0].plans
    before = set(plans)
    pics = np.stack([_pic(40, 72, 31), _pic(40, 72, 32)])
    masks = np.zeros((2, 40, 72), np.uint8)
    masks[0, 10:30, 20:50] = 255
    masks[1, :, :36] = 200
    with Audit() as au:
        out = hip.generate_inpaint(_embeds(2, seed=77), [601, 602], pics, masks, 72, 40, 2, 0.5, mask_blur=4, want_float=True)
    for k in set(plans) - before:
        plans.pop(k)
    bad = la.failures(au.checks)
    per = la.entry_table(au.checks)
    print(f"[audit] inpaint 72x40 B2: {len(au.checks)} launches checked, {la.summary_line(au.checks)}")
    assert not bad, bad
    assert per["inpaint_mask_prepare"][:2] == [1, 0.0] and per["inpaint_composite_rgb8"][:2] == [1, 0.0]
    assert per["scheduler_step_inpaint"][:2] == [2, 0.0]              # the non-last and the last form
    assert "scheduler_step" not in per and "latents_renoise" not in per
    assert per["vae_posterior_renoise"][0] == 1 and per["vae_posterior_renoise"][1] <= 1.0
    assert all(k[0] == 1 for k in au.record_keys() - au.checked_keys())       # only the down convs are checked outside HOOKED
    assert np.isfinite(out["latents"]).all() and 0 < out["latent_mask"].sum() < out["latent_mask"].size


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


def _wmask(s=0):
    m = np.zeros((64, 64), np.uint8)
    m[12 + s:44 + s, 20:52] = 255
    return m


def _mk(s, **extra):
    kw = dict(init_image=_pic(64, 64, 40 + s), denoising_strength=0.5, mask=_wmask(s))
    kw.update(extra)
    return _Req(prompt=f"inpaint {s}", seed=s, **kw)


def test_run_job_serves_a_mask_in_every_form(worker):
    from PIL import Image
    eng = worker._engine
    plain_req = _Req(prompt="inpaint 3", seed=3)
    i2i_req = _Req(prompt="inpaint 3", seed=3, init_image=_pic(64, 64, 43), denoising_strength=0.5)
    plain_before, i2i_before = worker.run_job(_Job(plain_req)), worker.run_job(_Job(i2i_req))
    n0 = eng.stats["inpaint_requests"], eng.stats["unet_evals"], eng.stats["img2img_requests"]
    png, seed = worker.run_job(_Job(_mk(3)))
    assert seed == 3 and png != plain_before[0] and png != i2i_before[0]
    assert eng.stats["inpaint_requests"] == n0[0] + 1 and eng.stats["unet_evals"] == n0[1] + 2 and eng.stats["img2img_requests"] == n0[2]
    m = _wmask(3)
    mpng = _png(m)
    b64 = base64.b64encode(mpng).decode()
    forms = (dict(mask=mpng), dict(mask=b64), dict(mask="data:image/png;base64," + b64), dict(mask=Image.fromarray(m, "L")),
             dict(mask=m[..., None]), dict(mask=np.repeat(m[..., None], 3, axis=2)),
             dict(mask=np.concatenate([np.repeat(m[..., None], 3, axis=2), np.full((64, 64, 1), 255, np.uint8)], axis=2)),
             dict(mask=None, mask_image=m), dict(mask=None, mask_image=b64))
    for form in forms:
        assert worker.run_job(_Job(_mk(3, **form)))[0] == png, list(form)
    assert worker.run_job(_Job(_mk(3, mask=255 - m, inpainting_mask_invert=True)))[0] == png
    assert worker.run_job(_Job(_mk(3, inpainting_mask_invert=True)))[0] != png
    # the unmasked pixels come back byte for byte: alpha is 0 far from the masked square (blur 4: r = 10)
    got = _png_rgb(png)
    alpha = ir.blur(m[None], 4)[0]
    assert np.array_equal(got[alpha == 0], _pic(64, 64, 43)[alpha == 0]) and (alpha == 0).sum() > 1000
    # another blur, another strength, a mask and a picture of another size (both fitted): all reach the chain
    assert worker.run_job(_Job(_mk(3, mask_blur=0)))[0] != png
    assert worker.run_job(_Job(_mk(3, denoising_strength=0.8)))[0] != png
    assert _png_rgb(worker.run_job(_Job(_mk(3, size="88x72", mask=np.full((10, 10), 255, np.uint8))))[0]).shape == (72, 88, 3)
    # run_job_with_latents: the 8 x 8 pool of the final blended latents
    png2, _, blob = worker.run_job_with_latents(_Job(_mk(3)))
    assert png2 == png and len(blob) == 512 and np.isfinite(np.frombuffer(blob, np.float16).astype(np.float32)).all()
    # plain and image-to-image requests: the same bytes before and after inpaint requests ran
    assert worker.run_job(_Job(plain_req)) == plain_before and worker.run_job(_Job(i2i_req)) == i2i_before


def test_bytes_do_not_depend_on_batch_padding_or_lane(worker):
    from sdlcm_amd.backends.hip_worker import encode_png
    eng = worker._engine
    req = _mk(0)
    key = worker._job_key(req)
    assert key[6:] == ("inpaint", 0.5, 4.0)

    def batch(reqs, lane=0, pick=0):
        return encode_png(eng.run_batch(key, [worker._prepare(r, key) for r in reqs], lane)[pick][0])
    n0 = eng.stats["inpaint_requests"]
    pngs = {"alone": worker.run_job(_Job(req))[0], "batch of 2": batch([req, _mk(1)]),
            "padded third of 4": batch([_mk(1), _mk(2), req], pick=2)}
    assert eng.stats["inpaint_requests"] == n0 + 1 + 2 + 3
    if eng.n_lanes > 1:
        pngs["lane 1"] = batch([req], lane=1)
    for tag, png in pngs.items():
        assert png == pngs["alone"], tag
    item = worker._prepare(req, key)
    assert len(item) == 5 and item[3].shape == (64, 64, 3) and item[4].shape == (64, 64) and item[4].dtype == np.uint8


def _outcome(f):
    try:
        return f.result(600)
    except Exception as e:      # noqa
        return e


def test_errors_reach_the_right_job_inside_a_drained_batch(worker):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from tools import minipool
    bad = {1: (dict(mask=b"\x89PNG not a picture"), "Invalid mask"), 2: (dict(inpainting_fill=2), "inpainting_fill 2"),
           3: (dict(inpaint_full_res=True), "inpaint_full_res"), 4: (dict(enable_hr=True), "not combined"),
           5: (dict(mask_blur=40), "mask_blur"), 6: (dict(init_image=None), "without init_image")}
    solo = {s: worker.run_job(_Job(_mk(s))) for s in range(8) if s not in bad}
    pool = minipool.MiniPool(lambda worker_id: worker, {"m": "synthetic"}, "m")
    worker.bind_queue(pool.q)
    gate, inside = threading.Event(), threading.Event()
    hold = pool.submit_job(minipool.CustomJob(handler=lambda: (inside.set(), gate.wait(30))))
    assert inside.wait(30)
    try:
        futs = [pool.submit_job(minipool.GenerationJob(req=_mk(s, **bad.get(s, ({}, ""))[0]))) for s in range(8)]
        gate.set()
        hold.result(60)
        res = [_outcome(f) for f in futs]
        pool.q.join()
        for s in range(8):
            if s in bad:
                assert isinstance(res[s], RuntimeError) and bad[s][1] in str(res[s]), (s, res[s])
            else:
                assert res[s] == solo[s], s
    finally:
        worker.bind_queue(None)
        pool._worker = None
        pool.shutdown()


def test_the_sdxl_worker_refuses_a_mask():
    from sdlcm_amd.backends.hip_worker import HipLcmSDXLWorker
    with pytest.raises(RuntimeError, match="SDXL"):
        HipLcmSDXLWorker._job_key(_mk(1))
    with pytest.raises(RuntimeError, match="mask: inpainting is not served by the SDXL worker"):
        HipLcmSDXLWorker._job_key(_Req(prompt="x", seed=1, mask_image=_wmask()))
