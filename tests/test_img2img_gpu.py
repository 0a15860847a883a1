"""Image-to-image on the GPU: the three new launches against the float64 references and derived bounds of
tests/vae_encoder_reference.py, the whole encoder and its mid block against the CPU restatement, the chain against the CPU
restatement of the strength-cut pass, the worker's behaviour, and the hand-over launch audited inside a real chain."""
import io
import os
import sys
import threading
from dataclasses import dataclass, field
from typing import Optional

import numpy as np
import pytest
import torch

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


def _png_size(png):
    from PIL import Image
    return Image.open(io.BytesIO(png)).size


@pytest.fixture(scope="module")
def enc_sd():
    from sdlcm_amd import weights
    return weights.synthetic_vae_encoder()


@pytest.fixture(scope="module")
def enc(enc_sd):
    from sdlcm_amd import ops
    from sdlcm_amd.model import VAEEncoderHip
    from sdlcm_amd.pipeline import _default_workspace
    ops.set_workspace(_default_workspace(torch.device(DEV)))
    return VAEEncoderHip(enc_sd, device=DEV)


# ---------------------------------------------------------------------------------------------------------------------------
# the kernels
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,W", [(8, 8), (9, 11), (1, 5)])
def test_conv_in_u8_fp64(enc_sd, B, H, W):
    from sdlcm_amd import ops
    w16 = ver.pack3x3(enc_sd["encoder.conv_in.weight"]).to(DEV)
    b16 = enc_sd["encoder.conv_in.bias"].to(DEV)
    pics = [np.zeros((H, W, 3), np.uint8), np.full((H, W, 3), 255, np.uint8), _pic(H, W, 3), _pic(H, W, 4)]
    img = torch.from_numpy(np.stack(pics[:B] if B > 1 else pics[2:3] if (H, W) == (9, 11) else pics[:1]))
    if B == 1 and (H, W) == (8, 8):
        img = torch.from_numpy(np.stack(pics[1:2]))                       # the all-255 picture alone
    dimg = torch.cat([img, torch.full((1, H, W, 3), 9, dtype=torch.uint8)]).to(DEV)
    out = torch.full(((B + 1) * H * W, 128), -7.0, dtype=torch.float16, device=DEV)     # one image more: must stay untouched
    before = out.clone()
    ops.vae_enc_conv_in_u8(dimg, w16, out, B, H, W, 128, bias=b16)
    torch.cuda.synchronize()
    r = ver.conv_in_check(out, dimg, w16, b16, B, H, W)
    print(f"[img2img] conv_in B={B} {H}x{W}: worst |err| / bound = {r:.3g}")
    assert r <= 1.0
    assert la.tail_same(out, before, B * H * W * 128)
    # border handling decides: padding BEFORE the normalisation (neighbours -1) must fail the bound on a constant picture
    wrong = ver.conv_in_kernel_like(img, w16.cpu(), b16.cpu(), pad_minus_one=True).to(DEV)
    if H > 1:
        assert ver.conv_in_check(wrong, dimg, w16, b16, B, H, W) > 1.0


def _down_case(C, B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B + 1) * H * W, C, generator=g).half()
    w = ver.pack3x3((torch.randn(C, C, 3, 3, generator=g) * (9 * C) ** -0.5).half())
    b = (0.02 * torch.randn(C, generator=g)).half()
    return x.to(DEV), w.to(DEV), b.to(DEV)


def _run_down(x, w, b, B, H, W, C, stats=False):
    from sdlcm_amd import ops
    Ho, Wo = ver.down_size(H), ver.down_size(W)
    out = torch.full(((B + 1) * Ho * Wo, C), -7.0, dtype=torch.float16, device=DEV)    # guard rows beyond the output
    st = None
    if stats:
        st = ops.Stats(torch.zeros(ops.stats_floats(B * Ho * Wo, C, Ho * Wo), dtype=torch.float32, device=DEV))
    ops.conv3x3_down(x, w, out, B, H, W, C, C, bias=b, stats=st)
    torch.cuda.synchronize()
    return out, st


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,W", [(8, 8), (10, 6), (7, 9)])
@pytest.mark.parametrize("C", [128, 256, 512])
def test_conv3x3_down_fp64(enc, C, H, W, B):
    x, w, b = _down_case(C, B, H, W, seed=C + 10 * H + W)
    Ho, Wo = ver.down_size(H), ver.down_size(W)
    out, _ = _run_down(x, w, b, B, H, W, C)
    ref, bnd = ver.down_reference(x, w, b, B, H, W)
    r = la.worst_ratio(out[:B * Ho * Wo], ref, bnd)
    print(f"[img2img] down C={C} B={B} {H}x{W} -> {Ho}x{Wo}: worst |err| / bound = {r:.3g}")
    assert r <= 1.0
    assert bool((out[B * Ho * Wo:] == -7.0).all()), "guard rows beyond the output were written"
    if B == 3:                                                   # the same image alone: the same bits
        solo, _ = _run_down(x[2 * H * W:], w, b, 1, H, W, C)
        assert la.same_bits(solo[:Ho * Wo], out[2 * Ho * Wo:3 * Ho * Wo])


def _down_full_check(C, H, W, B, seed):
    """One down-conv launch of B images checked whole: against float64 under the bound, guard rows, fused statistics against the
    stored output, and the LAST image alone bit-equal (output and statistics slab count).  -> (output rows M, statistics)."""
    x, w, b = _down_case(C, B, H, W, seed=seed)
    Ho, Wo = ver.down_size(H), ver.down_size(W)
    rows = Ho * Wo
    out, st = _run_down(x, w, b, B, H, W, C, stats=True)
    ref, bnd = ver.down_reference(x, w, b, B, H, W)
    r = la.worst_ratio(out[:B * rows], ref, bnd)
    print(f"[img2img] down C={C} B={B} {H}x{W} -> {Ho}x{Wo} (M = {B * rows}): worst |err| / bound = {r:.3g}")
    assert r <= 1.0
    assert bool((out[B * rows:] == -7.0).all()), "guard rows beyond the output were written"
    assert rows % 32 == 0 and st.P == rows // 32
    sr = la.stats_check(st, out[:B * rows], B)
    print(f"[img2img]   fused statistics: worst ratio {sr:.3g}")
    assert sr <= 1.0
    if B > 1:
        solo, st1 = _run_down(x[(B - 1) * H * W:], w, b, 1, H, W, C, stats=True)
        assert la.same_bits(solo[:rows], out[(B - 1) * rows:B * rows]) and st1.P == st.P
        n1 = st.P * C * 2
        assert la.same_bits(st1.buf[:n1], st.buf[(B - 1) * n1:B * n1]), "a request's statistics depend on its batch"
    return B * rows


def test_conv3x3_down_split_k_and_statistics(enc):
    """Shapes whose canonical K partition has parts, picked by asking the library.  (a) the smallest one: split launch + reduce
    on the 64 x 64 tile; (b) 64 x 64 -> 32 x 32 at 128 channels, batch 4: M = 4096 rows, so the SAME partition on the 128 x 128
    tile (what the 64 x 64-latent level of a 512 x 512 request runs).  Alone and inside the batch a request has the same bits;
    the fused statistics (written by the reduce) are those of the stored output."""
    from sdlcm_amd import ops
    cands = [(C, hw) for C in (512, 256, 128) for hw in (64, 32, 16)]
    parts = {(C, hw): ops.canonical_splits(1, (hw // 2) ** 2, C, 9 * C) for C, hw in cands}
    print(f"[img2img] canonical_splits of the encoder's down shapes: {parts}")
    split = [k for k in cands if parts[k] > 1]
    assert split, "the library's split policy gives the low-resolution encoder levels parts (csrc/igemm.hip, pick_tile)"
    C, hw = split[-1]                                            # (a) the smallest that splits
    assert _down_full_check(C, hw, hw, 3, seed=9) < 4096
    assert parts[(128, 64)] > 1                                  # (b)
    assert _down_full_check(128, 64, 64, 4, seed=10) >= 4096


@pytest.mark.parametrize("B", [1, 2])
def test_conv3x3_down_unsplit_on_the_large_tile(enc, B):
    """What a real-size request runs at its high-resolution levels: more than 4096 output rows per image, so the canonical
    partition has ONE part (asserted by asking the library) and the launch is the 128 x 128 tile with the direct epilogue --
    bias, fp16 store and the fused statistics written by the tile itself, two slabs per wave.  144 x 128 -> 72 x 64 = 4608 rows
    per image at 128 channels (the smallest such shape with rows a multiple of 32)."""
    from sdlcm_amd import ops
    C, H, W = 128, 144, 128
    rows = ver.down_size(H) * ver.down_size(W)
    assert rows == 4608 and ops.canonical_splits(1, rows, C, 9 * C) == 1
    assert _down_full_check(C, H, W, B, seed=20 + B) >= 4096


def test_conv3x3_down_partial_last_tile_on_the_large_tile(enc):
    """M = 4140 rows (3 images of 46 x 30): the 128 x 128 tile with a last m-tile that is mostly outside the problem, rows per
    image no multiple of 32 (no fused statistics: P == 0).  Guard rows beyond the output stay untouched."""
    C, H, W, B = 128, 92, 60, 3
    x, w, b = _down_case(C, B, H, W, seed=33)
    rows = ver.down_size(H) * ver.down_size(W)
    assert B * rows == 4140
    out, st = _run_down(x, w, b, B, H, W, C, stats=True)
    ref, bnd = ver.down_reference(x, w, b, B, H, W)
    assert la.worst_ratio(out[:B * rows], ref, bnd) <= 1.0 and st.P == 0
    assert bool((out[B * rows:] == -7.0).all())
    solo, _ = _run_down(x[2 * H * W:], w, b, 1, H, W, C)
    assert la.same_bits(solo[:rows], out[2 * rows:3 * rows])


@pytest.mark.parametrize("h,w", [(8, 8), (9, 11)])
@pytest.mark.parametrize("B,dup", [(1, False), (1, True), (2, False), (2, True)])
def test_posterior_renoise_fp64(B, dup, h, w):
    from sdlcm_amd import ops
    from sdlcm_amd.scheduler import LCMSchedule
    s = LCMSchedule()
    sa, sb = s.renoise_coefficients(s.timesteps(2, 0.5)[0])
    g = torch.Generator().manual_seed(31 * B + h + int(dup))
    pre_m, pre_l = torch.randn(B + 1, h, w, 4, generator=g), 3.0 * torch.randn(B + 1, h, w, 4, generator=g)
    pre_l[0, 0, 0], pre_l[0, 0, 1] = 90.0, -90.0                  # logvar above 20 and below -30: the clamp is exercised
    qw = (torch.eye(8) + 0.1 * torch.randn(8, 8, generator=g)).contiguous()
    qb = 0.02 * torch.randn(8, generator=g)
    e0, e1 = torch.randn(B + 1, 4, h, w, generator=g), torch.randn(B + 1, 4, h, w, generator=g)
    rows = 2 * B if dup else B
    lat = torch.full((rows + 1, 4, h, w), -7.0, device=DEV)        # neighbouring memory: must stay untouched
    z = torch.full((B + 1, 4, h, w), -7.0, device=DEV)
    mom = torch.full((B + 1, 8, h, w), -7.0, device=DEV)
    d = [t.to(DEV) for t in (pre_m, pre_l, qw, qb, e0, e1)]
    ops.vae_posterior_renoise(*d, 0.18215, sa, sb, z, lat, B, h, w, moments=mom, dup=dup)
    torch.cuda.synchronize()
    ref = ver.posterior_reference(pre_m[:B], pre_l[:B], qw, qb, e0[:B], e1[:B], 0.18215, sa, sb)
    lv = ref["moments"][0][:, 4:]
    assert float(lv.max()) > 20 and float(lv.min()) < -30
    r = ver.posterior_check(z, lat, ref, B, dup, got_moments=mom)
    print(f"[img2img] posterior B={B} dup={dup} {h}x{w}: worst |err| / bound = {r:.3g}")
    assert r <= 1.0
    if dup:
        assert la.same_bits(lat[:B], lat[B:2 * B])
    assert bool((lat[rows] == -7.0).all()) and bool((z[B] == -7.0).all()) and bool((mom[B] == -7.0).all())
    # without the moments output: the same bits
    lat2, z2 = torch.zeros(rows, 4, h, w, device=DEV), torch.zeros(B, 4, h, w, device=DEV)
    ops.vae_posterior_renoise(*d, 0.18215, sa, sb, z2, lat2, B, h, w, dup=dup)
    torch.cuda.synchronize()
    assert la.same_bits(lat2, lat[:rows]) and la.same_bits(z2, z[:B])


def test_bad_arguments_return_an_error():
    from sdlcm_amd import ops
    from sdlcm_amd.lib import LcmHipError
    x = torch.zeros(64, 128, dtype=torch.float16, device=DEV)
    w = torch.zeros(128, 9 * 128, dtype=torch.float16, device=DEV)
    with pytest.raises(LcmHipError, match="each side >= 2"):
        ops.conv3x3_down(x, w, x, 1, 1, 64, 128, 128)
    with pytest.raises(LcmHipError, match="multiples of 64"):
        ops.conv3x3_down(x, w, x, 1, 8, 8, 96, 128)
    with pytest.raises(LcmHipError, match="bad shape"):
        ops.vae_enc_conv_in_u8(torch.zeros(1, 4, 4, 3, dtype=torch.uint8, device=DEV), w, x, 1, 4, 4, 24)


# ---------------------------------------------------------------------------------------------------------------------------
# the encoder
# ---------------------------------------------------------------------------------------------------------------------------
_REFS = {}


def _encoder_refs(enc_sd, H, W):
    """fp32 CPU reference moments of the two test pictures of this size, and the same with the activations rounded to fp16
    wherever the kernels store fp16 -- computed once per size."""
    if (H, W) not in _REFS:
        ref = ver.EncoderReference(enc_sd)
        img = torch.from_numpy(np.stack([_pic(H, W, 11), _pic(H, W, 12)]))
        _REFS[(H, W)] = (img, ref.moments(img), ref.moments(img, round16=True))
    return _REFS[(H, W)]


def _yardstick_check(tag, got, m32, m16):
    """The GPU may deviate from the fp32 reference by at most 4 x the deviation that fp16 storage alone causes on the CPU (the
    kernels' accumulation order differs from torch's), and never by more than 1e-2 x max|reference|."""
    yard = float((m16 - m32).abs().max())
    dev = float((got - m32).abs().max())
    cap = 1e-2 * float(m32.abs().max())
    print(f"[img2img] {tag}: fp16-storage yardstick {yard:.4g}, GPU deviation {dev:.4g}, cap {cap:.4g}")
    assert dev <= 4 * yard and dev <= cap
    return yard, dev


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("H,W", [(64, 64), (72, 88), (144, 128)])          # 144 x 128: the first down conv runs unsplit, M >= 4096
def test_whole_encoder_against_the_cpu_reference(enc, enc_sd, H, W, B):
    from sdlcm_amd import ops
    img, m32, m16 = _encoder_refs(enc_sd, H, W)
    with torch.inference_mode():
        pm, pl, h, w = enc.encode(img[:B].to(DEV), B, H, W)
        assert (h, w) == (H // 8, W // 8)
        z, lat, mom = (torch.zeros(B, c, h, w, device=DEV) for c in (4, 4, 8))
        zero = torch.zeros(B, 4, h, w, device=DEV)
        ops.vae_posterior_renoise(pm, pl, enc.w["quant.w"], enc.w["quant.b"], zero, zero, 1.0, 1.0, 0.0, z, lat, B, h, w, moments=mom)
        torch.cuda.synchronize()
    _yardstick_check(f"encoder {H}x{W} B={B}", mom.cpu(), m32[:B], m16[:B])
    if B == 2:                                                   # a request's bits do not depend on its batch
        with torch.inference_mode():
            pm1, pl1, _, _ = enc.encode(img[1:2].to(DEV), 1, H, W)
            torch.cuda.synchronize()
        assert la.same_bits(pm1[0], pm[1]) and la.same_bits(pl1[0], pl[1])


def test_mid_block_attention_past_the_decoders_range(enc, enc_sd):
    """The encoder never tiles: its mid block runs one 512-wide head over every latent pixel.  65 x 64 = 4160 keys is past the
    4096 the decoder's tiles ever reach.  Reference: the restatement in float64 (on the device) from the same fp16 input;
    yardstick as for the whole encoder, with the fp16-storage deviation computed in float64 too."""
    H, W, C = 65, 64, 512
    g = torch.Generator().manual_seed(2)
    x16 = torch.randn(1, C, H, W, generator=g).half()
    ref = ver.EncoderReference(enc_sd, dtype=torch.float64)
    ref.w = {k: v.to(DEV) for k, v in ref.w.items() if ".mid_block." in k}
    with torch.inference_mode():
        want = ref.mid_block(x16.to(DEV, torch.float64)).cpu()
        want16 = ref.mid_block(x16.to(DEV, torch.float64), round16=True).cpu()
        rows = x16.permute(0, 2, 3, 1).reshape(H * W, C).contiguous().to(DEV)
        out, _ = enc.mid_block(rows, C, 1, H, W)
        torch.cuda.synchronize()
    got = out.float().reshape(1, H, W, C).permute(0, 3, 1, 2).cpu().double()
    assert torch.isfinite(got).all()
    _yardstick_check("mid block 65x64 (4160 keys)", got, want, want16)


# ---------------------------------------------------------------------------------------------------------------------------
# the chain against the CPU restatement
# ---------------------------------------------------------------------------------------------------------------------------
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


def _cpu_chain(ora, enc_sd, pe, pic, steps, strength, seed, scaling=0.18215):
    """reference encoder (fp32) -> sample -> add_noise -> the oracle's strength-cut pass -> decode."""
    from oracle import glue
    from sdlcm_amd.pipeline import draw_noise_img2img
    h, w = pic.shape[0] // 8, pic.shape[1] // 8
    e0, rest = draw_noise_img2img(seed, h, w, steps)
    m = ver.EncoderReference(enc_sd).moments(torch.from_numpy(pic[None]))
    z = ver.sample(m, e0, scaling)
    ts = rr.strength_timesteps(steps, strength)
    with torch.inference_mode():
        y = ora.one_pass(pe, ora.renoise(z, ts[0], rest[0]), ts, rest[1:], 1.0)
        img = ora.vae.decode(y).numpy()
    return dict(moments=m, z=z.numpy(), latents=y.numpy(), image=img, image_u8=glue.postprocess_u8(img))


def test_chain_eager_captured_and_cpu(state, enc_sd):
    from sdlcm_amd.lib import LcmHipError
    from sdlcm_amd.pipeline import draw_noise_img2img
    hip, ora = state["hip"], state["ora"]
    B, seeds = 2, [9100, 9101]
    pe = _embeds(B, seed=41)
    pics = np.stack([_pic(64, 64, 21), _pic(64, 64, 22)])
    eager = hip.generate_img2img(pe, seeds, pics, 64, 64, 2, 0.5, want_float=True)
    assert eager["unet_evals"] == 2 and eager["rgb"].shape == (B, 64, 64, 3) and eager["init_latents"].shape == (B, 4, 8, 8)
    assert eager["moments"].shape == (B, 8, 8, 8)
    cap = hip.generate_img2img(pe, seeds, pics, 64, 64, 2, 0.5)
    rep = hip.generate_img2img(pe, seeds, pics, 64, 64, 2, 0.5)             # the second captured call replays both graphs
    for o in (cap, rep):
        for k in ("rgb", "latents", "pool8", "init_latents"):
            assert np.array_equal(o[k], eager[k]), k
    assert hip.lanes[0].enc_plans[(B, 64, 64)].graph is not None
    solo = hip.generate_img2img(pe[1:], seeds[1:], pics[1:], 64, 64, 2, 0.5)
    assert np.array_equal(solo["rgb"][0], rep["rgb"][1]) and np.array_equal(solo["init_latents"][0], rep["init_latents"][1])
    for b in range(B):
        ref = _cpu_chain(ora, enc_sd, pe[b:b + 1].float(), pics[b], 2, 0.5, seeds[b])
        a = np.clip(eager["image"][b:b + 1].transpose(0, 3, 1, 2) / 2 + 0.5, 0, 1)
        e = float(np.abs(a - np.clip(ref["image"] / 2 + 0.5, 0, 1)).max())
        print(f"[img2img] 64x64 steps 2 strength 0.5 request {b}: image[0,1] max|d| = {e:.4g}, "
              f"init_latents max|d| = {np.abs(eager['init_latents'][b] - ref['z'][0]).max():.3g}")
        assert e < 1e-2
        m16 = ver.EncoderReference(enc_sd).moments(torch.from_numpy(pics[b][None]), round16=True)
        _yardstick_check(f"chain moments request {b}", torch.from_numpy(eager["moments"][b:b + 1]), ref["moments"], m16)
        # init_latents are the posterior sample of the GPU's own moments (fp32 expression, scaled)
        e0 = draw_noise_img2img(seeds[b], 8, 8, 2)[0]
        zz = ver.sample(torch.from_numpy(eager["moments"][b:b + 1]).double(), e0.double(), 0.18215).numpy()
        assert np.abs(eager["init_latents"][b] - zz[0]).max() <= 1e-5 * max(1.0, np.abs(zz).max())
    with pytest.raises(ValueError, match="The combined original_steps x strength"):
        hip.generate_img2img(pe, seeds, pics, 64, 64, 8, 0.1)
    with pytest.raises(LcmHipError, match="uint8"):
        hip.generate_img2img(pe, seeds, pics[:, :32], 64, 64, 2, 0.5)


def test_a_checkpoint_without_an_encoder_raises_for_the_request(state):
    from sdlcm_amd import weights
    from sdlcm_amd.lib import LcmHipError
    from sdlcm_amd.pipeline import LcmHipPipeline
    hip = state["hip"]
    src, built, views = hip.vae_encoder_src, hip.vae_encoder, [L.vae_enc for L in hip.lanes]
    try:
        hip.vae_encoder_src, hip.vae_encoder = None, None
        for L in hip.lanes:
            L.vae_enc = None
        with pytest.raises(LcmHipError, match="no VAE encoder"):
            hip.generate_img2img(_embeds(1), [1], _pic()[None], 64, 64, 2, 0.5)
        assert np.isfinite(hip.generate(_embeds(1), [1], 64, 64, 2, 1.0)["latents"]).all()      # plain requests still run
    finally:
        hip.vae_encoder_src, hip.vae_encoder = src, built
        for L, v in zip(hip.lanes, views):
            L.vae_enc = v


def test_hand_over_launch_audited_inside_a_real_chain(state, monkeypatch):
    """tests/launch_audit.py's hook, extended by the three new entry points: the chain runs eagerly under the audit; conv_in,
    every Downsample2D and the posterior launch -- fed by the real encoder, feeding the real sampler pass -- are compared with
    float64 under their derived bounds; what they must not write stays unchanged; every other launch of the encoder and of the
    pass is checked as in any audited pass."""
    hip = state["hip"]
    monkeypatch.setitem(la.CHECKED, "vae_posterior_renoise", ("z_out", "lat", "moments"))
    monkeypatch.setitem(la.CHECKED, "vae_enc_conv_in_u8", ("out",))
    monkeypatch.setitem(la.CHECKED, "conv3x3_down", ("out",))

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

    plans = hip.lanes[0].plans
    before = set(plans)
    pics = np.stack([_pic(40, 72, 31), _pic(40, 72, 32)])
    with Audit() as au:
        out = hip.generate_img2img(_embeds(2, seed=77), [601, 602], pics, 72, 40, 2, 0.5, want_float=True)
    for k in set(plans) - before:
        plans.pop(k)
    bad = la.failures(au.checks)
    per = la.entry_table(au.checks)
    print(f"[audit] img2img 72x40 B2: {len(au.checks)} launches checked, {la.summary_line(au.checks)}")
    assert not bad, bad
    assert per["vae_posterior_renoise"][0] == 1 and per["vae_posterior_renoise"][1] <= 1.0
    assert per["vae_enc_conv_in_u8"][0] == 1 and per["conv3x3_down"][0] == 3
    assert "latents_renoise" not in per                   # the hand-over IS the re-noise: the pass launches none of its own
    assert all(k[0] == 1 for k in au.record_keys() - au.checked_keys())       # only the down convs are checked outside HOOKED
    assert np.isfinite(out["latents"]).all()


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
    kw = dict(init_image=_pic(64, 64, 40 + s), denoising_strength=0.5)
    kw.update(extra)
    return _Req(prompt=f"img2img {s}", seed=s, **kw)


def test_run_job_serves_init_image(worker):
    eng = worker._engine
    plain_req = _Req(prompt="img2img 3", seed=3)
    plain_before = worker.run_job(_Job(plain_req))
    assert eng.pipe.vae_encoder is None                    # a server that never saw a picture uploaded nothing more
    n0 = eng.stats["img2img_requests"], eng.stats["unet_evals"]
    png, seed = worker.run_job(_Job(_mk(3)))
    assert seed == 3 and _png_size(png) == (64, 64) and png != plain_before[0]
    assert eng.stats["img2img_requests"] == n0[0] + 1 and eng.stats["unet_evals"] == n0[1] + 2
    assert worker.run_job(_Job(plain_req)) == plain_before               # a plain request's bytes, before and after
    assert worker.run_job(_Job(_Req(prompt="img2img 3", seed=3, denoising_strength=0.3))) == plain_before
    # strength 1.0 with a picture is still not the plain request: the posterior sample enters at t0, it is not pure noise
    full = worker.run_job(_Job(_mk(3, denoising_strength=1.0)))[0]
    assert full != plain_before[0] and full != png
    # another picture, another strength, the init_images form, a picture of another size (fitted): all reach the chain
    assert worker.run_job(_Job(_mk(3, init_image=_pic(64, 64, 99))))[0] != png
    assert worker.run_job(_Job(_mk(3, denoising_strength=0.8)))[0] != png
    from sdlcm_amd.backends.hip_worker import encode_png
    assert worker.run_job(_Job(_mk(3, init_image=None, init_images=[encode_png(_pic(64, 64, 43))])))[0] == png
    big = worker.run_job(_Job(_mk(3, init_image=_pic(96, 80, 43))))[0]
    assert _png_size(big) == (64, 64) and big != png
    assert _png_size(worker.run_job(_Job(_mk(3, size="88x72", init_image=_pic(50, 50, 1))))[0]) == (88, 72)
    # run_job_with_latents: the 8 x 8 pool of the final latents
    png2, _, blob = worker.run_job_with_latents(_Job(_mk(3)))
    assert png2 == png and len(blob) == 512 and np.isfinite(np.frombuffer(blob, np.float16).astype(np.float32)).all()


def test_bytes_do_not_depend_on_batch_or_padding(worker):
    from sdlcm_amd.backends.hip_worker import encode_png
    eng = worker._engine
    req = _mk(0)
    key = worker._job_key(req)
    assert key[6:] == ("img2img", 0.5)

    def batch(reqs, lane=0):
        return encode_png(eng.run_batch(key, [worker._prepare(r, key) for r in reqs], lane)[0][0])

    def third(reqs):
        return encode_png(eng.run_batch(key, [worker._prepare(r, key) for r in reqs], 0)[2][0])
    pngs = {"alone": worker.run_job(_Job(req))[0], "batch of 2": batch([req, _mk(1)]),
            "padded third of 4": third([_mk(1), _mk(2), req, req])}
    if eng.n_lanes > 1:
        pngs["lane 1"] = batch([req], lane=1)
    for tag, png in pngs.items():
        assert png == pngs["alone"], tag


def test_a_pass_is_capped_at_what_both_stages_need(worker, monkeypatch):
    """The cap counts the strength-cut pass AND the encoder stage (its split down convs need fp32 slabs too): with a workspace
    that holds two requests' parts a batch of 4 runs as 2 + 2 and every request keeps its bytes."""
    eng = worker._engine
    pipe = eng.pipe
    key = worker._job_key(_mk(0))
    solo = [eng.run_batch(key, [worker._prepare(_mk(s), key)], 0)[0][0] for s in range(4)]
    P = pipe.plan(1, 8, 8, 2, False, 1.0, lane=0, refine=(0.5, 1, True), kind="from-state")
    need_s, need_e = pipe.splitk_need(P), pipe.encoder_splitk_need(64, 64)
    print(f"[img2img] split-K workspace per request at 64x64: pass {need_s} bytes, encoder stage {need_e} bytes")
    # the encoder's 32 x 32 level at 128 channels has 2 parts: 2 x 1024 x 128 fp32 at the least
    assert need_e >= 4 * 2 * 1024 * 128
    assert pipe.img2img_batch_cap(64, 64, 2, 0.5, sizes=eng.batch_sizes) == max(eng.batch_sizes)
    have, need = pipe.lanes[0].splitk_ws.numel() * 4, max(need_s, need_e)
    assert pipe.img2img_batch_cap(64, 64, 2, 0.5, sizes=(1, 2, 4, have // need * 2 + 8)) == 4
    # the encoder's need alone can decide: with the pass's need out of the way the cap is still bounded
    monkeypatch.setattr(type(pipe), "splitk_need", lambda self, P: 0)
    assert pipe.img2img_batch_cap(64, 64, 2, 0.5, sizes=(1, 2, 4, have // need_e * 2 + 8)) == 4
    monkeypatch.undo()
    calls = []
    real = pipe.generate_img2img
    monkeypatch.setattr(pipe, "generate_img2img", lambda pe, seeds, *a, **kw: calls.append(len(seeds)) or real(pe, seeds, *a, **kw))
    monkeypatch.setattr(type(pipe), "img2img_batch_cap", lambda self, *a, **kw: 2)
    got = eng.run_batch(key, [worker._prepare(_mk(s), key) for s in range(4)], 0)
    assert calls == [2, 2]
    for s in range(4):
        assert np.array_equal(got[s][0], solo[s])


def _outcome(f):
    try:
        return f.result(600)
    except Exception as e:      # noqa
        return e


def test_errors_reach_the_right_job_inside_a_drained_batch(worker):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from tools import minipool
    bad = {1: (dict(init_image=b"\x89PNG not a picture"), "init_image"), 3: (dict(denoising_strength=0.01), "denoising_strength"),
           4: (dict(enable_hr=True), "not combined"), 5: (dict(denoise_strength=0.5), "not combined"),
           6: (dict(controlnet_image=np.zeros((64, 64, 3), np.uint8)), "not combined")}
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


def test_the_sdxl_worker_refuses_a_picture():
    from sdlcm_amd.backends.hip_worker import HipLcmSDXLWorker
    with pytest.raises(RuntimeError, match="SDXL"):
        HipLcmSDXLWorker._job_key(_mk(1))
