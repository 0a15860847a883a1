"""Host side of image-to-image (init_image / init_images / denoising_strength): the encoder reference against torch, request
parsing and validation, batch keys, the draw order, the single-file key map, the synthetic weights -- and the self-test of the
three launch bounds of tests/vae_encoder_reference.py: each accepts the kernel's own arithmetic and rejects a result that is wrong
by one K term.  No GPU."""
import base64
import hashlib
import io
from dataclasses import dataclass, field
from typing import Optional

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import launch_audit as la
import vae_encoder_reference as ver
from sdlcm_amd import weights
from sdlcm_amd.backends import img2img
from sdlcm_amd.backends.hip_worker import HipLcmSDXLWorker, HipLcmWorker
from sdlcm_amd.scheduler import LCMSchedule

SMALL = dict(block_out_channels=(32, 32, 64, 64), norm_num_groups=32)


@dataclass
class _Style:
    style: Optional[str] = None
    level: int = 0


@dataclass
class _Req:
    prompt: str = "p"
    size: str = "64x64"
    num_inference_steps: int = 4
    guidance_scale: float = 1.0
    seed: Optional[int] = 1
    style_lora: _Style = field(default_factory=_Style)


def _req(**extra):
    r = _Req()
    for k, v in extra.items():
        setattr(r, k, v)
    return r


def _pic(h=64, w=64, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _png(arr):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(arr, "RGB").save(b, "PNG")
    return b.getvalue()


# ---- the reference against torch -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(8, 8), (7, 9), (10, 6)])
def test_reference_downsample_is_the_padded_stride_2_conv(H, W):
    sd = weights.synthetic_vae_encoder(SMALL)
    ref = ver.EncoderReference(sd, SMALL)
    p = "encoder.down_blocks.0.downsamplers.0.conv"
    x = torch.randn(2, 32, H, W, generator=torch.Generator().manual_seed(H))
    want = F.conv2d(F.pad(x, (0, 1, 0, 1)), sd[p + ".weight"].float(), sd[p + ".bias"].float(), stride=2)
    got = ref.downsample(x, p)
    assert got.shape == (2, 32, ver.down_size(H), ver.down_size(W)) and torch.equal(got, want)
    # ... and it is NOT the symmetric stride-2 convolution of the UNet
    sym = F.conv2d(x, sd[p + ".weight"].float(), sd[p + ".bias"].float(), stride=2, padding=1)
    assert sym.shape != want.shape or not torch.allclose(sym, want)
    # the float64 launch reference computes the same function from pixel-major fp16 operands
    x16 = x[:1].half()
    rows = x16.permute(0, 2, 3, 1).reshape(H * W, 32)
    y, _ = ver.down_reference(rows, ver.pack3x3(sd[p + ".weight"]), sd[p + ".bias"], 1, H, W)
    want16 = F.conv2d(F.pad(x16.double(), (0, 1, 0, 1)), sd[p + ".weight"].double(), sd[p + ".bias"].double(), stride=2)
    assert torch.allclose(y.reshape(ver.down_size(H), ver.down_size(W), 32).permute(2, 0, 1), want16[0], atol=1e-12)


def test_reference_conv_in_normalises_then_pads():
    sd = weights.synthetic_vae_encoder(SMALL)
    ref = ver.EncoderReference(sd, SMALL)
    img = torch.from_numpy(np.stack([_pic(9, 11, 1), np.zeros((9, 11, 3), np.uint8)]))
    x = 2.0 * img.permute(0, 3, 1, 2).float() / 255.0 - 1.0
    want = F.conv2d(x, sd["encoder.conv_in.weight"].float(), sd["encoder.conv_in.bias"].float(), padding=1)
    assert torch.equal(ref.conv_in(img), want)
    # an all-zero picture is -1 everywhere: the corner sees 4 taps of -1 and 5 of 0, not 9 of -1
    w = sd["encoder.conv_in.weight"].float()
    assert torch.allclose(want[1, :, 0, 0], sd["encoder.conv_in.bias"].float() - w[:, :, 1:, 1:].sum((1, 2, 3)), atol=1e-5)


def test_reference_encoder_shapes_and_sampling():
    sd = weights.synthetic_vae_encoder(SMALL)
    ref = ver.EncoderReference(sd, SMALL)
    img = torch.from_numpy(np.stack([_pic(24, 40, 3)]))
    m = ref.moments(img)
    assert m.shape == (1, 8, 3, 5) and torch.isfinite(m).all()
    m16 = ref.moments(img, round16=True)
    assert 0 < float((m16 - m).abs().max()) < 0.05 * float(m.abs().max())
    e0 = torch.randn(1, 4, 3, 5, generator=torch.Generator().manual_seed(1))
    z = ver.sample(m, e0, 0.18215)
    assert torch.allclose(z, (m[:, :4] + torch.exp(0.5 * m[:, 4:]) * e0) * 0.18215)
    assert torch.equal(ver.add_noise(z, e0, 1.0), z)


# ---- request parsing ---------------------------------------------------------------------------------------------------------
def test_parse_defaults_ranges_and_forms():
    pic = _pic()
    assert img2img.parse_img2img(_req()) is None
    assert img2img.parse_img2img(_req(denoising_strength=0.3)) is None          # no picture: the field means nothing here
    s, got = img2img.parse_img2img(_req(init_image=pic))
    assert s == 0.75 and np.array_equal(got, pic)
    assert img2img.parse_img2img(_req(init_image=pic, denoising_strength=0.05))[0] == 0.05
    assert img2img.parse_img2img(_req(init_image=pic, denoising_strength=1))[0] == 1.0
    for bad in (0.0, 0.04, 1.01, -1, float("nan"), "x", True):
        with pytest.raises(RuntimeError, match="denoising_strength"):
            img2img.parse_img2img(_req(init_image=pic, denoising_strength=bad))
    png = _png(pic)
    from PIL import Image
    for form in (dict(init_image=png), dict(init_image=Image.fromarray(pic, "RGB")), dict(init_images=[png]),
                 dict(init_images=[base64.b64encode(png).decode()]),
                 dict(init_images=["data:image/png;base64," + base64.b64encode(png).decode()])):
        assert np.array_equal(img2img.parse_img2img(_req(**form))[1], pic), list(form)
    for bad, text in ((dict(init_images=[]), "exactly one"), (dict(init_images=[png, png]), "exactly one"),
                      (dict(init_images=["@@not base64@@"]), "base64"), (dict(init_images=png), "list"),
                      (dict(init_image=b"not a picture"), "init_image"), (dict(init_image=np.zeros((4, 4), np.uint8)), "init_image"),
                      (dict(init_image=3.5), "init_image")):
        with pytest.raises(RuntimeError, match=text):
            img2img.parse_img2img(_req(**bad))
    # the key is computed more than once per job: every form, the base64 one included, is decoded once
    for form in (dict(init_image=png), dict(init_images=[base64.b64encode(png).decode()])):
        r = _req(**form)
        assert img2img.parse_img2img(r)[1] is img2img.parse_img2img(r)[1], list(form)
    # another size is fitted on the host
    assert img2img.fit_init(_pic(40, 72), 64, 48).shape == (48, 64, 3)
    assert img2img.fit_init(pic, 64, 64) is pic


def test_job_keys():
    pic = _pic()
    plain = HipLcmWorker._job_key(_req())
    assert len(plain) == 6
    assert HipLcmWorker._job_key(_req(denoising_strength=0.3)) == plain        # without a picture: unchanged
    k1 = HipLcmWorker._job_key(_req(init_image=pic))
    k2 = HipLcmWorker._job_key(_req(init_image=pic, denoising_strength=0.5))
    assert k1 == plain + ("img2img", 0.75) and k2 == plain + ("img2img", 0.5) and k1 != k2
    assert img2img.is_img2img_key(k1) and not img2img.is_img2img_key(plain)
    assert HipLcmWorker._job_key(_req(init_images=[_png(pic)], denoising_strength=0.5)) == k2
    for extra in (dict(enable_hr=True), dict(denoise_strength=0.5), dict(pass_number=2), dict(controlnet_image=pic)):
        with pytest.raises(RuntimeError, match="not combined"):
            HipLcmWorker._job_key(_req(init_image=pic, **extra))
    with pytest.raises(RuntimeError, match="SDXL"):
        HipLcmSDXLWorker._job_key(_req(init_image=pic))
    with pytest.raises(RuntimeError, match="SDXL"):
        HipLcmSDXLWorker._job_key(_req(init_images=[_png(pic)]))
    assert HipLcmSDXLWorker._job_key(_req()) == plain
    with pytest.raises(RuntimeError, match="The combined original_steps x strength"):
        img2img.check_schedule(LCMSchedule(), 4, 0.05)
    img2img.check_schedule(LCMSchedule(), 2, 0.5)


def test_draw_order_and_count():
    from sdlcm_amd.pipeline import draw_noise_img2img
    e0, rest = draw_noise_img2img(77, 9, 11, 3)
    g = torch.Generator().manual_seed(77)
    want = [torch.randn((1, 4, 9, 11), generator=g) for _ in range(4)]
    assert len(rest) == 3 and torch.equal(e0, want[0]) and all(torch.equal(a, b) for a, b in zip(rest, want[1:]))


# ---- weights -------------------------------------------------------------------------------------------------------------------
def _digest(sd):
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(sd[k].numpy().tobytes())
    return h.hexdigest()


def test_synthetic_vae_is_unchanged_by_the_encoder_function():
    before = _digest(weights.synthetic_vae(SMALL))
    enc = weights.synthetic_vae_encoder(SMALL)
    assert _digest(weights.synthetic_vae(SMALL)) == before
    assert all(k.startswith("encoder.") or k.startswith("quant_conv.") for k in enc)
    assert enc["encoder.conv_out.weight"].shape == (8, 64, 3, 3) and enc["quant_conv.weight"].shape == (8, 8, 1, 1)
    assert _digest(weights.synthetic_vae_encoder(SMALL)) == _digest(enc) != _digest(weights.synthetic_vae_encoder(SMALL, seed=5))


def test_single_file_key_map_round_trips_the_encoder():
    enc = weights.synthetic_vae_encoder(SMALL)
    ldm = {weights.ldm_vae_encoder_key(k): v for k, v in enc.items()}
    assert len(ldm) == len(enc)
    assert "encoder.down.1.block.0.nin_shortcut.weight" not in ldm and "encoder.down.2.block.0.nin_shortcut.weight" in ldm
    for k in ("encoder.down.0.downsample.conv.weight", "encoder.mid.attn_1.q.weight", "encoder.mid.block_2.conv1.bias",
              "encoder.norm_out.weight", "encoder.conv_out.bias", "quant_conv.weight"):
        assert k in ldm, k
    back = {weights._ldm_vae_key(k): v for k, v in ldm.items()}
    assert set(back) == set(enc) and all(back[k] is enc[k] for k in enc)
    # the loaders keep the decoder's dict as it was and carry the encoder beside it
    both = dict(weights.synthetic_vae(SMALL), **enc)
    split = weights.split_vae_encoder(both)
    assert set(split) == set(weights.synthetic_vae(SMALL)) and set(split.encoder) == set(enc)
    assert weights.has_vae_encoder(split.encoder) and not weights.has_vae_encoder(weights.split_vae_encoder(dict(split)).encoder)
    assert set(weights.audit_vae_encoder(split.encoder, SMALL)) == set(enc)
    with pytest.raises(RuntimeError, match="no VAE encoder"):
        weights.audit_vae_encoder({}, SMALL)
    one, two = weights.VaeStateDict(), weights.VaeStateDict()
    one.encoder["x"] = 1
    assert two.encoder == {}                                  # no state shared between instances


# ---- the bounds reject what is wrong by one K term ---------------------------------------------------------------------------
def test_conv_in_bound():
    g = torch.Generator().manual_seed(3)
    w = (torch.randn(128, 3, 3, 3, generator=g) * 27 ** -0.5).half()
    b = (0.02 * torch.randn(128, generator=g)).half()
    w16 = ver.pack3x3(w)
    img = torch.from_numpy(np.stack([_pic(9, 11, 5), np.zeros((9, 11, 3), np.uint8), np.full((9, 11, 3), 255, np.uint8)]))
    good = ver.conv_in_kernel_like(img, w16, b)
    assert ver.conv_in_check(good, img, w16, b, 3, 9, 11) <= 1.0
    assert ver.conv_in_check(ver.conv_in_kernel_like(img, w16, b, drop=(4, 1)), img, w16, b, 3, 9, 11) > 1.0, "one K term dropped"
    assert ver.conv_in_check(ver.conv_in_kernel_like(img, w16, b, pad_minus_one=True), img, w16, b, 3, 9, 11) > 1.0, "border padded with -1"
    # the hi + lo carry is what the bound assumes: a single fp16 operand must not pass it
    assert ver.conv_in_check(ver.conv_in_kernel_like(img, w16, b, single_fp16=True), img, w16, b, 3, 9, 11) > 1.0, "no lo part"


def _down_kernel_like(x16, w16, bias16, B, H, W, splits=1, drop_k=None):
    Cin = x16.shape[1]
    Ho, Wo = ver.down_size(H), ver.down_size(W)
    xp = F.pad(x16.float().reshape(B, H, W, Cin), (0, 0, 0, 1, 0, 1))
    A = torch.stack([xp[:, ky:ky + 2 * (Ho - 1) + 1:2, kx:kx + 2 * (Wo - 1) + 1:2] for ky in range(3) for kx in range(3)], 3)
    A = A.reshape(B * Ho * Wo, 9 * Cin)
    if drop_k is not None:
        A[:, drop_k] = 0
    nk, wf = 9 * Cin // 64, w16.float()
    tot = torch.zeros(A.shape[0], wf.shape[0])
    for s in range(splits):
        acc = torch.zeros_like(tot)
        for t in range(s * nk // splits, (s + 1) * nk // splits):
            acc = acc + A[:, t * 64:(t + 1) * 64] @ wf[:, t * 64:(t + 1) * 64].T
        tot = tot + acc
    return (tot + bias16.float()).half()


def test_down_bound():
    g = torch.Generator().manual_seed(4)
    B, H, W, C = 2, 7, 9, 128
    x = torch.randn(B * H * W, C, generator=g).half()
    w16 = ver.pack3x3((torch.randn(C, C, 3, 3, generator=g) * (9 * C) ** -0.5).half())
    b = (0.02 * torch.randn(C, generator=g)).half()
    ref, bnd = ver.down_reference(x, w16, b, B, H, W)
    for splits in (1, 3):
        assert la.worst_ratio(_down_kernel_like(x, w16, b, B, H, W, splits), ref, bnd) <= 1.0
    assert la.worst_ratio(_down_kernel_like(x, w16, b, B, H, W, 3, drop_k=700), ref, bnd) > 1.0, "one K term dropped"
    # the symmetric stride-2 convolution is another function (and, at odd sizes, another shape)
    sym = F.conv2d(x.float().reshape(B, H, W, C).permute(0, 3, 1, 2), w16.float().reshape(C, 3, 3, C).permute(0, 3, 1, 2), b.float(),
                   stride=2, padding=1)
    assert sym.shape[2:] != (ver.down_size(H), ver.down_size(W))


def test_posterior_bound():
    g = torch.Generator().manual_seed(6)
    B, h, w = 2, 9, 11
    pre_m, pre_l = torch.randn(B, h, w, 4, generator=g), 3.0 * torch.randn(B, h, w, 4, generator=g)
    pre_l[0, 0, 0], pre_l[0, 0, 1] = 90.0, -90.0                            # beyond the clamp on both sides
    qw = torch.eye(8) + 0.1 * torch.randn(8, 8, generator=g)
    qb = 0.02 * torch.randn(8, generator=g)
    e0, e1 = torch.randn(B, 4, h, w, generator=g), torch.randn(B, 4, h, w, generator=g)
    args = (pre_m, pre_l, qw, qb, e0, e1, 0.18215, 0.5477, 0.8367)
    ref = ver.posterior_reference(*args)
    lv = ref["moments"][0][:, 4:]
    assert float(lv.max()) > 20 and float(lv.min()) < -30
    z, lat = ver.posterior_kernel_like(*args)
    assert ver.posterior_check(z, lat, ref, B, False) <= 1.0
    z, lat = ver.posterior_kernel_like(*args, drop=(1, 6))
    assert ver.posterior_check(z, lat, ref, B, False) > 1.0, "one term of quant_conv dropped"
    z, lat = ver.posterior_kernel_like(*args, no_clamp=True)
    assert ver.posterior_check(z, lat, ref, B, False) > 1.0, "logvar not clamped"
    z, lat = ver.posterior_kernel_like(*args)
    both = torch.cat([lat, lat])
    assert ver.posterior_check(z, both, ref, B, True) <= 1.0
    both[B] += 1e-6
    assert ver.posterior_check(z, both, ref, B, True) == float("inf"), "the classifier-free-guidance copy must be bit-equal"
