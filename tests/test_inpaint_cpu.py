"""Host side of inpainting (mask / mask_image / mask_blur / inpainting_mask_invert / inpainting_fill / inpaint_full_res): request
parsing in every accepted form, every error message, the batch keys -- and the integer mask rules of tests/inpaint_reference.py:
the weight table sums to 65536, the fixed-point blur stays within one level of a float64 Gaussian with the same borders, the
latent-mask tie and the overlay's two exact ends.  No GPU."""
import base64
import io
from dataclasses import dataclass, field
from typing import Optional

import numpy as np
import pytest

import inpaint_reference as ir
from sdlcm_amd.backends import img2img, inpaint
from sdlcm_amd.backends.hip_worker import HipLcmSDXLWorker, HipLcmWorker
from sdlcm_amd.pipeline import mask_blur_weights
from sdlcm_amd.scheduler import LCMSchedule


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


def _mask(h=64, w=64, seed=1):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def _png(arr):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(arr).save(b, "PNG")
    return b.getvalue()


# ---- request parsing ---------------------------------------------------------------------------------------------------------
def test_a_request_without_a_mask_is_untouched():
    pic = _pic()
    assert inpaint.parse_inpaint(_req()) is None
    assert inpaint.parse_inpaint(_req(init_image=pic)) is None
    # without a mask the other inpainting fields mean nothing, whatever they say
    r = _req(init_image=pic, mask_blur=99, inpainting_fill=3, inpaint_full_res=True, inpainting_mask_invert=True, denoising_strength=0.5)
    assert inpaint.parse_inpaint(r) is None
    plain = HipLcmWorker._job_key(_req())
    assert HipLcmWorker._job_key(r) == plain + ("img2img", 0.5) and img2img.is_img2img_key(HipLcmWorker._job_key(r))
    assert HipLcmWorker._job_key(_req(mask_blur=3, inpainting_fill=0)) == plain


def test_parse_every_form_of_the_mask():
    from PIL import Image
    pic, m = _pic(), _mask()
    s, blur, got_pic, got = inpaint.parse_inpaint(_req(init_image=pic, mask=m))
    assert (s, blur) == (0.75, 4.0) and np.array_equal(got_pic, pic) and np.array_equal(got, m) and got.dtype == np.uint8
    png = _png(m)
    b64 = base64.b64encode(png).decode()
    gray3 = np.repeat(m[..., None], 3, axis=2)
    rgba = np.concatenate([gray3, np.full((64, 64, 1), 7, np.uint8)], axis=2)          # the alpha channel is not the mask
    forms = (dict(mask=png), dict(mask=bytearray(png)), dict(mask=b64), dict(mask="data:image/png;base64," + b64),
             dict(mask=Image.fromarray(m, "L")), dict(mask=m[..., None]), dict(mask=gray3), dict(mask=rgba),
             dict(mask_image=m), dict(mask_image=b64), dict(mask=None, mask_image=png))
    for form in forms:
        out = inpaint.parse_inpaint(_req(init_image=pic, **form))
        assert out[3].shape == (64, 64) and out[3].dtype == np.uint8 and np.array_equal(out[3], m), list(form)
    # ``mask`` wins over its alias; a colour mask goes through PIL's "L" (ITU-R 601 luma)
    assert np.array_equal(inpaint.parse_inpaint(_req(init_image=pic, mask=m, mask_image=255 - m))[3], m)
    col = _pic(seed=5)
    assert np.array_equal(inpaint.parse_inpaint(_req(init_image=pic, mask=col))[3], np.asarray(Image.fromarray(col, "RGB").convert("L")))
    # a JPEG mask decodes too
    jb = io.BytesIO()
    Image.fromarray(m, "L").save(jb, "JPEG", quality=95)
    assert inpaint.parse_inpaint(_req(init_image=pic, mask=jb.getvalue()))[3].shape == (64, 64)
    # the picture may come as init_images, the strength is image-to-image's
    out = inpaint.parse_inpaint(_req(init_images=[_png(pic)], mask=m, denoising_strength=0.5, mask_blur=0))
    assert out[0] == 0.5 and out[1] == 0.0 and np.array_equal(out[2], pic)
    # inverted on the host
    assert np.array_equal(inpaint.parse_inpaint(_req(init_image=pic, mask=m, inpainting_mask_invert=1))[3], 255 - m)
    assert np.array_equal(inpaint.parse_inpaint(_req(init_image=pic, mask=m, inpainting_mask_invert=False))[3], m)
    # decoded once per request object (the key is computed more than once per job)
    r = _req(init_image=pic, mask=b64)
    assert inpaint.parse_inpaint(r)[3] is inpaint.parse_inpaint(r)[3]
    # accepted values of the fields that are only checked
    for ok in (dict(inpainting_fill=1), dict(inpaint_full_res=False), dict(inpaint_full_res=0), dict(mask_blur=32), dict(mask_blur=0.5)):
        assert inpaint.parse_inpaint(_req(init_image=pic, mask=m, **ok)) is not None, ok
    # another size is fitted on the host with LANCZOS in "L"
    small = _mask(40, 72)
    fit = inpaint.fit_mask(small, 64, 48)
    assert fit.shape == (48, 64) and fit.dtype == np.uint8
    assert np.array_equal(fit, np.asarray(Image.fromarray(small, "L").resize((64, 48), Image.LANCZOS)))
    assert inpaint.fit_mask(m, 64, 64) is m


def test_every_error_message():
    pic, m = _pic(), _mask()
    cases = [
        (dict(mask=m), "without init_image"),
        (dict(mask_image=m), "without init_image"),
        (dict(init_image=pic, mask=b"not a picture"), "Invalid mask: not a decodable PNG or JPEG"),
        (dict(init_image=pic, mask="@@not base64@@"), "Invalid mask: not base64"),
        (dict(init_image=pic, mask=3.5), "Invalid mask: expected PNG / JPEG bytes"),
        (dict(init_image=pic, mask=np.zeros((4, 4, 2), np.uint8)), "Invalid mask: expected an H x W"),
        (dict(init_image=pic, mask=np.zeros((4, 4), np.float32)), "Invalid mask: expected an H x W"),
        (dict(init_image=pic, mask=np.zeros((4,), np.uint8)), "Invalid mask: expected an H x W"),
        (dict(init_image=pic, mask=m, inpaint_full_res=True), "inpaint_full_res.*only masked.*not served"),
        (dict(init_image=pic, mask=m, inpaint_full_res=1), "inpaint_full_res"),
        (dict(init_image=pic, mask=m, denoising_strength=0.01), "Invalid denoising_strength"),
        (dict(init_image=b"junk", mask=m), "init_image"),
    ]
    for fill in (0, 2, 3, "original", True):
        cases.append((dict(init_image=pic, mask=m, inpainting_fill=fill), f"Invalid inpainting_fill {fill!r}: only 1 \\(original\\) is served"))
    for blur in (-1, 32.5, float("nan"), "x", True):
        cases.append((dict(init_image=pic, mask=m, mask_blur=blur), "Invalid mask_blur .* expected a number in \\[0, 32\\]"))
    for fields, text in cases:
        with pytest.raises(RuntimeError, match=text):
            inpaint.parse_inpaint(_req(**fields))
        with pytest.raises(RuntimeError, match=text):                  # ... and from the batch key, where a job meets them
            HipLcmWorker._job_key(_req(**fields))


def test_job_keys():
    pic, m = _pic(), _mask()
    plain = HipLcmWorker._job_key(_req())
    k1 = HipLcmWorker._job_key(_req(init_image=pic, mask=m))
    k2 = HipLcmWorker._job_key(_req(init_image=pic, mask=m, denoising_strength=0.5, mask_blur=0))
    assert k1 == plain + ("inpaint", 0.75, 4.0) and k2 == plain + ("inpaint", 0.5, 0.0)
    assert k1[6:] == (inpaint.KEY_TAG, 0.75, 4.0)
    assert inpaint.is_inpaint_key(k1) and not inpaint.is_inpaint_key(plain)
    # never a pass shared with image-to-image jobs, and the mask itself is per image
    i2i = HipLcmWorker._job_key(_req(init_image=pic))
    assert not inpaint.is_inpaint_key(i2i) and not img2img.is_img2img_key(k1) and i2i == plain + ("img2img", 0.75)
    assert HipLcmWorker._job_key(_req(init_image=pic, mask=255 - m, inpainting_mask_invert=True)) == k1
    assert HipLcmWorker._job_key(_req(init_images=[_png(pic)], mask_image=_png(m))) == k1
    for extra in (dict(enable_hr=True), dict(denoise_strength=0.5), dict(pass_number=2), dict(controlnet_image=pic)):
        with pytest.raises(RuntimeError, match="mask is not combined with"):
            HipLcmWorker._job_key(_req(init_image=pic, mask=m, **extra))
    for form in (dict(mask=m), dict(mask_image=m), dict(init_image=pic, mask=m)):
        with pytest.raises(RuntimeError, match="SDXL"):
            HipLcmSDXLWorker._job_key(_req(**form))
    assert HipLcmSDXLWorker._job_key(_req()) == plain
    with pytest.raises(RuntimeError, match="The combined original_steps x strength"):
        inpaint.check_schedule(LCMSchedule(), 4, 0.05)


# ---- the integer rules -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", [0.5, 1, 4, 12, 32])
def test_weight_table_sums_to_65536(sigma):
    r, w = mask_blur_weights(sigma)
    assert r == int(2.5 * sigma + 0.5) == ir.blur_radius(sigma) and len(w) == 2 * r + 1 and w.dtype == np.uint32
    assert int(w.astype(np.int64).sum()) == 65536
    assert np.array_equal(w.astype(np.int64), ir.blur_weights(sigma))       # the pipeline's table is the reference's
    assert np.array_equal(w, w[::-1]) and int(w.argmax()) == r and (w[:r] <= w[1:r + 1]).all()
    # a constant mask is a fixed point of both passes: 255 * 65536 + 32768 still fits uint32 and shifts back to 255
    for v in (0, 1, 127, 255):
        m = np.full((1, 5, 7), v, np.uint8)
        assert np.array_equal(ir.blur(m, sigma), m)


def test_no_blur_is_the_identity():
    assert mask_blur_weights(0)[0] == 0 and mask_blur_weights(0.1)[0] == 0
    m = _mask(9, 11)[None]
    assert np.array_equal(ir.blur(m, 0), m)


@pytest.mark.parametrize("sigma", [1, 4, 12])
def test_integer_blur_is_within_one_level_of_the_float64_gaussian(sigma):
    rng = np.random.default_rng(int(sigma))
    m = np.stack([(rng.random((40, 56)) < 0.5).astype(np.uint8) * 255, rng.integers(0, 256, (40, 56), dtype=np.uint8)])
    err = np.abs(ir.blur(m, sigma).astype(np.float64) - ir.blur_float64(m, sigma)).max()
    print(f"[inpaint] sigma {sigma}: max |integer blur - float64 Gaussian| = {err:.3f} levels")
    assert err <= 1.0
    # the edge is replicated: a mask that is white in its first column only keeps more than half of it at the border
    edge = np.zeros((1, 8, 8), np.uint8)
    edge[:, :, 0] = 255
    a = ir.blur(edge, sigma)
    assert a[0, 0, 0] >= 128 and (np.diff(a[0, 0].astype(int)) <= 0).all()


def test_latent_mask_tie_and_overlay_ends():
    a = np.zeros((1, 8, 16), np.uint8)
    a[0, :4, :8] = 255                                      # exactly 32 of 64 white: block sum 8160 = 64 * 255 / 2, the tie -> 1
    a[0, :4, 8:] = 255
    a[0, 3, 15] = 254                                       # one level under the tie -> 0
    assert ir.latent_mask(a).tolist() == [[[1, 0]]]
    gen, init = _pic(8, 16, 1)[None], _pic(8, 16, 2)[None]
    assert np.array_equal(ir.composite(gen, init, np.full((1, 8, 16), 255, np.uint8)), gen)
    assert np.array_equal(ir.composite(gen, init, np.zeros((1, 8, 16), np.uint8)), init)
    mid = ir.composite(gen, init, np.full((1, 8, 16), 128, np.uint8)).astype(int)
    lo, hi = np.minimum(gen, init).astype(int), np.maximum(gen, init).astype(int)
    assert (mid >= lo).all() and (mid <= hi).all()
