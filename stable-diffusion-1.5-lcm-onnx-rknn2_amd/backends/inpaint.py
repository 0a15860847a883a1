"""Inpainting: the ``mask`` / ``mask_blur`` / ``inpainting_mask_invert`` fields every AUTOMATIC1111 client can post to
``/sdapi/v1/img2img`` next to ``init_images`` (``inpainting_fill`` and ``inpaint_full_res`` are checked: only "original" on the
whole picture is served), read with ``getattr`` like the image-to-image fields.  No GPU code here: the chain itself is
``LcmHipPipeline.generate_inpaint``.
"""
from __future__ import annotations

import io

import numpy as np

from . import img2img as _img2img
from .hires import _number
from .refine import check_schedule  # noqa: F401  (the one schedule check, under this module's name too)

MIN_BLUR, MAX_BLUR = 0, 32
DEFAULT_BLUR = 4                                           # A1111's mask_blur default
FILL_ORIGINAL = 1                                          # A1111's inpainting_fill: 0 fill, 1 original, 2 latent noise, 3 latent nothing
KEY_TAG = "inpaint"
_MEMO = "_lcm_inpaint_parsed"


def is_inpaint_key(key) -> bool:
    """A batch key of inpaint jobs: the plain key + (KEY_TAG, strength, mask_blur)."""
    return len(key) > 6 and key[6] == KEY_TAG


def _source(req):
    """The request's mask as sent (``mask``, alias ``mask_image``), or None."""
    m = getattr(req, "mask", None)
    return m if m is not None else getattr(req, "mask_image", None)


def decode_mask(mask) -> np.ndarray:
    """PNG / JPEG bytes, a base64 string (with or without a ``data:`` prefix), a PIL image or a uint8 array of shape H x W,
    H x W x 1, H x W x 3 or H x W x 4 -> uint8 [H, W], 8-bit gray (PIL "L"); white means repaint."""
    from PIL import Image
    if isinstance(mask, str):
        try:
            mask = _img2img._unbase64(mask)
        except RuntimeError as e:
            raise RuntimeError(str(e).replace("init_images", "mask"))
    if isinstance(mask, np.ndarray):
        ok = mask.dtype == np.uint8 and mask.ndim in (2, 3) and mask.shape[0] >= 1 and mask.shape[1] >= 1
        if ok and mask.ndim == 3:
            ok = mask.shape[2] in (1, 3, 4)
        if not ok:
            raise RuntimeError(f"Invalid mask: expected an H x W, H x W x 1, H x W x 3 or H x W x 4 uint8 array, got {mask.dtype} "
                               f"{tuple(mask.shape)}")
        if mask.ndim == 2 or mask.shape[2] == 1:
            return np.ascontiguousarray(mask.reshape(mask.shape[0], mask.shape[1]))
        mask = Image.fromarray(np.ascontiguousarray(mask), "RGB" if mask.shape[2] == 3 else "RGBA")
    if isinstance(mask, (bytes, bytearray, memoryview)):
        try:
            with Image.open(io.BytesIO(bytes(mask))) as im:
                return np.ascontiguousarray(np.asarray(im.convert("L"), dtype=np.uint8))
        except Exception as e:
            raise RuntimeError(f"Invalid mask: not a decodable PNG or JPEG ({type(e).__name__}: {e})")
    if hasattr(mask, "convert") and hasattr(mask, "size"):           # a PIL image
        try:
            return np.ascontiguousarray(np.asarray(mask.convert("L"), dtype=np.uint8))
        except Exception as e:
            raise RuntimeError(f"Invalid mask: {type(e).__name__}: {e}")
    raise RuntimeError("Invalid mask: expected PNG / JPEG bytes, a base64 string, a PIL image or a uint8 array, got "
                       f"{type(mask).__name__}")


def parse_inpaint(req):
    """-> None for a request without a mask (today's path, key and bytes, whatever its other inpainting fields say), else
    (strength, mask_blur, picture uint8 [H, W, 3] at its own size, mask uint8 [h, w] at its own size, inverted already when
    ``inpainting_mask_invert`` is truthy).  Raises RuntimeError naming the offending field.  The decoded mask is remembered on
    the request object (the batch key is computed more than once per job)."""
    src = _source(req)
    if src is None:
        return None
    i2i = _img2img.parse_img2img(req)                      # the picture's own errors and denoising_strength's come first
    if i2i is None:
        raise RuntimeError("mask was sent without init_image / init_images: inpainting needs the picture to repaint")
    invert = bool(getattr(req, "inpainting_mask_invert", None))
    memo = getattr(req, _MEMO, None)
    if memo is not None and memo[0] is src and memo[1] is i2i[1] and memo[2] == invert:
        return memo[3]
    fill = getattr(req, "inpainting_fill", None)
    if fill is not None and (isinstance(fill, bool) or fill != FILL_ORIGINAL):
        raise RuntimeError(f"Invalid inpainting_fill {fill!r}: only 1 (original) is served")
    if getattr(req, "inpaint_full_res", None):
        raise RuntimeError("inpaint_full_res: inpainting \"only masked\" is not served (the whole picture is the inpaint area)")
    blur = _number(req, "mask_blur", MIN_BLUR, MAX_BLUR, DEFAULT_BLUR)
    m = decode_mask(src)
    if invert:
        m = 255 - m
    out = (i2i[0], round(float(blur), 6), i2i[1], m)
    try:
        object.__setattr__(req, _MEMO, (src, i2i[1], invert, out))
    except Exception:
        pass
    return out


def fit_mask(mask: np.ndarray, width: int, height: int) -> np.ndarray:
    """The mask at the request's size: as is when it fits, else PIL LANCZOS in "L" to width x height."""
    if mask.shape[0] == height and mask.shape[1] == width:
        return mask
    from PIL import Image
    return np.ascontiguousarray(np.asarray(Image.fromarray(mask, "L").resize((int(width), int(height)), Image.LANCZOS), dtype=np.uint8))
