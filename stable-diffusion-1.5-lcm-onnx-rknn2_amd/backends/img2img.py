"""Image-to-image: the ``init_image`` / ``denoising_strength`` fields of a request (A1111's ``/sdapi/v1/img2img`` sends
``init_images`` and ``denoising_strength``; the reference's only image-conditioned route, ``/v1/comfy/jobs``, hands an upload plus
``denoise`` to an external node), read with ``getattr`` like the refinement, ControlNet and hires fields.  No GPU code here: the
chain itself is ``LcmHipPipeline.generate_img2img``.
"""
from __future__ import annotations

import base64
import binascii

import numpy as np

from . import controlnet as _controlnet
from .hires import _number
from .refine import check_schedule  # noqa: F401  (the one schedule check, under this module's name too)

MIN_STRENGTH, MAX_STRENGTH = 0.05, 1.0
DEFAULT_STRENGTH = 0.75                                    # A1111's img2img default
KEY_TAG = "img2img"
_MEMO = "_lcm_img2img_parsed"


def is_img2img_key(key) -> bool:
    """A batch key of image-to-image jobs: the plain key + (KEY_TAG, strength)."""
    return len(key) > 6 and key[6] == KEY_TAG


def _source(req):
    """The request's picture as sent -> (the object it was sent as, is it a base64 string), or None for a request without one:
    ``init_image``, or the single entry of ``init_images`` (bytes or a base64 string, with or without a ``data:`` prefix)."""
    img = getattr(req, "init_image", None)
    if img is not None:
        return img, False
    imgs = getattr(req, "init_images", None)
    if imgs is None:
        return None
    if isinstance(imgs, (str, bytes, bytearray, memoryview)) or not hasattr(imgs, "__len__"):
        raise RuntimeError(f"Invalid init_images: expected a list with exactly one picture, got {type(imgs).__name__}")
    if len(imgs) != 1:
        raise RuntimeError(f"Invalid init_images: expected exactly one picture, got {len(imgs)}")
    return imgs[0], isinstance(imgs[0], str)


def _unbase64(one: str) -> bytes:
    txt = one.split(",", 1)[1] if one.startswith("data:") and "," in one else one
    try:
        return base64.b64decode(txt, validate=True)
    except (binascii.Error, ValueError) as e:
        raise RuntimeError(f"Invalid init_images: not base64 ({e})")


def decode_init(img) -> np.ndarray:
    """PNG / JPEG bytes, a PIL image or an H x W x 3 uint8 array -> uint8 [H, W, 3]; a JPEG goes through the HIP decoder when
    LCM_JPEG_DECODER is on (backends/controlnet.decode_hint serves both kinds of upload)."""
    try:
        return _controlnet.decode_hint(img)
    except RuntimeError as e:
        raise RuntimeError(str(e).replace("controlnet_image", "init_image"))


def parse_img2img(req):
    """-> None for a request without a picture (whatever its ``denoising_strength`` says: today's path, key and bytes), else
    (strength, picture uint8 [H, W, 3] at its own size).  Raises RuntimeError naming the offending field.  The decoded picture is
    remembered on the request object (the batch key is computed more than once per job)."""
    src = _source(req)
    if src is None:
        return None
    src, b64 = src
    memo = getattr(req, _MEMO, None)
    if memo is not None and memo[0] is src:                # keyed on the object as sent: a base64 entry is decoded once too
        return memo[1]
    s = _number(req, "denoising_strength", MIN_STRENGTH, MAX_STRENGTH, DEFAULT_STRENGTH)
    out = (round(s, 6), decode_init(_unbase64(src) if b64 else src))
    try:
        object.__setattr__(req, _MEMO, (src, out))
    except Exception:
        pass
    return out


def fit_init(img: np.ndarray, width: int, height: int) -> np.ndarray:
    """The picture at the request's size: as is when it fits, else PIL LANCZOS in RGB (backends/controlnet.fit_hint)."""
    return _controlnet.fit_hint(img, width, height)
