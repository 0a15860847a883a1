"""ControlNet requests: the ``controlnet_image`` / ``controlnet_conditioning_scale`` fields of a ``/generate`` request, read
with ``getattr`` like the refinement fields (the reference's schema has no such field yet: its ``prepare_controlnet_cond``,
backends/rknnlcm.py:693-697, has nothing behind it).  No GPU code here: the pass itself is
``LcmHipPipeline.generate(..., control=(hints, scale))``.
"""
from __future__ import annotations

import io
import os

import numpy as np

MIN_SCALE, MAX_SCALE = 0.0, 2.0
KEY_TAG = "controlnet"
_MEMO = "_lcm_controlnet_parsed"


def is_control_key(key) -> bool:
    """A batch key of ControlNet jobs: the plain key + (KEY_TAG, conditioning scale)."""
    return len(key) > 6 and key[6] == KEY_TAG


def decode_hint(img) -> np.ndarray:
    """PNG / JPEG bytes, a PIL image or an H x W x 3 uint8 array -> uint8 [H, W, 3] (RGB).  RuntimeError if it is none of them.
    A JPEG goes through the HIP decoder when LCM_JPEG_DECODER is on (backends/hip_worker.decode_jpeg), else through PIL."""
    if isinstance(img, np.ndarray):
        if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3 or img.shape[0] < 1 or img.shape[1] < 1:
            raise RuntimeError(f"Invalid controlnet_image: expected an H x W x 3 uint8 array, got {img.dtype} {tuple(img.shape)}")
        return np.ascontiguousarray(img)
    if isinstance(img, (bytes, bytearray, memoryview)):
        data = bytes(img)
        if data[:2] == b"\xff\xd8" and os.environ.get("LCM_JPEG_DECODER", "0").lower() in ("1", "true", "yes", "on", "hip"):
            try:
                from .hip_worker import decode_jpeg
                out = np.asarray(decode_jpeg(data))
                if out.ndim == 3 and out.shape[2] == 3 and out.dtype == np.uint8:
                    return np.ascontiguousarray(out)
            except Exception:
                pass                                   # a JPEG the HIP decoder leaves to PIL (progressive, CMYK ...), or a broken one
        try:
            from PIL import Image
            with Image.open(io.BytesIO(data)) as im:
                return np.ascontiguousarray(np.asarray(im.convert("RGB"), dtype=np.uint8))
        except Exception as e:
            raise RuntimeError(f"Invalid controlnet_image: not a decodable PNG or JPEG ({type(e).__name__}: {e})")
    if hasattr(img, "convert") and hasattr(img, "size"):           # a PIL image
        try:
            return np.ascontiguousarray(np.asarray(img.convert("RGB"), dtype=np.uint8))
        except Exception as e:
            raise RuntimeError(f"Invalid controlnet_image: {type(e).__name__}: {e}")
    raise RuntimeError(f"Invalid controlnet_image: expected PNG / JPEG bytes, a PIL image or an H x W x 3 uint8 array, got {type(img).__name__}")


def parse_control(req):
    """-> None for a request without ``controlnet_image``, else (scale, hint uint8 [H, W, 3] at the hint's own size).
    Raises RuntimeError naming the offending field.  The decoded hint is remembered on the request object (the batch key is
    computed more than once per job: in its own call and while the pool's queue is drained)."""
    img = getattr(req, "controlnet_image", None)
    if img is None:
        return None
    memo = getattr(req, _MEMO, None)
    if memo is not None and memo[0] is img:
        return memo[1]
    s = getattr(req, "controlnet_conditioning_scale", None)
    try:
        s = 1.0 if s is None else float(s)
    except (TypeError, ValueError):
        raise RuntimeError(f"Invalid controlnet_conditioning_scale {s!r}, expected a number in [{MIN_SCALE}, {MAX_SCALE}]")
    if not MIN_SCALE <= s <= MAX_SCALE:                   # NaN fails both comparisons
        raise RuntimeError(f"Invalid controlnet_conditioning_scale {s!r}, expected a number in [{MIN_SCALE}, {MAX_SCALE}]")
    out = (round(s, 6), decode_hint(img))
    try:
        object.__setattr__(req, _MEMO, (img, out))
    except Exception:
        pass
    return out


def fit_hint(hint: np.ndarray, width: int, height: int) -> np.ndarray:
    """The hint at the request's size: as is when it fits, else resized on the host with PIL LANCZOS in RGB, as the reference's
    prepare_controlnet_cond does -- to width x height (the reference hands PIL (height, width), which agrees for squares only)."""
    if hint.shape[0] == height and hint.shape[1] == width:
        return hint
    from PIL import Image
    return np.ascontiguousarray(np.asarray(Image.fromarray(hint, "RGB").resize((int(width), int(height)), Image.LANCZOS), dtype=np.uint8))


def load_controlnet_source(src: str, unet_cfg: dict, synthetic_model: bool):
    """``CONTROLNET=<dir or file>`` / ``synthetic`` -> (state dict, config)."""
    from .. import weights
    if src == "synthetic":
        if not synthetic_model:
            raise RuntimeError("CONTROLNET=synthetic goes with MODEL=synthetic* only")
        cfg = weights.controlnet_config(unet_cfg)
        return weights.synthetic_controlnet(cfg), cfg
    if not os.path.exists(src):
        raise RuntimeError(f"CONTROLNET={src}: no such file or directory")
    return weights.load_controlnet(src)
