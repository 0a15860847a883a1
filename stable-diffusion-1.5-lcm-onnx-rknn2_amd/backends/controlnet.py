"""ControlNet requests: the ``controlnet_image`` / ``controlnet_conditioning_scale`` fields of a ``/generate`` request, read
with ``getattr`` like the refinement fields (the reference's schema has no such field yet: its ``prepare_controlnet_cond``,
backends/rknnlcm.py:693-697, has nothing behind it), and A1111's preprocessor fields ``controlnet_module`` ("none" | "canny" |
"invert") with ``controlnet_threshold_a`` / ``controlnet_threshold_b`` (Canny's low / high).  No GPU code here: the pass itself
is ``LcmHipPipeline.generate(..., control=(hints, scale), preprocess=...)``; the preprocessor runs on the device there
(csrc/canny.hip).
"""
from __future__ import annotations

import io
import math
import os

import numpy as np

MIN_SCALE, MAX_SCALE = 0.0, 2.0
KEY_TAG = "controlnet"
_MEMO = "_lcm_controlnet_parsed"
MODULES = ("none", "canny", "invert")                  # the preprocessors served; "none": the image is the finished map
CANNY_LOW, CANNY_HIGH = 100, 200                       # A1111's defaults of threshold_a / threshold_b
MIN_THRESHOLD, MAX_THRESHOLD = 1, 255                  # A1111's slider range


def is_control_key(key) -> bool:
    """A batch key of ControlNet jobs: the plain key + (KEY_TAG, conditioning scale) and, with a preprocessor, its tail
    ("canny", lo, hi) or ("invert",) (``key_preprocessor``)."""
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


def key_preprocessor(key):
    """The preprocessor tail of a ControlNet batch key: () | ("canny", lo, hi) | ("invert",)."""
    return tuple(key[8:])


def _module_name(req):
    """The request's ``controlnet_module`` as a lower-case name; None when absent, None or "none"."""
    m = getattr(req, "controlnet_module", None)
    if m is None:
        return None
    if not isinstance(m, str):
        return m                                           # not a name: an error where a module is read at all
    m = m.strip().lower()
    return None if m in ("", "none") else m


def _threshold(req, field, default):
    v = getattr(req, field, None)
    what = f"Invalid {field} {v!r}, expected a number in [{MIN_THRESHOLD}, {MAX_THRESHOLD}]"
    if v is None:
        return default
    if isinstance(v, (bool, str, bytes)):
        raise RuntimeError(what)
    try:
        f = float(v)
    except (TypeError, ValueError):
        raise RuntimeError(what)
    if not MIN_THRESHOLD <= f <= MAX_THRESHOLD:            # NaN fails both comparisons
        raise RuntimeError(what)
    return int(math.floor(f))


def _parse_module(req):
    """-> () | ("canny", lo, hi) | ("invert",) of a request that carries a hint.  lo <= hi are the floored thresholds."""
    name = _module_name(req)
    if name is None:
        return ()
    if name == "canny":
        lo = _threshold(req, "controlnet_threshold_a", CANNY_LOW)
        hi = _threshold(req, "controlnet_threshold_b", CANNY_HIGH)
        return ("canny", min(lo, hi), max(lo, hi))
    if name == "invert":
        return ("invert",)
    raise RuntimeError(f"Unknown controlnet_module {name!r}: this worker serves {', '.join(repr(m) for m in MODULES)}")


def _parse(req):
    img = getattr(req, "controlnet_image", None)
    if img is None:
        name = _module_name(req)
        if name in ("canny", "invert"):
            raise RuntimeError(f"controlnet_module {name!r} needs a controlnet_image to work on")
        return None                                        # stray module / threshold fields of a plain request are not read
    fields = tuple(getattr(req, f, None) for f in ("controlnet_conditioning_scale", "controlnet_module", "controlnet_threshold_a",
                                                   "controlnet_threshold_b"))
    memo = getattr(req, _MEMO, None)
    if memo is not None and memo[0] is img and _same(memo[1], fields):
        return memo[2]
    s = fields[0]
    try:
        s = 1.0 if s is None else float(s)
    except (TypeError, ValueError):
        raise RuntimeError(f"Invalid controlnet_conditioning_scale {s!r}, expected a number in [{MIN_SCALE}, {MAX_SCALE}]")
    if not MIN_SCALE <= s <= MAX_SCALE:                   # NaN fails both comparisons
        raise RuntimeError(f"Invalid controlnet_conditioning_scale {s!r}, expected a number in [{MIN_SCALE}, {MAX_SCALE}]")
    pre = _parse_module(req)
    hint = memo[2][1] if memo is not None and memo[0] is img else decode_hint(img)     # same image object: decoded once
    out = (round(s, 6), hint, pre)
    try:
        object.__setattr__(req, _MEMO, (img, fields, out))
    except Exception:
        pass
    return out


def _same(a, b) -> bool:
    """Field tuples equal value for value, type for type (1 and 1.0 and True are different requests to the memo)."""
    try:
        return all(type(x) is type(y) and bool(x == y) for x, y in zip(a, b))
    except Exception:
        return False


def parse_control(req):
    """-> None for a request without ``controlnet_image``, else (scale, hint uint8 [H, W, 3] at the hint's own size).
    Raises RuntimeError naming the offending field (the preprocessor fields included: ``parse_preprocessor``).  The decoded
    hint is remembered on the request object (the batch key is computed more than once per job: in its own call and while
    the pool's queue is drained); the memo holds the image object and the values of the other fields it was parsed with, so
    a changed scale, module or threshold is parsed again."""
    out = _parse(req)
    return None if out is None else out[:2]


def parse_preprocessor(req):
    """-> the preprocessor of a request with a hint: () for none (the image is the finished map), ("canny", lo, hi) with the
    floored thresholds lo <= hi, or ("invert",); None for a request without ``controlnet_image``.  ``controlnet_module`` is
    absent, None, "none", "canny" or "invert" (any case); "canny" reads ``controlnet_threshold_a`` (low, default 100) and
    ``controlnet_threshold_b`` (high, default 200), numbers in [1, 255].  ``processor_res`` / ``pixel_perfect`` are not read: the
    map is computed at the request's size.  RuntimeError for anything else, and for a module without an image."""
    out = _parse(req)
    return None if out is None else out[2]


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
