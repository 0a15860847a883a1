"""Hires fix: the high-resolution fields every AUTOMATIC1111 client can send with ``/sdapi/v1/txt2img`` (``enable_hr``,
``hr_scale``, ``hr_resize_x`` / ``hr_resize_y``, ``hr_second_pass_steps``, ``denoising_strength``, ``hr_upscaler``), read from the
request with ``getattr`` like the refinement fields (the reference's ``A1111Txt2ImgRequest``, server/compat_endpoints.py, drops
them).  No GPU code here: the chain itself is ``LcmHipPipeline.generate(..., hires=)``.
"""
from __future__ import annotations

from ..lib import UPSCALE_MODES
from .refine import check_schedule  # noqa: F401  (the one schedule check, under this module's name too)

MIN_STRENGTH, MAX_STRENGTH = 0.05, 1.0
MIN_SCALE, MAX_SCALE = 1.0, 4.0
DEFAULT_SCALE, DEFAULT_STRENGTH, DEFAULT_UPSCALER = 2.0, 0.7, "Latent"
KEY_TAG = "hires"


def is_hires_key(key) -> bool:
    """A batch key of hires jobs: the plain key + (KEY_TAG, target width, target height, hr_steps, strength, mode)."""
    return len(key) > 6 and key[6] == KEY_TAG


def _number(req, name, lo, hi, default):
    v = getattr(req, name, None)
    if v is None:
        return default
    try:
        if isinstance(v, bool):
            raise ValueError
        f = float(v)
    except (TypeError, ValueError):
        raise RuntimeError(f"Invalid {name} {v!r}, expected a number in [{lo}, {hi}]")
    if not lo <= f <= hi:                                  # NaN fails both comparisons
        raise RuntimeError(f"Invalid {name} {v!r}, expected a number in [{lo}, {hi}]")
    return f


def _integer(req, name, what):
    v = getattr(req, name, None)
    if v is None:
        return 0
    try:
        if isinstance(v, bool) or int(v) != v:
            raise ValueError
        v = int(v)
    except (TypeError, ValueError):
        raise RuntimeError(f"Invalid {name} {v!r}, expected {what}")
    if v < 0:
        raise RuntimeError(f"Invalid {name} {v!r}, expected {what}")
    return v


def parse_hires(req, width: int, height: int, steps: int):
    """-> None for a request without ``enable_hr`` true (whatever its other hr_* fields say: today's path, key and bytes), else
    (target width, target height, hr_steps, strength, mode).  Raises RuntimeError naming the offending field."""
    if not getattr(req, "enable_hr", None):
        return None
    rx = _integer(req, "hr_resize_x", "0 or a multiple of 8 between the base size and 4x it")
    ry = _integer(req, "hr_resize_y", "0 or a multiple of 8 between the base size and 4x it")
    if rx > 0 and ry > 0:                                  # both given: they override hr_scale
        for name, v, base in (("hr_resize_x", rx, width), ("hr_resize_y", ry, height)):
            if v % 8 or not base <= v <= 4 * base:
                raise RuntimeError(f"Invalid {name} {v}, expected a multiple of 8 in [{base}, {4 * base}] (the base size to 4x it)")
        tw, th = rx, ry
    else:
        scale = _number(req, "hr_scale", MIN_SCALE, MAX_SCALE, DEFAULT_SCALE)
        tw, th = int(width * scale) // 8 * 8, int(height * scale) // 8 * 8            # A1111's rule
    strength = _number(req, "denoising_strength", MIN_STRENGTH, MAX_STRENGTH, DEFAULT_STRENGTH)
    hr_steps = _integer(req, "hr_second_pass_steps", "0 (the first pass's step count) or a positive integer") or int(steps)
    up = getattr(req, "hr_upscaler", None)
    up = DEFAULT_UPSCALER if up is None else up
    if not isinstance(up, str) or up not in UPSCALE_MODES:
        raise RuntimeError(f"Invalid hr_upscaler {up!r}: the latent upscalers served are " + ", ".join(repr(k) for k in UPSCALE_MODES))
    return (tw, th, hr_steps, round(strength, 6), UPSCALE_MODES[up])
