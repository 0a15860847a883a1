"""Variation seeds and seed-resize: the request fields every A1111 client sends with ``/sdapi/v1/txt2img`` (``subseed``,
``subseed_strength``, ``seed_resize_from_w``, ``seed_resize_from_h``), and what a latent walk from seed A to seed B is made of (N
requests that differ only in ``subseed_strength``).  No GPU code here: the blend and the paste are one launch of
``lcm_noise_variation_f32`` on the lane's stream (``LcmHipPipeline.generate(..., variation=)``; include/lcm_hip.h defines the
result).  Written after A1111's ``create_random_tensors`` / ``slerp`` as recalled; equality with A1111 is unverified.
"""
from __future__ import annotations

import math

import torch

MAX_SIDE = 256             # latent pixels per side of a seed-resize source (the kernel's domain)
NOT_COMBINED = "subseed / seed_resize_from is not combined with init_image"
SDXL_ERROR = "subseed / seed_resize_from: variation seeds are not served by the SDXL worker (SD1.5 and SD 2.x only)"


def _int_field(req, name):
    """A size field as an int; absent, None or anything that is no integer number counts as 0 (the field is then not in use)."""
    v = getattr(req, name, None)
    try:
        if v is None or isinstance(v, bool) or int(v) != v:
            return 0
        return int(v)
    except (TypeError, ValueError, OverflowError):
        return 0


def parse_variation(req, width, height):
    """-> None for a request without an active variation, else (subseed | None, t, hs, ws): the subseed (None: to be drawn, the
    request sent none or -1; also when t == 0, where it is never used), the strength, and the latent shape the noise is drawn at.
    A variation is active when ``subseed_strength`` > 0, or when both ``seed_resize_from_*`` are > 0 and name another latent shape
    than the request's (then (hs, ws) is that shape; otherwise the request's own).  Raises RuntimeError naming the value."""
    t = getattr(req, "subseed_strength", None)
    try:
        t = 0.0 if t is None else float(t)
    except (TypeError, ValueError):
        raise RuntimeError(f"Invalid subseed_strength {t!r}, expected a number in [0, 1]")
    if isinstance(getattr(req, "subseed_strength", None), bool) or not (math.isfinite(t) and 0.0 <= t <= 1.0):
        raise RuntimeError(f"Invalid subseed_strength {getattr(req, 'subseed_strength', None)!r}, expected a number in [0, 1]")
    h, w = int(height) // 8, int(width) // 8
    rw, rh = _int_field(req, "seed_resize_from_w"), _int_field(req, "seed_resize_from_h")
    hs, ws = h, w
    resized = rw > 0 and rh > 0 and (rh // 8, rw // 8) != (h, w)
    if resized:
        hs, ws = rh // 8, rw // 8
        if not (1 <= hs <= MAX_SIDE and 1 <= ws <= MAX_SIDE):
            raise RuntimeError(f"Invalid seed_resize_from {rw}x{rh}: a source of {ws}x{hs} latent pixels, expected 1..{MAX_SIDE} a side")
    if t <= 0.0 and not resized:
        return None
    sub = None
    if t > 0.0:
        sub = getattr(req, "subseed", None)
        if sub is not None:
            try:
                if isinstance(sub, bool) or int(sub) != sub:
                    raise ValueError
                sub = int(sub)
            except (TypeError, ValueError, OverflowError):
                raise RuntimeError(f"Invalid subseed {sub!r}, expected an integer (-1 or none: a random one)")
            if sub == -1:
                sub = None
    return sub, t, hs, ws


def resolve_subseed(subseed):
    """The seed policy of a request (backends/cuda_worker.py:210-213) for a subseed that was not sent."""
    return int(subseed) if subseed is not None else int(torch.randint(0, 100_000_000, (1,)).item())


class VariedItem(tuple):
    """A worker item ``(req, seed, noise, ...)`` of a request with an active variation: the tuple of its kind as it is, plus
    ``variation`` = (t, sub, base | None) for ``LcmHipPipeline.generate`` and ``ident`` = (subseed, t, hs, ws), the resolved
    variation (what ``refine.request_ident`` adds)."""
    variation = None
    ident = None


def attach(item, variation, ident):
    it = VariedItem(item)
    it.variation, it.ident = variation, ident
    return it
