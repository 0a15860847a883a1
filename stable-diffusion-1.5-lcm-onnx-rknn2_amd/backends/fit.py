"""Fitting an upload to the request's size: the ``resize_mode`` field every AUTOMATIC1111 client can post to
``/sdapi/v1/img2img`` (0 "just resize", 1 "crop and resize", 2 "resize and fill"; 3, the latent upscale, is not served), read
with ``getattr`` like the other image-to-image fields, and the choice between the two resamplers that give the same bytes:
PIL's ``Image.resize(..., Image.LANCZOS)`` on the host (``fit_init`` / ``fit_mask`` / ``fit_hint``, the fallback and the
oracle) and the HIP Lanczos resampler on the lane's stream (csrc/resize.hip, include/lcm_hip.h).  No GPU code here: a picture
the device is to fit travels to the pipeline at its own size as a ``Pending`` (``LcmHipPipeline.generate_img2img``,
``generate_inpaint`` and ``generate(control=)`` accept one per request).

``LCM_RESIZE=hip|pil`` picks the resampler; ``pil`` is the host path throughout.  ``resize_mode`` applies to ``init_image`` and to
the ``mask`` alike, as in A1111; ControlNet hints are always "just resize".  The mode is no part of the batch key (the picture is
per image), and a request without a picture does not have it read.
"""
from __future__ import annotations

import os
from typing import NamedTuple

import numpy as np

JUST_RESIZE, CROP_AND_RESIZE, RESIZE_AND_FILL = 0, 1, 2
MODES = {JUST_RESIZE: "just resize", CROP_AND_RESIZE: "crop and resize", RESIZE_AND_FILL: "resize and fill"}
MAX_SOURCE, MAX_OUTPUT = 8192, 4096                        # the sides the device path takes (include/lcm_hip.h)
DEFAULT_BACKEND = "hip"                                    # measured: profiles/resize_mi355x.json (tools/resize_bench.py)


class Pending(NamedTuple):
    """A picture the device is to fit: ``pixels`` uint8 [h, w] or [h, w, 3] at their own size, resampled to fit_w x fit_h, of
    which the request takes the width x height window at (x0, y0); window positions outside the fit replicate its edge.
    ``shape`` and ``dtype`` are those of the fitted picture, as for an upload that was fitted on the host."""
    pixels: np.ndarray
    fit_w: int
    fit_h: int
    x0: int
    y0: int
    width: int
    height: int

    @property
    def shape(self):
        return (self.height, self.width) + tuple(self.pixels.shape[2:])

    @property
    def dtype(self):
        return self.pixels.dtype


def backend() -> str:
    """The resampler in force: "hip" or "pil" (LCM_RESIZE; anything else is an error naming the two)."""
    v = (os.environ.get("LCM_RESIZE") or DEFAULT_BACKEND).strip().lower()
    if v not in ("hip", "pil"):
        raise RuntimeError(f"Unknown LCM_RESIZE={v!r}, expected 'hip' or 'pil'")
    return v


def parse_resize_mode(req) -> int:
    """The request's ``resize_mode``: absent, None or 0 -> 0; 1; 2.  RuntimeError for anything else, naming the value and the
    modes served."""
    v = getattr(req, "resize_mode", None)
    if v is None:
        return JUST_RESIZE
    if not isinstance(v, (bool, str, bytes)):
        try:
            if v == int(v) and int(v) in MODES:
                return int(v)
        except (TypeError, ValueError, OverflowError):
            pass
    served = ", ".join(f"{k} ({name})" for k, name in MODES.items())
    if not isinstance(v, (bool, str, bytes)) and v == 3:
        raise RuntimeError(f"Invalid resize_mode {v!r}: the latent upscale is not served; this worker serves {served}")
    raise RuntimeError(f"Invalid resize_mode {v!r}: this worker serves {served}")


def geometry(mode: int, src_w: int, src_h: int, width: int, height: int):
    """-> (fit_w, fit_h, x0, y0): the picture is resampled to fit_w x fit_h and the request's width x height pixels are the
    window at (x0, y0) of that grid.  Mode 1 (A1111's images.resize_image, "crop and resize") covers the request and keeps the
    centre; mode 2 ("resize and fill") fits inside it, centred, and x0 / y0 are negative or zero: the bands outside the fit
    replicate its nearest edge row or column."""
    if mode == JUST_RESIZE:
        return width, height, 0, 0
    r, rs = width / height, src_w / src_h
    if mode == CROP_AND_RESIZE:
        fw = width if r > rs else max(1, src_w * height // src_h)
        fh = height if r <= rs else max(1, src_h * width // src_w)
        return fw, fh, fw // 2 - width // 2, fh // 2 - height // 2
    if mode == RESIZE_AND_FILL:
        fw = width if r < rs else max(1, src_w * height // src_h)
        fh = height if r >= rs else max(1, src_h * width // src_w)
        return fw, fh, -(width // 2 - fw // 2), -(height // 2 - fh // 2)
    raise RuntimeError(f"Invalid resize_mode {mode!r}")


def in_domain(src_w: int, src_h: int, channels: int, fit_w: int, fit_h: int) -> bool:
    """Does the device path take this fit with PIL's bytes?  1 or 3 channels, source sides 1..8192, output sides 1..4096, and
    no taller than 100 x its width: ``Image.resize`` runs the vertical pass first for height > 100 * width when the height
    shrinks, which the device path does not follow.  Anything outside goes to PIL, silently."""
    return (channels in (1, 3) and 1 <= src_w <= MAX_SOURCE and 1 <= src_h <= MAX_SOURCE and 1 <= fit_w <= MAX_OUTPUT
            and 1 <= fit_h <= MAX_OUTPUT and src_h <= 100 * src_w)


def fit_host(img: np.ndarray, width: int, height: int, mode: int = JUST_RESIZE) -> np.ndarray:
    """The picture (uint8 [h, w] or [h, w, 3]) at the request's size under ``mode``, on the host: as is when it fits, else PIL
    LANCZOS to the mode's grid, then the centred crop (mode 1) or the edge-replicated bands (mode 2)."""
    sh, sw = img.shape[:2]
    if sh == height and sw == width:
        return img
    fw, fh, x0, y0 = geometry(mode, sw, sh, width, height)
    a = img
    if (fw, fh) != (sw, sh):
        from PIL import Image
        a = np.asarray(Image.fromarray(img, "L" if img.ndim == 2 else "RGB").resize((int(fw), int(fh)), Image.LANCZOS), dtype=np.uint8)
    ys = np.clip(np.arange(height) + y0, 0, fh - 1)
    xs = np.clip(np.arange(width) + x0, 0, fw - 1)
    return np.ascontiguousarray(a[ys][:, xs])


def prepare(img: np.ndarray, width: int, height: int, mode: int = JUST_RESIZE, host=None):
    """What ``_prepare`` hands on for an upload: the picture itself when it has the request's size (today's path, no launch), a
    ``Pending`` when the device is to fit it (LCM_RESIZE=hip and inside the domain), else the host's fit -- by ``host(img,
    width, height)`` (``fit_init`` / ``fit_mask`` / ``fit_hint``) for "just resize", by ``fit_host`` for the other modes."""
    sh, sw = img.shape[:2]
    if sh == height and sw == width:
        return img
    if backend() == "hip":
        fw, fh, x0, y0 = geometry(mode, sw, sh, width, height)
        if in_domain(sw, sh, 1 if img.ndim == 2 else img.shape[2], fw, fh) and in_domain(1, 1, 1, width, height):
            return Pending(np.ascontiguousarray(img), fw, fh, x0, y0, int(width), int(height))
    if host is not None and mode == JUST_RESIZE:
        return host(img, width, height)
    return fit_host(img, width, height, mode)


def is_pending(x) -> bool:
    return isinstance(x, Pending)


def stack(pics):
    """The per-request pictures of a batch for the pipeline: one array when every one is at the request's size (today's
    call), else the list."""
    return list(pics) if any(is_pending(p) for p in pics) else np.stack(pics)
