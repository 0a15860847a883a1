"""The 8-bit Lanczos resampler of include/lcm_hip.h ("Lanczos resampler") restated in numpy: PIL's ``ImagingResample`` for 8-bit
pixels -- double-precision coefficient tables with libm's ``sin``, 22-bit fixed point, a horizontal pass into a rounded and
clipped uint8 intermediate, then the vertical pass -- plus the output window and the fits of ``resize_mode`` 1 and 2
(backends/fit.py).  tests/test_resize_cpu.py holds it against ``Image.resize(..., Image.LANCZOS)`` byte for byte; the library's
host tables and its device passes are then held against this file and against PIL itself.
"""
from __future__ import annotations

import math

import numpy as np

PRECISION_BITS = 22
SUPPORT = 3.0


def _sinc(x: float) -> float:
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x                                 # math.sin is libm's; numpy's vectorised sin may differ in the last bit


def lanczos(x: float) -> float:
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


def ksize(n_in: int, n_out: int) -> int:
    return int(math.ceil(SUPPORT * max(n_in / n_out, 1.0))) * 2 + 1


def tables(n_in: int, n_out: int, o0: int = 0, n: int = None):
    """The integer tables of an axis for the window [o0, o0 + n) of the n_out outputs (default: all): bounds int32 [n, 2]
    (first source index, number of taps) and coefficients int32 [n, ksize], zero behind the taps.  A window index outside
    [0, n_out) takes the nearest output's row (edge replication)."""
    n = n_out if n is None else n
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = SUPPORT * fs
    ks = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    bounds = np.zeros((n, 2), np.int32)
    kk = np.zeros((n, ks), np.int32)
    for i in range(n):
        xx = min(max(o0 + i, 0), n_out - 1)
        center = (xx + 0.5) * scale
        xmin = max(0, int(center - support + 0.5))
        xmax = min(n_in, int(center + support + 0.5))
        cnt = xmax - xmin
        w = [lanczos((x + xmin - center + 0.5) * ss) for x in range(cnt)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        bounds[i] = (xmin, cnt)
        for x, v in enumerate(w):
            kk[i, x] = int(v * (1 << PRECISION_BITS) + 0.5) if v >= 0 else int(v * (1 << PRECISION_BITS) - 0.5)
    return bounds, kk


def _pass(src: np.ndarray, bounds: np.ndarray, kk: np.ndarray) -> np.ndarray:
    """One pass along axis 0 of src uint8 [n_in, ...] -> uint8 [n, ...]."""
    out = np.empty((bounds.shape[0],) + src.shape[1:], np.uint8)
    s64 = src.astype(np.int64)
    for i, (xmin, cnt) in enumerate(bounds):
        acc = np.tensordot(kk[i, :cnt].astype(np.int64), s64[xmin:xmin + cnt], axes=(0, 0)) + (1 << (PRECISION_BITS - 1))
        assert np.abs(acc).max() < 2 ** 31                 # the 32-bit accumulator of the definition never wraps
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def resize(img: np.ndarray, width: int, height: int, window=None) -> np.ndarray:
    """img uint8 [H, W] or [H, W, C] -> its Lanczos fit to width x height, or the window (x0, y0, w, h) of that fit.  Window
    pixels outside the fit replicate its nearest edge pixel."""
    a = np.ascontiguousarray(img)
    sh, sw = a.shape[:2]
    x0, y0, w, h = window if window is not None else (0, 0, width, height)
    full = window is None or (x0, y0, w, h) == (0, 0, width, height)
    if sw != width or not full:
        bh, kh = tables(sw, width, x0, w)
        a = np.moveaxis(_pass(np.moveaxis(a, 1, 0), bh, kh), 0, 1)
    if sh != height or not full:
        bv, kv = tables(sh, height, y0, h)
        a = _pass(a, bv, kv)
    return np.ascontiguousarray(a)


def in_domain(sw: int, sh: int, channels: int, width: int, height: int) -> bool:
    """The domain of the device path (include/lcm_hip.h)."""
    return (channels in (1, 3) and 1 <= sw <= 8192 and 1 <= sh <= 8192 and 1 <= width <= 4096 and 1 <= height <= 4096
            and sh <= 100 * sw)


def mode_geometry(mode: int, sw: int, sh: int, width: int, height: int):
    """-> (fit width, fit height, window x0, window y0) of resize_mode 0, 1 (crop and resize) or 2 (resize and fill) for a
    sw x sh source and a width x height request; the window is width x height."""
    if mode == 0:
        return width, height, 0, 0
    r, rs = width / height, sw / sh
    if mode == 1:
        fw = width if r > rs else max(1, sw * height // sh)
        fh = height if r <= rs else max(1, sh * width // sw)
        return fw, fh, fw // 2 - width // 2, fh // 2 - height // 2
    fw = width if r < rs else max(1, sw * height // sh)
    fh = height if r >= rs else max(1, sh * width // sw)
    return fw, fh, -(width // 2 - fw // 2), -(height // 2 - fh // 2)


def fit(img: np.ndarray, width: int, height: int, mode: int = 0) -> np.ndarray:
    """The picture fitted to the request's size under ``resize_mode`` ``mode``."""
    sh, sw = img.shape[:2]
    fw, fh, x0, y0 = mode_geometry(mode, sw, sh, width, height)
    return resize(img, fw, fh, (x0, y0, width, height))
