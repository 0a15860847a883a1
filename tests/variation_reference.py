"""Variation seeds and seed-resize as include/lcm_hip.h ("variation seeds") and pipeline.py's RNG contract state them, restated
on the CPU: the per-column blend and the centred paste in numpy float64, the same blend in float32 with the kernel's operation
order, and the draws.  Nothing here imports the package: it is the other side of the comparison."""
import numpy as np
import torch

DOT_LIMIT = 0.9995


# ---- the blend -----------------------------------------------------------------------------------------------------------------
def column_dots(low, high):
    """low, high [4,hs,ws] -> (S_ll, S_hh, S_lh, d), each float64 [4,ws]: the sums down the height axis and the cosine; d is NaN
    where a column is zero."""
    lo, hi = np.asarray(low, np.float64), np.asarray(high, np.float64)
    s_ll, s_hh, s_lh = (lo * lo).sum(1), (hi * hi).sum(1), (lo * hi).sum(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        d = s_lh / np.sqrt(s_ll * s_hh)
    return s_ll, s_hh, s_lh, d


def sphere_columns(low, high):
    """bool [4,ws]: the columns that take the sphere branch (by float64)."""
    s_ll, s_hh, _, d = column_dots(low, high)
    with np.errstate(invalid="ignore"):
        return (s_ll > 0) & (s_hh > 0) & (np.abs(d) <= DOT_LIMIT)


def blend_fp64(low, high, t):
    """The blend at the source shape, float64 [4,hs,ws].  t == 0: low itself."""
    lo, hi = np.asarray(low, np.float64), np.asarray(high, np.float64)
    t = float(t)
    if t == 0.0:
        return lo.copy()
    _, _, _, d = column_dots(lo, hi)
    sph = sphere_columns(lo, hi)
    om = np.arccos(np.where(sph, d, 0.0))
    so = np.sin(om)
    a = np.where(sph, np.sin((1.0 - t) * om) / so, 1.0 - t)
    b = np.where(sph, np.sin(t * om) / so, t)
    return a[:, None, :] * lo + b[:, None, :] * hi


def _fma32(a, b, c):
    """fp32 fma(a, b, c) through float64: the product of two fp32 numbers is exact there; the sum is rounded to float64 and then to
    fp32 (a double rounding that differs from the fused operation in rare half-way cases only)."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def blend_fp32(low, high, t):
    """blend_fp64's arithmetic in float32 with the kernel's operation order (include/lcm_hip.h): sums by fma over y ascending,
    d = S_lh / sqrt(S_ll S_hh), w = acos(d), a = sin((1 - t) w) / sin(w), b = sin(t w) / sin(w), r = fma(a, low, b high)."""
    lo, hi = np.asarray(low, np.float32), np.asarray(high, np.float32)
    t = np.float32(t)
    if t == 0:
        return lo.copy()
    s_ll = np.zeros((lo.shape[0], lo.shape[2]), np.float32)
    s_hh, s_lh = s_ll.copy(), s_ll.copy()
    for y in range(lo.shape[1]):
        s_ll, s_hh, s_lh = _fma32(lo[:, y], lo[:, y], s_ll), _fma32(hi[:, y], hi[:, y], s_hh), _fma32(lo[:, y], hi[:, y], s_lh)
    with np.errstate(invalid="ignore", divide="ignore"):
        d = s_lh / np.sqrt(s_ll * s_hh)
        sph = (s_ll > 0) & (s_hh > 0) & (np.abs(d) <= np.float32(DOT_LIMIT))
    om = np.arccos(np.where(sph, d, np.float32(0)))
    so = np.sin(om)
    one = np.float32(1)
    a = np.where(sph, np.sin((one - t) * om) / so, one - t).astype(np.float32)
    b = np.where(sph, np.sin(t * om) / so, t).astype(np.float32)
    return _fma32(a[:, None, :], lo, b[:, None, :] * hi)


# ---- the paste -----------------------------------------------------------------------------------------------------------------
def window(n, ns):
    """One axis of the centred paste of a source of ns cells into a target of n -> (first source cell, first target cell, cells)."""
    d = (n - ns) // 2                                    # Python floor division, also for a negative difference
    return max(-d, 0), max(d, 0), min(n, ns)


def paste(x, r):
    """x [4,h,w] with r [4,hs,ws] centred into it (the axes independent); x outside the window stays."""
    out = np.array(x, copy=True)
    sy, ty, ch = window(x.shape[1], r.shape[1])
    sx, tx, cw = window(x.shape[2], r.shape[2])
    out[:, ty:ty + ch, tx:tx + cw] = r[:, sy:sy + ch, sx:sx + cw]
    return out


def vary_fp64(x, base, sub, t):
    """The initial latents of a request with a variation, float64 [4,h,w]: x [4,h,w] its own draw, base [4,hs,ws] | None (None: x is
    the base), sub [4,hs,ws] | None (t == 0), t the strength."""
    low = np.asarray(x if base is None else base, np.float64)
    r = low if float(t) == 0.0 else blend_fp64(low, sub, t)
    return paste(np.asarray(x, np.float64), r)


# ---- the draws -----------------------------------------------------------------------------------------------------------------
def _randn(seed, h, w, n=1):
    g = torch.Generator(device="cpu").manual_seed(int(seed))
    return [torch.randn((1, 4, h, w), generator=g, dtype=torch.float32) for _ in range(n)]


def draws(seed, subseed, h, w, hs, ws, sigma=1.0, n_extra=0):
    """-> (x, step noises, sub, base | None): G(seed) draws x [1,4,h,w] and then the step noises, as for a plain request; the
    variation's generators G'(subseed) and -- only for another source shape -- G''(seed) draw sub and base at [1,4,hs,ws]."""
    first = _randn(seed, h, w, 1 + n_extra)
    sub = _randn(subseed, hs, ws)[0] * sigma
    base = _randn(seed, hs, ws)[0] * sigma if (hs, ws) != (h, w) else None
    return first[0] * sigma, first[1:], sub, base


def seed_pair(h, w, start=0, limit=0.9, tries=120):
    """The first (seed, subseed) = (s, s + 1000), s >= start, whose draws at [4,h,w] have |d| <= limit in every column by float64
    -> (seed, subseed, low, high as float32 numpy [4,h,w]).  None such among ``tries`` is an error of the test, not a skip."""
    for s in range(start, start + tries):
        lo, hi = _randn(s, h, w)[0][0].numpy(), _randn(s + 1000, h, w)[0][0].numpy()
        d = column_dots(lo, hi)[3]
        if np.all(np.abs(d) <= limit):
            return s, s + 1000, lo, hi
    raise AssertionError(f"no seed pair with every column |d| <= {limit} at {h}x{w} among {tries}")
