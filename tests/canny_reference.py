"""The Canny edge preprocessor of include/lcm_hip.h restated in numpy (no HIP, no torch): int32 Sobel gradients with
replicated borders, the channel of the largest L1 magnitude, non-maximum suppression in the 22.5 / 67.5 degree sectors with
15-bit fixed-point tangents, double threshold, and hysteresis by plain flood fill from the strong pixels.  The header's
text is the definition; this file follows it line by line and the GPU tests compare for equality."""
from __future__ import annotations

import math

import numpy as np

TG22 = 13573            # tan(22.5 deg) * 2^15, rounded


def thresholds(low, high):
    lo, hi = int(math.floor(low)), int(math.floor(high))
    return (hi, lo) if lo > hi else (lo, hi)


def gradients(rgb):
    """uint8 [H,W,3] -> (dx, dy, m) int32 [H,W]: the channel with the largest |dx| + |dy| (lowest index on a tie)."""
    p = np.pad(rgb.astype(np.int32), ((1, 1), (1, 1), (0, 0)), mode="edge")
    H, W = rgb.shape[:2]

    def s(dy, dx):
        return p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    gx = (s(-1, 1) - s(-1, -1)) + 2 * (s(0, 1) - s(0, -1)) + (s(1, 1) - s(1, -1))
    gy = (s(1, -1) - s(-1, -1)) + 2 * (s(1, 0) - s(-1, 0)) + (s(1, 1) - s(-1, 1))
    n = np.abs(gx) + np.abs(gy)
    c = np.argmax(n, axis=2)[..., None]                    # first occurrence: the lowest channel on a tie
    pick = lambda a: np.take_along_axis(a, c, axis=2)[..., 0]
    return pick(gx), pick(gy), pick(n)


def classes(rgb, lo, hi):
    """uint8 [H,W,3], integer thresholds lo <= hi -> uint8 [H,W]: 0 nothing, 1 weak, 2 strong."""
    dx, dy, m = gradients(rgb)
    H, W = m.shape
    mp = np.pad(m, 1)                                      # magnitudes outside the picture are 0

    def nb(oy, ox):
        return mp[1 + oy:1 + oy + H, 1 + ox:1 + ox + W]
    x = np.abs(dx)
    y = np.abs(dy) << 15
    t22 = x * TG22
    t67 = t22 + (x << 16)
    horiz = (m > nb(0, -1)) & (m >= nb(0, 1))
    vert = (m > nb(-1, 0)) & (m >= nb(1, 0))
    neg = (dx ^ dy) < 0                                    # s = -1: compare (y-1, x+1) and (y+1, x-1)
    diag = np.where(neg, (m > nb(-1, 1)) & (m > nb(1, -1)), (m > nb(-1, -1)) & (m > nb(1, 1)))
    peak = np.where(y < t22, horiz, np.where(y > t67, vert, diag))
    keep = peak & (m > lo)
    return np.where(keep, np.where(m > hi, 2, 1), 0).astype(np.uint8)


def link(cls):
    """uint8 [H,W] classes -> bool [H,W]: class > 0 and 8-connected through class > 0 pixels to a class-2 pixel.  Plain flood
    fill from the strong pixels with an explicit stack."""
    H, W = cls.shape
    out = cls == 2
    stack = list(zip(*np.nonzero(out)))
    while stack:
        y, x = stack.pop()
        for oy in (-1, 0, 1):
            for ox in (-1, 0, 1):
                v, u = y + oy, x + ox
                if 0 <= v < H and 0 <= u < W and cls[v, u] and not out[v, u]:
                    out[v, u] = True
                    stack.append((v, u))
    return out


def link_rgb(cls):
    """uint8 [H,W] or [B,H,W] classes -> uint8 [..., H, W, 3] edge picture (0 / 255)."""
    if cls.ndim == 3:
        return np.stack([link_rgb(c) for c in cls])
    return np.repeat((link(cls).astype(np.uint8) * 255)[..., None], 3, axis=2)


def canny(rgb, low=100, high=200):
    """uint8 [H,W,3] or [B,H,W,3] -> the edge picture, uint8 of the same shape, every pixel 0,0,0 or 255,255,255."""
    rgb = np.asarray(rgb)
    if rgb.ndim == 4:
        return np.stack([canny(r, low, high) for r in rgb])
    lo, hi = thresholds(low, high)
    return link_rgb(classes(rgb, lo, hi))


def growth_rounds(cls):
    """How many synchronous 8-neighbour growth rounds the hysteresis needs on this class map (what a bounded-iteration
    shortcut would have to reach)."""
    on = cls == 2
    rounds = 0
    while True:
        p = np.pad(on, 1)
        H, W = on.shape
        grown = on.copy()
        for oy in (0, 1, 2):
            for ox in (0, 1, 2):
                grown |= p[oy:oy + H, ox:ox + W]
        grown &= cls > 0
        if np.array_equal(grown, on):
            return rounds
        on, rounds = grown, rounds + 1


def smoothed_noise(h, w, seed, passes=5):
    """A smoothed-noise RGB picture: uniform noise box-filtered ``passes`` times and stretched back to 0..255."""
    g = np.random.default_rng(seed)
    a = g.random((h, w, 3))
    for _ in range(passes):
        p = np.pad(a, ((1, 1), (1, 1), (0, 0)), mode="edge")
        a = sum(p[i:i + h, j:j + w] for i in range(3) for j in range(3)) / 9.0
    lo, hi = a.min(), a.max()
    return np.clip((a - lo) / max(hi - lo, 1e-9) * 255.0 + 0.5, 0, 255).astype(np.uint8)


def spiral(h, w, strong=True):
    """A one-pixel-wide rectangular spiral of class 1 with one empty line between turns, walked from the corner (0, 0) inwards;
    the inner end is the only class-2 pixel (strong=False: none).  It is one chain: only its two ends have a single 8-neighbour."""
    cls = np.zeros((h, w), np.uint8)
    top, left, bottom, right = 0, 0, h - 1, w - 1
    y = x = 0
    cls[0, 0] = 1
    leg = 0
    while top <= bottom and left <= right:
        ty, tx = ((top, right), (bottom, right), (bottom, left), (top, left))[leg % 4]
        if (ty, tx) == (y, x):
            break
        while (y, x) != (ty, tx):
            y += (ty > y) - (ty < y)
            x += (tx > x) - (tx < x)
            cls[y, x] = 1
        if leg % 4 == 0:
            top += 2
        elif leg % 4 == 1:
            right -= 2
        elif leg % 4 == 2:
            bottom -= 2
        else:
            left += 2
        leg += 1
    if strong:
        cls[y, x] = 2
    return cls
