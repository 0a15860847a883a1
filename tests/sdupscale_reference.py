"""SD upscale on the CPU: the tile geometry (written after A1111's images.split_grid as recalled), A1111's combine_grid in its own
paste order with PIL (``combine_pil``) and the integer definition of include/lcm_hip.h (``combine_int``).  The two combines are
byte-equal at the geometries of tests/test_sdupscale_cpu.py (Pillow 12.2.0); equality with A1111 itself is unverified."""
import math

import numpy as np

# (W, H, tile_w, tile_h, overlap): two-deep cover, exact fits, one tile, one pixel more than a tile, unequal tile sides, three-deep
# cover (104 = 0 / 20 / 40 + 64), and the served size (9 tiles of 512 x 512)
GEOMETRIES = [(160, 112, 64, 64, 16), (128, 128, 64, 64, 16), (200, 72, 64, 64, 24), (136, 136, 64, 64, 8), (64, 64, 64, 64, 16),
              (65, 130, 64, 64, 16), (192, 96, 64, 48, 32), (104, 88, 64, 64, 40), (1024, 1024, 512, 512, 64)]


def axis(size, tile, overlap):
    """Tile offsets of one axis, in Python floats; the last one is size - tile outright ((n - 1) * d may round to just below it:
    size 77, tile 16, overlap 7)."""
    n = math.ceil((size - overlap) / (tile - overlap))
    d = (size - tile) / (n - 1) if n > 1 else 0
    out = []
    for k in range(n):
        v = int(k * d)
        if v + tile >= size or k == n - 1:
            v = size - tile
        out.append(v)
    return out


def geometry(W, H, tile_w, tile_h, overlap):
    """-> (xs, ys); tile k = r * len(xs) + c lies at (xs[c], ys[r])."""
    return axis(W, tile_w, overlap), axis(H, tile_h, overlap)


def facts(v, size, tile, overlap):
    """The four facts the combine launch relies on."""
    return (v[0] == 0 and all(x > 0 for x in v[1:]) and all(b > a for a, b in zip(v, v[1:]))
            and all(b - a <= tile - overlap for a, b in zip(v, v[1:])) and v[-1] + tile == size)


def random_tiles(W, H, tile_w, tile_h, overlap, seed=0):
    xs, ys = geometry(W, H, tile_w, tile_h, overlap)
    return np.random.default_rng(seed).integers(0, 256, (len(xs) * len(ys), tile_h, tile_w, 3), dtype=np.uint8)


def combine_pil(tiles, W, H, overlap, xs, ys):
    """A1111's combine_grid: rows are pasted left to right into a row picture (the first tile whole, every other one's first
    ``overlap`` columns through a linear-gradient "L" mask, the rest plainly), the row pictures top to bottom in the same way.
    Masks are uint8(float32(i) * 255 / overlap).  tiles uint8 [T, tile_h, tile_w, 3] -> uint8 [H, W, 3]."""
    from PIL import Image
    T, th, tw, _ = tiles.shape
    cols = len(xs)

    def mask(a):
        return Image.fromarray((a * 255 / overlap).astype(np.uint8), "L")
    if overlap > 0:
        mask_w = mask(np.arange(overlap, dtype=np.float32).reshape(1, overlap).repeat(th, axis=0))
        mask_h = mask(np.arange(overlap, dtype=np.float32).reshape(overlap, 1).repeat(W, axis=1))
    combined = Image.new("RGB", (W, H))
    for r, y in enumerate(ys):
        row = Image.new("RGB", (W, th))
        for c, x in enumerate(xs):
            tile = Image.fromarray(tiles[r * cols + c], "RGB")
            if x == 0:
                row.paste(tile, (0, 0))
                continue
            if overlap > 0:
                row.paste(tile.crop((0, 0, overlap, th)), (x, 0), mask=mask_w)
            row.paste(tile.crop((overlap, 0, tw, th)), (x + overlap, 0))
        if y == 0:
            combined.paste(row, (0, 0))
            continue
        if overlap > 0:
            combined.paste(row.crop((0, 0, W, overlap)), (0, y), mask=mask_h)
        combined.paste(row.crop((0, overlap, W, th)), (0, y + overlap))
    return np.asarray(combined, dtype=np.uint8)


def _div255(a):
    a = a + 128
    return (a + (a >> 8)) >> 8


def _blend(p, t, m):
    return _div255(p * (255 - m) + t * m)


def combine_int(tiles, W, H, overlap, xs, ys):
    """The integer definition of include/lcm_hip.h (tile grid combine), literally: fold over the columns into row pictures, fold
    over the rows into the output.  int32 arithmetic on whole column / row slabs."""
    T, th, tw, _ = tiles.shape
    cols = len(xs)
    t32 = tiles.astype(np.int32)
    out = np.zeros((H, W, 3), np.int32)
    m_w = (255 * np.arange(overlap, dtype=np.int32)) // overlap if overlap > 0 else None
    for r, y in enumerate(ys):
        row = np.zeros((th, W, 3), np.int32)
        for c, x in enumerate(xs):
            t = t32[r * cols + c]
            if c == 0:
                row[:, :tw] = t
                continue
            if overlap > 0:
                m = m_w[None, :, None]
                row[:, x:x + overlap] = _blend(row[:, x:x + overlap], t[:, :overlap], m)
            row[:, x + overlap:x + tw] = t[:, overlap:]
        if r == 0:
            out[:th] = row
            continue
        if overlap > 0:
            m = m_w[:, None, None]
            out[y:y + overlap] = _blend(out[y:y + overlap], row[:overlap], m)
        out[y + overlap:y + th] = row[overlap:]
    return out.astype(np.uint8)
