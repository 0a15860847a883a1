"""CPU side of the JPEG *decoder* tests: a numpy restatement of the pixel arithmetic fixed in include/lcm_hip.h (dequantise,
"slow integer" inverse DCT, "fancy" chroma upsampling, 16-bit fixed point YCbCr -> RGB), written from ITU-T T.81 and the header
text, independently of the library.  The coefficient blocks come from the entropy decoder tests/jpeg_reference.py already
has (``decode_entropy`` handles every sampling and grayscale).

The yardstick for this file is PIL / libjpeg-turbo: tests/test_jpeg_decode_cpu.py::test_restatement_equals_pil asks for zero
differing bytes, and gets them for every class of file (4:4:4, 4:2:2, 4:2:0, gray; with and without restart markers;
optimised tables; widths down to 1).  No class keeps a difference, so no class is left to PIL on account of arithmetic."""
import numpy as np

import jpeg_reference as R

ZZ = R.ZZ

# round(x * 2**13)
F0_298, F0_390, F0_541, F0_765, F0_899, F1_175 = 2446, 3196, 4433, 6270, 7373, 9633
F1_501, F1_847, F1_961, F2_053, F2_562, F3_072 = 12299, 15137, 16069, 16819, 20995, 25172


def _wrap32(x):
    """int64 -> the value a 32-bit two's complement register holds (sums and products commute with it)."""
    return ((x + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def _pass(d, shift):
    """One 1-D pass of the slow integer inverse DCT along axis -2 of int64 [..., 8, n]; result (x + half) >> shift."""
    d0, d1, d2, d3, d4, d5, d6, d7 = [d[..., k, :] for k in range(8)]
    z1 = (d2 + d6) * F0_541
    e2 = z1 - d6 * F1_847
    e3 = z1 + d2 * F0_765
    e0 = (d0 + d4) << 13
    e1 = (d0 - d4) << 13
    a10, a13, a11, a12 = e0 + e3, e0 - e3, e1 + e2, e1 - e2
    t0, t1, t2, t3 = d7, d5, d3, d1
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * F1_175
    t0, t1, t2, t3 = t0 * F0_298, t1 * F2_053, t2 * F3_072, t3 * F1_501
    z1, z2 = -z1 * F0_899, -z2 * F2_562
    z3 = -z3 * F1_961 + z5
    z4 = -z4 * F0_390 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    outs = [a10 + t3, a11 + t2, a12 + t1, a13 + t0, a13 - t0, a12 - t1, a11 - t2, a10 - t3]
    return np.stack([_wrap32(x + (1 << (shift - 1))) >> shift for x in outs], axis=-2)


def idct_blocks(deq):
    """Dequantised coefficients int64 [..., 8, 8] (natural order, [v][u]) -> samples 0..255, int64 [..., 8, 8]."""
    w = _pass(deq, 11)                                   # columns, two extra bits kept
    w = _pass(np.swapaxes(w, -1, -2), 18)                # rows
    return np.clip(np.swapaxes(w, -1, -2) + 128, 0, 255)


def _shift_cols(r):
    left = np.concatenate([r[:, :1], r[:, :-1]], 1)
    right = np.concatenate([r[:, 1:], r[:, -1:]], 1)
    return left, right


def upsample(c, hf, vf):
    """A chroma component's own samples int64 [ch][cw] -> [ch * vf][cw * hf] by libjpeg's default rules."""
    ch, cw = c.shape
    if hf == 1 and vf == 1:
        return c
    if cw <= 2:                                          # too narrow for the triangle filter: replicated
        return np.repeat(np.repeat(c, vf, 0), hf, 1)
    if hf == 2 and vf == 1:
        left, right = _shift_cols(c)
        o = np.empty((ch, 2 * cw), np.int64)
        o[:, 0::2] = (3 * c + left + 1) >> 2
        o[:, 1::2] = (3 * c + right + 2) >> 2
        o[:, 0], o[:, -1] = c[:, 0], c[:, -1]
        return o
    assert hf == 2 and vf == 2
    up = np.concatenate([c[:1], c[:-1]], 0)
    down = np.concatenate([c[1:], c[-1:]], 0)
    v = np.empty((2 * ch, cw), np.int64)
    v[0::2] = 3 * c + up
    v[1::2] = 3 * c + down
    left, right = _shift_cols(v)
    o = np.empty((2 * ch, 2 * cw), np.int64)
    o[:, 0::2] = (3 * v + left + 8) >> 4
    o[:, 1::2] = (3 * v + right + 7) >> 4
    return o


def pixels(coefs, width, height, sampling, qtables):
    """coefs int16 [my][mx][blocks][64] (zigzag), sampling [(h, v)] per component, qtables [int64[64] natural] per component
    -> uint8 [height][width][3]."""
    hmax, vmax = max(h for h, _ in sampling), max(v for _, v in sampling)
    my, mx = coefs.shape[:2]
    nat = np.zeros(coefs.shape, np.int64)
    nat[..., ZZ] = coefs.astype(np.int64)
    planes, b = [], 0
    for (h, v), q in zip(sampling, qtables):
        if len(sampling) == 1:
            h = v = 1                                    # a single component is not interleaved: one block per MCU
        blk = nat[:, :, b:b + h * v] * np.asarray(q, np.int64)
        b += h * v
        px = idct_blocks(blk.reshape(my, mx, v, h, 8, 8))
        planes.append(px.transpose(0, 2, 4, 1, 3, 5).reshape(my * v * 8, mx * h * 8))
    y = planes[0][:height, :width]
    if len(planes) == 1:
        return np.stack([y] * 3, -1).astype(np.uint8)
    up = []
    for c, (h, v) in zip(planes[1:], sampling[1:]):
        ch, cw = -(-height * v // vmax), -(-width * h // hmax)
        up.append(upsample(c[:ch, :cw], hmax // h, vmax // v)[:height, :width])
    cb, cr = up[0] - 128, up[1] - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    bl = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, bl], -1), 0, 255).astype(np.uint8)


def component_tables(d):
    """The quantisation table of every component of a decode_entropy result: PIL writes table 0 for Y and table 1 for Cb, Cr
    (one table only at quality 100 with identical contents is still written as two)."""
    qt = d["qtables"]
    return [qt[0]] + [qt[1 if 1 in qt else 0]] * (len(d["sampling"]) - 1)


def decode(data):
    """JFIF bytes -> uint8 [H][W][3]."""
    d = R.decode_entropy(data)
    return pixels(d["coefs"], d["width"], d["height"], d["sampling"], component_tables(d))


def pil_rgb(data):
    import io
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def make_jpeg(rgb, quality, subsampling, **kw):
    """subsampling 0 / 1 / 2 = 4:4:4 / 4:2:2 / 4:2:0 (PIL's numbers), "gray" = mode L."""
    import io
    from PIL import Image
    im = Image.fromarray(rgb)
    buf = io.BytesIO()
    if subsampling == "gray":
        im.convert("L").save(buf, format="JPEG", quality=quality, **kw)
    else:
        im.save(buf, format="JPEG", quality=quality, subsampling=subsampling, **kw)
    return buf.getvalue()


SAMPLINGS = [0, 1, 2, "gray"]
# (width, height): odd sizes, one pixel, widths whose chroma is 1, 2 and 3 samples wide, and one at least 1536 wide
SIZES = [(1, 1), (3, 5), (4, 4), (5, 3), (17, 33), (333, 517), (1552, 24)]
VARIANTS = {"plain": {}, "rst_rows": dict(restart_marker_rows=1), "rst_blocks": dict(restart_marker_blocks=3), "optimize": dict(optimize=True)}


QUALITIES = (40, 75, 92, 100)


def case_files(sizes=SIZES, qualities=QUALITIES):
    """(name, file bytes) over sizes x qualities x samplings x variants, each file from its own seeded photograph."""
    for (w, h) in sizes:
        for q in qualities:
            for sub in SAMPLINGS:
                for vn, kw in VARIANTS.items():
                    yield f"{w}x{h} sub={sub} q={q} {vn}", make_jpeg(R.photo(w, h, 7 * w + h + q), q, sub, **kw)
