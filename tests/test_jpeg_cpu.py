"""The host half of the JPEG output (csrc/jpeg.cpp) through the C ABI, without a GPU: quantisation tables against PIL's, the
entropy layer against the test's own decoder (tests/jpeg_reference.py) -- it must be lossless --, determinism over the thread
count, PIL as a strict reader, and rate / distortion against PIL's own encoder on seeded photographs."""
import ctypes as C
import warnings

import numpy as np
import pytest

import jpeg_reference as R


@pytest.fixture(scope="module")
def L():
    import __graft_entry__
    __graft_entry__.build()
    from sdlcm_amd import lib
    return lib.load()


def encode(L, coefs, W, H, quality, threads=1, cap=None):
    coefs = np.ascontiguousarray(coefs, np.int16)
    assert coefs.nbytes == L.lcm_jpeg_coef_bytes(W, H)
    bound = int(L.lcm_jpeg_bound(W, H))
    cap = bound if cap is None else cap
    out = np.empty(max(cap, 1), np.uint8)
    n = C.c_longlong(-1)
    rc = L.lcm_jpeg_encode_coefs(coefs.ctypes.data, W, H, quality, threads, out.ctypes.data, cap, C.byref(n))
    if rc != 0:
        return rc, L.lcm_last_error()
    assert 0 < n.value <= bound
    return 0, out[:n.value].tobytes()


def strict_pil(data, W, H):
    """libjpeg reports corrupt data (bad Huffman codes, premature end, extraneous bytes) as warnings: all of them are errors."""
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        im = R.pil_decode(data)
    assert im.size == (W, H) and im.mode == "RGB"
    return np.asarray(im)


@pytest.mark.parametrize("q", [1, 25, 50, 75, 92, 95, 100])
def test_quant_tables_equal_pils(L, q):
    from PIL import Image
    import io
    tab = np.zeros(128, np.uint8)
    assert L.lcm_jpeg_quant_tables(q, tab.ctypes.data) == 0
    ql, qc = R.quant_tables(q)
    assert np.array_equal(tab[:64], ql) and np.array_equal(tab[64:], qc)
    img = R.photo(32, 16, 3)
    theirs = Image.open(io.BytesIO(R.pil_jpeg(img, q))).quantization
    rc, data = encode(L, R.round_coefs(R.front_end(img, q)), 32, 16, q)
    assert rc == 0
    ours = Image.open(io.BytesIO(data)).quantization
    assert sorted(ours) == sorted(theirs) == [0, 1]
    assert all(list(ours[k]) == list(theirs[k]) for k in theirs)
    # and PIL's DQT segments, read by the test's own parser, hold the values the library reports
    d = R.decode_entropy(R.pil_jpeg(img, q))
    assert np.array_equal(d["qtables"][0], tab[:64]) and np.array_equal(d["qtables"][1], tab[64:])


def test_quant_tables_reject_bad_quality(L):
    tab = np.zeros(128, np.uint8)
    for q in (0, 101, -3):
        assert L.lcm_jpeg_quant_tables(q, tab.ctypes.data) == -1 and b"quality" in L.lcm_last_error()
    assert L.lcm_jpeg_coef_bytes(17, 33) == 2 * 3 * 768 and L.lcm_jpeg_coef_bytes(0, 5) == 0 and L.lcm_jpeg_bound(5, 0) == 0


def _hard_coefs(W, H, seed):
    """Coefficients that exercise the coder rather than look like an image: photo-like blocks, DC at +-2047 (reached from a
    predictor of 0, the baseline DC difference range), AC at +-1023, runs of >= 16 zeros (ZRL, once, twice and three times),
    all-zero blocks, a block with only the last coefficient set, dense large values (long codes: many 0xFF bytes)."""
    rng = np.random.default_rng(seed)
    my, mx = -(-H // 16), -(-W // 16)
    c = np.rint(rng.laplace(0, 6, (my, mx, 6, 64)) * (rng.random((my, mx, 6, 64)) < 0.3)).astype(np.int64)
    c[..., 0] = np.rint(rng.normal(0, 200, (my, mx, 6)))
    flat = c.reshape(-1, 64)
    n = flat.shape[0]
    kinds = rng.integers(0, 12, n)
    for i in range(n):
        k = kinds[i]
        if k == 0:
            flat[i] = 0
        elif k == 1:
            flat[i] = 0
            flat[i, 63] = rng.choice([-1023, 1023, 1, -1])
        elif k == 2:
            flat[i, 1:] = 0
            flat[i, [17, 34, 63]] = [5, -1023, 1023]                    # runs of 16, 16 and 28 zeros
        elif k == 3:
            flat[i, 1:] = rng.choice([-1023, 1023, -512, 511, 1022], 63)
        elif k == 4:
            flat[i, 1:] = 0
            flat[i, 49] = -3                                            # 48 zeros: three ZRL
    c = np.clip(c, -1023, 1023)
    # DC extremes where the difference stays inside +-2047: reached from a predictor of 0 and followed by a DC of 0
    c[:, 0, :, 0] = [2047, 0, -2047, 0, -2047, 2047]
    if mx > 1:
        c[:, 1, 4:, 0] = 0
    return c.astype(np.int16)


@pytest.mark.parametrize("W,H", [(16, 16), (17, 33), (288, 240), (1000, 40), (40, 200)])
def test_entropy_layer_is_lossless(L, W, H):
    """(40, 200) has 13 MCU rows: RSTn wraps past 7.  (1000, 40) has 3 rows of 63 MCUs: a row is not a thread's share."""
    for q, coefs in ((75, R.round_coefs(R.front_end(R.photo(W, H, W + H), 75))), (100, _hard_coefs(W, H, W * 7 + H))):
        files = []
        for threads in (1, 2, 8):
            rc, data = encode(L, coefs, W, H, q, threads)
            assert rc == 0, data
            files.append(data)
        assert files[0] == files[1] == files[2]
        d = R.decode_entropy(files[0])
        my, mx = -(-H // 16), -(-W // 16)
        assert d["markers"] == ["SOI", "APP0", "DQT", "DQT", "SOF0", "DHT", "DHT", "DHT", "DHT", "DRI", "SOS", "EOI"]
        assert (d["width"], d["height"], d["sampling"], d["dri"]) == (W, H, [(2, 2), (1, 1), (1, 1)], mx)
        assert d["rst"] == [k % 8 for k in range(my - 1)]
        assert np.array_equal(d["coefs"], coefs)
        strict_pil(files[0], W, H)


def test_hard_coefficients_hold_what_they_claim(L):
    c = _hard_coefs(288, 240, 5)
    rc, data = encode(L, c, 288, 240, 100)
    assert rc == 0
    assert c[..., 0].max() == 2047 and c[..., 0].min() == -2047 and c[..., 1:].max() == 1023 and c[..., 1:].min() == -1023
    assert (np.abs(c).sum(-1) == 0).any()
    assert data.count(b"\xff\x00") > 100                                # stuffed bytes
    zr = c.reshape(-1, 64)[:, 1:] != 0
    assert any(np.diff(np.flatnonzero(np.r_[True, row])).max(initial=0) > 16 for row in zr)


def test_huffman_tables_are_the_standard_ones_pil_writes(L):
    img = R.photo(48, 32, 9)
    rc, data = encode(L, R.round_coefs(R.front_end(img, 75)), 48, 32, 75)
    assert rc == 0
    ours, theirs = R.decode_entropy(data)["dht"], R.decode_entropy(R.pil_jpeg(img, 75))["dht"]
    assert sorted(ours) == sorted(theirs) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    assert ours == theirs


def test_encode_argument_checks(L):
    c = np.zeros((1, 1, 6, 64), np.int16)
    bound = int(L.lcm_jpeg_bound(16, 16))
    rc, msg = encode(L, c, 16, 16, 75, cap=bound - 1)
    assert rc == -1 and b"output buffer" in msg
    rc, msg = encode(L, c, 16, 16, 0)
    assert rc == -1 and b"quality" in msg
    out = np.empty(bound, np.uint8)
    n = C.c_longlong(0)
    assert L.lcm_jpeg_encode_coefs(c.ctypes.data, 0, 16, 75, 1, out.ctypes.data, bound, C.byref(n)) == -1
    assert b"bad shape" in L.lcm_last_error()
    assert L.lcm_jpeg_encode_coefs(None, 16, 16, 75, 1, out.ctypes.data, bound, C.byref(n)) == -1
    # outside the baseline categories: refused, not written as a broken stream
    c[0, 0, 0, 5] = 1024
    rc, msg = encode(L, c, 16, 16, 75)
    assert rc == -1 and b"baseline range" in msg
    c[0, 0, 0, 5] = 0
    c[0, 0, 0, 0], c[0, 0, 1, 0] = 2047, -2047
    rc, msg = encode(L, c, 16, 16, 75)
    assert rc == -1 and b"baseline range" in msg


PHOTOS = [(512, 384, 11), (400, 300, 12), (333, 517, 13)]


@pytest.mark.parametrize("W,H,seed", PHOTOS)
@pytest.mark.parametrize("q", [40, 75, 92])
def test_quality_against_pil(L, W, H, seed, q):
    """Same tables, sampling and Huffman tables as PIL (libjpeg, 4:2:0, standard tables): what is left is libjpeg's integer DCT
    against a float one, and 2 bytes + padding + a DC restart per MCU row.  The yardstick is PIL's file, decoded by PIL.
    Bounds: the measured worst case over these nine cases plus the stated slack (jpeg_reference.X_DB / Y_PCT)."""
    img = R.photo(W, H, seed)
    theirs = R.pil_jpeg(img, q, subsampling=2)
    rc, ours = encode(L, R.round_coefs(R.front_end(img, q)), W, H, q, 8)
    assert rc == 0
    p_ours, p_theirs = R.psnr(strict_pil(ours, W, H), img), R.psnr(strict_pil(theirs, W, H), img)
    growth = 100.0 * (len(ours) - len(theirs)) / len(theirs)
    print(f"jpeg vs PIL {W}x{H} q={q}: PSNR ours {p_ours:.4f} PIL {p_theirs:.4f} (gap {p_theirs - p_ours:+.4f} dB), "
          f"size ours {len(ours)} PIL {len(theirs)} ({growth:+.3f} %)")
    assert p_theirs - p_ours <= R.X_DB
    assert growth <= R.Y_PCT
