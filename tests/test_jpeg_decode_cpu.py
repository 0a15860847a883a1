"""The host half of the JPEG input (csrc/jpeg_dec.cpp) through the C ABI, without a GPU, and the yardstick of the device half:
the numpy restatement of the pixel arithmetic (tests/jpeg_decode_reference.py) against PIL / libjpeg-turbo -- zero differing
bytes --, the library's coefficient blocks against the test's own entropy decoder for every thread count, the round trip
through the library's encoder, every unsupported kind of file, and truncated / damaged files."""
import ctypes as C
import io

import numpy as np
import pytest

import jpeg_decode_reference as D
import jpeg_reference as R

EINVAL, EUNSUPPORTED = -1, -3


@pytest.fixture(scope="module")
def L():
    import __graft_entry__
    __graft_entry__.build()
    from sdlcm_amd import lib
    return lib.load()


@pytest.fixture(scope="module")
def files():
    return list(D.case_files())


def info_of(L, data):
    from sdlcm_amd import lib
    info = lib.JpegInfo()
    rc = L.lcm_jpeg_dec_info(data, len(data), C.byref(info))
    return rc, info


def dec_coefs(L, data, threads=1):
    """-> (rc, int16 [my][mx][blocks][64] | error text).  The buffer starts as 0x7F7F: every value must be written."""
    rc, info = info_of(L, data)
    if rc != 0:
        return rc, L.lcm_last_error()
    out = np.full(info.coefs_bytes // 2, 0x7F7F, np.int16)
    rc = L.lcm_jpeg_dec_coefs(data, len(data), threads, out.ctypes.data, out.nbytes)
    if rc != 0:
        return rc, L.lcm_last_error()
    return 0, out.reshape(info.mcus_y, info.mcus_x, info.blocks_per_mcu, 64)


def test_restatement_equals_pil(files):
    """The yardstick itself.  Both sides are deterministic integer procedures: the target is zero differing bytes."""
    assert len(files) == len(D.SIZES) * len(D.QUALITIES) * len(D.SAMPLINGS) * len(D.VARIANTS)
    worst = []
    for name, data in files:
        mine, pil = D.decode(data), D.pil_rgb(data)
        assert mine.shape == pil.shape, name
        n = int((mine != pil).sum())
        if n:
            worst.append((name, n, int(np.abs(mine.astype(int) - pil).max())))
    print(f"restatement vs PIL: {len(files)} files, {len(worst)} with differing bytes {worst[:5]}")
    assert not worst


def test_info_reports_what_the_file_holds(L, files):
    for name, data in files:
        rc, info = info_of(L, data)
        assert rc == 0, (name, L.lcm_last_error())
        d = R.decode_entropy(data)
        samp = d["sampling"]
        assert (info.width, info.height, info.ncomp) == (d["width"], d["height"], len(samp)), name
        assert info.sampling == ({(1, 1): 0, (2, 1): 1, (2, 2): 2}[samp[0]] if len(samp) == 3 else 0), name
        assert info.restart_interval == d["dri"], name
        assert (info.mcus_y, info.mcus_x, info.blocks_per_mcu) == d["coefs"].shape[:3], name
        assert info.coefs_bytes == d["coefs"].nbytes and info.work_bytes == d["coefs"].size, name
        qt = np.frombuffer(bytes(info.qt), np.uint8).reshape(3, 64)
        for c, t in enumerate(D.component_tables(d)):
            assert np.array_equal(qt[c], t), name


def test_blocks_equal_the_python_decoder_for_every_thread_count(L, files):
    for name, data in files:
        want = R.decode_entropy(data)["coefs"]
        for threads in (1, 3, 8):
            rc, got = dec_coefs(L, data, threads)
            assert rc == 0, (name, threads, got)
            assert np.array_equal(got, want), (name, threads)


def _encode(L, coefs, W, H, q, threads=8):
    coefs = np.ascontiguousarray(coefs, np.int16)
    cap = int(L.lcm_jpeg_bound(W, H))
    out = np.empty(cap, np.uint8)
    n = C.c_longlong(0)
    assert L.lcm_jpeg_encode_coefs(coefs.ctypes.data, W, H, q, threads, out.ctypes.data, cap, C.byref(n)) == 0, L.lcm_last_error()
    return out[:n.value].tobytes()


@pytest.mark.parametrize("W,H", [(16, 16), (17, 33), (288, 240), (1000, 40), (40, 200)])
def test_round_trip_through_the_librarys_encoder(L, W, H):
    """Files the library's own encoder wrote (one restart interval per MCU row): dec_coefs gives back the coefficients, for
    every thread count, and encoding them again gives back the file.  Photo-like blocks and the coder's extremes."""
    rng = np.random.default_rng(W * 3 + H)
    my, mx = -(-H // 16), -(-W // 16)
    hard = np.clip(np.rint(rng.laplace(0, 40, (my, mx, 6, 64)) * (rng.random((my, mx, 6, 64)) < 0.4)), -1023, 1023).astype(np.int16)
    hard[..., 0] = 0
    hard[:, 0, :, 0] = [2047, 0, -2047, 0, -2047, 2047]
    hard[:, :, 0, 63] = 1023
    hard[:, :, 1, 1:] = 0
    for q, coefs in ((75, R.round_coefs(R.front_end(R.photo(W, H, W + H), 75))), (100, hard)):
        data = _encode(L, coefs, W, H, q)
        for threads in (1, 3, 8):
            rc, got = dec_coefs(L, data, threads)
            assert rc == 0, got
            assert np.array_equal(got, coefs)
        assert _encode(L, got, W, H, q, 3) == data


def _pil(rgb, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, format="JPEG", **kw)
    return buf.getvalue()


def _segment(data, marker):
    """(offset of the 0xFF of the first segment with this marker, its length field)."""
    i = 2
    while True:
        assert data[i] == 0xFF
        ln = int.from_bytes(data[i + 2:i + 4], "big")
        if data[i + 1] == marker:
            return i, ln
        i += 2 + ln


def unsupported_files():
    """name -> bytes of every kind the library leaves to PIL.  Written by PIL where PIL can; hand-patched headers otherwise
    (those need not be decodable by anything: only the marker walk is asked)."""
    from PIL import Image
    rgb = R.photo(48, 40, 3)
    base = bytearray(_pil(rgb, quality=90, subsampling=2))
    out = {"progressive": _pil(rgb, quality=90, progressive=True)}
    buf = io.BytesIO()
    Image.fromarray(rgb).convert("CMYK").save(buf, format="JPEG", quality=90)
    out["cmyk"] = buf.getvalue()
    sof, _ = _segment(base, 0xC0)
    for name, marker in (("arithmetic", 0xC9), ("progressive marker", 0xC2), ("lossless", 0xC3)):
        b = bytearray(base)
        b[sof + 1] = marker
        out[name] = bytes(b)
    b = bytearray(base)
    b[sof + 4] = 12
    out["12 bit"] = bytes(b)
    for name, hv in (("luma 1x2", 0x12), ("luma 4x1", 0x41), ("luma 2x4", 0x24)):
        b = bytearray(base)
        b[sof + 11] = hv
        out[name] = bytes(b)
    b = bytearray(base)
    b[sof + 14] = 0x21                                                   # Cb 2x1
    out["chroma 2x1"] = bytes(b)
    adobe = b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00"
    app0, ln = _segment(base, 0xE0)
    out["adobe transform 0 (rgb)"] = bytes(base[:app0]) + adobe + b"\x00" + bytes(base[app0 + 2 + ln:])
    out["adobe transform 2 (ycck)"] = bytes(base[:app0]) + adobe + b"\x02" + bytes(base[app0 + 2 + ln:])
    b = bytearray(base[:app0] + base[app0 + 2 + ln:])                    # no JFIF marker, component ids R G B
    s2, _ = _segment(b, 0xC0)
    sos, _ = _segment(b, 0xDA)
    for c, ch in enumerate(b"RGB"):
        b[s2 + 10 + 3 * c] = ch
        b[sos + 5 + 2 * c] = ch
    out["ids RGB without JFIF"] = bytes(b)
    dqt, _ = _segment(base, 0xDB)
    b = bytearray(base)
    b[dqt + 4] |= 0x10
    out["16-bit DQT"] = bytes(b)
    out["second scan after the first"] = bytes(base[:-2]) + b"\xff\xda\x00\x08\x01\x01\x00\x00\x3f\x00" + b"\xff\xd9"
    out["tables after the scan"] = bytes(base[:-2]) + b"\xff\xdd\x00\x04\x00\x00" + b"\xff\xd9"
    sos, ln = _segment(base, 0xDA)
    b = bytearray(base)
    b[sos + 2 + ln - 3] = 1                                              # Ss = 1
    out["spectral selection"] = bytes(b)
    b = bytearray(base)
    b[sof + 5:sof + 7] = b"\x00\x00"                                     # height 0: DNL
    out["height by DNL"] = bytes(b)
    gray = bytearray(_pil(rgb[..., 0], quality=90))
    s3, _ = _segment(gray, 0xC0)
    gray[s3 + 11] = 0x22
    out["gray 2x2"] = bytes(gray)
    return out


def test_unsupported_kinds_return_the_unsupported_code(L):
    files = unsupported_files()
    assert len(files) == 19
    for name, data in files.items():
        rc, info = info_of(L, data)
        assert rc == EUNSUPPORTED, (name, rc, L.lcm_last_error())
        out = np.zeros(1 << 16, np.int16)
        assert L.lcm_jpeg_dec_coefs(data, len(data), 4, out.ctypes.data, out.nbytes) == EUNSUPPORTED, name
    # the supported kinds PIL does not write by default: SOF1 and a file without a JFIF marker
    base = bytearray(_pil(R.photo(48, 40, 3), quality=90, subsampling=1))
    want = dec_coefs(L, bytes(base))[1]
    sof, _ = _segment(base, 0xC0)
    base[sof + 1] = 0xC1
    rc, got = dec_coefs(L, bytes(base), 2)
    assert rc == 0 and np.array_equal(got, want)
    assert np.array_equal(D.pil_rgb(bytes(base)), D.pixels(got, 48, 40, [(2, 1), (1, 1), (1, 1)],
                                                           D.component_tables(R.decode_entropy(_pil(R.photo(48, 40, 3), quality=90, subsampling=1)))))
    app0, ln = _segment(base, 0xE0)
    rc, got = dec_coefs(L, bytes(base[:app0] + base[app0 + 2 + ln:]), 2)
    assert rc == 0 and np.array_equal(got, want)


def test_damaged_files_are_errors_not_crashes(L):
    """Cut at 25 % and 50 %, inside a marker, a removed / repeated / renumbered RSTn, no EOI, garbage, and a buffer that is too
    small: errors.  Bytes removed, added or overwritten inside the scan may by chance leave a valid stream (40 zero bytes in a
    4:2:0 scan do), so for those the verdict must agree with the test's own decoder on the same bytes: both accept with equal
    blocks or both reject.  Two deliberate differences are allowed for: the library does not ask the padding bits to be 1
    (libjpeg does not either), and it refuses coefficients outside the 8-bit ranges, which the Python decoder does not check.
    The copies are exact-size heap blocks; test_host_decoder_under_address_sanitizer traps reads past them."""
    rgb = R.photo(120, 88, 5)
    bad = {}
    for vn, kw in (("plain", {}), ("rst", dict(restart_marker_rows=1))):
        for sub in (0, 2):
            d = _pil(rgb, quality=85, subsampling=sub, **kw)
            bad[f"{vn} {sub} cut 25 %"] = d[:len(d) // 4]
            bad[f"{vn} {sub} cut 50 %"] = d[:len(d) // 2]
            bad[f"{vn} {sub} no EOI"] = d[:-2]
            bad[f"{vn} {sub} cut 1"] = d[:-3]
            mid = len(d) * 3 // 5
            bad[f"damaged {vn} {sub} 40 bytes removed"] = d[:mid] + d[mid + 40:]
            bad[f"damaged {vn} {sub} 40 zero bytes added"] = d[:mid] + bytes(40) + d[mid:]
            for cut in (3, 10, 30, 170, 400):
                bad[f"{vn} {sub} cut inside the header at {cut}"] = d[:cut]
    d = _pil(rgb, quality=85, subsampling=2, restart_marker_rows=1)
    k = d.index(b"\xff\xd1")
    bad["RST1 removed"] = d[:k] + d[k + 2:]
    bad["RST1 twice"] = d[:k] + b"\xff\xd1" + d[k:]
    bad["RST1 renumbered"] = d[:k] + b"\xff\xd5" + d[k + 2:]
    bad["not a jpeg"] = b"\x89PNG\r\n\x1a\n" + bytes(100)
    bad["SOI only"] = b"\xff\xd8"
    bad["empty"] = b""
    rng = np.random.default_rng(1)
    for i in range(40):                                                  # seeded byte damage inside the scan
        b = bytearray(d)
        for _ in range(3):
            b[int(rng.integers(len(d) // 3, len(d) - 2))] = int(rng.integers(0, 256))
        bad[f"damaged {i}"] = bytes(b)
    n_err = 0
    for name, data in bad.items():
        exact = np.frombuffer(data, np.uint8).copy()                     # its own allocation of exactly len(data) bytes
        rc, _ = info_of(L, bytes(data))
        out = np.full(120 * 88 * 3, 0x7F7F, np.int16)                    # room for any sampling of this image
        rc2 = L.lcm_jpeg_dec_coefs(exact.ctypes.data, len(data), 8, out.ctypes.data, out.nbytes)
        if name.startswith("damaged"):
            assert rc2 in (0, EINVAL, EUNSUPPORTED), name                # valid by chance, corrupt, or a marker made inside the scan
            n_err += rc2 != 0
            try:
                want, why = R.decode_entropy(bytes(data))["coefs"], ""
            except Exception as e:                                       # noqa: BLE001
                want, why = None, str(e)
            if rc2 == 0:
                assert want is not None or "padding" in why, (name, why)
                if want is not None:
                    assert np.array_equal(out[:want.size].reshape(want.shape), want), name
            else:
                in_range = want is not None and np.abs(want[..., 0]).max() <= 2047 and np.abs(want[..., 1:]).max() <= 1023
                assert not in_range, (name, L.lcm_last_error())
            continue
        assert rc2 == EINVAL, (name, rc, rc2, L.lcm_last_error())
        assert L.lcm_last_error(), name
    assert n_err >= 20                                                   # most damage is caught by the structure checks
    good = _pil(rgb, quality=85)
    rc, info = info_of(L, good)
    out = np.zeros(info.coefs_bytes // 2, np.int16)
    assert L.lcm_jpeg_dec_coefs(good, len(good), 1, out.ctypes.data, out.nbytes - 2) == EINVAL
    assert b"coefficient buffer" in L.lcm_last_error()
    assert L.lcm_jpeg_dec_coefs(None, 10, 1, out.ctypes.data, out.nbytes) == EINVAL
    assert L.lcm_jpeg_dec_info(good, len(good), None) == EINVAL


def test_seeded_fuzz_of_small_files(L):
    """~200 files over (size, sampling, quality, restart interval, optimised tables): host blocks == Python blocks, and the
    restatement on them == PIL."""
    rng = np.random.default_rng(20240607)
    n = 0
    for i in range(200):
        w, h = int(rng.integers(1, 70)), int(rng.integers(1, 70))
        sub = D.SAMPLINGS[int(rng.integers(0, 4))]
        q = int(rng.integers(1, 101))
        kw = {}
        ri = int(rng.integers(0, 6))
        if ri:
            kw["restart_marker_blocks"] = ri
        if rng.random() < 0.3:
            kw["optimize"] = True
        data = D.make_jpeg(R.photo(w, h, i), q, sub, **kw)
        d = R.decode_entropy(data)
        rc, got = dec_coefs(L, data, int(rng.integers(1, 9)))
        assert rc == 0, (i, w, h, sub, q, kw, got)
        assert np.array_equal(got, d["coefs"]), (i, w, h, sub, q, kw)
        assert np.array_equal(D.pixels(got, w, h, d["sampling"], D.component_tables(d)), D.pil_rgb(data)), (i, w, h, sub, q, kw)
        n += 1
    assert n == 200


ASAN_DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include <thread>
#include <vector>
#include "include/lcm_hip.h"
void lcm_set_error(const char*, ...) {}
void lcm_host_pool_for_each(size_t n, void (*fn)(void*, size_t), void* ctx) {
    std::vector<std::thread> t;
    for (size_t i = 0; i < n; ++i) t.emplace_back(fn, ctx, i);
    for (auto& x : t) x.join();
}
int main(int argc, char** argv) {
    int cnt[3] = {0, 0, 0};
    for (int a = 1; a < argc; ++a) {
        FILE* f = fopen(argv[a], "rb");
        if (!f) return 2;
        fseek(f, 0, SEEK_END); long n = ftell(f); fseek(f, 0, SEEK_SET);
        unsigned char* d = (unsigned char*)malloc(n ? n : 1);          // exactly the file: a read past it is a report
        if (n && fread(d, 1, n, f) != (size_t)n) return 2;
        fclose(f);
        lcm_jpeg_info I;
        int rc = lcm_jpeg_dec_info(d, n, &I);
        if (rc == 0) { void* c = malloc(I.coefs_bytes); rc = lcm_jpeg_dec_coefs(d, n, 4, c, I.coefs_bytes); free(c); }
        cnt[rc == 0 ? 0 : rc == LCM_EINVAL ? 1 : 2]++;
        free(d);
    }
    printf("ok %d einval %d unsupported %d\\n", cnt[0], cnt[1], cnt[2]);
    return 0;
}
"""


def test_host_decoder_under_address_sanitizer(tmp_path):
    """csrc/jpeg_dec.cpp built for the host alone with AddressSanitizer and UBSan (statically linked runtime; no GPU code,
    nothing of the library), run on every unsupported kind, and on cuts and seeded byte damage of files of every sampling: no
    report."""
    import os
    import shutil
    import subprocess
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no host g++")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, "stable-diffusion-1.5-lcm-onnx-rknn2_amd", "csrc", "jpeg_dec.cpp")
    (tmp_path / "drv.cpp").write_text(ASAN_DRIVER)
    exe = str(tmp_path / "drv")
    r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-static-libasan", "-static-libubsan", "-I", root, str(tmp_path / "drv.cpp"), src, "-o", exe],
                       capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr):
        pytest.skip("the host compiler has no static sanitizer runtime")
    assert r.returncode == 0, r.stderr[-2000:]
    files = list(unsupported_files().values())
    rng = np.random.default_rng(3)
    for _, b in D.case_files(sizes=[(1, 1), (5, 3), (17, 33), (120, 88)], qualities=(40, 92)):
        files.append(b)
        files += [b[:int(c)] for c in rng.integers(0, len(b), 4)]
        for _ in range(8):
            x = bytearray(b)
            for _ in range(int(rng.integers(1, 5))):
                x[int(rng.integers(2, len(b)))] = int(rng.integers(0, 256))
            files.append(bytes(x))
    names = []
    for i, b in enumerate(files):
        (tmp_path / f"{i:05d}.jpg").write_bytes(b)
        names.append(str(tmp_path / f"{i:05d}.jpg"))
    for k in range(0, len(names), 400):
        r = subprocess.run([exe] + names[k:k + 400], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
        assert r.stdout.startswith("ok ")
    print(f"host decoder under ASan + UBSan: {len(names)} files, no report")
