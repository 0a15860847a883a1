"""The device half of the JPEG input on the MI355X: every byte of ``lcm_jpeg_idct_rgb8`` (csrc/jpeg_dec.hip) against the numpy
restatement of the fixed integer arithmetic (tests/jpeg_decode_reference.py; tolerance 0) and against PIL, pitch / offset /
edge cases, coefficient extremes, graph capture, argument checks, and ``HipSuperResWorker`` with a JPEG input end to end against
the LCM_JPEG_DECODER=pil path, byte for byte."""
import ctypes as C
import hashlib
import io
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_decode_reference as D
import jpeg_reference as R
import sr_reference as sr_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLING = {0: [(1, 1)] * 3, 1: [(2, 1), (1, 1), (1, 1)], 2: [(2, 2), (1, 1), (1, 1)]}


@pytest.fixture(scope="module")
def L():
    from sdlcm_amd import lib
    return lib.load()


def host_coefs(L, data, threads=8):
    from sdlcm_amd import lib
    info = lib.JpegInfo()
    assert L.lcm_jpeg_dec_info(data, len(data), C.byref(info)) == 0, L.lcm_last_error()
    out = np.zeros(info.coefs_bytes // 2, np.int16)
    assert L.lcm_jpeg_dec_coefs(data, len(data), threads, out.ctypes.data, out.nbytes) == 0, L.lcm_last_error()
    return info, out.reshape(info.mcus_y, info.mcus_x, info.blocks_per_mcu, 64)


def make_info(W, H, ncomp, sampling, qt):
    from sdlcm_amd import lib
    info = lib.JpegInfo()
    info.width, info.height, info.ncomp, info.sampling = W, H, ncomp, sampling
    hs, vs = (2 if sampling >= 1 else 1), (2 if sampling == 2 else 1)
    info.mcus_x, info.mcus_y = -(-W // (8 * hs)), -(-H // (8 * vs))
    info.blocks_per_mcu = 1 if ncomp == 1 else hs * vs + 2
    info.coefs_bytes = info.mcus_x * info.mcus_y * info.blocks_per_mcu * 128
    info.work_bytes = info.coefs_bytes // 2
    flat = np.zeros(192, np.uint8)
    flat[:64 * ncomp] = np.concatenate([np.asarray(t, np.uint8) for t in qt])
    info.qt[:] = flat.tolist()
    return info


def gpu_pixels(L, info, coefs, pitch=None, base_offset=0, fill=0xA5):
    """-> (uint8 [H][W][3] from the kernel, the whole output buffer).  pitch / base_offset place the rows in a larger,
    misaligned device buffer pre-filled with ``fill``; the work buffer starts as 0xEE."""
    from sdlcm_amd import lib
    W, H = info.width, info.height
    pitch = 3 * W if pitch is None else pitch
    total = base_offset + H * pitch
    dev = torch.from_numpy(np.ascontiguousarray(coefs, np.int16).reshape(-1)).to("cuda:0")
    work = torch.full((int(info.work_bytes),), 0xEE, dtype=torch.uint8, device="cuda:0")
    out = torch.full((total,), fill, dtype=torch.uint8, device="cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    lib.check(L.lcm_jpeg_idct_rgb8(C.c_void_p(dev.data_ptr()), dev.numel() * 2, C.byref(info), C.c_void_p(work.data_ptr()),
                                   work.numel(), C.c_void_p(out.data_ptr() + base_offset), pitch, s), "lcm_jpeg_idct_rgb8")
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    rows = np.lib.stride_tricks.as_strided(host[base_offset:], (H, 3 * W), (pitch, 1))
    return rows.reshape(H, W, 3).copy(), host


def restatement(info, coefs):
    qt = np.frombuffer(bytes(info.qt), np.uint8).reshape(3, 64).astype(np.int64)
    samp = [(1, 1)] if info.ncomp == 1 else SAMPLING[info.sampling]
    return D.pixels(coefs, info.width, info.height, samp, [qt[c] for c in range(info.ncomp)])


def test_every_byte_equals_the_restatement_and_pil(L):
    """The case list of tests/test_jpeg_decode_cpu.py (sizes x qualities x samplings x variants).  Run twice per file: the
    output pre-filled with 0x00 and with 0xFF, so that a pixel that is not written cannot pass both."""
    n = 0
    for name, data in D.case_files():
        info, coefs = host_coefs(L, data)
        want = restatement(info, coefs)
        for fill in (0x00, 0xFF):
            got, _ = gpu_pixels(L, info, coefs, fill=fill)
            assert np.array_equal(got, want), (name, fill, int((got != want).sum()))
        assert np.array_equal(want, D.pil_rgb(data)), name
        n += 1
    assert n == len(D.SIZES) * len(D.QUALITIES) * len(D.SAMPLINGS) * len(D.VARIANTS)


@pytest.mark.parametrize("sub", D.SAMPLINGS)
def test_large_images_equal_pil(L, sub):
    for (w, h, q) in ((1536, 1536, 92), (2000, 1333, 75)):
        data = D.make_jpeg(R.photo(w, h, w + h), q, sub, restart_marker_rows=1)
        info, coefs = host_coefs(L, data)
        got, _ = gpu_pixels(L, info, coefs)
        assert np.array_equal(got, D.pil_rgb(data)), (w, h, sub)


@pytest.mark.parametrize("sub", D.SAMPLINGS)
def test_pitch_offset_and_one_pixel_last_mcu(L, sub):
    """Rows at a pitch of 3W + 10 from a base offset of 3 in a buffer of 0xA5: no byte outside the rows changes.  4609x20: the
    last MCU holds one pixel."""
    for (w, h) in ((301, 100), (4609, 20), (7, 9)):
        data = D.make_jpeg(R.photo(w, h, 3 * w + h), 92, sub)
        info, coefs = host_coefs(L, data)
        want = restatement(info, coefs)
        pitch, off = 3 * w + 10, 3
        got, buf = gpu_pixels(L, info, coefs, pitch, off)
        assert np.array_equal(got, want), (w, h, sub)
        mask = np.ones(buf.size, bool)
        for y in range(h):
            mask[off + y * pitch:off + y * pitch + 3 * w] = False
        assert (buf[mask] == 0xA5).all(), (w, h, sub)
        assert np.array_equal(want, D.pil_rgb(data))


@pytest.mark.parametrize("sampling,ncomp", [(0, 3), (1, 3), (2, 3), (0, 1)])
def test_coefficient_extremes(L, sampling, ncomp):
    """+-2047 DC and +-1023 AC, dense, sparse and mixed with ordinary blocks, under the tables of quality 100 (all ones: the
    range clamp decides), 92 and 40 (the 32-bit wrap of the header's arithmetic decides)."""
    rng = np.random.default_rng(7 + sampling + ncomp)
    W, H = 150, 70
    for q in (100, 92, 40):
        ql, qc = R.quant_tables(q)
        info = make_info(W, H, ncomp, sampling, [ql, qc, qc][:ncomp])
        shape = (info.mcus_y, info.mcus_x, info.blocks_per_mcu, 64)
        c = np.rint(rng.laplace(0, 30, shape) * (rng.random(shape) < 0.3)).astype(np.int64)
        c[..., 0] = rng.choice([-2047, 2047, 0, 300, -300], shape[:3])
        kind = rng.integers(0, 6, shape[:3])
        ext = rng.choice([-1023, 1023], shape)
        c = np.where((kind == 0)[..., None], ext, c)                              # dense extremes
        c = np.where((kind == 1)[..., None] & (rng.random(shape) < 0.1), ext, c)  # sparse extremes
        c[..., 0] = np.where(kind <= 1, rng.choice([-2047, 2047], shape[:3]), c[..., 0])
        c[kind == 2, 1:] = 0                                                      # DC only
        c = np.clip(c, -1023, 1023).astype(np.int16)
        c[..., 0] = np.where(kind <= 1, np.where(c[..., 0] > 0, 2047, -2047), c[..., 0])
        want = restatement(info, c)
        got, _ = gpu_pixels(L, info, c)
        assert np.array_equal(got, want), (q, int((got != want).sum()))
        assert want.min() == 0 and want.max() == 255


def test_graph_capture_replays_the_launches(L):
    from sdlcm_amd import lib
    data = D.make_jpeg(R.photo(288, 240, 41), 92, 2)
    info, coefs = host_coefs(L, data)
    eager, _ = gpu_pixels(L, info, coefs)
    dev = torch.from_numpy(coefs.reshape(-1)).to("cuda:0")
    work = torch.zeros(int(info.work_bytes), dtype=torch.uint8, device="cuda:0")
    out = torch.zeros(240, 288, 3, dtype=torch.uint8, device="cuda:0")
    stream = torch.cuda.Stream("cuda:0")
    torch.cuda.synchronize()
    ex = C.c_void_p()
    with torch.cuda.stream(stream):
        s = C.c_void_p(stream.cuda_stream)
        lib.check(L.lcm_graph_begin(s), "lcm_graph_begin")
        rc = L.lcm_jpeg_idct_rgb8(C.c_void_p(dev.data_ptr()), dev.numel() * 2, C.byref(info), C.c_void_p(work.data_ptr()), work.numel(),
                                  C.c_void_p(out.data_ptr()), 3 * 288, s)
        lib.check(L.lcm_graph_end(s, C.byref(ex)), "lcm_graph_end")
        lib.check(rc, "lcm_jpeg_idct_rgb8 under capture")
        stream.synchronize()
        assert int(out.max()) == 0                            # captured, not run
        for _ in range(2):
            out.zero_()
            lib.check(L.lcm_graph_launch(ex, s), "lcm_graph_launch")
            stream.synchronize()
            assert np.array_equal(out.cpu().numpy(), eager)
    L.lcm_graph_destroy(ex)


def test_bad_arguments_are_refused_before_anything_is_enqueued(L):
    ql, qc = R.quant_tables(75)
    coefs = torch.zeros(2 * 2 * 6 * 64, dtype=torch.int16, device="cuda:0")
    work = torch.full((2 * 2 * 6 * 64,), 0x12, dtype=torch.uint8, device="cuda:0")
    out = torch.full((32 * 32 * 3,), 0x34, dtype=torch.uint8, device="cuda:0")
    c, w, o = C.c_void_p(coefs.data_ptr()), C.c_void_p(work.data_ptr()), C.c_void_p(out.data_ptr())
    s = torch.cuda.current_stream().cuda_stream
    good = make_info(32, 32, 3, 2, [ql, qc, qc])
    ip = C.byref(good)
    nb, wb = coefs.numel() * 2, work.numel()

    def variant(**kw):
        i = make_info(32, 32, 3, 2, [ql, qc, qc])
        for k, v in kw.items():
            setattr(i, k, v)
        return C.byref(i)
    for args, word in (((None, nb, ip, w, wb, o, 96, s), b"null pointer"), ((c, nb, None, w, wb, o, 96, s), b"null pointer"),
                       ((c, nb, ip, None, wb, o, 96, s), b"null pointer"), ((c, nb, ip, w, wb, None, 96, s), b"null pointer"),
                       ((c, nb - 2, ip, w, wb, o, 96, s), b"coefficient buffer"), ((c, nb, ip, w, wb - 1, o, 96, s), b"work buffer"),
                       ((c, nb, ip, w, wb, o, 95, s), b"pitch"), ((c, nb, variant(width=0), w, wb, o, 96, s), b"bad shape"),
                       ((c, nb, variant(height=70000), w, wb, o, 96, s), b"bad shape"),
                       ((c, nb, variant(ncomp=4), w, wb, o, 96, s), b"components"),
                       ((c, nb, variant(sampling=3), w, wb, o, 96, s), b"sampling"),
                       ((c, nb, variant(ncomp=1, sampling=2), w, wb, o, 96, s), b"sampling"),
                       ((C.c_void_p(coefs.data_ptr() + 2), nb - 2, variant(width=16), w, wb, o, 96, s), b"aligned")):
        assert L.lcm_jpeg_idct_rgb8(*args) == -1
        assert word in L.lcm_last_error(), L.lcm_last_error()
    torch.cuda.synchronize()
    assert bool((out == 0x34).all()) and bool((work == 0x12).all())


# ------------------------------------------------------------------------------------------------------------------------------
# worker
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def worker():
    from sdlcm_amd.backends.sr_worker import HipSuperResWorker
    wk = HipSuperResWorker(0, "synthetic", 224, 672)
    yield wk
    wk.close()


def _both(worker, monkeypatch, data, **kw):
    monkeypatch.setenv("LCM_JPEG_DECODER", "hip")
    ours = worker.upscale_bytes(data, **kw)
    monkeypatch.setenv("LCM_JPEG_DECODER", "pil")
    theirs = worker.upscale_bytes(data, **kw)
    return ours, theirs


@pytest.mark.parametrize("fmt", ["png", "jpeg"])
@pytest.mark.parametrize("mag", [1, 2])
def test_worker_equals_the_pil_path_byte_for_byte(worker, monkeypatch, fmt, mag):
    rgb = sr_ref.test_images()(96, 80, 2)
    for sub in (2, 0, 1, "gray"):
        for kw in ({}, dict(restart_marker_rows=1)):
            data = D.make_jpeg(rgb, 90, sub, **kw)
            ours, theirs = _both(worker, monkeypatch, data, magnitude=mag, out_format=fmt, quality=92)
            assert ours == theirs, (sub, kw)
            assert len(ours) > 1000
    monkeypatch.setenv("LCM_JPEG_DECODER", "hip")
    data = D.make_jpeg(rgb, 90, 2)
    if mag == 1:
        assert worker.upscale_once(data, out_format=fmt, quality=92) == worker.upscale_bytes(data, magnitude=1, out_format=fmt, quality=92)


def test_worker_uses_the_library_and_falls_back(worker, monkeypatch):
    """The library path is really taken (its decoder object appears, PIL's decode is not called), a progressive / CMYK / damaged
    JPEG and a PNG go through PIL with the result they had, and mode "dri" leaves files without restart markers to PIL."""
    from sdlcm_amd.backends import sr_worker, hip_worker
    rgb = sr_ref.test_images()(96, 80, 3)
    calls = []
    real = sr_worker._decode
    monkeypatch.setattr(sr_worker, "_decode", lambda b: (calls.append(len(b)), real(b))[1])
    kw = dict(magnitude=1, out_format="png", quality=92)
    monkeypatch.setenv("LCM_JPEG_DECODER", "hip")
    plain, rst = D.make_jpeg(rgb, 90, 2), D.make_jpeg(rgb, 90, 2, restart_marker_rows=1)
    a = worker.upscale_bytes(plain, **kw)
    assert calls == [] and worker.net.jpeg_dec is not None
    assert np.array_equal(hip_worker.decode_jpeg(plain), D.pil_rgb(plain))
    monkeypatch.setenv("LCM_JPEG_DECODER", "dri")
    assert worker.upscale_bytes(plain, **kw) == a and len(calls) == 1
    worker.upscale_bytes(rst, **kw)
    assert len(calls) == 1
    monkeypatch.setenv("LCM_JPEG_DECODER", "hip")
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, format="JPEG", quality=90, progressive=True)
    prog = buf.getvalue()
    buf = io.BytesIO()
    Image.fromarray(rgb).convert("CMYK").save(buf, format="JPEG", quality=90)
    cmyk = buf.getvalue()
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, format="PNG")
    png = buf.getvalue()
    for name, data in (("progressive", prog), ("cmyk", cmyk), ("png", png)):
        n = len(calls)
        ours, theirs = _both(worker, monkeypatch, data, **kw)
        assert ours == theirs, name
        assert len(calls) == n + 2, name                      # PIL decoded it both times
        monkeypatch.setenv("LCM_JPEG_DECODER", "hip")
        assert np.array_equal(hip_worker.decode_jpeg(data), np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))), name
    # a truncated file fails as it did: PIL's error
    for env in ("hip", "pil"):
        monkeypatch.setenv("LCM_JPEG_DECODER", env)
        with pytest.raises(OSError):
            worker.upscale_bytes(plain[:len(plain) // 2], **kw)


def test_sr_max_pixels_is_refused_from_the_header(worker, monkeypatch):
    from sdlcm_amd.backends import sr_worker
    rgb = sr_ref.test_images()(96, 80, 4)
    data = D.make_jpeg(rgb, 90, 2)
    monkeypatch.setattr(sr_worker, "_decode", lambda b: pytest.fail("decoded before the size check"))
    monkeypatch.setenv("LCM_JPEG_DECODER", "hip")
    monkeypatch.setenv("SR_MAX_PIXELS", str(96 * 80 - 1))
    with pytest.raises(RuntimeError, match=rf"Image too large: 96x80 exceeds SR_MAX_PIXELS={96 * 80 - 1}"):
        worker.upscale_bytes(data, magnitude=1, out_format="png", quality=92)
    monkeypatch.setenv("SR_MAX_PIXELS", str(96 * 80 * 9 - 1))
    with pytest.raises(RuntimeError, match=rf"Image too large: 288x240 exceeds SR_MAX_PIXELS={96 * 80 * 9 - 1}"):
        worker.upscale_bytes(data, magnitude=2, out_format="jpeg", quality=92)
    monkeypatch.undo()
    monkeypatch.setenv("LCM_JPEG_DECODER", "pil")
    monkeypatch.setenv("SR_MAX_PIXELS", str(96 * 80 - 1))
    with pytest.raises(RuntimeError, match=rf"Image too large: 96x80 exceeds SR_MAX_PIXELS={96 * 80 - 1}"):
        worker.upscale_bytes(data, magnitude=1, out_format="png", quality=92)


def test_sizes_pil_refuses_stay_pils_and_errors_keep_their_order(worker, monkeypatch):
    """A header of 65535 x 65535 is PIL's to refuse (decompression bomb): nothing is allocated for it.  A request that is both
    too large and of a bad quality reports the quality, as the PIL path does."""
    from sdlcm_amd.backends import hip_worker
    data = bytearray(D.make_jpeg(sr_ref.test_images()(96, 80, 4), 90, 2))
    i = 2
    while data[i + 1] != 0xC0:
        i += 2 + int.from_bytes(data[i + 2:i + 4], "big")
    data[i + 5:i + 9] = b"\xff\xff\xff\xff"
    for env in ("hip", "pil"):
        monkeypatch.setenv("LCM_JPEG_DECODER", env)
        with pytest.raises(Image.DecompressionBombError):
            hip_worker.decode_jpeg(bytes(data))
        with pytest.raises(Image.DecompressionBombError):
            worker.upscale_bytes(bytes(data), magnitude=1, out_format="png", quality=92)
    assert worker.net.jpeg_dec is None or worker.net.jpeg_dec._pinned is None or worker.net.jpeg_dec._pinned.numel() < 1 << 28
    good = D.make_jpeg(sr_ref.test_images()(96, 80, 4), 90, 2)
    monkeypatch.setenv("SR_MAX_PIXELS", "100")
    for env in ("hip", "pil"):
        monkeypatch.setenv("LCM_JPEG_DECODER", env)
        with pytest.raises(RuntimeError, match=r"quality must be 1\.\.100"):
            worker.upscale_bytes(good, magnitude=1, out_format="jpeg", quality=0)
        with pytest.raises(RuntimeError, match="Image too large"):
            worker.upscale_bytes(good, magnitude=1, out_format="jpeg", quality=92)


def test_two_workers_on_two_threads(monkeypatch):
    from sdlcm_amd.backends.sr_worker import HipSuperResWorker
    monkeypatch.setenv("LCM_JPEG_DECODER", "hip")
    files = [D.make_jpeg(sr_ref.test_images()(120 + 8 * i, 90, i), 90, [2, 0, 1][i % 3], restart_marker_rows=1) for i in range(6)]
    workers = [HipSuperResWorker(i, "synthetic", 224, 672) for i in range(2)]
    serial = [workers[0].upscale_bytes(f, magnitude=1, out_format="jpeg", quality=92) for f in files]
    results, errors = [None, None], []

    def run(i):
        try:
            results[i] = [workers[i].upscale_bytes(f, magnitude=1, out_format="jpeg", quality=92) for _ in range(3) for f in files]
        except Exception as e:                                # noqa: BLE001
            errors.append(e)
    threads = [threading.Thread(target=run, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for wk in workers:
        wk.close()
    assert not errors, errors
    assert results[0] == results[1] == serial * 3


CHILD = """
import hashlib, sys
sys.path.insert(0, {root!r})
import sdlcm_amd
from sdlcm_amd.backends.sr_worker import HipSuperResWorker
wk = HipSuperResWorker(0, "synthetic", 224, 672)
data = open({jpg!r}, "rb").read()
print("SHA", hashlib.sha256(wk.upscale_bytes(data, magnitude=1, out_format="jpeg", quality=92)).hexdigest())
wk.close()
"""


def test_a_fresh_process_gives_the_same_bytes(worker, monkeypatch, tmp_path):
    """LCM_JPEG_THREADS = 1 and 8, each in a fresh child process (300x200 4:2:0 with a restart marker per MCU row)."""
    monkeypatch.setenv("LCM_JPEG_DECODER", "hip")
    jpg = tmp_path / "in.jpg"
    jpg.write_bytes(D.make_jpeg(sr_ref.test_images()(300, 200, 5), 90, 2, restart_marker_rows=1))
    here = hashlib.sha256(worker.upscale_bytes(jpg.read_bytes(), magnitude=1, out_format="jpeg", quality=92)).hexdigest()
    for thr in ("1", "8"):
        env = dict(os.environ, LCM_JPEG_THREADS=thr, LCM_JPEG_DECODER="hip")
        env.pop("LCM_JPEG_ENCODER", None)
        r = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT, jpg=str(jpg))], env=env, capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        sha = [ln.split()[1] for ln in r.stdout.splitlines() if ln.startswith("SHA ")]
        assert sha == [here], (thr, r.stdout[-500:])
