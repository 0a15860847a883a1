"""The device half of the JPEG output on the MI355X: every coefficient of ``lcm_jpeg_dct_rgb8`` (csrc/jpeg.hip) against the
unrounded float64 restatement (tests/jpeg_reference.py), the integer colour / sampling path exactly on flat colours, graph
capture, argument checks, and ``HipSuperResWorker``'s jpeg format end to end against PIL's encoding of the same pixels."""
import ctypes as C
import hashlib
import io
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_reference as R
import sr_reference as sr_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# |gpu - unrounded reference|: half a unit of rounding + the fp32 error of the transform.  A coefficient is at most 1024 in
# magnitude, where an fp32 ulp is 1.2e-4; a separable 8 + 8 term transform accumulates at most ~32 half-ulps = 2e-3; the table
# entries are >= 1, so dividing by them does not enlarge it.
TOL = 0.5 + 2e-3


@pytest.fixture(scope="module")
def L():
    from sdlcm_amd import lib
    return lib.load()


def gpu_coefs(L, rgb, quality, pitch=None, base_offset=0, stream=None):
    """rgb uint8 [H][W][3] -> int16 [my][mx][6][64] from the kernel.  pitch / base_offset place the rows in a larger, misaligned
    device buffer whose other bytes are 0xA5.  The output starts as 0x7F7F everywhere: every value must be written."""
    from sdlcm_amd import lib
    H, W, _ = rgb.shape
    pitch = 3 * W if pitch is None else pitch
    host = np.full(base_offset + H * pitch, 0xA5, np.uint8)
    rows = np.lib.stride_tricks.as_strided(host[base_offset:], (H, 3 * W), (pitch, 1))
    rows[:] = rgb.reshape(H, 3 * W)
    buf = torch.from_numpy(host).to("cuda:0")
    n = int(L.lcm_jpeg_coef_bytes(W, H))
    out = torch.full((n // 2,), 0x7F7F, dtype=torch.int16, device="cuda:0")
    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    lib.check(L.lcm_jpeg_dct_rgb8(C.c_void_p(buf.data_ptr() + base_offset), W, H, pitch, quality, C.c_void_p(out.data_ptr()), n, s),
              "lcm_jpeg_dct_rgb8")
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(-(-H // 16), -(-W // 16), 6, 64)


def stripes(w, h):
    """Columns alternate between two colours whose chroma sums leave a remainder of 2 modulo 4: the even / odd output column
    bias of the 2x2 mean decides every chroma sample."""
    img = np.empty((h, w, 3), np.uint8)
    img[:, 0::2] = [200, 30, 90]
    img[:, 1::2] = [201, 33, 97]
    img[h // 2:, 0::2] = [10, 250, 3]
    img[h // 2:, 1::2] = [13, 251, 4]
    return img


CASES = {
    "288x240": lambda: (R.photo(288, 240, 21), None, 0),
    "17x33": lambda: (R.photo(17, 33, 22), None, 0),
    "1536x1536": lambda: (R.photo(1536, 1536, 23), None, 0),
    "301x100 pitch 3W+10 base+3": lambda: (R.photo(301, 100, 24), 3 * 301 + 10, 3),
    "4609x20 (several strips, 1-pixel last MCU)": lambda: (R.photo(4609, 20, 25), None, 0),
    "stripes 70x50": lambda: (stripes(70, 50), None, 0),
}


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("q", [40, 92, 100])
def test_every_coefficient_against_the_unrounded_reference(L, name, q):
    rgb, pitch, off = CASES[name]()
    got = gpu_coefs(L, rgb, q, pitch, off)
    ref = R.front_end(rgb, q)
    assert got.shape == ref.shape
    err = np.abs(got.astype(np.float64) - ref)
    print(f"jpeg coefficients {name} q={q}: max |gpu - unrounded| = {err.max():.6f} (bound {TOL}), "
          f"{(got != np.rint(ref)).mean() * 100:.4f} % differ from rint(reference)")
    assert err.max() <= TOL


def test_planes_are_the_integer_reference_on_flat_colours(L):
    """One flat colour per MCU, q = 100 (every table entry 1): the DCT of a constant block is exact in fp32, so DC must EQUAL
    8 * (plane value - 128) of the integer reference and every AC coefficient must be 0.  256 colours: the corners of the cube,
    the primaries, and seeded random ones.  (The even / odd column bias of the chroma mean cannot show on a flat colour: the
    "stripes" case of the coefficient test covers it.)"""
    rng = np.random.default_rng(31)
    cols = rng.integers(0, 256, (256, 3)).astype(np.uint8)
    fixed = [(0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255),
             (1, 1, 1), (254, 254, 254), (128, 128, 128), (127, 127, 127)]
    cols[:len(fixed)] = fixed
    img = np.repeat(np.repeat(cols.reshape(16, 16, 3), 16, 0), 16, 1)
    got = gpu_coefs(L, img, 100)
    y, cb, cr = R.planes(img)
    want = np.zeros_like(got)
    want[:, :, 0:4, 0] = (8 * (y[::16, ::16] - 128))[:, :, None]
    want[:, :, 4, 0] = 8 * (cb[::8, ::8] - 128)
    want[:, :, 5, 0] = 8 * (cr[::8, ::8] - 128)
    assert np.array_equal(got, want)
    # edge replication: a 250x250 crop of the same image pads with its last column / row, i.e. the same flat MCUs
    assert np.array_equal(gpu_coefs(L, img[:250, :250], 100), want)


def test_graph_capture_replays_the_launch(L):
    from sdlcm_amd import lib
    rgb = R.photo(288, 240, 41)
    eager = gpu_coefs(L, rgb, 92)
    src = torch.from_numpy(rgb).to("cuda:0")
    n = int(L.lcm_jpeg_coef_bytes(288, 240))
    out = torch.zeros(n // 2, dtype=torch.int16, device="cuda:0")
    stream = torch.cuda.Stream("cuda:0")
    torch.cuda.synchronize()
    ex = C.c_void_p()
    with torch.cuda.stream(stream):
        s = C.c_void_p(stream.cuda_stream)
        lib.check(L.lcm_graph_begin(s), "lcm_graph_begin")
        rc = L.lcm_jpeg_dct_rgb8(C.c_void_p(src.data_ptr()), 288, 240, 3 * 288, 92, C.c_void_p(out.data_ptr()), n, s)
        lib.check(L.lcm_graph_end(s, C.byref(ex)), "lcm_graph_end")
        lib.check(rc, "lcm_jpeg_dct_rgb8 under capture")
        stream.synchronize()
        assert int(out.abs().max()) == 0                      # captured, not run
        lib.check(L.lcm_graph_launch(ex, s), "lcm_graph_launch")
        stream.synchronize()
    assert np.array_equal(out.cpu().numpy().reshape(eager.shape), eager)
    L.lcm_graph_destroy(ex)


def test_bad_arguments_are_refused_before_anything_is_enqueued(L):
    buf = torch.zeros(3 * 32 * 32, dtype=torch.uint8, device="cuda:0")
    out = torch.full((2 * 2 * 384,), 0x1234, dtype=torch.int16, device="cuda:0")
    p, o, n = C.c_void_p(buf.data_ptr()), C.c_void_p(out.data_ptr()), out.numel() * 2
    s = torch.cuda.current_stream().cuda_stream
    for args, word in (((p, 0, 32, 96, 75, o, n, s), b"bad shape"), ((p, 32, 0, 96, 75, o, n, s), b"bad shape"),
                       ((p, 32, 32, 96, 0, o, n, s), b"quality"), ((p, 32, 32, 96, 101, o, n, s), b"quality"),
                       ((p, 32, 32, 96, 75, o, n - 2, s), b"coefficient buffer"), ((p, 32, 32, 95, 75, o, n, s), b"pitch"),
                       ((None, 32, 32, 96, 75, o, n, s), b"null pointer")):
        assert L.lcm_jpeg_dct_rgb8(*args) == -1
        assert word in L.lcm_last_error(), (args[1:5], L.lcm_last_error())
    torch.cuda.synchronize()
    assert bool((out == 0x1234).all())


@pytest.fixture(scope="module")
def worker():
    from sdlcm_amd.backends.sr_worker import HipSuperResWorker
    wk = HipSuperResWorker(0, "synthetic", 224, 672)
    yield wk
    wk.close()


def _png(rgb):
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, format="PNG")
    return buf.getvalue()


def _strict(data):
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        im = R.pil_decode(data)
    return im


@pytest.mark.parametrize("q", [40, 75, 92])
def test_worker_jpeg_end_to_end_against_pil(worker, q):
    rgb = sr_ref.test_images()(96, 80, 2)
    data = _png(rgb)
    up = worker.upscale_rgb(rgb, 1)
    ours = worker.upscale_bytes(data, magnitude=1, out_format="jpeg", quality=q)
    assert ours == worker.upscale_bytes(data, magnitude=1, out_format="jpeg", quality=q)
    assert ours == worker.upscale_once(data, out_format="jpeg", quality=q)
    im = _strict(ours)
    assert im.size == (288, 240) and im.mode == "RGB"
    theirs = R.pil_jpeg(up, q)                                                    # PIL's default for RGB is 4:2:0
    p_ours, p_theirs = R.psnr(np.asarray(im), up), R.psnr(np.asarray(_strict(theirs)), up)
    print(f"worker jpeg q={q}: PSNR ours {p_ours:.4f} PIL {p_theirs:.4f}, size ours {len(ours)} PIL {len(theirs)}")
    assert p_theirs - p_ours <= R.X_DB
    # the file holds the coefficients of the pixels upscale_rgb returns
    d = R.decode_entropy(ours)
    assert (d["width"], d["height"], d["dri"]) == (288, 240, 18)
    assert np.abs(d["coefs"].astype(np.float64) - R.front_end(up, q)).max() <= TOL


def test_worker_jpeg_pil_switch_and_quality_check(worker, monkeypatch):
    rgb = sr_ref.test_images()(96, 80, 2)
    data = _png(rgb)
    up = worker.upscale_rgb(rgb, 1)
    monkeypatch.setenv("LCM_JPEG_ENCODER", "pil")
    for q in (40, 92):
        assert worker.upscale_bytes(data, magnitude=1, out_format="jpeg", quality=q) == R.pil_jpeg(up, q)
    monkeypatch.delenv("LCM_JPEG_ENCODER")
    for q in (0, 101):
        with pytest.raises(RuntimeError, match=r"quality must be 1\.\.100"):
            worker.upscale_bytes(data, magnitude=1, out_format="jpeg", quality=q)
    # the helper for host pixels runs the same launch and coder
    from sdlcm_amd.backends.hip_worker import encode_jpeg
    assert encode_jpeg(up, 92) == worker.upscale_bytes(data, magnitude=1, out_format="jpeg", quality=92)


CHILD = """
import hashlib, sys
sys.path.insert(0, {root!r})
import sdlcm_amd
from sdlcm_amd.backends.sr_worker import HipSuperResWorker
wk = HipSuperResWorker(0, "synthetic", 224, 672)
data = open({png!r}, "rb").read()
print("SHA", hashlib.sha256(wk.upscale_bytes(data, magnitude=1, out_format="jpeg", quality=92)).hexdigest())
wk.close()
"""


def test_bytes_do_not_depend_on_the_thread_count(worker, tmp_path):
    """LCM_JPEG_THREADS = 1 and 8, each in a fresh child process (300x200 -> 900x600: 38 restart intervals)."""
    rgb = sr_ref.test_images()(300, 200, 5)
    png = tmp_path / "in.png"
    png.write_bytes(_png(rgb))
    here = hashlib.sha256(worker.upscale_bytes(png.read_bytes(), magnitude=1, out_format="jpeg", quality=92)).hexdigest()
    for thr in ("1", "8"):
        env = dict(os.environ, LCM_JPEG_THREADS=thr)
        env.pop("LCM_JPEG_ENCODER", None)
        r = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT, png=str(png))], env=env, capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        sha = [ln.split()[1] for ln in r.stdout.splitlines() if ln.startswith("SHA ")]
        assert sha == [here], (thr, r.stdout[-500:])
