"""Super-resolution on the MI355X: every launch of a pass against a float64 reference built from its own fp16 operands, the chroma
path against PIL, whole passes against the CPU restatement (tests/sr_reference.py), determinism and the worker's formats."""
import ctypes as C
import io
import threading

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

import sr_reference as ref

pytestmark = pytest.mark.gpu
U = 2.0 ** -24                      # fp32 unit roundoff


@pytest.fixture(scope="module")
def net():
    from sdlcm_amd import superres as S
    return S.SuperResNet("synthetic", "cuda:0", 224, 672)


def _p(t):
    return C.c_void_p(t.data_ptr())


def _conv_bound(x, w, b, pad, ref64):
    """|kernel - ref| <= half an fp16 ulp of the stored value (2^-11 relative, 2^-25 absolute below the normal range) + the
    fp32 accumulation error of K products in any order (K u sum|x w|, plus the bias add)."""
    K = w.shape[1] * w.shape[2] * w.shape[3]
    s = F.conv2d(x.abs(), w.abs(), b.abs(), padding=pad)
    return 2.0 ** -11 * ref64.abs() + 2.0 ** -25 + (K + 2) * U * s


def test_every_launch_against_fp64(net):
    """150x100 image, 60x60 tiles (plan 3 x 2, overlapping starts, partial MFMA blocks): conv1, conv2, conv3 and conv4+shuffle
    each checked on the operands the kernels actually read."""
    from sdlcm_amd import lib
    L, w, dev = lib.load(), net.w, net.device
    rgb = ref.test_images()(150, 100, 7)
    W, H, t = 150, 100, 60
    xs, ys = ref.plan_axis(W, t), ref.plan_axis(H, t)
    T = len(xs) * len(ys)
    src = torch.from_numpy(rgb).to(dev)
    a = torch.empty(T, t, t, 64, dtype=torch.float16, device=dev)
    b = torch.empty_like(a)
    c = torch.empty(T, t, t, 32, dtype=torch.float16, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    lib.check(L.lcm_sr_conv1(_p(src), W, H, t, t, 0, T, _p(w["w1"]), _p(w["b1"]), _p(a), s))
    lib.check(L.lcm_sr_conv3x3(_p(a), T, t, t, 64, _p(w["w2"]), _p(w["b2"]), _p(b), s))
    lib.check(L.lcm_sr_conv3x3(_p(b), T, t, t, 32, _p(w["w3"]), _p(w["b3"]), _p(c), s))
    ys_out = []
    for fill in (0, 255):                                          # every byte written: the result does not depend on the fill
        y8 = torch.full((3 * H, 3 * W), fill, dtype=torch.uint8, device=dev)
        lib.check(L.lcm_sr_conv4_shuffle(_p(c), W, H, t, t, 0, T, _p(w["w4"]), _p(w["b4"]), 3, _p(y8), s))
        ys_out.append(y8.cpu().numpy())
    torch.cuda.synchronize()
    assert np.array_equal(ys_out[0], ys_out[1])
    sd = {k: v.double() for k, v in net.sd.items()}
    h16 = lambda k: net.sd[k].half().double()                      # noqa: E731  the fp16 weights the kernels read

    # conv1: input = fp16(Y / 255) of each tile, Y from PIL
    Y = np.asarray(Image.fromarray(rgb).convert("YCbCr"))[..., 0]
    x = torch.stack([torch.from_numpy(Y[y0:y0 + t, x0:x0 + t].astype(np.float32) / 255.0) for y0 in ys for x0 in xs])[:, None]
    x = x.half().double()
    r1 = F.conv2d(x, h16("conv1.weight"), sd["conv1.bias"], padding=2)
    bound = _conv_bound(x, h16("conv1.weight"), sd["conv1.bias"], 2, r1)
    got = a.permute(0, 3, 1, 2).double().cpu()
    err = (got - F.relu(r1)).abs()
    print(f"conv1: max err {err.max():.3g}, max err/bound {(err / bound).max():.3f}")
    assert (err <= bound).all()
    for name, inp, out, pad in (("conv2", a, b, 1), ("conv3", b, c, 1)):
        xi = inp.permute(0, 3, 1, 2).double().cpu()
        rr = F.conv2d(xi, h16(f"{name}.weight"), sd[f"{name}.bias"], padding=pad)
        bound = _conv_bound(xi, h16(f"{name}.weight"), sd[f"{name}.bias"], pad, rr)
        err = (out.permute(0, 3, 1, 2).double().cpu() - F.relu(rr)).abs()
        print(f"{name}: max err {err.max():.3g}, max err/bound {(err / bound).max():.3f}")
        assert (err <= bound).all(), name
    # conv4 + shuffle + ownership: tiles painted in the reference's order, then 255 y truncated
    xi = c.permute(0, 3, 1, 2).double().cpu()
    r4 = F.conv2d(xi, h16("conv4.weight"), sd["conv4.bias"], padding=1)
    s4 = F.conv2d(xi.abs(), h16("conv4.weight").abs(), sd["conv4.bias"].abs(), padding=1)
    shuf = lambda v: v.reshape(T, 1, 3, 3, t, t).permute(0, 1, 4, 2, 5, 3).reshape(T, 3 * t, 3 * t)   # noqa: E731
    r4, s4 = shuf(r4), shuf(s4)
    pre = np.zeros((3 * H, 3 * W))
    eb = np.zeros((3 * H, 3 * W))
    for i, (y0, x0) in enumerate((y0, x0) for y0 in ys for x0 in xs):
        pre[3 * y0:3 * y0 + 3 * t, 3 * x0:3 * x0 + 3 * t] = 255.0 * r4[i].numpy()
        # fp32 accumulation of 288 products + bias, the fp32 product 255 y: in units of the output byte
        eb[3 * y0:3 * y0 + 3 * t, 3 * x0:3 * x0 + 3 * t] = 255.0 * (290 * U * s4[i].numpy()) + 2 * U * 255.0
    want = np.clip(np.floor(pre), 0, 255)
    near = np.abs(pre - np.rint(pre)) <= eb                       # 255 y within the bound of an integer: either side is right
    d = np.abs(ys_out[0].astype(np.int64) - want)
    inside = float(((pre > 0) & (pre < 255)).mean())
    print(f"conv4: {100 * inside:.1f} % of pre-clip Y inside (0, 1); {int(near.sum())} pixels near an integer; "
          f"max |d| {d.max()} ({int((d != 0).sum())} differ)")
    assert inside >= 0.9
    assert (d[~near] == 0).all() and (d <= 1).all()


def test_chroma_against_pil(net):
    """Horizontal pass == PIL's bicubic of the kernels' own Cb / Cr planes (PIL-exact resampling); within 2 of PIL's resampled planes;
    the merge == PIL's vertical bicubic of the horizontal planes + the kernels' YCbCr -> RGB tables."""
    from sdlcm_amd import lib
    L, dev = lib.load(), net.device
    rgb = ref.test_images()(203, 117, 11)
    H, W = rgb.shape[:2]
    src = torch.from_numpy(rgb).to(dev)
    cc = torch.empty(H, 3 * W, 2, dtype=torch.uint8, device=dev)
    yp = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (3 * H, 3 * W), dtype=np.uint8)).to(dev)
    out = torch.empty(3 * H, 3 * W, 3, dtype=torch.uint8, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    lib.check(L.lcm_sr_chroma_h(_p(src), W, H, 3, _p(cc), s))
    lib.check(L.lcm_sr_merge(_p(yp), _p(cc), W, H, 3, _p(out), s))
    cc, out, yp = cc.cpu().numpy(), out.cpu().numpy(), yp.cpu().numpy()
    mine = ref.rgb_to_ycc(rgb)
    pil = np.asarray(Image.fromarray(rgb).convert("YCbCr"))
    for ch, name in ((1, "Cb"), (2, "Cr")):
        exact_h = np.asarray(Image.fromarray(mine[..., ch]).resize((3 * W, H), Image.BICUBIC))
        np.testing.assert_array_equal(cc[..., ch - 1], exact_h)
        pil_h = np.asarray(Image.fromarray(pil[..., ch]).resize((3 * W, H), Image.BICUBIC))
        d = np.abs(cc[..., ch - 1].astype(int) - pil_h)
        print(f"{name} horizontal x3 vs PIL's plane: exact {100 * (d == 0).mean():.2f} %, max |d| {d.max()}")
        # the planes differ by <= 1 (tests/test_superres_cpu.py); the x3 bicubic's weights have sum |w| <= 1.15, so the resampled
        # difference is < 1.15 + 1 (rounding of each side's fixed-point result) -- at most 2
        assert d.max() <= 2
    full = [np.asarray(Image.fromarray(cc[..., i]).resize((3 * W, 3 * H), Image.BICUBIC, box=(0, 0, 3 * W, H))) for i in (0, 1)]
    np.testing.assert_array_equal(out, ref.ycc_to_rgb(np.stack([yp, full[0], full[1]], -1)))


SHAPES = [(64, 64), (225, 224), (512, 512), (640, 360)]


# Per-channel bound against the CPU restatement (PIL colour): 1 from Y (truncation near an integer, test_every_launch_against_fp64)
# plus the chroma: the kernels' Cb / Cr tables are within 1 of PIL's, PIL's bicubic x3 turns that into at most 2
# (test_chroma_against_pil), amplified by at most 1.772 in YCbCr -> RGB (3.54), plus 1 for the inverse tables: 1 + 3.54 + 1 -> 5.
# The issue's 4 assumed an exact chroma plane; measured: 4 of 63.7 M channel values of the 4608^2 pass reach 5, none above.
TOL = 5


def _print_dist(tag, d):
    hist = np.bincount(d.ravel(), minlength=5)
    print(f"{tag}: max |d| {d.max()}, histogram {hist.tolist()}")


@pytest.mark.parametrize("w,h", SHAPES)
def test_pass_against_cpu_restatement(net, w, h):
    rgb = ref.test_images()(w, h, w + h)
    got = net.upscale_rgb(rgb, 1)
    want = ref.upscale_once(net.sd, rgb, 224)
    assert got.shape == (3 * h, 3 * w, 3)
    d = np.abs(got.astype(np.int16) - want).astype(np.int64)
    _print_dist(f"{w}x{h} x3", d)
    assert d.max() <= TOL


@pytest.mark.parametrize("w,mag", [(512, 2), (64, 3)])
def test_multi_pass_against_cpu_restatement(net, w, mag):
    """Each later pass is restated from the GPU's previous pass (the reference re-decodes its own lossless output; feeding
    the CPU chain its own intermediate would compound the 1-level colour-table differences of the earlier passes)."""
    rgb = ref.test_images()(w, w, 3)
    got = net.upscale_rgb(rgb, mag)
    assert got.shape == (w * 3 ** mag, w * 3 ** mag, 3)
    prev = net.upscale_rgb(rgb, mag - 1)
    want = ref.upscale_once(net.sd, prev, 224)
    d = np.abs(got.astype(np.int16) - want).astype(np.int64)
    _print_dist(f"{w}^2 magnitude {mag}", d)
    assert d.max() <= TOL
    assert np.array_equal(net.upscale_rgb(prev, 1), got)          # device chaining == re-running on the decoded image


def test_deterministic_across_calls_workers_threads_and_chunking(monkeypatch):
    from sdlcm_amd.backends.sr_worker import HipSuperResWorker
    from sdlcm_amd import superres as S
    rgb = ref.test_images()(640, 360, 5)
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, format="PNG")
    data = buf.getvalue()
    w0, w1 = HipSuperResWorker(0, "synthetic", 224, 672), HipSuperResWorker(1, "synthetic", 224, 672)
    first = w0.upscale_bytes(data, magnitude=1, out_format="png", quality=92)
    assert w0.upscale_bytes(data, magnitude=1, out_format="png", quality=92) == first
    assert w1.upscale_bytes(data, magnitude=1, out_format="png", quality=92) == first
    res = [None, None]

    def run(i, wk):
        res[i] = wk.upscale_bytes(data, magnitude=1, out_format="png", quality=92)
    ts = [threading.Thread(target=run, args=(i, wk)) for i, wk in enumerate((w0, w1))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert res[0] == first and res[1] == first
    one = S.SuperResNet("synthetic", "cuda:0", 224, 672, ws_mb=1)
    assert one.tiles_per_chunk(224, 224) == 1
    assert np.array_equal(one.upscale_rgb(rgb, 1), ref.decode(first))
    w0.close()
    w1.close()


def test_worker_formats_and_errors():
    from sdlcm_amd.backends.sr_worker import HipSuperResWorker
    wk = HipSuperResWorker(0, "synthetic", 224, 672)
    rgb = ref.test_images()(96, 80, 2)
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, format="PNG")
    data = buf.getvalue()
    j1 = wk.upscale_bytes(data, magnitude=1, out_format="jpeg", quality=92)
    j2 = wk.upscale_bytes(data, magnitude=1, out_format="jpeg", quality=40)
    assert j1[:2] == b"\xff\xd8" and j1 != j2
    assert Image.open(io.BytesIO(j1)).size == (288, 240)
    png = wk.upscale_once(data)
    assert np.array_equal(ref.decode(png), wk.upscale_rgb(rgb, 1))
    for m in (0, 4):
        with pytest.raises(RuntimeError, match=r"magnitude must be 1\.\.3"):
            wk.upscale_bytes(data, magnitude=m, out_format="png", quality=92)
    big = np.zeros((3000, 3000, 3), np.uint8)
    with pytest.raises(RuntimeError, match=r"Image too large: 9000x9000 exceeds SR_MAX_PIXELS=24000000"):
        wk.upscale_rgb(big, 2)                                      # refused before the first pass runs
    wk.close()
