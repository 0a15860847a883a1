"""Super-resolution worker, host side: tile plan and ownership, the ONNX / safetensors weight readers, argument errors (Python and
C ABI, no launch), and the integer colour formulas of csrc/sr.hip against PIL on every colour."""
import numpy as np
import pytest
import torch
from PIL import Image

import sr_reference as ref
from sdlcm_amd import superres as S

SIZES = [(224, 224), (225, 225), (447, 447), (448, 448), (512, 512), (1536, 1536), (640, 360), (100, 100), (64, 300)]


def kernel_owner_map(w, h, tile):
    """The kernels' closed form (csrc/sr.hip tile_start / tile_owner) evaluated on the host."""
    tw, th = min(tile, w), min(tile, h)
    nx, ny = -(-w // tw), -(-h // th)
    gx, gy = np.arange(w), np.arange(h)
    ox = np.where(gx >= w - tw, nx - 1, gx // tw)
    oy = np.where(gy >= h - th, ny - 1, gy // th)
    return oy[:, None] * nx + ox[None, :], [min(i * tw, w - tw) for i in range(nx)], [min(i * th, h - th) for i in range(ny)]


@pytest.mark.parametrize("w,h", SIZES)
def test_tile_plan_and_ownership_match_painting_order(w, h):
    ids, xs, ys = kernel_owner_map(w, h, 224)
    assert xs == ref.plan_axis(w, min(224, w)) == S.tile_plan(w, min(224, w))
    assert ys == ref.plan_axis(h, min(224, h)) == S.tile_plan(h, min(224, h))
    painted = ref.owner_map(w, h, 224)
    assert (painted >= 0).all()
    np.testing.assert_array_equal(ids, painted)


# ---- a protobuf writer for ONNX fixtures in the model zoo's layout ---------------------------------------------------------
def _vint(v):
    v &= (1 << 64) - 1
    out = bytearray()
    while True:
        b = v & 0x7F
        v >>= 7
        out.append(b | (0x80 if v else 0))
        if not v:
            return bytes(out)


def _f(num, payload):                      # length-delimited field
    return _vint(num << 3 | 2) + _vint(len(payload)) + payload


def _fi(num, v):                           # varint field
    return _vint(num << 3) + _vint(v)


def _tensor(name, a, raw=True):
    a = np.asarray(a)
    body = b"".join(_fi(1, d) for d in a.shape)
    if a.dtype == np.int64:
        body += _fi(2, 7) + _f(8, name.encode()) + _f(9, a.astype("<i8").tobytes())
    else:
        body += _fi(2, 1) + _f(8, name.encode())
        body += _f(9, a.astype("<f4").tobytes()) if raw else _f(4, a.astype("<f4").tobytes())
    return body


def _attr_ints(name, vals):
    return _f(5, _f(1, name.encode()) + b"".join(_fi(8, v) for v in vals) + _fi(20, 7))


def _node(op, ins, outs, attrs=b""):
    return b"".join(_f(1, i.encode()) for i in ins) + b"".join(_f(2, o.encode()) for o in outs) + _f(4, op.encode()) + attrs


def make_onnx(path, sd, raw=True, perm=(0, 1, 4, 2, 5, 3), drop_conv=None, bad_shape=None):
    nodes, inits, x = [], [], "input"
    for i, (k, p) in enumerate(((5, 2), (3, 1), (3, 1), (3, 1)), 1):
        if drop_conv == i:
            continue
        w = sd[f"conv{i}.weight"].numpy()
        if bad_shape == i:
            w = w[:, :, :-1, :]
        wn, bn = f"W{i}_{np.random.randint(1 << 30)}", f"B{i}"          # names carry no meaning: read by node order
        inits += [_tensor(wn, w, raw), _tensor(bn, sd[f"conv{i}.bias"].numpy(), raw)]
        attrs = _attr_ints("kernel_shape", [k, k]) + _attr_ints("pads", [p] * 4) + _attr_ints("strides", [1, 1])
        nodes.append(_node("Conv", [x, wn, bn], [f"c{i}"], attrs))
        x = f"c{i}"
        if i < 4:
            nodes.append(_node("Relu", [x], [f"r{i}"]))
            x = f"r{i}"
    inits += [_tensor("s1", np.array([-1, 1, 3, 3, 224, 224], np.int64)), _tensor("s2", np.array([-1, 1, 672, 672], np.int64))]
    nodes += [_node("Reshape", [x, "s1"], ["rs"]), _node("Transpose", ["rs"], ["tr"], _attr_ints("perm", list(perm))),
              _node("Reshape", ["tr", "s2"], ["output"])]
    graph = b"".join(_f(1, n) for n in nodes) + _f(2, b"torch-jit-export") + b"".join(_f(5, t) for t in inits)
    model = _fi(1, 7) + _f(2, b"pytorch") + _f(7, graph) + _f(8, _f(1, b"") + _fi(2, 10))
    with open(path, "wb") as fh:
        fh.write(model)
    return path


@pytest.mark.parametrize("raw", [True, False])
def test_onnx_reader_zoo_layout(tmp_path, raw):
    sd = S.synthetic_weights(3)
    got = S.read_onnx(make_onnx(str(tmp_path / "sr.onnx"), sd, raw=raw))
    assert sorted(got) == sorted(sd)
    for k in sd:
        assert torch.equal(got[k], sd[k].float()), k


def test_onnx_reader_refuses_other_graphs(tmp_path):
    sd = S.synthetic_weights(3)
    with pytest.raises(ValueError, match=r"conv2 has weight \(64, 64, 2, 3\)"):
        S.read_onnx(make_onnx(str(tmp_path / "a.onnx"), sd, bad_shape=2))
    with pytest.raises(ValueError, match="expected 4 Conv nodes .* found 3"):
        S.read_onnx(make_onnx(str(tmp_path / "b.onnx"), sd, drop_conv=3))
    with pytest.raises(ValueError, match=r"perm \[0, 1, 4, 2, 5, 3\], found \[\[0, 1, 2, 4, 3, 5\]\]"):
        S.read_onnx(make_onnx(str(tmp_path / "c.onnx"), sd, perm=(0, 1, 2, 4, 3, 5)))


def test_model_path_resolution_and_safetensors(tmp_path):
    from safetensors.torch import save_file
    sd = S.synthetic_weights(5)
    rk = str(tmp_path / "super-resolution-10.rknn")
    with pytest.raises(FileNotFoundError) as e:
        S.resolve_model_path(rk)
    for p in (rk, str(tmp_path / "super-resolution-10.onnx"), str(tmp_path / "super-resolution-10.safetensors")):
        assert p in str(e.value)
    st = str(tmp_path / "super-resolution-10.safetensors")
    save_file({k: v.contiguous() for k, v in sd.items()}, st)
    assert S.resolve_model_path(rk) == st
    onnx = make_onnx(str(tmp_path / "super-resolution-10.onnx"), sd)
    assert S.resolve_model_path(rk) == onnx                         # .onnx before .safetensors
    a, b = S.load_weights(rk), S.load_weights(st)
    for k in sd:
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], sd[k].float()), k
    with pytest.raises(FileNotFoundError, match="tried"):
        S.load_weights(str(tmp_path / "nothing.onnx"))


def test_argument_errors():
    for m in (0, 4):
        with pytest.raises(RuntimeError, match=r"^magnitude must be 1\.\.3$"):
            S.check_magnitude(m)
    with pytest.raises(RuntimeError, match=r"^Image too large: 5000x5000 exceeds SR_MAX_PIXELS=24000000$"):
        S.check_pixels(5000, 5000, 24000000)
    S.check_pixels(4898, 4898, 24000000)
    from sdlcm_amd.backends import sr_worker
    with pytest.raises(RuntimeError, match="out_format must be 'png' or 'jpeg'"):
        sr_worker._check_format("webp")
    with pytest.raises(ValueError, match="scale of exactly 3"):
        S.SuperResNet("synthetic", "cpu", 224, 448)


def test_c_abi_sr_argument_validation_without_gpu():
    import ctypes as C
    from sdlcm_amd import lib
    L = lib.load()
    buf = C.create_string_buffer(64)
    p = C.cast(buf, C.c_void_p)
    p = C.c_void_p((p.value + 15) // 16 * 16)
    cases = [
        (lambda: L.lcm_sr_conv1(None, 8, 8, 8, 8, 0, 1, p, p, p, None), b"null pointer"),
        (lambda: L.lcm_sr_conv1(p, 8, 8, 0, 8, 0, 1, p, p, p, None), b"at least 1x1"),
        (lambda: L.lcm_sr_conv1(p, 8, 8, 9, 8, 0, 1, p, p, p, None), b"larger than the image"),
        (lambda: L.lcm_sr_conv1(p, 9, 8, 8, 8, 1, 2, p, p, p, None), b"outside the plan's 2 tiles"),
        (lambda: L.lcm_sr_conv3x3(p, 1, 8, 8, 48, p, p, p, None), b"cout=48 not supported"),
        (lambda: L.lcm_sr_conv3x3(p, 0, 8, 8, 64, p, p, p, None), b"T=0"),
        (lambda: L.lcm_sr_conv4_shuffle(p, 8, 8, 8, 8, 0, 1, p, p, 2, p, None), b"upscale factor 2 not supported"),
        (lambda: L.lcm_sr_conv4_shuffle(p, 8, 8, 8, 8, 0, 1, None, p, 3, p, None), b"null pointer"),
        (lambda: L.lcm_sr_chroma_h(p, 8, 8, 4, p, None), b"upscale factor 4"),
        (lambda: L.lcm_sr_chroma_h(p, 0, 8, 3, p, None), b"out of range"),
        (lambda: L.lcm_sr_merge(p, None, 8, 8, 3, p, None), b"null pointer"),
    ]
    for call, msg in cases:
        assert call() == -1 and msg in L.lcm_last_error(), (msg, L.lcm_last_error())


def _all_colours():
    c = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(c >> 16) & 255, (c >> 8) & 255, c & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)


def test_colour_formulas_against_pil_on_every_colour():
    rgb = _all_colours()
    pil = np.asarray(Image.fromarray(rgb).convert("YCbCr"))
    mine = ref.rgb_to_ycc(rgb)
    np.testing.assert_array_equal(mine[..., 0], pil[..., 0])                     # Y: exact
    for ch, name in ((1, "Cb"), (2, "Cr")):
        d = np.abs(mine[..., ch].astype(np.int16) - pil[..., ch])
        print(f"{name}: exact on {100 * (d == 0).mean():.3f} % of colours, max |d| {d.max()}")
        assert d.max() <= 1
    ycc = rgb                                                                  # every (Y, Cb, Cr) triple
    pil = np.asarray(Image.fromarray(ycc, "YCbCr").convert("RGB"))
    mine = ref.ycc_to_rgb(ycc)
    for ch, name in enumerate("RGB"):
        d = np.abs(mine[..., ch].astype(np.int16) - pil[..., ch])
        print(f"YCbCr->{name}: exact on {100 * (d == 0).mean():.3f} % of triples, max |d| {d.max()}")
        assert d.max() <= 1


def test_synthetic_weights_keep_y_inside_the_unit_interval():
    sd = S.load_weights("synthetic")
    mk = ref.test_images()
    for w, h in ((64, 64), (225, 224), (640, 360)):
        y = ref.y_float(sd, mk(w, h, 1), 224, torch.float32)
        frac = float(((y > 0) & (y < 1)).mean())
        print(f"{w}x{h}: {100 * frac:.2f} % of pre-clip Y inside (0, 1)")
        assert frac >= 0.9
