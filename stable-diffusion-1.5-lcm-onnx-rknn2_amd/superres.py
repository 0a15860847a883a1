"""Super-resolution post-process on the MI355X: the HIP replacement for the server's RKNN ``SuperResWorker``
(server/lcm_sr_server.py:312-405).

The model is the ONNX model zoo's ``super-resolution-10`` (sub-pixel CNN): conv1 5x5 1->64, conv2 3x3 64->64, conv3 3x3 64->32
(each + ReLU), conv4 3x3 32->r*r, pixel shuffle r (r = 3).  A pass runs it on the luma plane of the image cut into independent
``input_size`` tiles (the reference's tile plan and row-major overwrite order, seams included), upscales Cb / Cr with PIL's
bicubic and merges -- all on the device (csrc/sr.hip).  Deliberate deviations from the reference:

  * an image side shorter than the tile is run at its own size (the network is fully convolutional; the NPU model's fixed
    224x224 input cannot take such an image at all), e.g. the 64x64 previews;
  * between the passes of ``magnitude`` > 1 the image stays on the device as uint8 RGB.  For PNG this is the reference's lossless
    round trip; for JPEG only the final image is encoded (the reference re-encodes every pass, losing quality each time);
  * JPEG output is written by the library (``JpegEncoder``: csrc/jpeg.hip + csrc/jpeg.cpp), not by PIL: same tables, sampling
    and Huffman tables as PIL's default, a float DCT and one restart interval per MCU row, so the bytes differ from PIL's.
"""
from __future__ import annotations

import math
import os
import struct

import numpy as np
import torch

from . import lib as _lib

R = 3                                   # the upscale factor the kernels implement
_LAYERS = (("conv1", 64, 1, 5), ("conv2", 64, 64, 3), ("conv3", 32, 64, 3), ("conv4", R * R, 32, 3))
SHUFFLE_PERM = (0, 1, 4, 2, 5, 3)       # Reshape [1,1,r,r,H,W] -> Transpose -> Reshape [1,1,rH,rW]


def max_pixels() -> int:
    return int(os.environ.get("SR_MAX_PIXELS", "24000000"))


def check_pixels(w: int, h: int, limit: int | None = None) -> None:
    limit = max_pixels() if limit is None else limit
    if w * h > limit:
        raise RuntimeError(f"Image too large: {w}x{h} exceeds SR_MAX_PIXELS={limit}")      # lcm_sr_server.py:354-357


def check_magnitude(magnitude) -> int:
    mag = int(magnitude)
    if mag < 1 or mag > 3:
        raise RuntimeError("magnitude must be 1..3")                                      # lcm_sr_server.py:400-401
    return mag


def check_quality(quality) -> int:
    q = int(quality)
    if q < 1 or q > 100:
        raise RuntimeError("quality must be 1..100")
    return q


def jpeg_threads() -> int:
    """Restart intervals coded at a time (csrc/jpeg.cpp).  The file's bytes do not depend on it."""
    return max(1, int(os.environ.get("LCM_JPEG_THREADS", "8")))


# Which JPEG inputs the library decodes when LCM_JPEG_DECODER is not set: "hip" = every supported file, "dri" = only files
# with restart markers (their entropy decoding runs on LCM_JPEG_THREADS threads), "pil" = none.  "pil" until the gate of
# DESIGN.md section 7 ("JPEG input") has been measured on an MI355X: no such measurement exists yet.
JPEG_DECODER_DEFAULT = "pil"


def jpeg_decoder_mode() -> str:
    """LCM_JPEG_DECODER: "pil" (PIL decodes every input, as before the library had a decoder), "hip", "dri"; anything else,
    or unset, is JPEG_DECODER_DEFAULT."""
    m = os.environ.get("LCM_JPEG_DECODER", "").lower()
    return m if m in ("pil", "hip", "dri") else JPEG_DECODER_DEFAULT


def tile_plan(size: int, tile: int) -> list:
    """Tile starts along one axis (lcm_sr_server.py _plan_tiles): 0, t, 2t, ... while a whole tile fits, then size - t.
    ``tile`` is the tile side actually used: min(input_size, size)."""
    xs = list(range(0, max(1, size - tile + 1), tile))
    if not xs or xs[-1] != size - tile:
        xs.append(max(0, size - tile))
    return xs


# ------------------------------------------------------------------------------------------------------------------------
# weights
# ------------------------------------------------------------------------------------------------------------------------
def _varint(buf, i):
    v = s = 0
    while True:
        b = buf[i]
        i += 1
        v |= (b & 0x7F) << s
        s += 7
        if b < 0x80:
            return v, i


def _fields(buf):
    """Yields (field number, wire type, value) of one protobuf message: ints for varints, bytes for fixed and length-
    delimited fields."""
    i, n = 0, len(buf)
    while i < n:
        key, i = _varint(buf, i)
        f, wt = key >> 3, key & 7
        if wt == 0:
            v, i = _varint(buf, i)
        elif wt == 1:
            v, i = buf[i:i + 8], i + 8
        elif wt == 2:
            ln, i = _varint(buf, i)
            v, i = buf[i:i + ln], i + ln
        elif wt == 5:
            v, i = buf[i:i + 4], i + 4
        else:
            raise ValueError(f"ONNX: unsupported protobuf wire type {wt}")
        if i > n:
            raise ValueError("ONNX: truncated protobuf message")
        yield f, wt, v


def _ints(wt, v):
    if wt == 0:
        return [v - (1 << 64) if v >= 1 << 63 else v]
    out, i = [], 0
    while i < len(v):                    # packed repeated int64
        x, i = _varint(v, i)
        out.append(x - (1 << 64) if x >= 1 << 63 else x)
    return out


def _tensor(buf):
    """TensorProto -> (name, float32 ndarray).  FLOAT tensors (raw_data or float_data) and INT64 (shape constants)."""
    dims, dtype, name, raw, fdata, idata = [], 1, "", None, [], []
    for f, wt, v in _fields(buf):
        if f == 1:
            dims += _ints(wt, v)
        elif f == 2:
            dtype = v
        elif f == 4:
            fdata.append(np.frombuffer(bytes(v), "<f4"))
        elif f == 7:
            idata += _ints(wt, v)
        elif f == 8:
            name = bytes(v).decode()
        elif f == 9:
            raw = bytes(v)
    if dtype == 1:
        a = np.frombuffer(raw, "<f4") if raw is not None else (np.concatenate(fdata) if fdata else np.zeros(0, np.float32))
    elif dtype == 7:
        a = np.frombuffer(raw, "<i8") if raw is not None else np.asarray(idata, np.int64)
    else:
        raise ValueError(f"ONNX: tensor {name!r} has data_type {dtype}; only FLOAT and INT64 are read")
    n = int(np.prod(dims)) if dims else 1
    if a.size != n:
        raise ValueError(f"ONNX: tensor {name!r} holds {a.size} values for dims {dims}")
    return name, a.reshape(dims).copy()


def _node(buf):
    node = {"input": [], "output": [], "op": "", "attrs": {}}
    for f, wt, v in _fields(buf):
        if f == 1:
            node["input"].append(bytes(v).decode())
        elif f == 2:
            node["output"].append(bytes(v).decode())
        elif f == 4:
            node["op"] = bytes(v).decode()
        elif f == 5:
            an, ints, t = "", [], None
            for g, gwt, gv in _fields(v):
                if g == 1:
                    an = bytes(gv).decode()
                elif g in (3, 8):
                    ints += _ints(gwt, gv)
                elif g == 5:
                    t = _tensor(gv)[1]
            node["attrs"][an] = t if t is not None else ints
    return node


def read_onnx(path: str) -> dict:
    """Minimal ONNX reader for super-resolution-10: ModelProto -> graph -> nodes / initializers.  W and B come from the Conv
    nodes in graph order (initializer names are not relied on); kernel sizes, pads, strides, shapes and the pixel-shuffle
    transpose are checked.  -> {conv1.weight, conv1.bias, ..., conv4.bias} as float32 torch tensors."""
    with open(path, "rb") as f:
        buf = memoryview(f.read())
    graph = None
    for fld, _, v in _fields(buf):
        if fld == 7:
            graph = v
    if graph is None:
        raise ValueError(f"ONNX {path}: no graph in the model")
    inits, nodes = {}, []
    for fld, _, v in _fields(graph):
        if fld == 1:
            nodes.append(_node(v))
        elif fld == 5:
            name, a = _tensor(v)
            inits[name] = a
    for n in nodes:                      # Constant nodes feed Reshape shapes in some exports
        if n["op"] == "Constant" and "value" in n["attrs"] and n["output"]:
            inits[n["output"][0]] = n["attrs"]["value"]
    convs = [n for n in nodes if n["op"] == "Conv"]
    if len(convs) != len(_LAYERS):
        raise ValueError(f"ONNX {path}: expected {len(_LAYERS)} Conv nodes (super-resolution-10), found {len(convs)}")
    sd = {}
    for n, (name, cout, cin, k) in zip(convs, _LAYERS):
        if len(n["input"]) < 3 or n["input"][1] not in inits or n["input"][2] not in inits:
            raise ValueError(f"ONNX {path}: {name} needs weight and bias initializers")
        w, b = inits[n["input"][1]], inits[n["input"][2]]
        if tuple(w.shape) != (cout, cin, k, k) or tuple(b.shape) != (cout,):
            raise ValueError(f"ONNX {path}: {name} has weight {tuple(w.shape)} / bias {tuple(b.shape)}, expected "
                             f"({cout}, {cin}, {k}, {k}) / ({cout},)")
        a = n["attrs"]
        ks = list(a.get("kernel_shape", [k, k]))
        pads = list(a.get("pads", [0, 0, 0, 0]))
        strides = list(a.get("strides", [1, 1]))
        dil = list(a.get("dilations", [1, 1]))
        if ks != [k, k] or pads != [k // 2] * 4 or strides != [1, 1] or dil != [1, 1] or a.get("group", [1]) != [1]:
            raise ValueError(f"ONNX {path}: {name} has kernel_shape {ks}, pads {pads}, strides {strides}, dilations {dil}; "
                             f"expected {[k, k]}, {[k // 2] * 4}, [1, 1], [1, 1]")
        sd[f"{name}.weight"] = torch.from_numpy(np.ascontiguousarray(w, np.float32))
        sd[f"{name}.bias"] = torch.from_numpy(np.ascontiguousarray(b, np.float32))
    tr = [n for n in nodes if n["op"] == "Transpose"]
    if len(tr) != 1 or tuple(tr[0]["attrs"].get("perm", [])) != SHUFFLE_PERM:
        got = [list(n["attrs"].get("perm", [])) for n in tr]
        raise ValueError(f"ONNX {path}: pixel shuffle must be one Transpose with perm {list(SHUFFLE_PERM)}, found {got}")
    return sd


def check_state_dict(sd: dict) -> dict:
    out = {}
    for name, cout, cin, k in _LAYERS:
        for part, shape in (("weight", (cout, cin, k, k)), ("bias", (cout,))):
            key = f"{name}.{part}"
            if key not in sd:
                raise ValueError(f"super-resolution weights lack {key}")
            t = torch.as_tensor(sd[key]).detach().to("cpu", torch.float32).contiguous()
            if tuple(t.shape) != shape:
                raise ValueError(f"super-resolution weights: {key} has shape {tuple(t.shape)}, expected {shape}")
            out[key] = t
    return out


def synthetic_weights(seed: int = 0) -> dict:
    """Seeded stand-in for super-resolution-10 (no checkpoint ships here).  He-scaled weights with a positive conv1 bias keep
    the activations alive; conv4 is a small perturbation around "copy the input" (each sub-pixel = 0.9 x centre tap of a
    channel that carries the input, + 0.05) so the output stays inside (0, 1) on natural images instead of saturating."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, cout, cin, k in _LAYERS:
        fan = cin * k * k
        sd[f"{name}.weight"] = torch.randn(cout, cin, k, k, generator=g) * math.sqrt(2.0 / fan) * (0.5 if name == "conv4" else 1.0)
        sd[f"{name}.bias"] = torch.randn(cout, generator=g) * 0.02
    # a pass-through path: conv1 channel 0 = input (centre tap), conv2 ch 0 and conv3 ch 0 copy it, conv4 reads it
    for name, k in (("conv1", 5), ("conv2", 3), ("conv3", 3)):
        w = sd[f"{name}.weight"]
        w[0].zero_()
        w[0, 0, k // 2, k // 2] = 1.0
        sd[f"{name}.bias"][0] = 0.0
    w4 = sd["conv4.weight"] * 0.02
    w4[:, 0, 1, 1] += 0.9
    sd["conv4.weight"] = w4
    sd["conv4.bias"] = torch.full((R * R,), 0.05) + torch.randn(R * R, generator=g) * 0.005
    return sd


def resolve_model_path(path: str) -> str:
    """A ``.rknn`` path (the server's default SR_MODEL_PATH) resolves to a sibling ``.onnx`` with the same stem, then to a
    ``.safetensors``.  Raises naming every path tried."""
    if path.endswith(".rknn"):
        stem = path[:-len(".rknn")]
        tried = [path]
        for cand in (stem + ".onnx", stem + ".safetensors"):
            tried.append(cand)
            if os.path.isfile(cand):
                return cand
        raise FileNotFoundError("super-resolution model: an .rknn file cannot run on this backend and no sibling was found; "
                                f"tried {', '.join(tried)}")
    if not os.path.isfile(path):
        raise FileNotFoundError(f"super-resolution model not found: tried {path}")
    return path


def load_weights(model_path: str) -> dict:
    """``synthetic`` | ``.onnx`` | ``.safetensors`` / torch state dict (PyTorch SuperResolutionNet layout) | ``.rknn`` (sibling)."""
    if model_path == "synthetic" or model_path.startswith("synthetic:"):
        seed = int(model_path.split(":", 1)[1]) if ":" in model_path else 0
        return check_state_dict(synthetic_weights(seed))
    path = resolve_model_path(model_path)
    if path.endswith(".onnx"):
        return check_state_dict(read_onnx(path))
    if path.endswith(".safetensors"):
        from safetensors.torch import load_file
        return check_state_dict(load_file(path))
    return check_state_dict(torch.load(path, map_location="cpu", weights_only=True))


def pack_weights(sd: dict) -> dict:
    """fp32 state dict -> the kernels' layouts (include/lcm_hip.h, super-resolution): fp16 weights, fp32 biases (CPU)."""
    w1 = sd["conv1.weight"].reshape(64, 25).t().contiguous()                       # [tap][64]
    w2 = sd["conv2.weight"].permute(0, 2, 3, 1).contiguous()                       # [Cout][ky][kx][Cin]
    w3 = sd["conv3.weight"].permute(0, 2, 3, 1).contiguous()
    w4 = sd["conv4.weight"].permute(2, 3, 1, 0).contiguous()                       # [ky][kx][Cin][r*r]
    return {"w1": w1.half(), "b1": sd["conv1.bias"].float(), "w2": w2.half(), "b2": sd["conv2.bias"].float(),
            "w3": w3.half(), "b3": sd["conv3.bias"].float(), "w4": w4.half(), "b4": sd["conv4.bias"].float()}


def _ptr(t) -> int:
    return t.data_ptr()


class JpegEncoder:
    """Device RGB8 -> baseline 4:2:0 JPEG file bytes: ``lcm_jpeg_dct_rgb8`` (csrc/jpeg.hip) on the caller's stream, the
    coefficients into a pinned host buffer, ``lcm_jpeg_encode_coefs`` (csrc/jpeg.cpp) on the host.  The pixels never cross to
    the host.  The pinned buffer and the output buffer are kept between calls (they grow to the largest image seen), so an
    instance serves one thread at a time."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.L = _lib.load()
        self._pinned = None
        self._out = None

    def encode_device(self, rgb, quality: int, stream) -> bytes:
        """rgb: uint8 [H][W][3] device tensor whose rows are dense (any row pitch), produced on ``stream``."""
        import ctypes
        q = check_quality(quality)
        if rgb.dtype != torch.uint8 or rgb.dim() != 3 or rgb.shape[2] != 3 or rgb.stride(2) != 1 or rgb.stride(1) != 3:
            raise ValueError(f"JPEG encoder expects a uint8 [H][W][3] device tensor with dense rows, got {tuple(rgb.shape)} "
                             f"{rgb.dtype} strides {tuple(rgb.stride())}")
        L = self.L
        H, W = int(rgb.shape[0]), int(rgb.shape[1])
        nbytes = int(L.lcm_jpeg_coef_bytes(W, H))
        if nbytes <= 0:
            raise RuntimeError(f"JPEG cannot hold a {W}x{H} image (1..65535 a side)")
        if self._pinned is None or self._pinned.numel() * 2 < nbytes:
            self._pinned = torch.empty(nbytes // 2, dtype=torch.int16, pin_memory=True)
        host = self._pinned[:nbytes // 2]
        with torch.cuda.device(self.device), torch.cuda.stream(stream):
            coefs = torch.empty(nbytes // 2, dtype=torch.int16, device=self.device)
            _lib.check(L.lcm_jpeg_dct_rgb8(_ptr(rgb), W, H, int(rgb.stride(0)), q, _ptr(coefs), nbytes, stream.cuda_stream),
                       "lcm_jpeg_dct_rgb8")
            host.copy_(coefs, non_blocking=True)
        stream.synchronize()
        cap = int(L.lcm_jpeg_bound(W, H))
        if self._out is None or self._out.size < cap:
            self._out = np.empty(cap, np.uint8)          # a worst-case bound: only the pages the file touches become real
        n = ctypes.c_longlong(0)
        _lib.check(L.lcm_jpeg_encode_coefs(host.data_ptr(), W, H, q, jpeg_threads(), self._out.ctypes.data, self._out.size,
                                           ctypes.byref(n)), "lcm_jpeg_encode_coefs")
        return self._out[:n.value].tobytes()


class JpegDecoder:
    """JPEG file bytes -> uint8 [H][W][3] device tensor: ``lcm_jpeg_dec_info`` / ``lcm_jpeg_dec_coefs`` (csrc/jpeg_dec.cpp) on the
    host into a pinned buffer, the copy of the coefficients and ``lcm_jpeg_idct_rgb8`` (csrc/jpeg_dec.hip) on the caller's
    stream.  The pixels are PIL's ``Image.open(...).convert("RGB")`` byte for byte and never exist on the host.  The pinned
    buffer is kept between calls (it grows to the largest image seen), so an instance serves one thread at a time."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.L = _lib.load()
        self._pinned = None
        self._copied = None              # event after the last copy out of the pinned buffer

    def header(self, data):
        """-> lib.JpegInfo, or None for anything the library does not decode (progressive, CMYK, ...; not a JPEG at all)."""
        import ctypes
        info = _lib.JpegInfo()
        rc = self.L.lcm_jpeg_dec_info(data, len(data), ctypes.byref(info))
        return info if rc == 0 else None

    def decode_device(self, data, stream, magnitude: int = 0, mode: str = "hip"):
        """None = unsupported or corrupt: the caller decodes with PIL (every file PIL read before is still read, and what it
        refused is still refused by it).  With ``magnitude`` >= 1, SR_MAX_PIXELS is checked for every pass from the header,
        before anything is decoded.  ``mode`` "dri": files without restart markers are left to the caller as well."""
        import ctypes
        data = bytes(data)
        info = self.header(data)
        if info is None or (mode == "dri" and info.restart_interval == 0):
            return None
        W, H = int(info.width), int(info.height)
        from PIL import Image
        if Image.MAX_IMAGE_PIXELS is not None and W * H > Image.MAX_IMAGE_PIXELS:
            return None                  # PIL warns about, or refuses, an image of this size: that stays PIL's business
        limit = max_pixels()
        for k in range(int(magnitude)):
            check_pixels(W * R ** k, H * R ** k, limit)
        L = self.L
        nbytes = int(info.coefs_bytes)
        if self._copied is not None:
            self._copied.synchronize()   # the previous call's copy has left the pinned buffer
        if self._pinned is None or self._pinned.numel() * 2 < nbytes:
            self._pinned = torch.empty(nbytes // 2, dtype=torch.int16, pin_memory=True)
        host = self._pinned[:nbytes // 2]
        if L.lcm_jpeg_dec_coefs(data, len(data), jpeg_threads(), host.data_ptr(), nbytes) != 0:
            return None
        with torch.cuda.device(self.device), torch.cuda.stream(stream):
            coefs = torch.empty(nbytes // 2, dtype=torch.int16, device=self.device)
            coefs.copy_(host, non_blocking=True)
            if self._copied is None:
                self._copied = torch.cuda.Event()
            self._copied.record(stream)
            work = torch.empty(int(info.work_bytes), dtype=torch.uint8, device=self.device)
            out = torch.empty(H, W, 3, dtype=torch.uint8, device=self.device)
            _lib.check(L.lcm_jpeg_idct_rgb8(_ptr(coefs), nbytes, ctypes.byref(info), _ptr(work), int(info.work_bytes), _ptr(out),
                                            3 * W, stream.cuda_stream), "lcm_jpeg_idct_rgb8")
        return out


class SuperResNet:
    """Device-resident super-resolution-10 (weights packed to fp16 once) and the pass driver.  One instance per worker: it
    owns a stream; a call allocates its workspace on that stream, so instances may run on several threads at once."""

    def __init__(self, model_path: str, device="cuda:0", input_size: int = 224, output_size: int = 672, ws_mb: int | None = None):
        if int(output_size) != R * int(input_size):
            raise ValueError(f"super-resolution: output_size / input_size = {output_size}/{input_size}; the kernels "
                             f"implement a scale of exactly {R}")
        if not torch.cuda.is_available():
            raise _lib.LcmHipError("super-resolution needs an MI355X; no CPU fallback exists on this path")
        self.tile = int(input_size)
        if self.tile < 1:
            raise ValueError(f"super-resolution: input_size {input_size} must be at least 1")
        self.device = torch.device(device)
        self.L = _lib.load()
        self.sd = load_weights(model_path)
        with torch.cuda.device(self.device):
            self.stream = torch.cuda.Stream(self.device)
            self.w = {k: v.to(self.device) for k, v in pack_weights(self.sd).items()}
        self.jpeg = None                 # JpegEncoder, built by the first upscale_jpeg
        self.jpeg_dec = None             # JpegDecoder, built by the first decode_jpeg
        self.ws_bytes = int(float(os.environ.get("LCM_SR_WS_MB", "1024")) * (1 << 20)) if ws_mb is None else int(ws_mb * (1 << 20))

    def tiles_per_chunk(self, tw: int, th: int) -> int:
        return max(1, self.ws_bytes // (tw * th * 64 * 2 * 2))       # two fp16 [th][tw][64] activation buffers per tile

    def _pass(self, src):
        """One upscale_once on the device: uint8 [H][W][3] -> uint8 [3H][3W][3] (enqueued on self.stream)."""
        L, w, s = self.L, self.w, self.stream.cuda_stream
        H, W = int(src.shape[0]), int(src.shape[1])
        tw, th = min(self.tile, W), min(self.tile, H)
        nx, ny = len(tile_plan(W, tw)), len(tile_plan(H, th))
        nt = nx * ny
        chunk = min(nt, self.tiles_per_chunk(tw, th))
        dev = self.device
        a = torch.empty(chunk * th * tw * 64, dtype=torch.float16, device=dev)
        b = torch.empty(chunk * th * tw * 64, dtype=torch.float16, device=dev)
        yp = torch.empty(R * H, R * W, dtype=torch.uint8, device=dev)
        cc = torch.empty(H, R * W, 2, dtype=torch.uint8, device=dev)
        out = torch.empty(R * H, R * W, 3, dtype=torch.uint8, device=dev)
        _lib.check(L.lcm_sr_chroma_h(_ptr(src), W, H, R, _ptr(cc), s), "lcm_sr_chroma_h")
        for t0 in range(0, nt, chunk):
            n = min(chunk, nt - t0)
            _lib.check(L.lcm_sr_conv1(_ptr(src), W, H, tw, th, t0, n, _ptr(w["w1"]), _ptr(w["b1"]), _ptr(a), s), "lcm_sr_conv1")
            _lib.check(L.lcm_sr_conv3x3(_ptr(a), n, th, tw, 64, _ptr(w["w2"]), _ptr(w["b2"]), _ptr(b), s), "lcm_sr_conv3x3 conv2")
            _lib.check(L.lcm_sr_conv3x3(_ptr(b), n, th, tw, 32, _ptr(w["w3"]), _ptr(w["b3"]), _ptr(a), s), "lcm_sr_conv3x3 conv3")
            _lib.check(L.lcm_sr_conv4_shuffle(_ptr(a), W, H, tw, th, t0, n, _ptr(w["w4"]), _ptr(w["b4"]), R, _ptr(yp), s),
                       "lcm_sr_conv4_shuffle")
        _lib.check(L.lcm_sr_merge(_ptr(yp), _ptr(cc), W, H, R, _ptr(out), s), "lcm_sr_merge")
        return out

    def upscale_device(self, src, magnitude: int):
        """uint8 [H][W][3] device tensor -> device tensor after ``magnitude`` passes, enqueued on self.stream (not synchronised).
        SR_MAX_PIXELS is checked for every pass before any work starts."""
        mag = check_magnitude(magnitude)
        H, W = int(src.shape[0]), int(src.shape[1])
        limit = max_pixels()
        for k in range(mag):
            check_pixels(W * R ** k, H * R ** k, limit)
        with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
            x = src.contiguous()
            for _ in range(mag):
                x = self._pass(x)
        return x

    def upscale_rgb(self, rgb, magnitude: int = 1) -> np.ndarray:
        """uint8 [H][W][3] host array -> uint8 [3^m H][3^m W][3] host array.  Intermediate passes stay on the device."""
        rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
        if rgb.ndim != 3 or rgb.shape[2] != 3:
            raise ValueError(f"upscale_rgb expects uint8 [H][W][3], got shape {rgb.shape}")
        mag = check_magnitude(magnitude)
        for k in range(mag):
            check_pixels(rgb.shape[1] * R ** k, rgb.shape[0] * R ** k)
        with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
            src = torch.from_numpy(rgb).to(self.device, non_blocking=False)
            out = self.upscale_device(src, mag)
            host = out.cpu()
        self.stream.synchronize()
        return host.numpy()

    def upscale_jpeg(self, rgb, magnitude: int = 1, quality: int = 92) -> bytes:
        """uint8 [H][W][3] host array -> JPEG file bytes of the image after ``magnitude`` passes.  The passes, the JPEG front
        end (csrc/jpeg.hip) and the copy of its coefficients run on self.stream; the upscaled RGB stays on the device."""
        rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
        if rgb.ndim != 3 or rgb.shape[2] != 3:
            raise ValueError(f"upscale_jpeg expects uint8 [H][W][3], got shape {rgb.shape}")
        mag = check_magnitude(magnitude)
        q = check_quality(quality)
        for k in range(mag):
            check_pixels(rgb.shape[1] * R ** k, rgb.shape[0] * R ** k)
        if self.jpeg is None:
            self.jpeg = JpegEncoder(self.device)
        with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
            src = torch.from_numpy(rgb).to(self.device, non_blocking=False)
            out = self.upscale_device(src, mag)
        return self.jpeg.encode_device(out, q, self.stream)

    def decode_jpeg(self, data, magnitude: int = 1):
        """JPEG file bytes -> uint8 [H][W][3] device tensor on self.stream (csrc/jpeg_dec.cpp + csrc/jpeg_dec.hip), or None when
        the bytes are not a JPEG the library decodes or LCM_JPEG_DECODER leaves them to PIL.  SR_MAX_PIXELS is checked for
        ``magnitude`` passes from the header before any decoding."""
        mode = jpeg_decoder_mode()
        if mode == "pil" or bytes(data[:2]) != b"\xff\xd8":
            return None
        mag = check_magnitude(magnitude)
        if self.jpeg_dec is None:
            self.jpeg_dec = JpegDecoder(self.device)
        return self.jpeg_dec.decode_device(data, self.stream, mag, mode)

    def upscale_device_rgb(self, src, magnitude: int = 1) -> np.ndarray:
        """upscale_rgb for an image that is already on the device (produced on self.stream): -> host array."""
        mag = check_magnitude(magnitude)
        with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
            host = self.upscale_device(src, mag).cpu()
        self.stream.synchronize()
        return host.numpy()

    def upscale_device_jpeg(self, src, magnitude: int = 1, quality: int = 92) -> bytes:
        """upscale_jpeg for an image that is already on the device (produced on self.stream): no pixel crosses to the host."""
        mag = check_magnitude(magnitude)
        q = check_quality(quality)
        if self.jpeg is None:
            self.jpeg = JpegEncoder(self.device)
        out = self.upscale_device(src, mag)
        return self.jpeg.encode_device(out, q, self.stream)

    def close(self):
        self.w = {}
        self.sd = {}
        self.jpeg = None
        self.jpeg_dec = None
