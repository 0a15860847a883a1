"""CPU restatement of the reference super-resolution worker (server/lcm_sr_server.py upscale_once) for the superres tests:
the tile plan painted in the reference's order, PIL for colour conversion and the chroma resize, and a torch network in fp32 or
fp64.  Written from the semantics, independently of sdlcm_amd.superres."""
import io

import numpy as np
import torch
import torch.nn.functional as F
from PIL import Image


def plan_axis(size, tile):
    xs = list(range(0, max(1, size - tile + 1), tile))
    if not xs or xs[-1] != size - tile:
        xs.append(max(0, size - tile))
    return xs


def owner_map(w, h, tile):
    """Paint tile ids in the reference's order (y outer, x inner; later tiles overwrite): int [h][w] of row-major tile ids.
    A side shorter than the tile uses its own size as the tile side (the HIP path's documented deviation)."""
    tw, th = min(tile, w), min(tile, h)
    xs, ys = plan_axis(w, tw), plan_axis(h, th)
    ids = np.full((h, w), -1, np.int64)
    for yi, y0 in enumerate(ys):
        for xi, x0 in enumerate(xs):
            ids[y0:y0 + th, x0:x0 + tw] = yi * len(xs) + xi
    return ids


def test_images():
    """Gradients + noise + edges at the sizes the GPU tests use (seeded)."""
    def make(w, h, seed):
        rng = np.random.default_rng(seed)
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
        r = 40 + 170 * xx / max(w - 1, 1)
        g = 30 + 180 * yy / max(h - 1, 1)
        b = 128 + 80 * np.sin(xx / 9.0) * np.cos(yy / 13.0)
        img = np.stack([r, g, b], -1) + rng.normal(0, 12, (h, w, 3))
        img[(xx // 37 + yy // 29) % 5 == 0] *= 0.55                                  # hard edges
        img[h // 3:h // 3 + 4, :] = [250, 245, 30]
        return np.clip(np.rint(img), 0, 255).astype(np.uint8)
    return make


def net_forward(sd, x, dtype=torch.float64, round_fp16_operands=True):
    """super-resolution-10 on a [N,1,h,w] input -> [N,1,3h,3w] float (no clipping).  With round_fp16_operands the input and
    weights are the fp16 values the kernels read; the arithmetic stays in `dtype` throughout (no intermediate rounding)."""
    def p(t):
        t = t.to(torch.float32)
        return (t.half() if round_fp16_operands else t).to(dtype)
    x = p(x)
    for i, pad in ((1, 2), (2, 1), (3, 1)):
        x = F.relu(F.conv2d(x, p(sd[f"conv{i}.weight"]), sd[f"conv{i}.bias"].to(dtype), padding=pad))
    x = F.conv2d(x, p(sd["conv4.weight"]), sd["conv4.bias"].to(dtype), padding=1)
    n, _, h, w = x.shape
    return x.reshape(n, 1, 3, 3, h, w).permute(0, 1, 4, 2, 5, 3).reshape(n, 1, 3 * h, 3 * w)     # ONNX Transpose perm


def y_float(sd, rgb, tile, dtype=torch.float64):
    """Pre-clip network output out_y [3h][3w] of one pass (tiles painted in the reference's order)."""
    img = Image.fromarray(rgb).convert("YCbCr")
    y = np.asarray(img)[..., 0].astype(np.float32) / 255.0
    h, w = y.shape
    tw, th = min(tile, w), min(tile, h)
    out = np.zeros((3 * h, 3 * w), np.float64)
    yt = torch.from_numpy(y)
    for y0 in plan_axis(h, th):
        for x0 in plan_axis(w, tw):
            crop = yt[y0:y0 + th, x0:x0 + tw][None, None]
            out[3 * y0:3 * y0 + 3 * th, 3 * x0:3 * x0 + 3 * tw] = net_forward(sd, crop, dtype)[0, 0].double().numpy()
    return out


def upscale_once(sd, rgb, tile=224, dtype=torch.float32):
    """uint8 RGB -> uint8 RGB, the reference's upscale_once with the network in `dtype` and PIL for colour."""
    h, w = rgb.shape[:2]
    out_y = y_float(sd, rgb, tile, dtype).astype(np.float32)
    y8 = np.uint8(np.clip(out_y * np.float32(255.0), 0, 255.0))
    _, cb, cr = Image.fromarray(rgb).convert("YCbCr").split()
    merged = Image.merge("YCbCr", [Image.fromarray(y8, mode="L"), cb.resize((3 * w, 3 * h), Image.BICUBIC),
                                   cr.resize((3 * w, 3 * h), Image.BICUBIC)]).convert("RGB")
    return np.asarray(merged)


def upscale(sd, rgb, magnitude, tile=224):
    x = rgb
    for _ in range(magnitude):
        x = upscale_once(sd, x, tile)
    return x


def decode(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


# ---- host copy of the kernels' integer colour formulas (csrc/sr.hip): 6-bit tables of c * 64 -----------------------
def _tab(num, den, v):
    p = num * v.astype(np.int64)
    return np.sign(p) * (np.abs(p) // den)                     # truncation toward zero, as C integer division


def rgb_to_ycc(rgb):
    r, g, b = [rgb[..., i].astype(np.int64) for i in range(3)]
    y = ((19136 * r + 500) // 1000 + (37568 * g + 500) // 1000 + (7296 * b + 500) // 1000) >> 6
    cb = ((_tab(-168736, 15625, r) + _tab(-331264, 15625, g) + 32 * b) >> 6) + 128
    cr = ((32 * r + _tab(-418688, 15625, g) + _tab(-81312, 15625, b)) >> 6) + 128
    return np.stack([y, np.clip(cb, 0, 255), np.clip(cr, 0, 255)], -1).astype(np.uint8)


def ycc_to_rgb(ycc):
    y, cb, cr = [ycc[..., i].astype(np.int64) for i in range(3)]
    vb, vr = cb - 128, cr - 128
    r = y + (_tab(11216, 125, vr) >> 6)
    g = y + ((_tab(-344136, 15625, vb) + _tab(-714136, 15625, vr)) >> 6)
    b = y + (_tab(14176, 125, vb) >> 6)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)
