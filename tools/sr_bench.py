#!/usr/bin/env python3
"""Super-resolution timings on one MI355X (csrc/sr.hip through sdlcm_amd.superres; synthetic weights of the
super-resolution-10 shapes).

  python tools/sr_bench.py [--reps N] [--out FILE.json]

Per shape: the GPU part of a pass (device events around the launches of upscale_device, input already on the device), the
per-kernel split (lcm_profile_begin/end events), host PNG decode and encode, whole HipSuperResWorker.upscale_bytes calls, and
a torch-CPU fp32 restatement of the network (16 threads) for comparison.  Floors for a pass: network FLOPs at the dense-fp16
MFMA peak and the layer-by-layer activation traffic at HBM bandwidth."""
import argparse
import ctypes as C
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import sdlcm_amd  # noqa: E402,F401
from sdlcm_amd import lib, superres as S  # noqa: E402
from sdlcm_amd.backends.sr_worker import HipSuperResWorker  # noqa: E402
from sdlcm_amd.backends.hip_worker import encode_png  # noqa: E402
import sr_reference as ref  # noqa: E402

PEAK_FLOPS = 2.5e15          # dense fp16 MFMA
PEAK_BW = 8.0e12             # HBM3E bytes/s
MAC_PER_PX = 25 * 64 + 9 * 64 * 64 + 9 * 64 * 32 + 9 * 32 * 9


def floors(W, H, tile):
    tw, th = min(tile, W), min(tile, H)
    px = len(S.tile_plan(W, tw)) * len(S.tile_plan(H, th)) * tw * th
    flops = 2.0 * MAC_PER_PX * px
    # per tile pixel: conv1 writes 64 fp16, conv2 reads 64 writes 64, conv3 reads 64 writes 32, conv4 reads 32; + images
    bytes_ = px * 2 * (64 + 64 + 64 + 64 + 32 + 32) + W * H * 3 * 2 + 9 * W * H * (1 + 3 + 3) + 3 * W * H * 2
    return px, flops, bytes_


def time_gpu(net, rgb, reps):
    src = torch.from_numpy(rgb).to(net.device)
    with torch.cuda.stream(net.stream):
        for _ in range(2):
            net.upscale_device(src, 1)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ts = []
        for _ in range(reps):
            e0.record(net.stream)
            net.upscale_device(src, 1)
            e1.record(net.stream)
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        L = lib.load()
        L.lcm_profile_begin(64)
        net.upscale_device(src, 1)
        net.stream.synchronize()
        buf = C.create_string_buffer(1 << 14)
        n = L.lcm_profile_end(buf, len(buf))
    per = {}
    for line in buf.value.decode().splitlines()[:max(n, 0)]:
        k, ms = line.split("\t")
        per[k] = per.get(k, 0.0) + float(ms)
    return float(np.median(ts)), float(np.min(ts)), per


def time_host(fn, reps):
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default="")
    ap.add_argument("--cpu-threads", type=int, default=16)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "sr_bench needs the MI355X"
    torch.set_num_threads(a.cpu_threads)
    net = S.SuperResNet("synthetic", "cuda:0", 224, 672)
    wk = HipSuperResWorker(0, "synthetic", 224, 672)
    mk = ref.test_images()
    rows = []
    for name, (W, H) in (("512->1536", (512, 512)), ("1536->4608", (1536, 1536)), ("640x360", (640, 360)), ("64", (64, 64))):
        rgb = mk(W, H, 1)
        med, best, per = time_gpu(net, rgb, a.reps)
        px, flops, bytes_ = floors(W, H, 224)
        png = io.BytesIO()
        from PIL import Image
        Image.fromarray(rgb).save(png, format="PNG")
        data = png.getvalue()
        out = net.upscale_rgb(rgb, 1)
        row = dict(shape=name, W=W, H=H, tile_pixels=px, gpu_pass_ms_median=round(med, 4), gpu_pass_ms_min=round(best, 4),
                   kernels_ms={k: round(v, 4) for k, v in per.items()},
                   floor_mfma_ms=round(flops / PEAK_FLOPS * 1e3, 4), floor_hbm_ms=round(bytes_ / PEAK_BW * 1e3, 4),
                   tflops=round(flops / (med * 1e-3) / 1e12, 1),
                   decode_ms=round(time_host(lambda: ref.decode(data), 3), 2),
                   encode_png_ms=round(time_host(lambda: encode_png(out), 3), 2),
                   upscale_bytes_ms=round(time_host(lambda: wk.upscale_bytes(data, magnitude=1, out_format="png", quality=92), 3), 2))
        if W * H <= 640 * 360:
            row["cpu_fp32_pass_ms"] = round(time_host(lambda: ref.y_float(net.sd, rgb, 224, torch.float32), 1), 1)
        print(json.dumps(row), flush=True)
        rows.append(row)
    data = io.BytesIO()
    from PIL import Image
    Image.fromarray(mk(512, 512, 1)).save(data, format="PNG")
    m2 = time_host(lambda: wk.upscale_bytes(data.getvalue(), magnitude=2, out_format="png", quality=92), 3)
    rows.append(dict(shape="512 magnitude 2 (4608^2 PNG out)", upscale_bytes_ms=round(m2, 1)))
    print(json.dumps(rows[-1]))
    res = dict(device=torch.cuda.get_device_name(0), reps=a.reps, rows=rows)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    wk.close()


if __name__ == "__main__":
    main()
