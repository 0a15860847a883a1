#!/usr/bin/env python3
"""Super-resolution timings on one MI355X (csrc/sr.hip through sdlcm_amd.superres; synthetic weights of the
super-resolution-10 shapes).

  python tools/sr_bench.py [--reps N] [--out FILE.json]
  python tools/sr_bench.py --jpeg [--reps N] [--trace-dir DIR] [--out FILE.json]      the JPEG output path (below)
  rocprofv3 --kernel-trace --stats -d DIR -o NAME --output-format csv -- python tools/sr_bench.py --jpeg-launch-only WxH

Per shape: the GPU part of a pass (device events around the launches of upscale_device, input already on the device), the
per-kernel split (lcm_profile_begin/end events), host PNG decode and encode, whole HipSuperResWorker.upscale_bytes calls, and
a torch-CPU fp32 restatement of the network (16 threads) for comparison.  Floors for a pass: network FLOPs at the dense-fp16
MFMA peak and the layer-by-layer activation traffic at HBM bandwidth.

--jpeg, per shape at quality 92: the lcm_jpeg_dct_rgb8 launch on the upscaled image (device events; with --trace-dir also the
kernel time of a profiler run made by --jpeg-launch-only) against its floor of 3 B/pixel in + 3 B/pixel out at HBM bandwidth,
the copy of the coefficients to pinned memory, lcm_jpeg_encode_coefs at 1 and 8 threads, and whole upscale_bytes(jpeg) calls
through the library against the SAME calls with LCM_JPEG_ENCODER=pil, alternating in rounds; the spread of a path is the
range of its per-round medians.

--jpeg-in, per input size at quality 92, 4:2:0, with and without a restart marker per MCU row: PIL decode + upload against
lcm_jpeg_dec_info + lcm_jpeg_dec_coefs (1 and 8 threads) + the copy of the coefficients + lcm_jpeg_idct_rgb8 (device events;
floor: 2 B per coefficient in + 3 B per pixel out at HBM bandwidth), and whole upscale_bytes(jpeg in, jpeg out) calls with
LCM_JPEG_DECODER=hip against the SAME calls with LCM_JPEG_DECODER=pil, alternating in rounds as above.
  rocprofv3 --kernel-trace --stats -d DIR -o NAME --output-format csv -- python tools/sr_bench.py --jpeg-in-launch-only WxH"""
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


JPEG_SHAPES = (("512->1536", (512, 512)), ("1536->4608", (1536, 1536)), ("640x360->1080p", (640, 360)))
JPEG_Q = 92


def _events(fn, stream, reps, warm=3):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(reps):
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return ts


def _trace_kernel_us(trace_dir, grid):
    """Median duration (us) of the jpeg kernel dispatches with this grid (work-items x, y) in the kernel-trace CSVs under
    trace_dir, or None."""
    import csv
    import glob
    ds = []
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            for row in csv.DictReader(f):
                if "jpeg_dct_rgb8_kernel" not in row.get("Kernel_Name", ""):
                    continue
                if (int(row.get("Grid_Size_X", 0)), int(row.get("Grid_Size_Y", 0))) != grid:
                    continue
                ds.append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    return (round(float(np.median(ds)), 2), len(ds)) if ds else None


def jpeg_launch_only(shape, reps):
    """The launch alone on a seeded image of the given size, for a profiler run (nothing is timed here)."""
    W, H = (int(v) for v in shape.lower().split("x"))
    L = lib.load()
    rgb = torch.from_numpy(ref.test_images()(W, H, 1)).to("cuda:0")
    n = int(L.lcm_jpeg_coef_bytes(W, H))
    coefs = torch.empty(n // 2, dtype=torch.int16, device="cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    for _ in range(reps + 3):
        lib.check(L.lcm_jpeg_dct_rgb8(rgb.data_ptr(), W, H, 3 * W, JPEG_Q, coefs.data_ptr(), n, s), "lcm_jpeg_dct_rgb8")
    torch.cuda.synchronize()
    print(json.dumps(dict(shape=shape, launches=reps + 3)))


def jpeg_main(a):
    L = lib.load()
    net = S.SuperResNet("synthetic", "cuda:0", 224, 672)
    wk = HipSuperResWorker(0, "synthetic", 224, 672)
    mk = ref.test_images()
    rows = []
    from PIL import Image
    for name, (W, H) in JPEG_SHAPES:
        rgb = mk(W, H, 1)
        OW, OH = 3 * W, 3 * H
        with torch.cuda.stream(net.stream):
            up = net.upscale_device(torch.from_numpy(rgb).to(net.device), 1)
            n = int(L.lcm_jpeg_coef_bytes(OW, OH))
            coefs = torch.empty(n // 2, dtype=torch.int16, device=net.device)
            host = torch.empty(n // 2, dtype=torch.int16, pin_memory=True)
            s = net.stream.cuda_stream
            kern = _events(lambda: lib.check(L.lcm_jpeg_dct_rgb8(up.data_ptr(), OW, OH, 3 * OW, JPEG_Q, coefs.data_ptr(), n, s)),
                           net.stream, a.reps)
            d2h = _events(lambda: host.copy_(coefs, non_blocking=True), net.stream, a.reps)
        net.stream.synchronize()
        cap = int(L.lcm_jpeg_bound(OW, OH))
        out = np.empty(cap, np.uint8)
        ln = C.c_longlong(0)
        code = {}
        for thr in (1, 8):
            fn = lambda: lib.check(L.lcm_jpeg_encode_coefs(host.data_ptr(), OW, OH, JPEG_Q, thr, out.ctypes.data, cap, C.byref(ln)))  # noqa: E731
            fn()
            code[thr] = round(time_host(fn, a.reps), 2)
        png = io.BytesIO()
        Image.fromarray(rgb).save(png, format="PNG")
        data = png.getvalue()
        call = lambda: wk.upscale_bytes(data, magnitude=1, out_format="jpeg", quality=JPEG_Q)  # noqa: E731
        per = {"hip": [], "pil": []}
        sizes = {}
        for rnd in range(3 + 1):                      # round 0 warms both paths up and is dropped
            for path in ("hip", "pil"):
                if path == "pil":
                    os.environ["LCM_JPEG_ENCODER"] = "pil"
                else:
                    os.environ.pop("LCM_JPEG_ENCODER", None)
                ts = []
                for _ in range(a.reps if rnd else 2):
                    t = time.perf_counter()
                    sizes[path] = len(call())
                    ts.append((time.perf_counter() - t) * 1e3)
                if rnd:
                    per[path].append(float(np.median(ts)))
        os.environ.pop("LCM_JPEG_ENCODER", None)
        floor_us = (3.0 * OW * OH + n) / PEAK_BW * 1e6
        k_med = float(np.median(kern)) * 1e3
        row = dict(shape=name, out_w=OW, out_h=OH, quality=JPEG_Q, reps=a.reps,
                   kernel_us_events_median=round(k_med, 2), kernel_us_events_min=round(min(kern) * 1e3, 2),
                   kernel_floor_us_8TBps=round(floor_us, 2), kernel_floor_fraction_events=round(floor_us / k_med, 3),
                   d2h_ms_median=round(float(np.median(d2h)), 3), coef_bytes=n,
                   host_coding_ms_1_thread=code[1], host_coding_ms_8_threads=code[8], jpeg_file_bytes=int(ln.value),
                   upscale_bytes_jpeg_ms=dict(
                       library_round_medians=[round(v, 2) for v in per["hip"]], pil_round_medians=[round(v, 2) for v in per["pil"]],
                       library_median=round(float(np.median(per["hip"])), 2), pil_median=round(float(np.median(per["pil"])), 2),
                       library_spread=round(max(per["hip"]) - min(per["hip"]), 2), pil_spread=round(max(per["pil"]) - min(per["pil"]), 2)),
                   file_bytes=sizes)
        if a.trace_dir:
            grid = (((OW + 15) // 16 + 15) // 16 * 256, (OH + 15) // 16)
            tr = _trace_kernel_us(a.trace_dir, grid)
            if tr:
                row["kernel_us_rocprof_median"], row["kernel_rocprof_dispatches"] = tr
                row["kernel_floor_fraction_rocprof"] = round(floor_us / tr[0], 3)
        e = row["upscale_bytes_jpeg_ms"]
        e["library_faster_by_more_than_spread"] = bool(e["library_median"] + e["library_spread"] + e["pil_spread"] < e["pil_median"])
        print(json.dumps(row), flush=True)
        rows.append(row)
    res = dict(device=torch.cuda.get_device_name(0), reps=a.reps, jpeg_threads=S.jpeg_threads(), rows=rows)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    wk.close()


JPEG_IN_SHAPES = (("512x512", (512, 512)), ("1536x1536", (1536, 1536)), ("4608x3072", (4608, 3072)))


def _jpeg_in_file(W, H, dri):
    from PIL import Image
    buf = io.BytesIO()
    kw = dict(restart_marker_rows=1) if dri else {}
    Image.fromarray(ref.test_images()(W, H, 1)).save(buf, format="JPEG", quality=JPEG_Q, subsampling=2, **kw)
    return buf.getvalue()


def _host_decode(L, data, threads, pinned=None):
    info = lib.JpegInfo()
    lib.check(L.lcm_jpeg_dec_info(data, len(data), C.byref(info)), "lcm_jpeg_dec_info")
    if pinned is None:
        pinned = torch.empty(info.coefs_bytes // 2, dtype=torch.int16, pin_memory=True)
    lib.check(L.lcm_jpeg_dec_coefs(data, len(data), threads, pinned.data_ptr(), info.coefs_bytes), "lcm_jpeg_dec_coefs")
    return info, pinned


def jpeg_in_launch_only(shape, reps):
    """The two launches of lcm_jpeg_idct_rgb8 alone on a seeded 4:2:0 file of the given size, for a profiler run."""
    W, H = (int(v) for v in shape.lower().split("x"))
    L = lib.load()
    info, pinned = _host_decode(L, _jpeg_in_file(W, H, True), 8)
    coefs = pinned.to("cuda:0")
    work = torch.empty(info.work_bytes, dtype=torch.uint8, device="cuda:0")
    out = torch.empty(H, W, 3, dtype=torch.uint8, device="cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    for _ in range(reps + 3):
        lib.check(L.lcm_jpeg_idct_rgb8(coefs.data_ptr(), info.coefs_bytes, C.byref(info), work.data_ptr(), info.work_bytes,
                                       out.data_ptr(), 3 * W, s), "lcm_jpeg_idct_rgb8")
    torch.cuda.synchronize()
    print(json.dumps(dict(shape=shape, launches=reps + 3)))


def jpeg_in_main(a):
    from PIL import Image
    L = lib.load()
    wk = HipSuperResWorker(0, "synthetic", 224, 672)
    stream = torch.cuda.current_stream()
    rows = []
    for name, (W, H) in JPEG_IN_SHAPES:
        for dri in (True, False):
            data = _jpeg_in_file(W, H, dri)
            pil = lambda: torch.from_numpy(np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))).to("cuda:0")  # noqa: E731
            pil()
            pil_ms = time_host(lambda: (pil(), torch.cuda.synchronize()), a.reps)
            info, pinned = _host_decode(L, data, 8)
            hdr = lib.JpegInfo()
            hdr_ms = time_host(lambda: L.lcm_jpeg_dec_info(data, len(data), C.byref(hdr)), a.reps)
            ent = {thr: round(time_host(lambda: _host_decode(L, data, thr, pinned), a.reps), 3) for thr in (1, 2, 4, 8, 16)}
            coefs = torch.empty(info.coefs_bytes // 2, dtype=torch.int16, device="cuda:0")
            work = torch.empty(info.work_bytes, dtype=torch.uint8, device="cuda:0")
            out = torch.empty(H, W, 3, dtype=torch.uint8, device="cuda:0")
            s = stream.cuda_stream
            h2d = _events(lambda: coefs.copy_(pinned, non_blocking=True), stream, a.reps)
            kern = _events(lambda: lib.check(L.lcm_jpeg_idct_rgb8(coefs.data_ptr(), info.coefs_bytes, C.byref(info), work.data_ptr(),
                                                                  info.work_bytes, out.data_ptr(), 3 * W, s)), stream, a.reps)
            assert np.array_equal(out.cpu().numpy(), np.asarray(Image.open(io.BytesIO(data)).convert("RGB")))
            call = lambda: wk.upscale_bytes(data, magnitude=1, out_format="jpeg", quality=JPEG_Q)  # noqa: E731
            per = {"hip": [], "pil": []}
            shas = {}
            for rnd in range(3 + 1):                  # round 0 warms both paths up and is dropped
                for path in ("hip", "pil"):
                    os.environ["LCM_JPEG_DECODER"] = path
                    ts = []
                    for _ in range(a.reps if rnd else 2):
                        t = time.perf_counter()
                        res = call()
                        ts.append((time.perf_counter() - t) * 1e3)
                    shas[path] = hash(res)
                    if rnd:
                        per[path].append(float(np.median(ts)))
            os.environ.pop("LCM_JPEG_DECODER", None)
            assert shas["hip"] == shas["pil"]
            floor_us = (info.coefs_bytes + 3.0 * W * H) / PEAK_BW * 1e6
            k_med = float(np.median(kern)) * 1e3
            e = dict(library_round_medians=[round(v, 2) for v in per["hip"]], pil_round_medians=[round(v, 2) for v in per["pil"]],
                     library_median=round(float(np.median(per["hip"])), 2), pil_median=round(float(np.median(per["pil"])), 2),
                     library_spread=round(max(per["hip"]) - min(per["hip"]), 2), pil_spread=round(max(per["pil"]) - min(per["pil"]), 2))
            e["library_faster_by_more_than_spread"] = bool(e["library_median"] + e["library_spread"] + e["pil_spread"] < e["pil_median"])
            row = dict(shape=name, W=W, H=H, quality=JPEG_Q, sampling="4:2:0", restart_markers=dri, file_bytes=len(data), reps=a.reps,
                       pil_decode_plus_upload_ms=round(pil_ms, 3), header_ms=round(hdr_ms, 4), entropy_decode_ms_by_threads=ent,
                       coef_bytes=int(info.coefs_bytes), h2d_ms_median=round(float(np.median(h2d)), 3),
                       kernels_us_events_median=round(k_med, 2), kernels_us_events_min=round(min(kern) * 1e3, 2),
                       kernels_floor_us_8TBps=round(floor_us, 2), kernels_floor_fraction_events=round(floor_us / k_med, 3),
                       upscale_bytes_jpeg_in_jpeg_out_ms=e)
            if a.trace_dir:
                tr = _trace_dec_us(a.trace_dir, W, H)
                if tr:
                    row.update(tr)
                    row["kernels_floor_fraction_rocprof"] = round(floor_us / tr["kernels_us_rocprof_median_sum"], 3)
            print(json.dumps(row), flush=True)
            rows.append(row)
    res = dict(device=torch.cuda.get_device_name(0), reps=a.reps, jpeg_threads=S.jpeg_threads(), rows=rows)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    wk.close()


def _trace_dec_us(trace_dir, W, H):
    """Median durations (us) of the two decoder kernels for a W x H 4:2:0 image in the kernel-trace CSVs under trace_dir."""
    import csv
    import glob
    nblocks = ((W + 15) // 16) * ((H + 15) // 16) * 6
    grids = {"jpeg_idct_kernel": ((nblocks + 31) // 32 * 256, 1), "jpeg_upsample_rgb_kernel": ((((W + 3) // 4 + 255) // 256) * 256, H)}
    ds = {k: [] for k in grids}
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            for row in csv.DictReader(f):
                for k, g in grids.items():
                    if k in row.get("Kernel_Name", "") and (int(row.get("Grid_Size_X", 0)), int(row.get("Grid_Size_Y", 0))) == g:
                        ds[k].append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    if not all(ds.values()):
        return None
    med = {k: round(float(np.median(v)), 2) for k, v in ds.items()}
    return dict(kernels_us_rocprof_median=med, kernels_us_rocprof_median_sum=round(sum(med.values()), 2),
                kernels_rocprof_dispatches={k: len(v) for k, v in ds.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default="")
    ap.add_argument("--jpeg", action="store_true", help="measure the JPEG output path instead")
    ap.add_argument("--jpeg-launch-only", default="", metavar="WxH", help="only launch lcm_jpeg_dct_rgb8 (for a profiler run)")
    ap.add_argument("--jpeg-in", action="store_true", help="measure the JPEG input path instead")
    ap.add_argument("--jpeg-in-launch-only", default="", metavar="WxH", help="only launch lcm_jpeg_idct_rgb8 (for a profiler run)")
    ap.add_argument("--trace-dir", default="", help="with --jpeg / --jpeg-in: kernel-trace CSVs of the launch-only runs")
    ap.add_argument("--cpu-threads", type=int, default=16)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "sr_bench needs the MI355X"
    torch.set_num_threads(a.cpu_threads)
    if a.jpeg_launch_only:
        return jpeg_launch_only(a.jpeg_launch_only, a.reps)
    if a.jpeg_in_launch_only:
        return jpeg_in_launch_only(a.jpeg_in_launch_only, a.reps)
    if a.jpeg_in:
        return jpeg_in_main(a)
    if a.jpeg:
        return jpeg_main(a)
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
