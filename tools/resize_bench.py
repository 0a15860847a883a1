#!/usr/bin/env python3
"""What fitting an upload costs on one MI355X host: PIL on the host against the HIP Lanczos resampler.

  legs          RGB sources of 1024x1024, 2048x1536 and 4032x3024, each fitted to 512x512.  Wall-clock milliseconds from "host
                uint8 array in hand" to "fitted tensor ready on the device", synchronise included:
                  (a) pil_then_upload   backends/img2img.fit_init (PIL LANCZOS on the caller's thread), then the upload of the
                                        fitted picture -- the path before the device resampler;
                  (b) upload_then_hip   the raw upload into a device buffer that already exists, then ops.resize_lanczos_u8
                                        into slot 0 of a [1,512,512,3] tensor -- what the pipeline's upload() enqueues.
                The two are timed alternately after warm calls; median, min, 10th / 90th percentile.  Beside them: the PIL
                call alone, the raw upload alone, and the resampler alone (table upload + both launches) as device-event
                milliseconds of 20 back-to-back calls divided by 20, median / min / max over 7 rounds.  Every (b) result is
                compared with (a)'s for equality.
  worker        run_job wall-clock milliseconds (MODEL=synthetic, 512x512, 4 steps) of an image-to-image request that carries
                the 2048x1536 picture, under LCM_RESIZE=pil and LCM_RESIZE=hip alternately, and of the same request carrying
                the fitted picture.

  python tools/resize_bench.py [--reps 15] [--rows legs,worker] [--out profiles/resize_mi355x.json]

The default of LCM_RESIZE follows the legs: "hip" only if (b) is below (a) at all three sizes (``verdict``)."""
import argparse
import json
import os
import sys
import time
from dataclasses import dataclass, field
from typing import Any, Optional

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = ((1024, 1024), (2048, 1536), (4032, 3024))
OUT = 512


def summarise(ts):
    import numpy as np
    return dict(ms_median=round(float(np.median(ts)), 4), ms_min=round(float(min(ts)), 4), ms_p10=round(float(np.percentile(ts, 10)), 4),
                ms_p90=round(float(np.percentile(ts, 90)), 4), n=len(ts))


def device_ms(fn, n=20, rounds=7):
    import numpy as np
    import torch
    for _ in range(5):
        fn()
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(n):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / n)
    return dict(ms_median=round(float(np.median(out)), 5), ms_min=round(min(out), 5), ms_max=round(max(out), 5), calls_per_round=n,
                rounds=rounds)


def photo(w, h, seed):
    """A seeded picture with smooth shapes and sensor-like noise, uint8 [h, w, 3]."""
    import numpy as np
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    base = np.stack([128 + 100 * np.sin(x / 97.0 + seed), 128 + 100 * np.cos(y / 61.0), 128 + 90 * np.sin((x + y) / 143.0)], -1)
    return np.clip(base + rng.normal(0, 12, (h, w, 3)).astype(np.float32), 0, 255).astype(np.uint8)


def wall(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def legs(reps):
    import numpy as np
    import torch
    from sdlcm_amd import ops
    from sdlcm_amd.backends import img2img
    dev = "cuda:0"
    rows = {}
    for i, (sw, sh) in enumerate(SOURCES):
        a = photo(sw, sh, 3 + i)
        src = torch.empty(a.size, dtype=torch.uint8, device=dev).view(a.shape)
        slot = torch.empty((1, OUT, OUT, 3), dtype=torch.uint8, device=dev)
        ws = torch.empty(ops.resize_ws_bytes(sw, sh, 3, OUT, OUT), dtype=torch.uint8, device=dev)
        fitted = {}

        def leg_a():
            fitted["a"] = torch.from_numpy(img2img.fit_init(a, OUT, OUT)).to(dev)

        def leg_b():
            src.copy_(torch.from_numpy(a), non_blocking=True)
            ops.resize_lanczos_u8(src, slot[0], ws, OUT, OUT)

        for _ in range(3):
            leg_a(), leg_b()
        ts = dict(pil_then_upload=[], upload_then_hip=[], pil_alone=[], raw_upload_alone=[])
        for _ in range(reps):
            ts["pil_then_upload"].append(wall(leg_a))
            ts["upload_then_hip"].append(wall(leg_b))
            ts["pil_alone"].append(wall(lambda: img2img.fit_init(a, OUT, OUT)))
            ts["raw_upload_alone"].append(wall(lambda: src.copy_(torch.from_numpy(a), non_blocking=True)))
        row = {k: summarise(v) for k, v in ts.items()}
        row["hip_resampler_alone_device_ms"] = device_ms(lambda: ops.resize_lanczos_u8(src, slot[0], ws, OUT, OUT))
        row["same_bytes"] = bool(torch.equal(fitted["a"], slot[0]))
        row["source_bytes"] = int(a.size)
        row["hip_below_pil"] = bool(row["upload_then_hip"]["ms_median"] < row["pil_then_upload"]["ms_median"])
        rows[f"{sw}x{sh}_to_{OUT}x{OUT}"] = row
    return rows


@dataclass
class _Style:
    style: Optional[str] = None
    level: int = 0


@dataclass
class _Req:
    prompt: str
    size: str = f"{OUT}x{OUT}"
    num_inference_steps: int = 4
    guidance_scale: float = 1.0
    seed: Optional[int] = None
    style_lora: _Style = field(default_factory=_Style)
    init_image: Any = None
    denoising_strength: Optional[float] = None


@dataclass
class _Job:
    req: _Req


def worker_rows(reps):
    import torch
    os.environ["MODEL"] = "synthetic"
    os.environ.setdefault("MODEL_ROOT", "/nonexistent")
    from sdlcm_amd.backends import img2img
    from sdlcm_amd.backends.worker_factory import create_hip_worker
    big = photo(2048, 1536, 4)
    fitted = img2img.fit_init(big, OUT, OUT)
    mk = lambda pic: _Job(_Req(prompt="a lighthouse at dusk", seed=7, init_image=pic, denoising_strength=0.5))
    jobs = {"fitted_by_the_caller": ("hip", fitted), "upload_2048x1536_pil": ("pil", big), "upload_2048x1536_hip": ("hip", big)}
    w = create_hip_worker(worker_id=0)
    try:
        outs, ts = {}, {k: [] for k in jobs}
        for rep in range(3 + reps):
            for k, (mode, pic) in jobs.items():
                os.environ["LCM_RESIZE"] = mode
                job = mk(pic)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                outs[k] = w.run_job(job)
                if rep >= 3:
                    ts[k].append((time.perf_counter() - t0) * 1e3)
        rows = {k: summarise(v) for k, v in ts.items()}
        rows["same_png_bytes"] = bool(outs["fitted_by_the_caller"] == outs["upload_2048x1536_pil"] == outs["upload_2048x1536_hip"])
        return rows
    finally:
        os.environ.pop("LCM_RESIZE", None)
        w.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--rows", default="legs,worker")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    sys.path.insert(0, HERE)
    import PIL
    import torch
    import sdlcm_amd  # noqa: F401
    if not torch.cuda.is_available():
        raise SystemExit("resize_bench needs an MI355X: nothing here is measured on a CPU")
    want = a.rows.split(",")
    res = dict(device=torch.cuda.get_device_name(0), pillow=PIL.__version__, host_cpus_usable=len(os.sched_getaffinity(0)), reps=a.reps,
               rows={})
    if "legs" in want:
        res["rows"]["legs"] = legs(a.reps)
        res["verdict"] = dict(hip_below_pil_at_all_sizes=all(r["hip_below_pil"] for r in res["rows"]["legs"].values()),
                              same_bytes_at_all_sizes=all(r["same_bytes"] for r in res["rows"]["legs"].values()))
        res["verdict"]["default"] = "hip" if all(res["verdict"].values()) else "pil"
    if "worker" in want:
        res["rows"]["worker_run_job"] = worker_rows(a.reps)
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
