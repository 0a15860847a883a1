#!/usr/bin/env python3
"""What the Canny preprocessor costs on one MI355X.

  kernels       lcm_canny_rgb8 (five launches) at 512x512, batch 1 and batch 8, on a smoothed-noise picture at thresholds
                (100, 200) and (5, 400) and on a picture of a spiral with lines and gaps four pixels wide (two edge chains
                that run the whole spiral: long thin components, the hard case for the union-find); lcm_canny_link alone on
                a one-pixel spiral class map; lcm_invert_u8.  Device-event milliseconds of 50 back-to-back calls divided by
                50, median / min / max over 9 rounds.
  worker        run_job wall-clock milliseconds (MODEL=synthetic, CONTROLNET=synthetic, 512x512, 4 steps) of a ControlNet
                request with a finished hint and of the same request with a photo and controlnet_module="canny", timed
                alternately after warm calls; median, min, 10th / 90th percentile.

  python tools/canny_bench.py [--reps 40] [--rows kernels,finished,canny] [--root DIR] [--out profiles/canny_bench_mi355x.json]

--root DIR imports the package from another checkout (the parent commit, to compare the finished-hint row: that path is not
touched by the preprocessor, so the two must agree within the spread of repeated runs); there only ``--rows finished`` exists.
No pass/fail threshold: this records."""
import argparse
import json
import os
import sys
import time
from dataclasses import dataclass, field
from typing import Any, Optional

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def summarise(ts):
    import numpy as np
    return dict(ms_median=round(float(np.median(ts)), 4), ms_min=round(float(min(ts)), 4), ms_p10=round(float(np.percentile(ts, 10)), 4),
                ms_p90=round(float(np.percentile(ts, 90)), 4), n=len(ts))


def device_ms(fn, n=50, rounds=9):
    import numpy as np
    import torch
    for _ in range(10):
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


def kernels(S):
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(HERE, "tests"))
    import canny_reference as cy
    from sdlcm_amd import ops
    rows = {}
    noise = cy.smoothed_noise(S, S, 1)
    sp = cy.spiral(S, S)
    wide = np.kron((cy.spiral(S // 4, S // 4) > 0).astype(np.uint8), np.ones((4, 4), np.uint8))[:S, :S]   # lines and gaps 4 pixels wide
    sp_pic = np.repeat((np.pad(wide, ((0, S - wide.shape[0]), (0, S - wide.shape[1]))) * 255)[..., None], 3, axis=2)
    for B in (1, 8):
        ws = torch.empty(ops.canny_ws_bytes(B, S, S), dtype=torch.uint8, device="cuda:0")
        out = torch.empty(B, S, S, 3, dtype=torch.uint8, device="cuda:0")
        for name, pic, lo, hi in (("noise_100_200", noise, 100, 200), ("noise_5_400", noise, 5, 400), ("spiral_picture_100_200", sp_pic, 100, 200)):
            x = torch.from_numpy(np.ascontiguousarray(np.stack([pic] * B))).to("cuda:0")
            r = device_ms(lambda: ops.canny_rgb8(x, out, ws, B, S, S, lo, hi))
            got = out.cpu().numpy()
            r["edge_pixels_per_image"] = int((got[0, ..., 0] == 255).sum())
            if B == 1:                                     # the reference at this size takes seconds: once
                r["equals_reference"] = bool(np.array_equal(got[0], cy.canny(pic, lo, hi)))
            rows[f"canny_rgb8_{name}_b{B}"] = r
        cls = torch.from_numpy(np.ascontiguousarray(np.stack([sp] * B))).to("cuda:0")
        r = device_ms(lambda: ops.canny_link(cls, out, ws, B, S, S))
        r["edge_pixels_per_image"] = int((out.cpu().numpy()[0, ..., 0] == 255).sum())
        r["chain_length"] = int((sp > 0).sum())
        rows[f"canny_link_spiral_map_b{B}"] = r
        x = torch.from_numpy(np.ascontiguousarray(np.stack([noise] * B))).to("cuda:0")
        rows[f"invert_u8_b{B}"] = device_ms(lambda: ops.invert_u8(x, out))
    return rows


@dataclass
class _Style:
    style: Optional[str] = None
    level: int = 0


@dataclass
class _Req:
    prompt: str
    size: str = "512x512"
    num_inference_steps: int = 4
    guidance_scale: float = 1.0
    seed: Optional[int] = None
    style_lora: _Style = field(default_factory=_Style)
    controlnet_image: Any = None
    controlnet_conditioning_scale: Optional[float] = None
    controlnet_module: Any = None
    controlnet_threshold_a: Any = None
    controlnet_threshold_b: Any = None


@dataclass
class _Job:
    req: _Req


def worker_rows(S, reps, want):
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(HERE, "tests"))
    import canny_reference as cy
    os.environ["MODEL"] = "synthetic"
    os.environ.setdefault("MODEL_ROOT", "/nonexistent")
    os.environ["CONTROLNET"] = "synthetic"
    from sdlcm_amd.backends.worker_factory import create_hip_worker
    photo = cy.smoothed_noise(S, S, 1)
    edge = cy.canny(photo, 100, 200)
    jobs = {}
    if "finished" in want:
        jobs["finished_hint"] = lambda: _Job(_Req(prompt="a lighthouse at dusk", size=f"{S}x{S}", seed=7, controlnet_image=edge))
    if "canny" in want:
        jobs["module_canny"] = lambda: _Job(_Req(prompt="a lighthouse at dusk", size=f"{S}x{S}", seed=7, controlnet_image=photo,
                                                 controlnet_module="canny"))
    w = create_hip_worker(worker_id=0)
    try:
        outs = {}
        for k, mk in jobs.items():
            for _ in range(5):
                outs[k] = w.run_job(mk())
        ts = {k: [] for k in jobs}
        for _ in range(reps):
            for k, mk in jobs.items():
                job = mk()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                w.run_job(job)
                ts[k].append((time.perf_counter() - t0) * 1e3)
        rows = {k: summarise(v) for k, v in ts.items()}
        if len(jobs) == 2:
            paired = np.asarray(ts["module_canny"]) - np.asarray(ts["finished_hint"])
            rows["module_canny_minus_finished_hint"] = dict(same_png_bytes=bool(outs["module_canny"] == outs["finished_hint"]),
                                                            **{"paired_" + k: v for k, v in summarise(list(paired)).items()})
        return rows
    finally:
        w.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--rows", default="kernels,finished,canny")
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import torch
    import sdlcm_amd  # noqa: F401
    want = a.rows.split(",")
    res = dict(device=torch.cuda.get_device_name(0), weights="seeded synthetic SD1.5 + ControlNet architecture", size=a.size, steps=4,
               reps=a.reps, label=a.label, rows={})
    if "kernels" in want:
        res["rows"]["kernels"] = kernels(a.size)
    if "finished" in want or "canny" in want:
        res["rows"]["worker_run_job"] = worker_rows(a.size, a.reps, want)
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
