#!/usr/bin/env python3
"""What a refinement request (denoise_strength / pass_number) costs through the worker's run_job on one MI355X, synthetic SD1.5
weights, 512x512 4 steps, one request at a time:

  plain         a plain request (today's path)
  warm pass     pass p of a request whose pass p - 1 was served before: one pass from the cached latents
  cold p=3      pass 3 with nothing cached: the plain pass and three refinement passes in one captured graph
  three plain   three plain requests one after the other (what the UI's three-pass preset costs without the feature)

  python tools/refine_bench.py [--reps N] [--out profiles/refine_bench.json]

Times are wall-clock milliseconds of run_job (conditioning, upload, graph replay, download, PNG), median and minimum of N,
after every plan involved was built and captured."""
import argparse
import json
import os
import sys
import time
from dataclasses import dataclass
from typing import Optional

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import sdlcm_amd  # noqa: E402,F401


@dataclass
class Req:
    prompt: str
    size: str = "512x512"
    num_inference_steps: int = 4
    guidance_scale: float = 1.0
    seed: Optional[int] = 1
    denoise_strength: Optional[float] = None
    pass_number: Optional[int] = None
    total_passes: Optional[int] = None


@dataclass
class Job:
    req: Req


def timed(fn, reps, before=None):
    ts = []
    for _ in range(reps):
        if before is not None:
            before()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(ms_median=round(float(np.median(ts)), 3), ms_min=round(min(ts), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--size", default="512x512")
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--strength", type=float, default=0.5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    os.environ["MODEL"] = "synthetic"
    os.environ.setdefault("MODEL_ROOT", "/nonexistent")
    from sdlcm_amd.backends.worker_factory import create_hip_worker
    w = create_hip_worker(worker_id=0)
    eng = w._engine
    mk = lambda **kw: Job(Req(prompt="a lighthouse at dusk", size=a.size, num_inference_steps=a.steps, **kw))
    plain, p2, p3 = mk(), mk(denoise_strength=a.strength, pass_number=2), mk(denoise_strength=a.strength, pass_number=3)
    try:
        # build every plan: plain, cold chain of 3, one pass from the cache
        w.run_job(plain)
        eng.refine_cache.clear()
        w.run_job(p3)
        w.run_job(p3)
        rows = dict(plain=timed(lambda: w.run_job(plain), a.reps))
        n0 = eng.stats["unet_evals"]
        rows["warm_pass"] = timed(lambda: w.run_job(p3), a.reps)          # x^2 is cached: one pass
        rows["warm_pass"]["unet_evals"] = (eng.stats["unet_evals"] - n0) // a.reps
        n0 = eng.stats["unet_evals"]
        rows["cold_p3"] = timed(lambda: w.run_job(p3), a.reps, before=eng.refine_cache.clear)
        rows["cold_p3"]["unet_evals"] = (eng.stats["unet_evals"] - n0) // a.reps
        rows["three_plain"] = timed(lambda: [w.run_job(plain) for _ in range(3)], a.reps)
        res = dict(device=torch.cuda.get_device_name(0), weights="seeded synthetic SD1.5 architecture", size=a.size, steps=a.steps,
                   strength=a.strength, reps=a.reps, rows=rows)
        print(json.dumps(res), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
    finally:
        w.close()


if __name__ == "__main__":
    main()
