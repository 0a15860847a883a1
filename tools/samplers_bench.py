#!/usr/bin/env python3
"""What sampler_name costs on one MI355X, synthetic SD1.5 weights:

  launch        lcm_sampler_step alone, device events around a window of back-to-back launches: a DPM++ 2M step (c1 != 0) and an
                Euler a step (cn != 0) at latent shape 64x64, B = 1 / 8, with and without classifier-free guidance (dup);
                microseconds per launch, median of 5 windows
  run_job       a 512x512 4-step batch-1 LCM request at the worker (``HipLcmWorker.run_job``), timed alone (the row --plain-only
                takes on another checkout); then ("run_job_in_turn") a 20-step LCM request and a 20-step ``DPM++ 2M Karras``
                request at the same guidance, timed in turn; wall-clock milliseconds, median of ``reps`` calls

  python tools/samplers_bench.py [--reps N] [--out profiles/samplers_bench_mi355x.json] [--parent FILE [FILE ...]] [--mine FILE [FILE ...]]
  python tools/samplers_bench.py --plain-only [--root DIR] --out FILE
        the plain run_job row alone, with the package imported from DIR (a checkout of the parent commit, built): the parent's
        figure.  Runs of the two trees are ALTERNATED by the caller (parent, this tree, parent, this tree, ... each a process of its
        own); --parent / --mine merge the files into the output, whose "plain_vs_parent" then holds every run's median and the
        spread between runs of one tree -- the yardstick for a difference between the trees.

Every shape is run (plans built, tuned, captured) before its timed window.  No pass/fail threshold: this records."""
import argparse
import json
import os
import sys
import time
import types

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402


def summarise(ts):
    return dict(ms_median=round(float(np.median(ts)), 3), ms_min=round(min(ts), 3), ms_p90=round(float(np.percentile(ts, 90)), 3), n=len(ts))


def job(seed, **kw):
    d = dict(prompt="a photo of an astronaut riding a horse on mars", size="512x512", num_inference_steps=4, guidance_scale=1.0,
             seed=seed, style_lora=None)
    d.update(kw)
    return types.SimpleNamespace(req=types.SimpleNamespace(**d))


def time_run_job(worker, rows, reps, warm=5):
    """{name: request fields} timed in turn, ``reps`` rounds, after ``warm`` calls each."""
    for kw in rows.values():
        for i in range(warm):
            worker.run_job(job(i, **kw))
    ts = {k: [] for k in rows}
    for i in range(reps):
        for k, kw in rows.items():
            t0 = time.perf_counter()
            worker.run_job(job(100 + i, **kw))
            ts[k].append((time.perf_counter() - t0) * 1e3)
    return {k: summarise(v) for k, v in ts.items()}


WINDOW_S = 0.3


def _window_ms(torch, fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def events_us(torch, fn):
    """microseconds per launch over a window of back-to-back launches sized from a trial of 200 to last about WINDOW_S"""
    for _ in range(10):
        fn()
    launches = max(200, int(WINDOW_S * 1e3 / (_window_ms(torch, fn, 200) / 200)))
    return 1e3 * _window_ms(torch, fn, launches) / launches


def time_launch(torch):
    from sdlcm_amd import ops
    out, h = {}, 64
    rows = {"DPM++ 2M (c1 != 0)": (0.6174, 0.7866, 0.0371, 1.7327, -0.756, 0.0), "Euler a (cn != 0)": (0.0683, 0.9977, 0.0687, 0.6127, 0.0, 0.7836)}
    for name, row in rows.items():
        for B in (1, 8):
            for cfg in (False, True):
                lat = torch.randn(2 * B if cfg else B, 4, h, h, device="cuda") * 0.1
                eps = torch.randn(2 * B if cfg else B, h, h, 4, device="cuda") * 0.1
                x0p, noise = torch.zeros(B, 4, h, h, device="cuda"), torch.randn(B, 4, h, h, device="cuda") * 0.1
                kw = dict(eps_uncond=eps[:B], guidance=2.0, dup=True) if cfg else {}
                fn = lambda: ops.sampler_step(eps[B:] if cfg else eps, lat[B:] if cfg else lat, x0p, noise if row[5] else None, *row, B, h, h,
                                              pred="epsilon", **kw)
                us = float(np.median([events_us(torch, fn) for _ in range(5)]))
                n = B * 4 * h * h * 4
                out[f"{name} {h}x{h} B={B}{' CFG' if cfg else ''}"] = dict(us_per_launch=round(us, 2),
                                                                          bytes_moved=n * ((5 if cfg else 3) + 1 + (1 if row[4] else 0) + (1 if row[5] else 0)))
    return out


def spread(files):
    meds = [json.load(open(f))["run_job"]["plain"]["ms_median"] for f in files]
    return dict(ms_medians=meds, ms_mean=round(float(np.mean(meds)), 3), ms_spread=round(max(meds) - min(meds), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "samplers_bench_mi355x.json"))
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--parent", nargs="*", default=[])
    ap.add_argument("--mine", nargs="*", default=[])
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import torch
    import sdlcm_amd  # noqa: F401
    assert torch.cuda.is_available(), "samplers_bench needs the MI355X"
    os.environ["MODEL"] = "synthetic"
    os.environ.setdefault("MODEL_ROOT", "/nonexistent")
    from sdlcm_amd.backends.worker_factory import create_hip_worker
    worker = create_hip_worker(worker_id=0)
    doc = dict(device=torch.cuda.get_device_name(0), request="512x512, batch 1, guidance 1.0, synthetic SD1.5 weights", reps=a.reps)
    try:
        doc["run_job"] = time_run_job(worker, {"plain": {}}, a.reps)               # 4-step LCM alone, as --plain-only times it: comparable
        if not a.plain_only:
            doc["run_job_in_turn"] = time_run_job(worker, {"LCM 20 steps": dict(num_inference_steps=20),
                                                           "DPM++ 2M Karras 20 steps": dict(num_inference_steps=20, sampler_name="DPM++ 2M Karras")},
                                                  max(5, a.reps // 3))
            doc["launch"] = time_launch(torch)
            doc["stats"] = {"sampler_requests": worker._engine.stats["sampler_requests"]}
    finally:
        worker.close()
    if a.parent or a.mine:
        doc["plain_vs_parent"] = dict(parent=spread(a.parent), this_tree=spread(a.mine),
                                      note="medians of the plain run_job row, one process per entry, the two trees alternated")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
