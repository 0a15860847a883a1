#!/usr/bin/env python3
"""What a hires-fix request (enable_hr) costs on one MI355X, synthetic SD1.5 weights, measured at ``LcmHipPipeline.generate``:

  hires         512x512 -> 1024x1024, 4 + 4 steps, strength 0.7, "Latent" (bilinear): stage 1 without a decode, the hand-over
                launch, stage 2 with one decode -- at batch 1 and batch 4
  plain 512     a plain 512x512 4-step request (what stage 1 would cost with its decode)
  plain 1024    a plain 1024x1024 4-step request (the only other route to a picture of that size)
  stage 1       the "latents" plan alone against the plain 512x512 plan, graph replay to graph replay: what leaving the VAE
                decode and RGB epilogue out saves

  python tools/hires_bench.py [--reps N] [--out profiles/hires_bench_mi355x.json]
  python tools/hires_bench.py --plain-only        the two plain rows alone (runs on a tree without the feature: the parent's times)
  python tools/hires_bench.py --parent FILE       merge a --plain-only result taken on the parent commit into the output

``call`` rows are wall-clock milliseconds of generate() (draws, upload, graph replay, download; ends in a stream synchronise);
``replay`` rows the captured graphs alone between two stream synchronisations.  Every plan is built, tuned and captured and every
shape run three times before its timed window; rows of one batch are timed alternately, ``reps`` rounds; median and minimum.
No pass/fail threshold: this records."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import sdlcm_amd  # noqa: E402,F401


def summarise(ts):
    return dict(ms_median=round(float(np.median(ts)), 3), ms_min=round(min(ts), 3))


def alternate(rows, reps, warm=3):
    """rows: {name: callable}.  Warm each, then time them in turn, ``reps`` rounds."""
    for fn in rows.values():
        for _ in range(warm):
            fn()
    ts = {k: [] for k in rows}
    for _ in range(reps):
        for k, fn in rows.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            ts[k].append((time.perf_counter() - t0) * 1e3)
    return {k: summarise(v) for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batches", default="1,4")
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--hr-steps", type=int, default=4)
    ap.add_argument("--strength", type=float, default=0.7)
    ap.add_argument("--base", type=int, default=512)
    ap.add_argument("--target", type=int, default=1024)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--parent", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from sdlcm_amd import weights
    from sdlcm_amd.pipeline import LcmHipPipeline
    hip = LcmHipPipeline(weights.synthetic_unet(), weights.synthetic_vae(), device="cuda:0")
    stream = hip.stream
    res = dict(device=torch.cuda.get_device_name(0), weights="seeded synthetic SD1.5 architecture", base=a.base, target=a.target,
               steps=a.steps, hr_steps=a.hr_steps, strength=a.strength, upscaler="Latent", reps=a.reps, rows={})
    try:
        for B in [int(x) for x in a.batches.split(",")]:
            pe = torch.randn(B, 77, 768, generator=torch.Generator().manual_seed(5)).to(torch.float16)
            seeds = list(range(100, 100 + B))
            rows = {f"plain_{a.base}": lambda: hip.generate(pe, seeds, a.base, a.base, a.steps, 1.0),
                    f"plain_{a.target}": lambda: hip.generate(pe, seeds, a.target, a.target, a.steps, 1.0)}
            if not a.plain_only:
                hires = (a.target, a.target, a.hr_steps, a.strength, 0)
                rows["hires"] = lambda: hip.generate(pe, seeds, a.base, a.base, a.steps, 1.0, hires=hires)
            call = alternate(rows, a.reps)
            out = dict(call=call)
            if not a.plain_only:
                def replay(P):
                    def run():
                        hip.replay(P)
                        stream.synchronize()
                    return run
                h = a.base // 8
                P0 = hip.plan(B, h, h, a.steps, False, 1.0)
                P1 = hip.plan(B, h, h, a.steps, False, 1.0, kind="latents")
                with torch.cuda.stream(stream):
                    rp = alternate({f"plain_{a.base}": replay(P0), "stage1_latents_only": replay(P1)}, a.reps)
                saved = rp[f"plain_{a.base}"]["ms_median"] - rp["stage1_latents_only"]["ms_median"]
                out["replay"] = dict(rp, stage1_saving_ms=round(saved, 3),
                                     stage1_saving_share=round(saved / rp[f"plain_{a.base}"]["ms_median"], 4))
            res["rows"][f"batch_{B}"] = out
            hip.drop_plans()
            torch.cuda.empty_cache()
        if a.parent:
            with open(a.parent) as f:
                res["parent_commit_plain"] = json.load(f)["rows"]
        print(json.dumps(res), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
    finally:
        hip.close()


if __name__ == "__main__":
    main()
