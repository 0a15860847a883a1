#!/usr/bin/env python3
"""What an image-to-image request (init_image) costs on one MI355X, synthetic SD1.5 weights, measured at
``LcmHipPipeline.generate_img2img``:

  img2img       a 512x512 picture -> VAE encoder -> posterior / re-noise launch -> 4 steps over timesteps(4, 0.5) -> decode,
                at batch 1 and batch 8
  plain         a plain 512x512 request of the same number of steps (the same UNet and decoder work, no encoder)
  encoder       the encoder stage alone: its captured graph between two stream synchronisations

  python tools/img2img_bench.py [--reps N] [--out profiles/img2img_bench_mi355x.json]

``call`` rows are wall-clock milliseconds of the call (draws, upload, graph replays, download; ends in a stream synchronise);
``replay`` rows the captured graph alone.  Every sampler plan is built, tuned and captured; the encoder stage is captured but
never autotuned (it runs on the shipped plan entries and the heuristic).  Every shape is run three times before its timed window; rows of one batch are timed alternately, ``reps`` rounds; median and minimum.  No pass/fail threshold: this records."""
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
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--strength", type=float, default=0.5)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from sdlcm_amd import weights
    from sdlcm_amd.pipeline import LcmHipPipeline
    hip = LcmHipPipeline(weights.synthetic_unet(), weights.synthetic_vae(), device="cuda:0")
    hip.set_vae_encoder_source(weights.synthetic_vae_encoder())
    stream = hip.stream
    res = dict(device=torch.cuda.get_device_name(0), weights="seeded synthetic SD1.5 architecture", size=a.size, steps=a.steps,
               strength=a.strength, reps=a.reps, rows={})
    try:
        for B in [int(x) for x in a.batches.split(",")]:
            pe = torch.randn(B, 77, 768, generator=torch.Generator().manual_seed(5)).to(torch.float16)
            seeds = list(range(100, 100 + B))
            pics = np.random.default_rng(7).integers(0, 256, (B, a.size, a.size, 3), dtype=np.uint8)
            rows = {"plain": lambda: hip.generate(pe, seeds, a.size, a.size, a.steps, 1.0),
                    "img2img": lambda: hip.generate_img2img(pe, seeds, pics, a.size, a.size, a.steps, a.strength)}
            out = dict(call=alternate(rows, a.reps))
            E = hip.lanes[0].enc_plans[(B, a.size, a.size)]

            def encoder():
                E.graph.launch()
                stream.synchronize()
            with torch.cuda.stream(stream):
                out["replay"] = alternate({"encoder": encoder}, a.reps)
            res["rows"][f"batch_{B}"] = out
            hip.drop_plans()
            torch.cuda.empty_cache()
        print(json.dumps(res), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
    finally:
        hip.close()


if __name__ == "__main__":
    main()
