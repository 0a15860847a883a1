#!/usr/bin/env python3
"""What the mask of an inpaint request costs on one MI355X, synthetic SD1.5 weights, measured at ``LcmHipPipeline``:

  img2img       generate_img2img: a 512x512 picture -> VAE encoder -> posterior / re-noise launch -> 4 steps over
                timesteps(4, 0.5) -> decode, at batch 1 and batch 8
  inpaint       generate_inpaint with the same inputs plus a mask (mask_blur 4): the same stages, the masked step in place of the
                step, plus the mask launches and the overlay
  added         the launches an inpaint request adds, alone, between two stream synchronisations: lcm_inpaint_mask_prepare
                (three launches) and lcm_inpaint_composite_rgb8, and each masked step against the step it replaces

  python tools/inpaint_bench.py [--reps N] [--out profiles/inpaint_bench_mi355x.json]

``call`` rows are wall-clock milliseconds of the call (draws, uploads, graph replays, downloads; ends in a stream synchronise);
the two kinds are timed alternately after three warm calls each, ``reps`` rounds; median, minimum and the 10th / 90th
percentiles (the spread).  ``added`` rows are device-event milliseconds of 50 back-to-back repetitions, divided by 50.  The
expectation to confirm or refute: inpaint - img2img = the mask launches + the overlay (+ two more small uploads / downloads).
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
    return dict(ms_median=round(float(np.median(ts)), 3), ms_min=round(min(ts), 3), ms_p10=round(float(np.percentile(ts, 10)), 3),
                ms_p90=round(float(np.percentile(ts, 90)), 3))


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
    return {k: summarise(v) for k, v in ts.items()}, ts


def device_ms(fn, stream, n=50, rounds=7):
    """Median over ``rounds`` of (device-event time of n back-to-back fn()) / n, on ``stream``."""
    out = []
    with torch.cuda.stream(stream):
        for _ in range(5):
            fn()
        for _ in range(rounds):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            stream.synchronize()
            a.record(stream)
            for _ in range(n):
                fn()
            b.record(stream)
            b.synchronize()
            out.append(a.elapsed_time(b) / n)
    return round(float(np.median(out)), 5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--strength", type=float, default=0.5)
    ap.add_argument("--mask-blur", type=float, default=4.0)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from sdlcm_amd import ops, weights
    from sdlcm_amd.pipeline import LcmHipPipeline
    hip = LcmHipPipeline(weights.synthetic_unet(), weights.synthetic_vae(), device="cuda:0")
    hip.set_vae_encoder_source(weights.synthetic_vae_encoder())
    stream = hip.stream
    S = a.size
    res = dict(device=torch.cuda.get_device_name(0), weights="seeded synthetic SD1.5 architecture", size=S, steps=a.steps,
               strength=a.strength, mask_blur=a.mask_blur, reps=a.reps, rows={})
    try:
        for B in [int(x) for x in a.batches.split(",")]:
            pe = torch.randn(B, 77, 768, generator=torch.Generator().manual_seed(5)).to(torch.float16)
            seeds = list(range(100, 100 + B))
            pics = np.random.default_rng(7).integers(0, 256, (B, S, S, 3), dtype=np.uint8)
            masks = np.zeros((B, S, S), np.uint8)
            masks[:, S // 4: 3 * S // 4, S // 3:] = 255
            rows = {"img2img": lambda: hip.generate_img2img(pe, seeds, pics, S, S, a.steps, a.strength),
                    "inpaint": lambda: hip.generate_inpaint(pe, seeds, pics, masks, S, S, a.steps, a.strength, mask_blur=a.mask_blur)}
            call, ts = alternate(rows, a.reps)
            paired = np.asarray(ts["inpaint"]) - np.asarray(ts["img2img"])          # the same round: the same neighbours on the host
            out = dict(call=call, inpaint_minus_img2img=dict(ms_of_medians=round(call["inpaint"]["ms_median"] - call["img2img"]["ms_median"], 3),
                                                             **{"paired_" + k: v for k, v in summarise(list(paired)).items()}))
            # the added launches alone, on the plan's own buffers
            P = next(p for p in hip.lanes[0].plans.values() if p.kind == "inpaint" and p.B == B)
            Q = next(p for p in hip.lanes[0].plans.values() if p.kind == "from-state" and p.B == B)
            r, wts = hip._mask_weights(a.mask_blur)
            h = w = S // 8
            ts_cut = hip.sched.timesteps(a.steps, a.strength)
            coef, _ = hip.sched.step_coefficients(ts_cut, 0)
            ksa, ksb = hip.sched.renoise_coefficients(ts_cut[1]) if a.steps > 1 else (1.0, 0.0)
            added = dict(
                mask_prepare=device_ms(lambda: ops.inpaint_mask_prepare(P.mask, wts, r, P.alpha, P.mask_tmp, P.latmask, B, S, S), stream),
                composite=device_ms(lambda: ops.inpaint_composite_rgb8(P.rgb, P.init_img, P.alpha, B, S, S), stream),
                step_inpaint=device_ms(lambda: ops.scheduler_step_inpaint(P.eps, P.lat, P.noise[1 % P.noise.shape[0]], P.xk[0], P.noise[0],
                                                                           P.latmask, coef, False, ksa, ksb, B, h, w), stream),
                step=device_ms(lambda: ops.scheduler_step(Q.eps, Q.lat, Q.noise[1 % Q.noise.shape[0]], coef, False, B, h, w), stream))
            added["mask_prepare_plus_composite"] = round(added["mask_prepare"] + added["composite"], 5)
            out["added_device_ms"] = added
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
