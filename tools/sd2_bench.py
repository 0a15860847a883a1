#!/usr/bin/env python3
"""SD 2.x timings on one MI355X: the synthetic SD 2.1-768 pipeline (865 M UNet with 64-wide heads and OpenCLIP-H context,
SD1.5 VAE, v-prediction LCM step) through LcmHipPipeline's captured graph.

  python tools/sd2_bench.py [--reps N] [--out FILE.json]        (GPU)
  python tools/sd2_bench.py --count-flops                       (CPU: re-derive the FLOP constants below)

Per configuration: the first call (plan, first-use autotuning of the shapes the shipped table does not hold, eager warm-up,
capture) and the steady state (graph replays with device-resident inputs, median of N, the same measurement as bench.py's
headline), as images/s and as the fraction of the dense fp16 MFMA roof the algorithmic FLOPs reach."""
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

PEAK_FLOPS = 2.5e15          # dense fp16 MFMA (MI355X_MICROARCH.md), as DESIGN.md section 7
# Algorithmic FLOPs (2 per multiply-add; convolutions, linears and the attention matmuls) of one SD2 UNet forward of one latent
# image and of one VAE decode, counted by --count-flops with torch's FlopCounterMode over the fp32 CPU oracle.
UNET_FLOPS = {512: 0.804257e12, 768: 2.14911e12}
VAE_FLOPS = {512: 2.51452e12, 768: 5.7543e12}
CONFIGS = [(512, 1, 1.0), (512, 8, 1.0), (768, 1, 1.0), (768, 8, 1.0), (512, 1, 7.5)]
STEPS = 4


def count_flops():
    from torch.utils.flop_counter import FlopCounterMode
    from sdlcm_amd import weights
    from sdlcm_amd.config import SD2_UNET, unet_config
    from oracle.unet import UNetOracle
    from oracle.vae import VAEDecoderOracle
    cfg = unet_config(SD2_UNET)
    u = UNetOracle(weights.synthetic_sd2_unet(), cfg)
    v = VAEDecoderOracle(weights.synthetic_vae())
    out = {}
    for S in (512, 768):
        x = torch.randn(1, 4, S // 8, S // 8)
        e = torch.randn(1, 77, 1024)
        with torch.inference_mode(), FlopCounterMode(display=False) as fu:
            u.forward(x, 999, e, None)
        with torch.inference_mode(), FlopCounterMode(display=False) as fv:
            v.decode_plain(x)
        out[S] = (fu.get_total_flops(), fv.get_total_flops())
        print(f"{S}: unet {out[S][0]:.6g} vae {out[S][1]:.6g}", flush=True)
    return out


def image_flops(S, guidance):
    ub = 2 if guidance > 1.0 else 1                     # classifier-free guidance: UNet batch 2 per image
    return STEPS * ub * UNET_FLOPS[S] + VAE_FLOPS[S]


def bench(reps):
    from sdlcm_amd import weights
    from sdlcm_amd.config import SD2_UNET, unet_config
    from sdlcm_amd.pipeline import LcmHipPipeline
    from sdlcm_amd.scheduler import LCMSchedule, SD21_768_SCHEDULE
    dev = "cuda:0"
    pipe = LcmHipPipeline(weights.synthetic_sd2_unet(), weights.synthetic_vae(), unet_config(SD2_UNET), device=dev,
                          schedule=LCMSchedule(**SD21_768_SCHEDULE))
    g = torch.Generator().manual_seed(0)
    rows = []
    for S, B, guid in CONFIGS:
        pe = torch.randn(B, 77, 1024, generator=g).half()
        kw = dict(negative_embeds=torch.randn(B, 77, 1024, generator=g).half()) if guid > 1 else {}
        seeds = list(range(B))
        keys0 = len(pipe._tuned_keys)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pipe.generate(pe, seeds, S, S, STEPS, guid, **kw)          # plan + first-use tuning + warm-up + capture + one replay
        first_s = time.perf_counter() - t0
        t0 = time.perf_counter()
        pipe.generate(pe, seeds, S, S, STEPS, guid, **kw)
        second_s = time.perf_counter() - t0
        P = pipe.plan(B, S // 8, S // 8, STEPS, guid > 1, guid)
        st = P.lane.stream
        ts = []
        with torch.cuda.stream(st):
            for _ in range(3):
                pipe.replay(P)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for _ in range(reps):
                e0.record(st)
                pipe.replay(P)
                e1.record(st)
                e1.synchronize()
                ts.append(e0.elapsed_time(e1))
        ms = float(np.median(ts))
        fl = image_flops(S, guid)
        row = dict(size=S, batch=B, steps=STEPS, guidance=guid, ms_per_pass=round(ms, 3), ms_min=round(min(ts), 3),
                   images_per_s=round(B / (ms * 1e-3), 3), tflop_per_image=round(fl / 1e12, 4),
                   pipeline_tflops=round(fl * B / (ms * 1e-3) / 1e12, 1),
                   frac_of_fp16_mfma_roof=round(fl * B / (ms * 1e-3) / PEAK_FLOPS, 4),
                   first_call_s=round(first_s, 2), second_call_s=round(second_s, 3),
                   shapes_tuned_on_first_use=len(pipe._tuned_keys) - keys0)
        print(json.dumps(row), flush=True)
        rows.append(row)
    pipe.close()
    return dict(device=torch.cuda.get_device_name(0), weights="seeded synthetic SD 2.1-768 architecture", rows=rows,
                peak_flops=PEAK_FLOPS, reps=reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default="")
    ap.add_argument("--count-flops", action="store_true")
    a = ap.parse_args()
    if a.count_flops:
        count_flops()
        return
    res = bench(a.reps)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
