#!/usr/bin/env python3
"""What a ControlNet hint costs on one MI355X: synthetic SD1.5 + synthetic ControlNet, 512x512 4 steps, batch 1 and batch 8, with
and without a hint, all in this one run and by bench.py's method (plans built and captured first, then warm graph replays
bracketed by events on the lane's stream).  Also the hint stack on its own (eager launches between two events) next to its
HBM floor, and the FLOP ratio computed from the layer shapes.

  python tools/bench_controlnet.py [--steps 4] [--reps 30] [--warmup 5] [--out profiles/controlnet_mi355x.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import sdlcm_amd  # noqa: E402,F401
from tools.check_profiles_fresh import CSRC, sources_sha256  # noqa: E402

SOURCES = [os.path.join(CSRC, f) for f in ("controlnet.hip", "igemm.hip", "igemm_common.h", "conv_halo.hip", "attention.hip",
                                           "norm.hip", "misc.hip", "mlp_fused.hip", "common.h")]


def flops(cfg, h, w, control):
    """Multiply-add FLOPs (2 per MAC) of one UNet evaluation (convs, linears, attention) and, with ``control``, of the
    ControlNet's conv_in + down + mid blocks and its thirteen 1x1 zero convolutions, from the layer shapes."""
    from sdlcm_amd.weights import controlnet_skip_channels
    boc, lpb, ctx = cfg["block_out_channels"], cfg["layers_per_block"], cfg["cross_attention_dim"]

    def res(cin, cout, hw):
        return 2 * hw * (9 * cin * cout + 9 * cout * cout + (cin * cout if cin != cout else 0))

    def tf(c, hw):
        return 2 * hw * (2 * c * c + 3 * c * c + c * c + c * c + c * c + 8 * c * c + 4 * c * c) + 4 * hw * hw * c + 4 * hw * 77 * c + 2 * 77 * 2 * c * ctx

    enc, H, W, ch, sizes = 2 * h * w * 36 * boc[0], h, w, boc[0], []
    for i, c in enumerate(boc):
        for _ in range(lpb):
            enc += res(ch, c, H * W) + (tf(c, H * W) if cfg["down_attn"][i] else 0)
            ch = c
            sizes.append((c, H * W))
        if i < len(boc) - 1:
            H, W = (H + 1) // 2, (W + 1) // 2
            enc += 2 * H * W * 9 * c * c
            sizes.append((c, H * W))
    mid = 2 * res(ch, ch, H * W) + tf(ch, H * W)
    if control:
        hw = [h * w] + [s for _, s in sizes]
        zero = sum(2 * n * c * c for c, n in zip(controlnet_skip_channels(cfg), hw)) + 2 * H * W * ch * ch
        return enc + mid + zero
    dec, skip = 0, [boc[0]] + [c for c, _ in sizes]
    hws = [h * w] + [s for _, s in sizes]
    rboc, up_attn = tuple(reversed(boc)), tuple(reversed(cfg["down_attn"]))
    for i, c in enumerate(rboc):
        for _ in range(lpb + 1):
            s, n = skip.pop(), hws.pop()
            dec += res(ch + s, c, n) + (tf(c, n) if up_attn[i] else 0)
            ch = c
        if i < len(rboc) - 1:
            dec += 2 * hws[-1] * 9 * c * c
    return enc + mid + dec + 2 * h * w * 9 * boc[0] * 4


def hint_bytes(B, H, W):
    """Bytes the hint stack must move once: the uint8 image in, every layer's fp16 activation written and read once, the
    embedding out."""
    cc = (16, 32, 96, 256)
    n, total, h, w = B * H * W, B * H * W * 3, H, W
    acts = [n * cc[0]]
    for i in range(6):
        if i & 1:
            h, w = (h + 1) // 2, (w + 1) // 2
        acts.append(B * h * w * cc[i // 2 + (i & 1)])
    return total + sum(2 * 2 * a for a in acts) + 2 * B * h * w * 320


def timed_replays(pipe, P, reps, warmup):
    stream = P.lane.stream
    with torch.cuda.stream(stream):
        for _ in range(warmup):
            pipe.replay(P)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for a, b in ev:
            a.record()
            pipe.replay(P)
            b.record()
        stream.synchronize()
    ts = sorted(a.elapsed_time(b) for a, b in ev)
    return dict(ms_median=round(float(np.median(ts)), 4), ms_min=round(ts[0], 4), ms_p90=round(ts[int(0.9 * (len(ts) - 1))], 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from sdlcm_amd import weights
    from sdlcm_amd.pipeline import LcmHipPipeline
    import controlnet_reference as cr
    S = a.size
    pipe = LcmHipPipeline(weights.synthetic_unet(), weights.synthetic_vae(), device="cuda:0")
    pipe.set_controlnet(weights.synthetic_controlnet())
    rows = {}
    try:
        for B in (1, 8):
            pe = torch.randn(B, 77, 768, generator=torch.Generator().manual_seed(5)).to(torch.float16)
            hints = np.stack([cr.test_hint(S, S, b) for b in range(B)])
            seeds = list(range(B))
            pipe.generate(pe, seeds, S, S, a.steps, 1.0)                                   # builds + captures the plan
            pipe.generate(pe, seeds, S, S, a.steps, 1.0, control=(hints, 1.0))
            plain = timed_replays(pipe, pipe.plan(B, S // 8, S // 8, a.steps), a.reps, a.warmup)
            P = pipe.plan(B, S // 8, S // 8, a.steps, control=1.0)
            ctl = timed_replays(pipe, P, a.reps, a.warmup)
            # the hint stack alone: eager launches on the lane's stream between two events
            cn = pipe.lane_controlnet(P.lane)
            with torch.cuda.stream(P.lane.stream):
                ts = []
                for _ in range(a.warmup + a.reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    cn.embed_hint(P.hint, B, S, S, P.hint_emb[:B * (S // 8) ** 2])
                    e1.record()
                    e1.synchronize()
                    ts.append(e0.elapsed_time(e1))
                ts = ts[a.warmup:]
                # copy bandwidth measured here: device-to-device copy of 512 MB
                src = torch.empty(256 << 20, dtype=torch.uint8, device="cuda:0")
                dst = torch.empty_like(src)
                cps = []
                for _ in range(8):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    dst.copy_(src)
                    e1.record()
                    e1.synchronize()
                    cps.append(e0.elapsed_time(e1))
                bw = 2 * src.numel() / (min(cps[2:]) * 1e-3)
            hb = hint_bytes(B, S, S)
            rows[f"batch{B}"] = dict(plain=plain, control=ctl, time_ratio=round(ctl["ms_median"] / plain["ms_median"], 4),
                                     hint_stack=dict(ms_median=round(float(np.median(ts)), 4), ms_min=round(min(ts), 4), bytes=hb,
                                                     copy_GBps=round(bw / 1e9, 1), hbm_floor_ms=round(hb / bw * 1e3, 4)))
        cfg = pipe.unet.cfg
        fu, fc = flops(cfg, S // 8, S // 8, False), flops(cfg, S // 8, S // 8, True)
        res = dict(device=torch.cuda.get_device_name(0), weights="seeded synthetic SD1.5 + ControlNet architecture", size=S,
                   steps=a.steps, reps=a.reps, rows=rows, unet_gflop=round(fu / 1e9, 2), controlnet_gflop=round(fc / 1e9, 2),
                   flop_ratio=round((fu + fc) / fu, 4), sources=SOURCES, source_sha256=sources_sha256(SOURCES))
        print(json.dumps(res), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
    finally:
        pipe.close()


if __name__ == "__main__":
    main()
