#!/usr/bin/env python3
"""Regenerate the narrow-tile table shipped with the package (narrow_plans_gfx950.json) and its timing sheet.

Every distinct contraction shape of the batch-1 SD1.5 pass (512 x 512 by default) with N >= 640 whose shipped launch puts at
most 256 workgroups on the chip is timed under the shipped plan and under the same plan with a 32-column tile
(ops.narrow_set), COLD (autotune._time_cold: weights come from HBM in situ; a warm replay favours the wrong tile), the two arms
alternating, ROUNDS rounds of REPS launches each.  An arm's figure is the mean over its rounds of the faster-half mean; its
spread is max - min over the rounds.  An entry is written only when the narrow figure is below the shipped plan's by more than
the larger of the two spreads.

Usage (GPU box):  python tools/make_narrow_plans.py OUT.json SHEET.txt [size ...]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ["LCM_TUNE_CACHE"] = ""
import torch  # noqa: E402
import sdlcm_amd  # noqa: E402,F401
from sdlcm_amd import autotune, lib, ops, weights  # noqa: E402
from sdlcm_amd.pipeline import LcmHipPipeline  # noqa: E402

REPS, ROUNDS = 20, 3
out_json, out_sheet = sys.argv[1], sys.argv[2]
sizes = [int(v) for v in sys.argv[3:]] or [512]

ops.narrow_clear()                                    # the arms are set here, key by key
plans = lib.known_plans()
pipe = LcmHipPipeline(weights.synthetic_unet(), weights.synthetic_vae(), device="cuda:0")
table, lines = {}, []
lines.append(f"# narrow (64 x 32 / patch x 32) tile against the shipped plan, cold, {ROUNDS} alternating rounds x {REPS} launches per arm;")
lines.append("# us = mean over rounds of the faster-half mean; spread = max - min over rounds; kept: narrow < shipped - max(spreads)")
lines.append(f"# device: {torch.cuda.get_device_name(0)}")
lines.append(f"{'kind,M,N,K,aux':28s} {'plan':>14s} {'wgs':>5s} {'shipped us':>11s} {'spread':>7s} {'narrow us':>10s} {'spread':>7s}  verdict")
for size in sizes:
    P = pipe.plan(1, size // 8, size // 8, 4)
    pipe.tune(P)
    stream = P.lane.stream
    with torch.cuda.stream(stream):
        with ops.recording() as recs:
            pipe._enqueue(P, 1.0)
        stream.synchronize()
        seen = {}
        for key, meta, fn in recs:
            if key is not None:
                seen.setdefault(key, (meta, fn))
        for key, (meta, fn) in sorted(seen.items()):
            kind, M, N, K, aux = key
            if key in table or N < 640 or N % 32 or kind not in (0, 2) or meta.get("geglu") or meta.get("phases", 1) == 4:
                continue
            if (kind == 0 and aux != 1) or (kind == 2 and (aux & 1)):
                continue
            bm, bn, sp, var = (int(v) for v in plans[key][:4]) if key in plans else (64, 64, 0, -1)
            parts = autotune._canonical_splits(key, meta, meta.get("m_img", M))
            wgs = -(-M // bm) * (N // bn if N % bn == 0 else -(-N // 64)) * parts
            if -(-M // bm) * -(-N // 64) * parts > 256:
                continue
            ops.narrow_set(*key)
            ops.profile_begin()
            fn()
            honoured = any(", 32, " in n for n, _ in ops.profile_end())
            arms = {"wide": [], "narrow": []}
            if honoured:
                for _ in range(ROUNDS):
                    for arm in ("wide", "narrow"):
                        ops.narrow_clear()
                        if arm == "narrow":
                            ops.narrow_set(*key)
                        arms[arm].append(autotune._time_cold(fn, REPS) * 1e3)
            ops.narrow_clear()
            for k in table:
                ops.narrow_set(*k)
            tag = ",".join(str(v) for v in key)
            plan = f"{bm}x{bn} s{parts} v{var}"
            if not honoured:
                lines.append(f"{tag:28s} {plan:>14s} {wgs:5d} {'-':>11s} {'-':>7s} {'-':>10s} {'-':>7s}  not a launch the narrow table applies to")
                continue
            w, n = sum(arms["wide"]) / ROUNDS, sum(arms["narrow"]) / ROUNDS
            sw, sn = max(arms["wide"]) - min(arms["wide"]), max(arms["narrow"]) - min(arms["narrow"])
            keep = n < w - max(sw, sn)
            if keep:
                table[key] = 32
                ops.narrow_set(*key)
            lines.append(f"{tag:28s} {plan:>14s} {wgs:5d} {w:11.2f} {sw:7.2f} {n:10.2f} {sn:7.2f}  {'kept' if keep else 'not kept'} ({n / w:.2f}x)")
            print(lines[-1], flush=True)
    pipe.drop_plans()
with open(out_json, "w") as f:
    json.dump({",".join(str(v) for v in k): bn for k, bn in sorted(table.items())}, f, indent=0)
with open(out_sheet, "w") as f:
    f.write("\n".join(lines) + "\n")
print(f"{len(table)} entries -> {out_json}; sheet -> {out_sheet}", flush=True)
