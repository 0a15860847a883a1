#!/usr/bin/env python3
"""What weighted and long prompts cost on one MI355X, synthetic SD1.5 weights, measured at the worker (``HipLcmWorker.run_job``):

  run_job       a 512x512 4-step batch-1 request: the plain n = 1 prompt timed alone (the row --plain-only takes on the parent), then
                ("run_job_in_turn") prompts of n = 1, 2, 3 chunks (77 n context rows) timed in turn, whose plans and graphs
                alternate on the lane: compare those rows with each other, not with the row taken alone; wall-clock milliseconds
                of run_job (tokenise, chunk, CLIP, emphasis, upload, graph replay, download, PNG), median of ``reps`` calls; every
                call's text ends in a word of its own, so none is served from the chunker's cache
  text          the conditioning stage alone for n = 1, 2, 3, on the lane's stream, between two stream synchronisations: "cold" with
                the chunker's cache emptied before every call (parse + tokenise + chunk + CLIP graph replay + emphasis launch or
                copy: a text seen for the first time), "cached" with the text's chunks looked up (what a pass pays after the key)
  emphasis      lcm_prompt_emphasis_f16 alone, device events around a window of back-to-back launches, 1 / 3 / 8 chunks of D = 768
  attention     cross-attention at Sk = 154 / 231 / 308 on the two kernels that can serve it (the streaming kernel, impl 1, and the
                register-staged one, impl 0; d = 160 is served by the latter alone): SD1.5's d = 40 at Sq 4096 and d = 80 at Sq 1024
                with 8 heads, SD 2.x's d = 64 at Sq 4096 with 5 heads and at Sq 1024 with 10; batch 1 and 8, K / V as column windows
                of a [B Sk, kv_total] buffer; the two kernels timed alternately, 5 rounds, median
                Every device-event window is sized from a trial of 200 launches to last about WINDOW_S = 0.5 s.

  python tools/prompt_bench.py [--reps N] [--out profiles/prompt_mi355x.json] [--parent FILE [FILE ...]]
  python tools/prompt_bench.py --plain-only --out FILE     the n = 1 run_job row alone (runs on a tree without the feature: the
                                                            parent commit's figure); --parent merges such files into the output

Every shape is run (plans built, tuned, captured) before its timed window.  No pass/fail threshold: this records."""
import argparse
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import sdlcm_amd  # noqa: E402,F401


def summarise(ts):
    return dict(ms_median=round(float(np.median(ts)), 3), ms_min=round(min(ts), 3), ms_p90=round(float(np.percentile(ts, 90)), 3), n=len(ts))


def words(n, tag="w"):
    return " ".join(f"{tag}{i}" for i in range(n))


def req(prompt, seed):
    # (a word of its own per call: no call finds its text in the chunker's cache)
    return types.SimpleNamespace(req=types.SimpleNamespace(prompt=f"{prompt} s{seed}", size="512x512", num_inference_steps=4, guidance_scale=1.0,
                                                           seed=seed, style_lora=None))


def time_run_job(worker, prompts, reps, warm=5):
    """{name: prompt} timed in turn, ``reps`` rounds, after ``warm`` calls each."""
    for p in prompts.values():
        for i in range(warm):
            worker.run_job(req(p, i))
    ts = {k: [] for k in prompts}
    for i in range(reps):
        for k, p in prompts.items():
            t0 = time.perf_counter()
            worker.run_job(req(p, 100 + i))
            ts[k].append((time.perf_counter() - t0) * 1e3)
    return {k: summarise(v) for k, v in ts.items()}


def time_text(worker, prompts, reps):
    eng = worker._engine
    stream = eng.pipe.lane(0).stream
    cache = eng.encode.chunker._cache
    out = {}
    for k, (p, n) in prompts.items():
        r = [req(p, 0).req]
        for cold in (True, False):
            ts = []
            with eng.lane_locks[0], torch.cuda.stream(stream):
                for i in range(reps + 5):
                    if cold:
                        cache.clear()
                    stream.synchronize()
                    t0 = time.perf_counter()
                    type(worker)._conditioning(eng, r, 512, 512, 1.0, 0, **({"n_ctx": n} if n > 1 else {}))
                    stream.synchronize()
                    if i >= 5:
                        ts.append((time.perf_counter() - t0) * 1e3)
            out[f"{k} {'cold' if cold else 'cached'}"] = summarise(ts)
    return out


WINDOW_S = 0.5


def _window_ms(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def events_ms(fn, launches=None):
    """ms per launch over a window of back-to-back launches; launches None: as many as a trial of 200 says fill WINDOW_S."""
    for _ in range(10):
        fn()
    if launches is None:
        launches = max(200, int(WINDOW_S * 1e3 / (_window_ms(fn, 200) / 200)))
    return _window_ms(fn, launches) / launches


def time_emphasis():
    from sdlcm_amd import ops
    out = {}
    for n in (1, 3, 8):
        z = (torch.randn(n * 77, 768, device="cuda") + 0.3).half()
        w = torch.full((n * 77,), 1.1, device="cuda")
        o = torch.empty_like(z)
        out[f"chunks={n}"] = dict(us_per_launch=round(1e3 * float(np.median([events_ms(lambda: ops.prompt_emphasis(z, w, o, n, 77, 768))
                                                                                 for _ in range(5)])), 2))
    return out


def time_attention(kv_total=20480):
    from sdlcm_amd import ops
    rows = {}
    for d, Sq, heads in ((40, 4096, 8), (80, 1024, 8), (64, 4096, 5), (64, 1024, 10)):
        C = heads * d
        for Sk in (154, 231, 308):
            for B in (1, 8):
                q = torch.randn(B * Sq, C, device="cuda").half()
                kv = torch.randn(B * Sk, kv_total, device="cuda").half()
                o = torch.empty(B * Sq, C, dtype=torch.float16, device="cuda")
                k, v = kv[:, 1280:1280 + C], kv[:, 1280 + C:1280 + 2 * C]
                call = lambda: ops.attention(q, k, v, o, B, heads, Sq, Sk, d, ldq=C, ldk=kv_total, ldv=kv_total, ldo=C, scale=0.0)
                ts = {0: [], 1: []}
                try:
                    for _ in range(5):
                        for impl in (1, 0):
                            ops.set_attention_impl(impl)
                            ts[impl].append(events_ms(call))
                finally:
                    ops.set_attention_impl(1)
                rows[f"d={d} heads={heads} Sq={Sq} Sk={Sk} B={B}"] = dict(streaming_us=round(1e3 * float(np.median(ts[1])), 2),
                                                           register_staged_us=round(1e3 * float(np.median(ts[0])), 2))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prompt_mi355x.json"))
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--parent", nargs="*", default=[])
    a = ap.parse_args()
    assert torch.cuda.is_available(), "prompt_bench needs the MI355X"
    os.environ["MODEL"] = "synthetic"
    os.environ.setdefault("MODEL_ROOT", "/nonexistent")
    from sdlcm_amd.backends.worker_factory import create_hip_worker
    worker = create_hip_worker(worker_id=0)
    plain = "a photo of an astronaut riding a horse on mars"
    doc = dict(device=torch.cuda.get_device_name(0), request="512x512, 4 steps, batch 1, guidance 1.0, synthetic SD1.5 weights",
               reps=a.reps)
    try:
        if a.plain_only:
            doc["run_job"] = time_run_job(worker, {"n=1": plain}, a.reps)
        else:
            p2, p3 = words(100) + " (sunset:1.3)", words(170) + " (sunset:1.3)"
            ck = worker._engine.encode.chunker
            assert (ck.chunk(p2).n, ck.chunk(p3).n) == (2, 3)
            doc["run_job"] = time_run_job(worker, {"n=1": plain}, a.reps)          # alone, as --plain-only times it: comparable
            doc["run_job_in_turn"] = time_run_job(worker, {"n=1": plain, "n=1 weighted": "a photo of an (astronaut:1.3) riding a horse on mars",
                                                           "n=2": p2, "n=3": p3}, a.reps)
            doc["text"] = time_text(worker, {"n=1": (plain, 1), "n=2": (p2, 2), "n=3": (p3, 3)}, a.reps)
            doc["emphasis"] = time_emphasis()
            doc["attention"] = time_attention()
            doc["stats"] = {k: worker._engine.stats[k] for k in ("prompt_chunks", "weighted_prompts")}
    finally:
        worker.close()
    if a.parent:
        doc["parent"] = [json.load(open(f))["run_job"]["n=1"] for f in a.parent]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
