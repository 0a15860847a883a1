#!/usr/bin/env python3
"""What an SD-upscale request costs on one MI355X, synthetic SD1.5 weights:

  launch        lcm_grid_combine_rgb8 alone, device events around a window of back-to-back launches (a few hundred ms): a 1024x1024
                picture from 9 tiles of 512x512 (overlap 64) and a 2048x2048 one from 25; microseconds per launch, median of 5 windows
  run_job       a 512x512 -> 1024x1024 request at 4 steps (Lanczos x 2, overlap 64, strength 0.5: 9 tiles, passes of 8 + 1) at the
                worker (``HipLcmWorker.run_job``), timed in turn with
  client        what a client must do today for the same picture on the same tree: PIL Lanczos upscale, 9 single image-to-image
                ``run_job``s of the crops, decode the 9 PNGs, PIL paste (A1111's combine_grid), encode the PNG with PIL
  plain         a plain 512x512 4-step ``run_job``, timed alone (the row --plain-only takes on another checkout)

  python tools/sdupscale_bench.py [--reps N] [--out profiles/sdupscale_bench_mi355x.json] [--parent FILE ...] [--mine FILE ...]
  python tools/sdupscale_bench.py --plain-only [--root DIR] --out FILE
        the plain run_job row alone, with the package imported from DIR (a checkout of the parent commit, built): the parent's
        figure.  Runs of the two trees are ALTERNATED by the caller (parent, this tree, parent, this tree, ... each a process of its
        own); --parent / --mine merge the files into the output, whose "plain_vs_parent" then holds every run's median and the
        spread between runs of one tree -- the yardstick for a difference between the trees.

Every shape is run (plans built, tuned, captured) before its timed window.  No pass/fail threshold: this records."""
import argparse
import io
import json
import os
import sys
import time
import types

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402

WINDOW_S = 0.3


def summarise(ts):
    return dict(ms_median=round(float(np.median(ts)), 3), ms_min=round(min(ts), 3), ms_p90=round(float(np.percentile(ts, 90)), 3), n=len(ts))


def job(seed, **kw):
    d = dict(prompt="a photo of an astronaut riding a horse on mars", size="512x512", num_inference_steps=4, guidance_scale=1.0,
             seed=seed, style_lora=None)
    d.update(kw)
    return types.SimpleNamespace(req=types.SimpleNamespace(**d))


def picture(h=512, w=512, seed=0):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([128 + 100 * np.sin(x / 37.0), 128 + 100 * np.cos(y / 29.0), 128 + 90 * np.sin((x + y) / 41.0)], -1)
    return np.clip(base + rng.normal(0, 10, (h, w, 3)), 0, 255).astype(np.uint8)


def in_turn(rows, reps, warm=3):
    """{name: callable(i)} timed in turn, ``reps`` rounds, after ``warm`` calls each."""
    for fn in rows.values():
        for i in range(warm):
            fn(i)
    ts = {k: [] for k in rows}
    for i in range(reps):
        for k, fn in rows.items():
            t0 = time.perf_counter()
            fn(100 + i)
            ts[k].append((time.perf_counter() - t0) * 1e3)
    return {k: summarise(v) for k, v in ts.items()}


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
    """microseconds per launch over a window of back-to-back launches sized from a trial of 50 to last about WINDOW_S"""
    for _ in range(10):
        fn()
    launches = max(50, int(WINDOW_S * 1e3 / (_window_ms(torch, fn, 50) / 50)))
    return 1e3 * _window_ms(torch, fn, launches) / launches


def time_launch(torch):
    from sdlcm_amd import ops
    from sdlcm_amd.backends import sdupscale as su
    out = {}
    for side in (1024, 2048):
        g = su.grid(side, side, 512, 512, 64)
        T = g.cols * g.rows
        tiles = torch.randint(0, 256, (T, 512, 512, 3), dtype=torch.uint8, device="cuda")
        dst = torch.empty(side, side, 3, dtype=torch.uint8, device="cuda")
        desc = ops.grid_desc(side, side, 512, 512, 64, g.xs, g.ys)
        us = float(np.median([events_us(torch, lambda: ops.grid_combine_rgb8(tiles, dst, desc)) for _ in range(5)]))
        out[f"{side}x{side} from {T} tiles of 512x512, overlap 64"] = dict(us_per_launch=round(us, 2), bytes_written=side * side * 3,
                                                                         bytes_of_tiles=T * 512 * 512 * 3)
    return out


def client_side(worker, pic, seed, scale=2, tile=512, overlap=64):
    """Today's way to the same picture, from outside the worker; the paste is the tests' restatement of A1111's combine_grid."""
    from PIL import Image
    if os.path.join(HERE, "tests") not in sys.path:
        sys.path.insert(0, os.path.join(HERE, "tests"))
    import sdupscale_reference as ref
    W, H = pic.shape[1] * scale, pic.shape[0] * scale
    up = np.asarray(Image.fromarray(pic).resize((W, H), Image.LANCZOS))
    xs, ys = ref.geometry(W, H, tile, tile, overlap)
    tiles = []
    for k, (x, y) in enumerate((x, y) for y in ys for x in xs):
        png, _ = worker.run_job(job(seed + k, init_image=np.ascontiguousarray(up[y:y + tile, x:x + tile]), denoising_strength=0.5))
        tiles.append(np.asarray(Image.open(io.BytesIO(png)).convert("RGB")))
    buf = io.BytesIO()
    Image.fromarray(ref.combine_pil(np.stack(tiles), W, H, overlap, xs, ys)).save(buf, format="PNG")
    return buf.getvalue()


def spread(files):
    meds = [json.load(open(f))["run_job"]["plain"]["ms_median"] for f in files]
    return dict(ms_medians=meds, ms_mean=round(float(np.mean(meds)), 3), ms_spread=round(max(meds) - min(meds), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--plain-reps", type=int, default=60)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "sdupscale_bench_mi355x.json"))
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--parent", nargs="*", default=[])
    ap.add_argument("--mine", nargs="*", default=[])
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import torch
    import sdlcm_amd  # noqa: F401
    assert torch.cuda.is_available(), "sdupscale_bench needs the MI355X"
    os.environ["MODEL"] = "synthetic"
    os.environ.setdefault("MODEL_ROOT", "/nonexistent")
    from sdlcm_amd.backends.worker_factory import create_hip_worker
    worker = create_hip_worker(worker_id=0)
    doc = dict(device=torch.cuda.get_device_name(0), request="512x512, 4 steps, batch 1, guidance 1.0, synthetic SD1.5 weights",
               reps=a.reps, plain_reps=a.plain_reps)
    try:
        doc["run_job"] = in_turn({"plain": lambda i: worker.run_job(job(i))}, a.plain_reps, warm=5)   # alone, as --plain-only times it
        if not a.plain_only:
            pic = picture()
            sdu = dict(init_image=pic, denoising_strength=0.5, script_name="SD upscale", script_args=[None, 64, "Lanczos", 2])
            doc["run_job_in_turn"] = in_turn({"sd upscale 512x512 -> 1024x1024 (9 tiles)": lambda i: worker.run_job(job(i, **sdu)),
                                              "client: PIL upscale + 9 img2img run_jobs + PIL combine": lambda i: client_side(worker, pic, i)},
                                             a.reps)
            doc["launch"] = time_launch(torch)
            doc["stats"] = {k: worker._engine.stats[k] for k in ("sdupscale_requests", "sdupscale_tiles")}
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
