"""Variation seeds and seed-resize on the GPU: lcm_noise_variation_f32 against the float64 reference (tests/variation_reference.py),
its paste windows, batch invariance and refusals; then the pipeline and the worker: what a subseed does to the picture, a latent
walk as one batch-8 pass, mixed batches, every request kind that serves a variation, the refinement cache, the errors, determinism.
End-to-end cases: 64 x 64 (one 96 x 64), 1 to 2 steps, synthetic weights.

Tolerance of the kernel tests (``tolerance`` below), measured, not assumed: the largest |float64 reference - float32 restatement|
(variation_reference.blend_fp32: the kernel's operation order in numpy float32) over THIS module's own inputs, relative to
max |low|, times 8 -- the device's sinf / acosf / sqrtf / division differ from numpy's by a few ulp each.  It is computed on the CPU
when the module runs and printed; measured where this was written: 3.11e-07 (the worst case is the 5 x 5 seed-resize source at t = 0.5),
hence a bound of 2.49e-06 relative to max |low|.  The inputs are conditioned so that float32 and float64 take the same branch in every column: the
sphere-branch cases use seed pairs with |d| <= 0.9 in every column (searched by the reference; none found would be an error), the
linear-branch cases are designed (parallel, antiparallel, zero columns, single-row columns), and no input has a column with
0.95 < |d| < 0.99999 (asserted for every input)."""
import os
import sys
import threading
import types

import numpy as np
import pytest
import torch

import variation_reference as vr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -777.0
SHAPES = [(8, 8), (8, 16), (16, 8), (8, 40), (1, 8), (64, 64)]
TS = [0.1, 0.5, 0.9, 1.0]
RESIZES = [((8, 8), (4, 6)), ((8, 8), (12, 16)), ((8, 8), (4, 12)), ((8, 8), (5, 5)), ((8, 8), (13, 11)), ((5, 5), (8, 8)),
           ((16, 8), (8, 6)), ((16, 8), (20, 16)), ((16, 8), (8, 16)), ((16, 8), (11, 5)), ((16, 8), (21, 13))]


def _clear(lo, hi):
    """no column where float32 and float64 may take different branches"""
    d = np.abs(vr.column_dots(lo, hi)[3])
    d = d[np.isfinite(d)]
    assert not ((d > 0.95) & (d < 0.99999)).any(), d.max()


def _source(hs, ws):
    """(low, high) float32 [4,hs,ws] for the sphere branch: every column |d| <= 0.9 by float64; a single row has no such column"""
    if hs == 1:
        lo, hi = vr._randn(1, hs, ws)[0][0].numpy(), vr._randn(1001, hs, ws)[0][0].numpy()
    else:
        _, _, lo, hi = vr.seed_pair(hs, ws)
        assert vr.sphere_columns(lo, hi).all()
    _clear(lo, hi)
    return lo, hi


def _designed():
    """8 x 8 with exactly parallel, antiparallel and zero columns among sphere columns"""
    _, _, lo, hi = vr.seed_pair(8, 8, start=500)
    lo, hi = lo.copy(), hi.copy()
    lo[0, :, 0] = 0.0
    hi[1, :, 1] = 0.0
    hi[2, :, 2] = 2.0 * lo[2, :, 2]
    hi[3, :, 3] = -0.5 * lo[3, :, 3]
    lo[0, :, 4] = hi[0, :, 4] = 0.0
    hi[1, :, 5] = lo[1, :, 5]
    _clear(lo, hi)
    assert (~vr.sphere_columns(lo, hi)).sum() == 6
    return lo, hi


@pytest.fixture(scope="module")
def sources():
    out = {s: _source(*s) for s in SHAPES}
    out.update({("src",) + src: _source(*src) for _, src in RESIZES})
    out["designed"] = _designed()
    return out


@pytest.fixture(scope="module")
def tolerance(sources):
    """8 x the largest |fp64 - fp32 restatement| / max |low| over every input of this module (module docstring)"""
    worst, where = 0.0, None
    for name, (lo, hi) in sources.items():
        for t in TS:
            e = np.abs(vr.blend_fp64(lo, hi, t) - vr.blend_fp32(lo, hi, t)).max() / np.abs(lo).max()
            if e > worst:
                worst, where = e, (name, t)
    print(f"\n[variation] largest |fp64 - fp32 restatement| / max|low| = {worst:.3g} at {where}; bound = {8 * worst:.3g}")
    assert 0 < worst < 1e-5
    return 8 * worst


def _launch(x, descs):
    """x float32 [B,4,h,w]; descs per slot None | (base | None, sub | None, t) -> the latents after one launch (numpy).  The latents
    sit between guard rows, the sources are checked to be left alone."""
    from sdlcm_amd import ops
    B, _, h, w = x.shape
    buf = torch.full((B + 2, 4, h, w), SENTINEL, dtype=torch.float32, device=DEV)
    lat = buf[1:B + 1]
    lat.copy_(torch.from_numpy(x))
    dd, kept = [], []
    for d in descs:
        if d is None:
            dd.append(None)
            continue
        base, sub, t = d
        ts = [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (base, sub)]
        kept += [(a, a.clone()) for a in ts if a is not None]
        hs, ws = next((a.shape[-2:] for a in ts if a is not None), (h, w))
        dd.append((ts[0], ts[1], hs, ws, t))
    ops.noise_variation(lat, B, h, w, dd)
    torch.cuda.synchronize()
    assert (buf[0] == SENTINEL).all() and (buf[-1] == SENTINEL).all(), "written outside the latents"
    assert all(torch.equal(a, b) for a, b in kept), "a source was written"
    return lat.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------------
# the kernel
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_blend_against_fp64(shape, sources, tolerance):
    lo, hi = sources[shape]
    sph = np.broadcast_to(vr.sphere_columns(lo, hi)[:, None, :], lo.shape)
    assert sph.all() or (shape[0] == 1 and not sph.any())
    for t in TS:
        inplace = _launch(lo[None], [(None, hi, t)])[0]
        out = _launch(np.full((1,) + lo.shape, 5.0, np.float32), [(lo, hi, t)])[0]
        assert inplace.tobytes() == out.tobytes(), "in place and out of place differ"
        ref = vr.blend_fp64(lo, hi, t)
        err = np.abs(inplace - ref).max() / np.abs(lo).max()
        print(f"\n[variation] {shape} t={t}: max|d| / max|low| = {err:.3g} (bound {tolerance:.3g})")
        assert err <= tolerance, (shape, t, err)
        if t == 1.0:
            assert np.array_equal(inplace[sph], hi[sph]), "t = 1 is not high bit for bit on the sphere branch"
            assert np.array_equal(inplace, hi)
    # t = 0, launched directly: low bit for bit, and high is never read (none is given)
    assert _launch(lo[None], [(None, None, 0.0)])[0].tobytes() == lo.tobytes()
    assert _launch(np.zeros((1,) + lo.shape, np.float32), [(lo, None, 0.0)])[0].tobytes() == lo.tobytes()
    assert _launch(lo[None], [(None, hi, 0.0)])[0].tobytes() == lo.tobytes()


def test_designed_linear_columns(sources, tolerance):
    lo, hi = sources["designed"]
    sph = np.broadcast_to(vr.sphere_columns(lo, hi)[:, None, :], lo.shape)
    for t in TS:
        got = _launch(lo[None], [(None, hi, t)])[0]
        assert np.isfinite(got).all()
        ref = vr.blend_fp64(lo, hi, t)
        assert np.abs(got - ref).max() / np.abs(lo).max() <= tolerance, t
        lin = (1.0 - t) * lo.astype(np.float64) + t * hi.astype(np.float64)
        assert np.abs(got - lin)[~sph].max() / np.abs(lo).max() <= tolerance
    assert np.abs(_launch(lo[None], [(None, hi, 0.5)])[0] - (0.5 * lo.astype(np.float64) + 0.5 * hi))[sph].max() > 0.01      # the rest is no lerp


@pytest.mark.parametrize("target,src", RESIZES, ids=[f"{s[0]}x{s[1]}-into-{t[0]}x{t[1]}" for t, s in RESIZES])
def test_seed_resize_windows(target, src, sources, tolerance):
    h, w = target
    lo, hi = sources[("src",) + src]
    x = np.random.default_rng(h * 100 + src[0]).standard_normal((1, 4, h, w)).astype(np.float32)
    sy, ty, ch = vr.window(h, src[0])
    sx, tx, cw = vr.window(w, src[1])
    inside = np.zeros((4, h, w), bool)
    inside[:, ty:ty + ch, tx:tx + cw] = True
    for t in (0.0, 0.5):
        got = _launch(x, [(lo, hi if t else None, t)])[0]
        assert np.array_equal(got[~inside], x[0][~inside]), "cells outside the window changed"
        ref = vr.vary_fp64(x[0], lo, hi, t)
        if t == 0.0:
            assert np.array_equal(got, ref.astype(np.float32)), "strength 0: low is pasted bit for bit"
        else:
            assert np.abs(got - ref).max() / np.abs(lo).max() <= tolerance
            assert np.abs(got[inside] - x[0][inside]).max() > 0.1


@pytest.mark.parametrize("B", [2, 8])
def test_a_slots_bytes_do_not_depend_on_the_batch(B, sources):
    h, w = 8, 8
    x = np.random.default_rng(B).standard_normal((B, 4, h, w)).astype(np.float32)
    lo8, hi8 = sources[(8, 8)]
    menu = [("in place", (None, hi8, 0.3)), None, ("smaller", sources[("src", 4, 6)] + (0.7,)), ("larger", sources[("src", 12, 16)] + (0.1,)),
            None, ("odd", sources[("src", 5, 5)] + (1.0,)), ("paste only", (sources[("src", 13, 11)][0], None, 0.0)), ("in place", (None, lo8, 0.9))]
    descs = [m if m is None else m[1] for m in (menu[:B] if B == 8 else [menu[0], menu[3]])]
    if B == 2:
        assert all(d is not None for d in descs)
    got = _launch(x, descs)
    for b, d in enumerate(descs):
        if d is None:
            assert np.array_equal(got[b], x[b]), f"inactive slot {b} was touched"
        else:
            solo = _launch(x[b:b + 1], [d])[0]
            assert got[b].tobytes() == solo.tobytes(), f"slot {b} of {B} differs from its solo launch"
            assert not np.array_equal(got[b], x[b])
    if B == 8:                                             # ... nor on the slot: the same request in slot 0 and in slot 5
        again = _launch(x[[5, 1, 2, 3, 4, 0, 6, 7]], [descs[5], None, None, None, None, descs[0], None, None])
        assert again[0].tobytes() == got[5].tobytes() and again[5].tobytes() == got[0].tobytes()


def test_refusals_launch_nothing(sources):
    from sdlcm_amd import ops
    from sdlcm_amd.lib import LcmHipError
    lo, hi = (torch.from_numpy(a).to(DEV) for a in sources[(8, 8)])
    lat = torch.full((9, 4, 8, 8), 3.0, dtype=torch.float32, device=DEV)
    d = (None, hi, 8, 8, 0.5)
    for args, what in (((lat, 9, 8, 8, [d] * 9), "9 requests"), ((lat, 1, 8, 8, [(None, hi, 8, 8, 1.5)]), r"strength 1\.5"),
                       ((lat, 1, 8, 8, [(lo, hi, 0, 8, 0.5)]), "source shape 0 x 8"), ((lat, 1, 8, 8, [(lo, hi, 8, 257, 0.5)]), "source shape 8 x 257"),
                       ((lat, 1, 257, 8, [d]), "target shape 257 x 8"), ((lat, 1, 8, 8, [(None, None, 8, 8, 0.5)]), "null pointer"),
                       ((lat, 2, 8, 8, [d, (lat[0], hi, 8, 8, 0.5)]), "overlaps")):
        with pytest.raises(LcmHipError, match=r"rc=-1.*" + what):
            ops.noise_variation(*args)
    torch.cuda.synchronize()
    assert (lat == 3.0).all()


# ---------------------------------------------------------------------------------------------------------------------------
# the pipeline and the worker
# ---------------------------------------------------------------------------------------------------------------------------
def _req(seed=11, **kw):
    d = dict(prompt="a lighthouse at dusk", size="64x64", num_inference_steps=2, guidance_scale=1.0, seed=seed, style_lora=None)
    d.update(kw)
    return types.SimpleNamespace(**d)


def _job(*a, **kw):
    return types.SimpleNamespace(req=_req(*a, **kw))


def _pic(seed=0, h=64, w=64):
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([128 + 100 * np.sin(x / 7.0 + seed), 128 + 100 * np.cos(y / 5.0), 128 + 90 * np.sin((x + y) / 9.0)], -1)
    return np.clip(base + np.random.default_rng(seed).normal(0, 12, (h, w, 3)), 0, 255).astype(np.uint8)


@pytest.fixture(scope="module")
def worker():
    os.environ["MODEL"] = "synthetic"
    os.environ.setdefault("MODEL_ROOT", "/nonexistent")
    os.environ["CONTROLNET"] = "synthetic"
    from sdlcm_amd.backends.worker_factory import create_hip_worker
    try:
        w = create_hip_worker(worker_id=0)
    finally:
        os.environ.pop("CONTROLNET", None)
    yield w
    w.close()


@pytest.fixture(scope="module")
def pe():
    return torch.randn(1, 77, 768, generator=torch.Generator().manual_seed(5)).to(torch.float16)


def _batch(worker, reqs, lane=0):
    """one pass of the engine for requests of one key -> their PNGs"""
    from sdlcm_amd.backends.hip_worker import encode_png
    key = worker._job_key(reqs[0])
    assert all(worker._job_key(r) == key for r in reqs)
    return [encode_png(r[0]) for r in worker._engine.run_batch(key, [worker._prepare(r, key) for r in reqs], lane)]


def test_a_subseed_at_full_strength_is_the_other_seeds_picture(worker):
    """one step, so no step noise: the initial latents are the whole of the seed's influence.  (Fails without the feature: the
    fields are ignored and seed 31's picture comes back.)"""
    eng = worker._engine
    n0 = eng.stats.get("variation_requests", 0)
    a = worker.run_job(_job(31, num_inference_steps=1))[0]
    b = worker.run_job(_job(77, num_inference_steps=1))[0]
    v, seed = worker.run_job(_job(31, num_inference_steps=1, subseed=77, subseed_strength=1.0))
    assert a != b and seed == 31
    assert v == b, "subseed 77 at strength 1.0 did not give seed 77's picture"
    assert eng.stats["variation_requests"] == n0 + 1
    half = worker.run_job(_job(31, num_inference_steps=1, subseed=77, subseed_strength=0.5))[0]
    assert half not in (a, b) and worker.run_job(_job(31, num_inference_steps=1, subseed=77, subseed_strength=0.5))[0] == half
    assert worker.run_job(_job(31, num_inference_steps=1, subseed=77, subseed_strength=0.0))[0] == a
    # no subseed sent: a random one is drawn, the picture moves (and two calls draw two)
    r1, r2 = (worker.run_job(_job(31, num_inference_steps=1, subseed_strength=0.5))[0] for _ in range(2))
    assert a not in (r1, r2) and r1 != r2


def test_generate_with_a_variation_against_the_reference_blend(worker, pe):
    from sdlcm_amd.pipeline import draw_variation
    pipe = worker._engine.pipe
    sigma = pipe.sched.init_noise_sigma
    for hs, ws, t in ((8, 8, 0.5), (6, 12, 0.3)):
        x, extra, sub, base = draw_variation(3, 4, 8, 8, hs, ws, sigma)
        _clear(*(a[0].numpy() for a in (x if base is None else base, sub)))
        got = pipe.generate(pe, [3], 64, 64, 1, 1.0, want_float=True, noises=[(x, extra)], variation=[(t, sub, base)])
        ref = vr.vary_fp64(x[0].numpy(), None if base is None else base[0].numpy(), sub[0].numpy(), t).astype(np.float32)
        want = pipe.generate(pe, [3], 64, 64, 1, 1.0, want_float=True, latents=[torch.from_numpy(ref)])
        plain = pipe.generate(pe, [3], 64, 64, 1, 1.0, want_float=True)
        img = lambda o: np.clip(o["image"] / 2 + 0.5, 0, 1)
        err = np.abs(img(got) - img(want)).max()
        print(f"\n[variation] generate(variation=) vs generate(latents=fp64 blend), source {hs}x{ws} t={t}: image max|d| = {err:.3g}; "
              f"vs the plain request {np.abs(img(got) - img(plain)).max():.3g}")
        assert err < 1e-2 < np.abs(img(got) - img(plain)).max()
        # the captured path gives the eager path's bytes
        assert np.array_equal(pipe.generate(pe, [3], 64, 64, 1, 1.0, noises=[(x, extra)], variation=[(t, sub, base)])["rgb"], got["rgb"])


def test_a_walk_is_one_batch_of_eight(worker):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from tools import minipool
    eng = worker._engine
    frames = [_req(21, subseed=22, subseed_strength=i / 7) for i in range(8)]
    solo = [worker.run_job(types.SimpleNamespace(req=r)) for r in frames]
    assert solo[0] == worker.run_job(_job(21)), "frame 0 (strength 0) is not the plain request"
    assert solo[7][0] != solo[0][0] and len({s[0] for s in solo}) == 8
    pool = minipool.MiniPool(lambda worker_id: worker, {"m": "synthetic"}, "m")
    worker.bind_queue(pool.q)
    try:
        gate, inside = threading.Event(), threading.Event()
        hold = pool.submit_job(minipool.CustomJob(handler=lambda: (inside.set(), gate.wait(30))))
        assert inside.wait(30)
        n0, v0 = len(eng.batcher.batches), eng.stats["variation_requests"]
        futs = [pool.submit_job(minipool.GenerationJob(req=r)) for r in frames]
        gate.set()
        hold.result(60)
        assert [f.result(600) for f in futs] == solo
        pool.q.join()
        assert list(eng.batcher.batches[n0:]) == [8], eng.batcher.batches[n0:]
        assert eng.stats["variation_requests"] == v0 + 7
    finally:
        worker.bind_queue(None)
        pool._worker = None
        pool.shutdown()


def test_plain_and_varied_requests_share_a_pass(worker):
    eng = worker._engine
    reqs = [_req(40), _req(41, subseed=5, subseed_strength=0.4), _req(42), _req(43, seed_resize_from_w=32, seed_resize_from_h=48)]
    solo = [worker.run_job(types.SimpleNamespace(req=r))[0] for r in reqs]
    assert solo[1] != worker.run_job(_job(41))[0] and solo[3] != worker.run_job(_job(43))[0]
    n0 = eng.stats["variation_requests"]
    assert _batch(worker, reqs) == solo
    assert eng.stats["variation_requests"] == n0 + 2
    assert _batch(worker, [reqs[1], reqs[0]]) == [solo[1], solo[0]]


def test_seed_resize_keeps_the_composition_draw(worker, pe):
    from sdlcm_amd.pipeline import draw_noise, draw_variation_sources
    kw = dict(size="96x64", seed_resize_from_w=64, seed_resize_from_h=64)
    a = worker.run_job(_job(9, **kw))[0]
    assert a != worker.run_job(_job(9, size="96x64"))[0] and a == worker.run_job(_job(9, **kw))[0]
    assert worker.run_job(_job(9, size="96x64", seed_resize_from_w=96, seed_resize_from_h=64))[0] == worker.run_job(_job(9, size="96x64"))[0]
    # the initial latents as the pass reads them: the centre window is the 64 x 64 request's draw, the rest the 96 x 64 draw
    pipe = worker._engine.pipe
    sigma = pipe.sched.init_noise_sigma
    _, base = draw_variation_sources(9, None, 8, 8, sigma, resized=True)
    taps = {}
    pipe.generate(pe, [9], 96, 64, 1, 1.0, taps=taps, variation=[(0.0, None, base)])
    lat0, x = taps["latents0"][0], draw_noise(9, 8, 12, 0, sigma)[0][0]
    assert torch.equal(base[0], draw_noise(9, 8, 8, 0, sigma)[0][0])
    assert torch.equal(lat0[:, :, 2:10], base[0]) and torch.equal(lat0[:, :, :2], x[:, :, :2]) and torch.equal(lat0[:, :, 10:], x[:, :, 10:])


KINDS = {"controlnet_image": lambda: dict(controlnet_image=_pic(5)),
         "enable_hr": lambda: dict(enable_hr=True, hr_scale=1.5, denoising_strength=0.7)}


@pytest.mark.parametrize("kind", list(KINDS))
def test_kinds_serve_a_variation_with_the_bytes_of_a_solo_run(worker, kind):
    var = dict(subseed=8, subseed_strength=0.35)
    reqs = [_req(60, **KINDS[kind](), **var), _req(61, **KINDS[kind]()), _req(62, **KINDS[kind](), seed_resize_from_w=48, seed_resize_from_h=32)]
    solo = [worker.run_job(types.SimpleNamespace(req=r))[0] for r in reqs]
    assert solo[0] != worker.run_job(_job(60, **KINDS[kind]()))[0] and solo[2] != worker.run_job(_job(62, **KINDS[kind]()))[0]
    assert _batch(worker, reqs + reqs[:1])[:3] == solo


def test_hires_starts_from_the_varied_plain_requests_latents(worker, pe):
    from sdlcm_amd.pipeline import draw_variation_sources
    pipe = worker._engine.pipe
    sub, _ = draw_variation_sources(5, 6, 8, 8, pipe.sched.init_noise_sigma)
    v = [(0.6, sub, None)]
    hr = pipe.generate(pe, [5], 64, 64, 2, 1.0, hires=(96, 96, 2, 0.7, 0), variation=v)
    plain = pipe.generate(pe, [5], 64, 64, 2, 1.0, variation=v)
    assert np.array_equal(hr["lowres_latents"], plain["latents"])
    assert not np.array_equal(plain["latents"], pipe.generate(pe, [5], 64, 64, 2, 1.0)["latents"])


def test_refinement_never_starts_from_the_unvaried_requests_cache(worker):
    eng = worker._engine
    if eng.refine_cache.cap <= 0:
        pytest.fail("the refinement cache is off: this test needs LCM_REFINE_CACHE_MB > 0")
    rk = dict(denoise_strength=0.6, total_passes=2)
    var = dict(subseed=14, subseed_strength=0.5)
    worker.run_job(_job(13, pass_number=1, **rk))                       # the unvaried request fills x^0 and x^1
    plain2 = worker.run_job(_job(13, pass_number=2, **rk))[0]
    s = dict(eng.stats)
    assert s["refine_cache_hits"] >= 1
    varied2 = worker.run_job(_job(13, pass_number=2, **rk, **var))[0]   # nothing of ITS chain is cached: from scratch
    assert eng.stats["refine_cache_hits"] == s["refine_cache_hits"] and eng.stats["refine_cache_misses"] == s["refine_cache_misses"] + 1
    assert varied2 != plain2
    worker.run_job(_job(13, pass_number=1, **rk, **var))
    s = dict(eng.stats)
    assert worker.run_job(_job(13, pass_number=2, **rk, **var))[0] == varied2      # now from its own x^1, and the same bytes
    assert eng.stats["refine_cache_hits"] == s["refine_cache_hits"] + 1
    assert worker.run_job(_job(13, pass_number=2, **rk, subseed=15, subseed_strength=0.5))[0] != varied2
    assert worker.run_job(_job(13, pass_number=2, **rk))[0] == plain2


def test_errors_are_the_jobs_own_also_in_a_drained_batch(worker):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from tools import minipool
    from sdlcm_amd.backends.hip_worker import HipLcmSDXLWorker
    var = dict(subseed=3, subseed_strength=0.5)
    msg = "subseed / seed_resize_from is not combined with init_image"
    with pytest.raises(RuntimeError, match=msg):
        worker.run_job(_job(1, init_image=_pic(3), denoising_strength=0.5, **var))
    with pytest.raises(RuntimeError, match=msg):
        worker.run_job(_job(1, init_image=_pic(3), denoising_strength=0.6, mask=np.pad(np.full((32, 32), 255, np.uint8), 16), **var))
    with pytest.raises(RuntimeError, match="variation seeds are not served by the SDXL worker"):       # (the key is made without an engine)
        HipLcmSDXLWorker._job_key(_req(1, **var))
    good = worker.run_job(_job(70, **var))
    bad = {1: (dict(init_image=_pic(3), denoising_strength=0.5, **var), msg), 2: (dict(subseed_strength=1.5), "Invalid subseed_strength 1.5"),
           4: (dict(init_image=_pic(3), denoising_strength=0.6, mask=np.pad(np.full((32, 32), 255, np.uint8), 16), seed_resize_from_w=32,
                    seed_resize_from_h=32), msg)}
    pool = minipool.MiniPool(lambda worker_id: worker, {"m": "synthetic"}, "m")
    worker.bind_queue(pool.q)
    try:
        gate, inside = threading.Event(), threading.Event()
        hold = pool.submit_job(minipool.CustomJob(handler=lambda: (inside.set(), gate.wait(30))))
        assert inside.wait(30)
        futs = [pool.submit_job(minipool.GenerationJob(req=_req(70, **bad.get(i, (var, ""))[0]))) for i in range(6)]
        gate.set()
        hold.result(60)
        for i, f in enumerate(futs):
            if i in bad:
                with pytest.raises(RuntimeError, match=bad[i][1]):
                    f.result(600)
            else:
                assert f.result(600) == good
        pool.q.join()
    finally:
        worker.bind_queue(None)
        pool._worker = None
        pool.shutdown()


def test_bytes_do_not_depend_on_the_lane_or_on_what_ran_before(worker):
    eng = worker._engine
    r = _req(90, subseed=91, subseed_strength=0.45, seed_resize_from_w=48, seed_resize_from_h=80)
    solo = worker.run_job(types.SimpleNamespace(req=r))[0]
    assert _batch(worker, [r], lane=0) == [solo]
    if eng.n_lanes > 1:
        assert _batch(worker, [r], lane=1) == [solo]
    worker.run_job(_job(5, prompt="something else entirely", subseed=1, subseed_strength=0.9))
    worker.run_job(_job(6, size="96x64"))
    assert worker.run_job(types.SimpleNamespace(req=r))[0] == solo
