"""Variation seeds and seed-resize without a GPU: parsing and job keys (backends/variation.py), every error and its message, the
draws of pipeline.draw_variation against the RNG contract, the properties of the float64 reference (tests/variation_reference.py),
the refinement cache's identity, and the library's refusals, which run before any launch."""
import ctypes as C
import os
import sys
import threading
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sdlcm_amd  # noqa: E402,F401
import variation_reference as vr  # noqa: E402
from sdlcm_amd.backends import refine as rf  # noqa: E402
from sdlcm_amd.backends import variation as va  # noqa: E402
from sdlcm_amd.backends.hip_worker import HipLcmSDXLWorker, HipLcmWorker  # noqa: E402
from sdlcm_amd.pipeline import draw_noise, draw_variation  # noqa: E402
from tools import minipool  # noqa: E402


def _req(**kw):
    d = dict(prompt="a cat", size="512x512", num_inference_steps=4, guidance_scale=1.0, seed=7, style_lora=None)
    d.update(kw)
    return types.SimpleNamespace(**d)


PIC = np.zeros((8, 8, 3), np.uint8)
INACTIVE = [dict(), dict(subseed=5), dict(subseed=5, subseed_strength=0), dict(subseed=5, subseed_strength=0.0), dict(subseed=-1),
            dict(subseed=-1, subseed_strength=0.0, seed_resize_from_w=-1, seed_resize_from_h=-1),      # what A1111 clients send by default
            dict(seed_resize_from_w=0, seed_resize_from_h=0), dict(seed_resize_from_w=256, seed_resize_from_h=0),
            dict(seed_resize_from_w=-8, seed_resize_from_h=256), dict(seed_resize_from_w=None, seed_resize_from_h=None),
            dict(seed_resize_from_w=512, seed_resize_from_h=512), dict(seed_resize_from_w=519, seed_resize_from_h=513),   # equal after // 8
            dict(subseed="not read", subseed_strength=None)]


@pytest.mark.parametrize("fields", INACTIVE, ids=[str(i) for i in range(len(INACTIVE))])
def test_inactive_forms_are_plain_requests(fields):
    today = (512, 512, 4, 1.0, None, 0)
    assert va.parse_variation(_req(**fields), 512, 512) is None
    assert HipLcmWorker._job_key(_req(**fields)) == today == HipLcmWorker._job_key(_req())
    assert HipLcmSDXLWorker._job_key(_req(**fields)) == today
    # ... and with a picture they are the image-to-image request of always
    i2i = dict(init_image=PIC, denoising_strength=0.5)
    assert HipLcmWorker._job_key(_req(**fields, **i2i)) == HipLcmWorker._job_key(_req(**i2i))


def test_active_forms_and_the_key():
    today = (512, 512, 4, 1.0, None, 0)
    assert va.parse_variation(_req(subseed=5, subseed_strength=0.25), 512, 512) == (5, 0.25, 64, 64)
    assert va.parse_variation(_req(subseed=5, subseed_strength=1), 512, 384) == (5, 1.0, 48, 64)
    assert va.parse_variation(_req(subseed_strength=0.5), 512, 512) == (None, 0.5, 64, 64)            # to be drawn
    assert va.parse_variation(_req(subseed=-1, subseed_strength=0.5), 512, 512) == (None, 0.5, 64, 64)
    assert va.parse_variation(_req(seed_resize_from_w=256, seed_resize_from_h=384), 512, 512) == (None, 0.0, 48, 32)
    assert va.parse_variation(_req(subseed=9, subseed_strength=0.1, seed_resize_from_w=768, seed_resize_from_h=256), 512, 512) == (9, 0.1, 32, 96)
    assert va.parse_variation(_req(subseed=9, subseed_strength=0.1, seed_resize_from_w=512, seed_resize_from_h=512), 512, 512) == (9, 0.1, 64, 64)
    assert va.parse_variation(_req(seed_resize_from_w=2048, seed_resize_from_h=8), 512, 512) == (None, 0.0, 1, 256)
    # the variation is per image: no part of the key of any kind that serves it
    for fields in (dict(subseed=5, subseed_strength=0.25), dict(seed_resize_from_w=256, seed_resize_from_h=384)):
        assert HipLcmWorker._job_key(_req(**fields)) == today
        for kind in (dict(denoise_strength=0.6, pass_number=2), dict(enable_hr=True, hr_scale=1.5, denoising_strength=0.7),
                     dict(controlnet_image=np.zeros((512, 512, 3), np.uint8))):
            assert HipLcmWorker._job_key(_req(**fields, **kind)) == HipLcmWorker._job_key(_req(**kind))


ERRORS = [(dict(subseed_strength=1.5), r"Invalid subseed_strength 1\.5"), (dict(subseed_strength=-0.1), r"Invalid subseed_strength -0\.1"),
          (dict(subseed_strength=float("nan")), r"Invalid subseed_strength nan"), (dict(subseed_strength=float("inf")), r"Invalid subseed_strength inf"),
          (dict(subseed_strength="much"), r"Invalid subseed_strength 'much'"), (dict(subseed_strength=True), r"Invalid subseed_strength True"),
          (dict(subseed_strength=0.5, subseed=1.5), r"Invalid subseed 1\.5"), (dict(subseed_strength=0.5, subseed="seven"), r"Invalid subseed 'seven'"),
          (dict(subseed_strength=0.5, subseed=True), r"Invalid subseed True"),
          (dict(seed_resize_from_w=4, seed_resize_from_h=512), r"Invalid seed_resize_from 4x512: a source of 0x64"),
          (dict(seed_resize_from_w=512, seed_resize_from_h=7), r"Invalid seed_resize_from 512x7"),
          (dict(seed_resize_from_w=2056, seed_resize_from_h=512), r"Invalid seed_resize_from 2056x512: a source of 257x64"),
          (dict(seed_resize_from_w=512, seed_resize_from_h=4096), r"expected 1\.\.256 a side"),
          (dict(subseed=3, subseed_strength=0.5, init_image=PIC, denoising_strength=0.5), r"subseed / seed_resize_from is not combined with init_image"),
          (dict(seed_resize_from_w=256, seed_resize_from_h=256, init_image=PIC, denoising_strength=0.5),
           r"subseed / seed_resize_from is not combined with init_image"),
          (dict(subseed=3, subseed_strength=0.5, init_image=PIC, denoising_strength=0.5, mask=np.zeros((8, 8), np.uint8)),
           r"subseed / seed_resize_from is not combined with init_image")]


@pytest.mark.parametrize("fields,msg", ERRORS, ids=[str(i) for i in range(len(ERRORS))])
def test_errors_and_their_messages(fields, msg):
    with pytest.raises(RuntimeError, match=msg):
        HipLcmWorker._job_key(_req(**fields))


def test_the_sdxl_worker_refuses_an_active_variation():
    for fields in (dict(subseed=5, subseed_strength=0.25), dict(seed_resize_from_w=256, seed_resize_from_h=384)):
        with pytest.raises(RuntimeError, match=r"variation seeds are not served by the SDXL worker"):
            HipLcmSDXLWorker._job_key(_req(**fields))
    with pytest.raises(RuntimeError, match=r"Invalid subseed_strength 2"):
        HipLcmSDXLWorker._job_key(_req(subseed_strength=2))


# ---- the draws -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(8, 8, 8, 8), (8, 12, 8, 8), (8, 8, 5, 11)])
def test_draw_variation_follows_the_rng_contract(shape):
    h, w, hs, ws = shape
    seed, subseed, sigma = 1234, 99, 1.5
    x, extra, sub, base = draw_variation(seed, subseed, h, w, hs, ws, sigma, n_extra=3)
    x0, extra0 = draw_noise(seed, h, w, 3, sigma)
    assert torch.equal(x, x0) and len(extra) == 3 and all(torch.equal(a, b) for a, b in zip(extra, extra0))
    assert torch.equal(sub, draw_noise(subseed, hs, ws, 0, sigma)[0]) and tuple(sub.shape) == (1, 4, hs, ws)
    if (hs, ws) == (h, w):
        assert base is None
    else:
        # a generator of its own, seeded with the request's seed: the first 4 hs ws normals of G(seed) at that shape
        g = torch.Generator(device="cpu").manual_seed(seed)
        assert torch.equal(base, torch.randn((1, 4, hs, ws), generator=g, dtype=torch.float32) * sigma)
    rx, rextra, rsub, rbase = vr.draws(seed, subseed, h, w, hs, ws, sigma, n_extra=3)
    assert torch.equal(rx, x) and torch.equal(rsub, sub) and all(torch.equal(a, b) for a, b in zip(rextra, extra))
    assert (rbase is None and base is None) or torch.equal(rbase, base)


# ---- the reference's own properties --------------------------------------------------------------------------------------------
def _pair(h, w, seed=3):
    g = np.random.default_rng(seed)
    return g.standard_normal((4, h, w)).astype(np.float32), g.standard_normal((4, h, w)).astype(np.float32)


def test_reference_endpoints_and_norms():
    lo, hi = _pair(16, 24)
    assert np.array_equal(vr.blend_fp64(lo, hi, 0.0), lo.astype(np.float64))
    assert np.abs(vr.blend_fp64(lo, hi, 1.0) - hi).max() < 1e-14
    assert np.array_equal(vr.blend_fp32(lo, hi, 0.0), lo)
    sph = vr.sphere_columns(lo, hi)
    assert sph.all()
    assert np.array_equal(vr.blend_fp32(lo, hi, 1.0), hi)                    # sin(w) / sin(w) == 1 and sin(0) == 0, exactly
    # The column norm of the result.  |a l + b h|^2 = a^2 |l|^2 + b^2 |h|^2 + 2 a b |l| |h| cos(w) with a, b >= 0 grows with both
    # norms when cos(w) >= 0 and is |l|^2 at |l| = |h| (a^2 + b^2 + 2 a b cos(w) = 1), so for the ACUTE columns it lies between the two
    # norms.  For an obtuse column it need not (this seed has such columns below both norms at t = 0.1); what holds for every
    # sphere-branch column is the sphere itself: with both columns at one norm the result has that norm.
    n_lo, n_hi = np.sqrt((lo.astype(np.float64) ** 2).sum(1)), np.sqrt((hi.astype(np.float64) ** 2).sum(1))
    acute = vr.column_dots(lo, hi)[3] >= 0
    assert acute.any() and (~acute).any()
    same = hi.astype(np.float64) * (n_lo / n_hi)[:, None, :]
    for t in (0.1, 0.5, 0.9):
        r = vr.blend_fp64(lo, hi, t)
        n = np.sqrt((r ** 2).sum(1))
        assert (n[acute] >= np.minimum(n_lo, n_hi)[acute] * (1 - 1e-12)).all() and (n[acute] <= np.maximum(n_lo, n_hi)[acute] * (1 + 1e-12)).all(), t
        assert np.abs(np.sqrt((vr.blend_fp64(lo, same, t) ** 2).sum(1)) / n_lo - 1).max() < 1e-12, t
        assert np.abs(vr.blend_fp32(lo, hi, t) - r).max() < 1e-5 * np.abs(lo).max()
    # a linear blend of the same columns falls inside the sphere: the reference is not a lerp
    lin = 0.5 * lo.astype(np.float64) + 0.5 * hi
    assert (np.sqrt((lin ** 2).sum(1)) < np.minimum(n_lo, n_hi)).any()


def test_reference_degenerate_columns_are_finite_and_linear():
    lo, hi = _pair(8, 8)
    lo[0, :, 0] = 0.0                                     # a zero column of low
    hi[1, :, 1] = 0.0                                     # ... of high
    hi[2, :, 2] = 2.0 * lo[2, :, 2]                       # exactly parallel
    hi[3, :, 3] = -0.5 * lo[3, :, 3]                      # exactly antiparallel
    lo[0, :, 4] = hi[0, :, 4] = 0.0                       # both zero
    sph = vr.sphere_columns(lo, hi)
    want = np.ones((4, 8), bool)
    want[0, 0] = want[1, 1] = want[2, 2] = want[3, 3] = want[0, 4] = False
    assert np.array_equal(sph, want)
    for t in (0.25, 0.3, 1.0):
        r64, r32 = vr.blend_fp64(lo, hi, t), vr.blend_fp32(lo, hi, t)
        assert np.isfinite(r64).all() and np.isfinite(r32).all()
        lin = (1 - t) * lo.astype(np.float64) + t * hi.astype(np.float64)
        assert np.abs(r64 - lin)[~np.broadcast_to(sph[:, None, :], lo.shape)].max() < 1e-15
    # a single row: every column is parallel or antiparallel to itself
    lo1, hi1 = _pair(1, 8)
    assert not vr.sphere_columns(lo1, hi1).any()
    assert np.allclose(vr.blend_fp64(lo1, hi1, 0.3), 0.7 * lo1.astype(np.float64) + 0.3 * hi1.astype(np.float64), rtol=0, atol=1e-15)


WINDOWS = [  # (h, w, hs, ws) -> target rows, target columns, source rows, source columns
    ((8, 8, 4, 6), (2, 6), (1, 7), (0, 4), (0, 6)),           # smaller
    ((8, 8, 12, 16), (0, 8), (0, 8), (2, 10), (4, 12)),       # larger: the centre crop fills the target
    ((8, 8, 4, 12), (2, 6), (0, 8), (0, 4), (2, 10)),         # wider but shorter: the axes are independent
    ((8, 8, 5, 5), (1, 6), (1, 6), (0, 5), (0, 5)),           # 5 into 8: (8 - 5) // 2 = 1
    ((5, 5, 8, 8), (0, 5), (0, 5), (2, 7), (2, 7)),           # 8 into 5: (5 - 8) // 2 = -2 (floor), the crop starts at 2
    ((16, 8, 8, 8), (4, 12), (0, 8), (0, 8), (0, 8)),
]


@pytest.mark.parametrize("shape,ty,tx,sy,sx", WINDOWS, ids=["x".join(map(str, c[0])) for c in WINDOWS])
def test_reference_paste_windows(shape, ty, tx, sy, sx):
    h, w, hs, ws = shape
    x = np.arange(4 * h * w, dtype=np.float64).reshape(4, h, w)
    r = -1.0 - np.arange(4 * hs * ws, dtype=np.float64).reshape(4, hs, ws)
    out = vr.paste(x, r)
    assert np.array_equal(out[:, ty[0]:ty[1], tx[0]:tx[1]], r[:, sy[0]:sy[1], sx[0]:sx[1]])
    outside = np.ones((4, h, w), bool)
    outside[:, ty[0]:ty[1], tx[0]:tx[1]] = False
    assert np.array_equal(out[outside], x[outside]) and (out[~outside] < 0).all()
    assert vr.window(h, hs) == (sy[0], ty[0], ty[1] - ty[0]) and vr.window(w, ws) == (sx[0], tx[0], tx[1] - tx[0])
    # strength 0 with a seed-resize: low is pasted, nothing is blended
    assert np.array_equal(vr.vary_fp64(x, r, None, 0.0), out)


# ---- the refinement cache's identity -------------------------------------------------------------------------------------------
def test_request_ident_carries_an_active_variation_and_only_then():
    key = (512, 512, 4, 1.0, None, 0, 0.6, 2)
    r = _req(denoise_strength=0.6, pass_number=2)
    plain = rf.request_ident(r, key, 7)
    assert plain == ("a cat", 7, 512, 512, 4, 1.0, None, 0) == rf.request_ident(r, key, 7, None)
    a = rf.request_ident(r, key, 7, (5, 0.25, 64, 64))
    assert a != plain and a[:len(plain)] == plain
    assert a != rf.request_ident(r, key, 7, (6, 0.25, 64, 64)) and a != rf.request_ident(r, key, 7, (5, 0.5, 64, 64))
    assert a != rf.request_ident(r, key, 7, (5, 0.25, 32, 64)) and a == rf.request_ident(r, key, 7, (5, 0.25, 64, 64))
    hash(a)


# ---- the worker's side, on a stand-in engine -----------------------------------------------------------------------------------
def _fake_worker(run_pass=lambda key, items: None):
    from sdlcm_amd.backends import hip_worker
    from sdlcm_amd.backends.batching import MicroBatcher
    from sdlcm_amd.backends import prompt_syntax as ps
    from sdlcm_amd.clip import HashTokenizer
    pipe = types.SimpleNamespace(sched=types.SimpleNamespace(init_noise_sigma=2.0), unet=types.SimpleNamespace(has_cond=True))
    enc = types.SimpleNamespace(chunker=ps.PromptChunker(HashTokenizer()), enc=types.SimpleNamespace(L=12))
    eng = types.SimpleNamespace(pipe=pipe, batch_sizes=(1, 2, 4, 8), passes=[], encode=enc)

    def run_batch(key, items, lane=0):
        eng.passes.append((key, list(items)))
        run_pass(key, items)
        return [(np.full((8, 8, 3), it[1] % 251, np.uint8), np.zeros((1, 4, 8, 8), np.float16)) for it in items]

    eng.batcher = MicroBatcher(run_batch, max_batch=8, lanes=1)
    w = object.__new__(hip_worker.HipLcmWorker)
    w.worker_id, w._engine = 0, eng
    w._bind_prompt_ctx()
    return w


def test_prepare_draws_on_the_callers_thread_and_leaves_plain_items_alone():
    w = _fake_worker()
    try:
        key = w._job_key(_req(size="64x64"))
        plain = w._prepare(_req(size="64x64"), key)
        assert type(plain) is tuple and len(plain) == 3
        for fields in INACTIVE:                            # (written for 512x512 requests)
            assert type(w._prepare(_req(**fields), w._job_key(_req()))) is tuple
        it = w._prepare(_req(size="64x64", subseed=21, subseed_strength=0.25), key)
        assert isinstance(it, tuple) and len(it) == 3 and it[1] == 7
        assert torch.equal(it[2][0], plain[2][0]) and all(torch.equal(a, b) for a, b in zip(it[2][1], plain[2][1]))   # the request's own draws
        t, sub, base = it.variation
        assert t == 0.25 and base is None and torch.equal(sub, draw_noise(21, 8, 8, 0, 2.0)[0])
        assert it.ident == (21, 0.25, 8, 8)
        it = w._prepare(_req(size="96x64", subseed=21, subseed_strength=0.5, seed_resize_from_w=64, seed_resize_from_h=64), w._job_key(_req(size="96x64")))
        t, sub, base = it.variation
        assert tuple(sub.shape) == tuple(base.shape) == (1, 4, 8, 8) and torch.equal(base, draw_noise(7, 8, 8, 0, 2.0)[0])
        assert it.ident == (21, 0.5, 8, 8)
        it = w._prepare(_req(size="96x64", seed_resize_from_w=64, seed_resize_from_h=64), w._job_key(_req(size="96x64")))
        assert it.variation[0] == 0.0 and it.variation[1] is None and it.ident == (None, 0.0, 8, 8)
        # no subseed sent: one is drawn by the seed's policy, and two requests get two
        a, b = (w._prepare(_req(size="64x64", subseed_strength=0.5, **kw), key) for kw in (dict(), dict(subseed=-1)))
        assert 0 <= a.ident[0] < 100_000_000 and 0 <= b.ident[0] < 100_000_000 and a.ident[0] != b.ident[0]
        assert torch.equal(a.variation[1], draw_noise(a.ident[0], 8, 8, 0, 2.0)[0])
    finally:
        w._engine.batcher.close()


def test_errors_reach_only_their_own_job_in_a_drained_batch():
    w = _fake_worker()
    pool = minipool.MiniPool(lambda worker_id: w, {"m": "synthetic"}, "m", queue_max=64)
    w.bind_queue(pool.q)
    bad = {1: (dict(subseed_strength=1.5), "Invalid subseed_strength 1.5"), 3: (dict(subseed=2, subseed_strength=0.5, init_image=PIC, denoising_strength=0.5),
                                                                                  "not combined with init_image"),
           5: (dict(seed_resize_from_w=4096, seed_resize_from_h=64), "Invalid seed_resize_from"), 6: (dict(subseed="x", subseed_strength=0.1), "Invalid subseed")}
    good = {2: dict(subseed=9, subseed_strength=0.5), 4: dict(seed_resize_from_w=32, seed_resize_from_h=32)}
    try:
        gate, inside = threading.Event(), threading.Event()
        hold = pool.submit_job(minipool.CustomJob(handler=lambda: (inside.set(), gate.wait(10))))
        assert inside.wait(10)
        futs = [pool.submit_job(minipool.GenerationJob(req=_req(size="64x64", seed=100 + i, **bad.get(i, (good.get(i, {}), ""))[0]))) for i in range(8)]
        gate.set()
        hold.result(10)
        for i, f in enumerate(futs):
            if i in bad:
                with pytest.raises(RuntimeError, match=bad[i][1]):
                    f.result(10)
            else:
                assert f.result(10)[1] == 100 + i
        pool.q.join()
        # plain and varied jobs share the passes: the four good jobs of the key were drained together
        passes = w._engine.passes
        assert sorted(len(p[1]) for p in passes) == [4]
        varied = sorted(it[1] for p in passes for it in p[1] if getattr(it, "variation", None) is not None)
        assert varied == [102, 104]
    finally:
        pool._worker = None
        pool.shutdown()


# ---- the library's refusals: checked before anything is enqueued, so they run here ---------------------------------------------
def test_the_library_refuses_bad_launches_without_a_gpu():
    from sdlcm_amd import lib
    L = lib.load()
    assert "lcm_noise_variation_f32" in lib.EXPORTS
    buf = C.create_string_buffer(16 * 8 * 8 * 3 + 64)
    base = (C.addressof(buf) + 15) & ~15
    lat0, src = base, base + 16 * 8 * 8 * 2

    def call(B=1, h=8, w=8, lat=lat0, **kw):
        arr = (lib.VariationDesc * max(B, 1))()
        for b in range(B):
            f = dict(low=src, high=src, hs=8, ws=8, t=0.5, active=1)
            f.update(kw)
            arr[b] = lib.VariationDesc(**f)
        return L.lcm_noise_variation_f32(lat, B, h, w, arr, None), L.lcm_last_error()
    for kw, what in ((dict(B=9), b"9 requests"), (dict(B=0), b"0 requests"), (dict(t=1.5), b"strength 1.5"), (dict(t=-0.25), b"strength"),
                     (dict(t=float("nan")), b"strength"), (dict(hs=0), b"source shape 0 x 8"), (dict(ws=257), b"source shape 8 x 257"),
                     (dict(h=0), b"target shape 0 x 8"), (dict(w=257), b"target shape 8 x 257"), (dict(low=None), b"null pointer"),
                     (dict(high=None), b"null pointer"), (dict(lat=None), b"null pointer"), (dict(low=src + 2), b"misaligned"),
                     (dict(low=lat0 + 16), b"overlaps"), (dict(high=lat0), b"overlaps"), (dict(low=lat0, hs=4), b"in place")):
        rc, msg = call(**kw)
        assert rc == -1 and what in msg, (kw, rc, msg)
    # no active slot: nothing to do, and nothing is launched
    assert call(active=0)[0] == 0
    assert L.lcm_noise_variation_f32(lat0, 1, 8, 8, None, None) == -1
