"""Multi-pass refinement on the GPU (denoise_strength / pass_number / total_passes): the two kernels against float64, the chain
against the CPU oracle chain (tests/refine_reference.py), and the worker's behaviour -- bytes that do not depend on batch, lane
or cache state, the work a request costs, isolation of a bad request, SD 2.x and SDXL."""
import io
import os
import sys
import threading
from dataclasses import dataclass, field
from typing import Optional

import numpy as np
import pytest
import torch

import launch_audit as la
import refine_reference as rr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -24
# final latents against the fp32 oracle: the bound of tests/test_configs_gpu.py (relative to the scale of the data)
LATENT_REL_TOL = 5e-3


@dataclass
class _Style:
    style: Optional[str] = None
    level: int = 0


@dataclass
class _Req:
    prompt: str
    size: str = "64x64"
    num_inference_steps: int = 4
    guidance_scale: float = 1.0
    seed: Optional[int] = None
    style_lora: _Style = field(default_factory=_Style)
    denoise_strength: Optional[float] = None
    pass_number: Optional[int] = None
    total_passes: Optional[int] = None


@dataclass
class _Job:
    req: _Req


def _dec(png):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(png)).convert("RGB")).astype(int)


# ---------------------------------------------------------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------------------------------------------------------
def _data(shape, seed, offset=0.0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale + offset


@pytest.mark.parametrize("B,h,w", [(1, 8, 8), (3, 9, 5), (8, 64, 64), (2, 45, 80)])
@pytest.mark.parametrize("offset", [0.0, 40.0])
@pytest.mark.parametrize("dup", [False, True])
def test_latents_renoise_fp64(B, h, w, offset, dup):
    from sdlcm_amd import ops
    from sdlcm_amd.scheduler import LCMSchedule
    sa, sb = LCMSchedule().renoise_coefficients(499)
    x = _data((B, 4, h, w), 1, offset, 20.0)
    n = _data((B, 4, h, w), 2)
    rows = 2 * B if dup else B
    lat = torch.full((rows + 1, 4, h, w), -7.0, device=DEV)           # one image more: must stay untouched
    ops.latents_renoise(x.to(DEV), n.to(DEV), sa, sb, lat, B, h, w, dup=dup)
    torch.cuda.synchronize()
    got = lat.cpu().numpy()
    ref, bnd = rr.renoise_fp64(x.numpy(), n.numpy(), sa, sb)
    err = np.abs(got[:B].astype(np.float64) - ref)
    print(f"[renoise] B={B} {h}x{w} offset={offset} dup={dup}: max err/bound = {(err / bnd).max():.3g}")
    assert (err <= bnd).all()
    if dup:
        assert np.array_equal(got[:B], got[B:2 * B])
    assert (got[rows] == -7.0).all()
    # the operation order the interface states -- one rounded product, then one fused multiply-add -- leaves two roundings
    ax = np.abs(np.float64(np.float32(sa)) * x.numpy().astype(np.float64))
    assert (err <= 1.0001 * U * (ax + np.abs(ref))).all()


@pytest.mark.parametrize("pred", ["epsilon", "v_prediction", "sample"])
@pytest.mark.parametrize("cfg", [False, True])
@pytest.mark.parametrize("B,h,w,offset", [(1, 8, 8, 0.0), (3, 9, 5, 0.0), (2, 32, 32, 30.0)])
def test_handover_step(pred, cfg, B, h, w, offset):
    """x^k: bit-equal to the existing `last` step and inside its fp64 bound; lat: bit-equal to lcm_latents_renoise of (x^k, noise)
    and inside the bound of the step followed by the re-noise."""
    from sdlcm_amd import ops
    from sdlcm_amd.scheduler import LCMSchedule
    s = LCMSchedule(prediction_type=pred)
    ts = s.timesteps(4, 0.5)
    coef, last = s.step_coefficients(ts, 3)
    assert last
    nsa, nsb = s.renoise_coefficients(ts[0])
    m = _data((B, h, w, 4), 3, offset * 0.1, 1.0 if pred != "sample" else 15.0)
    mu = _data((B, h, w, 4), 4, offset * 0.1, 1.0 if pred != "sample" else 15.0)
    x = _data((B, 4, h, w), 5, offset, 12.0)
    n = _data((B, 4, h, w), 6)
    g = 4.0
    kw = dict(eps_uncond=mu.to(DEV), guidance=g) if cfg else {}
    # the existing kernel, last = True
    want = x.clone().to(DEV)
    ops.scheduler_step(m.to(DEV), want, n.to(DEV), coef, True, B, h, w, pred=pred, **kw)
    # the hand-over form: state is the second half of a [2B] buffer under CFG, as the pipeline holds it
    rows = 2 * B if cfg else B
    lat = torch.full((rows + 1, 4, h, w), -7.0, device=DEV)
    state = lat[B:2 * B] if cfg else lat[:B]
    state.copy_(x)
    xk = torch.full((B + 1, 4, h, w), -7.0, device=DEV)
    ops.scheduler_step_handover(m.to(DEV), state, n.to(DEV), xk, coef, nsa, nsb, B, h, w, pred=pred, dup=cfg, **kw)
    again = torch.zeros(B, 4, h, w, device=DEV)
    ops.latents_renoise(xk[:B].contiguous(), n.to(DEV), nsa, nsb, again, B, h, w)
    torch.cuda.synchronize()
    assert la.same_bits(xk[:B], want), "x^k differs from the `last` step's output"
    assert la.same_bits(state, again), "hand-over re-noise differs from lcm_latents_renoise"
    if cfg:
        assert la.same_bits(lat[:B], lat[B:2 * B])
    assert (lat[rows] == -7.0).all() and (xk[B] == -7.0).all()
    ref, bnd = la.sampler_step_reference(m, x, None, coef, True, m_u=mu if cfg else None, guidance=g, pred=pred)
    r1 = la.worst_ratio(xk[:B].cpu(), ref, bnd)
    den = ref.numpy()
    ref2, b2 = rr.renoise_fp64(den, n.numpy(), nsa, nsb)
    b2 = b2 + float(np.float32(nsa)) * bnd.numpy()
    r2 = float((np.abs(state.cpu().numpy().astype(np.float64) - ref2) / b2).max())
    print(f"[handover] {pred} cfg={cfg} B={B} {h}x{w}: x^k err/bound {r1:.3g}, lat err/bound {r2:.3g}")
    assert r1 <= 1.0 and r2 <= 1.0


def test_handover_rejects_bad_arguments():
    from sdlcm_amd import ops
    from sdlcm_amd.lib import LcmHipError
    t = torch.zeros(1, 4, 8, 8, device=DEV)
    e = torch.zeros(1, 8, 8, 4, device=DEV)
    with pytest.raises(ValueError):
        ops.scheduler_step_handover(e, t, t, t.clone(), [1] * 6, 1.0, 0.0, 1, 8, 8, pred="x_start")
    with pytest.raises(LcmHipError):
        ops.latents_renoise(t.reshape(-1)[1:], t, 1.0, 0.0, t.clone(), 1, 8, 4)          # misaligned


# ---------------------------------------------------------------------------------------------------------------------------
# the chain against the CPU oracle chain
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def state():
    from sdlcm_amd import weights
    from sdlcm_amd.pipeline import LcmHipPipeline
    usd, vsd = weights.synthetic_unet(), weights.synthetic_vae()
    hip = LcmHipPipeline(usd, vsd, device=DEV)
    yield dict(hip=hip, ora=rr.RefineChainOracle(usd, vsd))
    hip.close()


def _embeds(B, seed=5):
    return torch.randn(B, 77, 768, generator=torch.Generator().manual_seed(seed)).to(torch.float16)


@pytest.mark.parametrize("size", [(64, 64), (96, 64)])
@pytest.mark.parametrize("d,steps,p", [(0.5, 4, 1), (0.7, 10, 1), (0.8, 8, 3)])
def test_chain_parity_with_the_cpu_oracle(state, d, steps, p, size):
    hip, ora = state["hip"], state["ora"]
    width, height = size
    seed = 1000 + steps
    pe = _embeds(1, seed=seed)
    ref = ora(pe.float(), width, height, steps, 1.0, seed, d, p)
    out = hip.generate(pe, [seed], width, height, steps, 1.0, want_float=True, strength=d, passes=p)
    assert out["xk_first"] == 0 and out["xk"].shape[0] == p + 1 and out["unet_evals"] == steps * (p + 1)
    xk = out["xk"].cpu().numpy()
    for k in range(p + 1):
        e = np.abs(xk[k] - ref["xk"][k])
        print(f"[refine] {width}x{height} d={d} steps={steps} p={p}: x^{k} max|d|={e.max():.4g} = {e.max() / ref['xk'][k].std():.3g} x std")
    assert np.array_equal(xk[p], out["latents"])
    a = np.clip(out["image"].transpose(0, 3, 1, 2) / 2 + 0.5, 0, 1)
    b = np.clip(ref["image"] / 2 + 0.5, 0, 1)
    e = np.abs(a - b)
    print(f"[refine] {width}x{height} d={d} steps={steps} p={p}: image[0,1] max|d|={e.max():.4g} mean|d|={e.mean():.4g}")
    gl = ref["xk"][p]
    lat = np.abs(out["latents"] - gl)
    assert e.max() < 1e-2
    assert lat.max() < LATENT_REL_TOL * gl.std(), f"x^{p}: max|d|={lat.max():.4g} against std {gl.std():.4g}"
    assert np.abs(out["rgb"].astype(int) - ref["image_u8"].astype(int)).max() <= 3
    # x^0 is the plain request's final latents, bit for bit; the captured graph gives the eager bytes
    plain = hip.generate(pe, [seed], width, height, steps, 1.0)
    assert np.array_equal(plain["latents"], xk[0])
    rep = hip.generate(pe, [seed], width, height, steps, 1.0, strength=d, passes=p)
    assert np.array_equal(rep["rgb"], out["rgb"]) and np.array_equal(rep["latents"], out["latents"])
    assert not np.array_equal(rep["rgb"], plain["rgb"])
    # from cached latents: any start depth gives the same bytes
    for k0 in range(p):
        part = hip.generate(pe, [seed], width, height, steps, 1.0, strength=d, passes=p, start=(k0, [rep["xk"][k0, 0]]))
        assert part["unet_evals"] == steps * (p - k0) and part["xk_first"] == k0
        assert np.array_equal(part["rgb"], rep["rgb"]) and np.array_equal(part["latents"], rep["latents"]), k0
        assert torch.equal(part["xk"], rep["xk"][k0:])


def test_chain_in_a_padded_batch_equals_the_solo_runs(state):
    """Three requests with seeds of their own in a batch of four (the last repeated): each gets the bytes of its solo run, from
    scratch and from cached x^1."""
    hip = state["hip"]
    pe = _embeds(3, seed=9)
    seeds = [11, 12, 13]
    solo = [hip.generate(pe[i:i + 1], [seeds[i]], 64, 64, 2, 1.0, strength=0.6, passes=2) for i in range(3)]
    both = hip.generate(torch.cat([pe, pe[2:]]), seeds + [13], 64, 64, 2, 1.0, strength=0.6, passes=2)
    warm = hip.generate(torch.cat([pe, pe[2:]]), seeds + [13], 64, 64, 2, 1.0, strength=0.6, passes=2,
                        start=(1, [solo[i]["xk"][1, 0] for i in (0, 1, 2, 2)]))
    for i in range(3):
        assert np.array_equal(both["rgb"][i], solo[i]["rgb"][0]) and np.array_equal(warm["rgb"][i], solo[i]["rgb"][0])
        assert np.array_equal(both["latents"][i], solo[i]["latents"][0])


def test_generate_argument_errors(state):
    from sdlcm_amd.lib import LcmHipError
    hip = state["hip"]
    pe = _embeds(1)
    with pytest.raises(ValueError, match="The combined original_steps x strength"):
        hip.generate(pe, [1], 64, 64, 7, 1.0, strength=0.1, passes=1)
    with pytest.raises(LcmHipError, match="strength needs passes"):
        hip.generate(pe, [1], 64, 64, 2, 1.0, strength=0.5)
    with pytest.raises(LcmHipError, match="start depth"):
        hip.generate(pe, [1], 64, 64, 2, 1.0, strength=0.5, passes=1, start=(1, [torch.zeros(4, 8, 8, device=DEV)]))


# ---------------------------------------------------------------------------------------------------------------------------
# the worker
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def worker():
    os.environ["MODEL"] = "synthetic"
    os.environ.setdefault("MODEL_ROOT", "/nonexistent")
    from sdlcm_amd.backends.worker_factory import create_hip_worker
    w = create_hip_worker(worker_id=0)
    yield w
    w.close()


def test_run_job_serves_denoise_strength_and_pass_number(worker, state):
    """The test that fails without the feature: denoise_strength changes the image, to what the oracle chain gives; pass 2
    differs from pass 1."""
    eng = worker._engine
    base = dict(prompt="a paper boat on a pond", size="64x64", seed=77, num_inference_steps=4)
    plain, seed = worker.run_job(_Job(_Req(**base)))
    p1, s1 = worker.run_job(_Job(_Req(**base, denoise_strength=0.5)))
    p2, _ = worker.run_job(_Job(_Req(**base, denoise_strength=0.5, pass_number=2, total_passes=3)))
    assert seed == s1 == 77 and p1[:8] == b"\x89PNG\r\n\x1a\n"
    assert p1 != plain and p2 != p1 and p2 != plain
    with torch.cuda.stream(eng.pipe.stream):
        pe = eng.encode([base["prompt"]]).float().cpu()
        eng.pipe.stream.synchronize()
    for p, png in ((1, p1), (2, p2)):
        ref = state["ora"](pe, 64, 64, 4, 1.0, 77, 0.5, p)
        d8 = np.abs(_dec(png) - ref["image_u8"][0].astype(int))
        print(f"[refine] run_job d=0.5 p={p}: u8 max diff {d8.max()}, differing pixels {(d8 > 0).mean():.4f}; "
              f"against the plain image: {np.abs(_dec(png) - _dec(plain)).max()}")
        assert d8.max() <= 3          # 1e-2 on [0,1] is 2.55 levels, plus the rounding to u8: the bound of test_pipeline_gpu.py
    # run_job_with_latents: the 8x8 pool of x^p
    from oracle import glue
    png, _, blob = worker.run_job_with_latents(_Job(_Req(**base, denoise_strength=0.5)))
    assert png == p1 and len(blob) == 512
    want = np.frombuffer(glue.latents_blob(state["ora"](pe, 64, 64, 4, 1.0, 77, 0.5, 1)["xk"][1]), np.float16).astype(np.float32)
    got = np.frombuffer(blob, np.float16).astype(np.float32)
    assert np.abs(got - want).max() < LATENT_REL_TOL * max(1.0, want.std()) + 2.0 ** -10 * np.abs(want).max()


def test_plain_requests_are_untouched(worker):
    eng = worker._engine
    base = dict(prompt="a quiet harbour", size="64x64", seed=5, num_inference_steps=2)
    plain = worker.run_job(_Job(_Req(**base)))
    before = dict(eng.stats), len(eng.refine_cache), set(eng.pipe.lanes[0].plans)
    same = worker.run_job(_Job(_Req(**base, denoise_strength=1.0)))
    same2 = worker.run_job(_Job(_Req(**base, denoise_strength=1.0, pass_number=1, total_passes=3)))
    assert same == plain and same2 == plain
    after = dict(eng.stats)
    assert after["unet_evals"] == before[0]["unet_evals"] + 4
    for k in ("refine_cache_hits", "refine_cache_misses", "refine_cache_puts"):
        assert after[k] == before[0][k]
    assert len(eng.refine_cache) == before[1] and set(eng.pipe.lanes[0].plans) == before[2]


def test_validation_errors_reach_the_caller_and_the_worker_goes_on(worker):
    base = dict(prompt="x", size="64x64", seed=1, num_inference_steps=2)
    for extra, name in ((dict(denoise_strength=0.01), "denoise_strength"), (dict(denoise_strength=1.5), "denoise_strength"),
                        (dict(pass_number=9), "pass_number"), (dict(denoise_strength=0.5, pass_number=0), "pass_number"),
                        (dict(pass_number=3, total_passes=2), "total_passes")):
        with pytest.raises(RuntimeError, match=name):
            worker.run_job(_Job(_Req(**base, **extra)))
    with pytest.raises(RuntimeError, match="The combined original_steps x strength"):
        worker.run_job(_Job(_Req(prompt="x", size="64x64", seed=1, num_inference_steps=7, denoise_strength=0.1)))
    assert worker.run_job(_Job(_Req(**base, denoise_strength=0.5)))[0][:4] == b"\x89PNG"


def test_bytes_do_not_depend_on_batch_lane_or_cache(worker):
    """One refinement request, eight ways; and what each way costs in UNet evaluations."""
    from sdlcm_amd.backends.hip_worker import encode_png
    eng = worker._engine
    steps = 2
    mk = lambda s, p=2: _Req(prompt=f"refine {s}", size="64x64", seed=s, num_inference_steps=steps, denoise_strength=0.6, pass_number=p)
    req = mk(0)
    key = worker._job_key(req)
    assert len(key) == 8

    def evals(fn):
        n0 = eng.stats["unet_evals"]
        r = fn()
        return r, eng.stats["unet_evals"] - n0

    def batch(reqs, lane=0):
        items = [worker._prepare(r, key) for r in reqs]
        return encode_png(eng.run_batch(key, items, lane)[0][0])
    cache = eng.refine_cache
    ident = (req.prompt, 0) + key[:6]
    pngs = {}
    cache.clear()
    pngs["alone"] = worker.run_job(_Job(req))[0]
    cache.clear()
    pngs["batch of 8"] = batch([req] + [mk(s) for s in range(1, 8)])
    cache.clear()
    pngs["padded batch of 3"] = batch([req, mk(1), mk(2), mk(2)])
    cache.clear()
    if eng.n_lanes > 1:
        pngs["lane 1"] = batch([req], lane=1)
    cache.clear()
    cap, cache.cap = cache.cap, 0
    try:
        pngs["cache off"], n = evals(lambda: batch([req]))
        assert n == 3 * steps and len(cache) == 0
        again, n = evals(lambda: batch([req]))
        assert n == 3 * steps and again == pngs["cache off"]
    finally:
        cache.cap = cap
    cache.clear()
    pngs["cold"], n = evals(lambda: worker.run_job(_Job(req))[0])
    assert n == 3 * steps, n
    assert all(ident + (0.6, k) in cache for k in (0, 1, 2))
    cache.clear()
    worker.run_job(_Job(mk(0, p=1)))
    pngs["warm"], n = evals(lambda: worker.run_job(_Job(req))[0])
    assert n == steps, n
    assert cache.evict(ident + (0.6, 1))
    pngs["after eviction of x^1"], n = evals(lambda: worker.run_job(_Job(req))[0])
    assert n == 2 * steps, n
    # a batch whose items start at different depths is split, and still gives every request its bytes
    cache.clear()
    worker.run_job(_Job(mk(0, p=1)))
    h0, m0 = eng.stats["refine_cache_hits"], eng.stats["refine_cache_misses"]
    items = [worker._prepare(r, key) for r in (req, mk(1))]
    mixed = eng.run_batch(key, items, 0)
    assert eng.stats["refine_cache_hits"] == h0 + 1 and eng.stats["refine_cache_misses"] == m0 + 1
    pngs["split by start depth"] = encode_png(mixed[0][0])
    assert encode_png(mixed[1][0]) == worker.run_job(_Job(mk(1)))[0]
    for tag, png in pngs.items():
        assert png == pngs["alone"], tag
    assert worker.run_job(_Job(mk(0, p=1)))[0] != pngs["alone"]


def _minipool():
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from tools import minipool
    return minipool


def _held_pool(worker, minipool):
    pool = minipool.MiniPool(lambda worker_id: worker, {"m": "synthetic"}, "m")
    worker.bind_queue(pool.q)
    gate, inside = threading.Event(), threading.Event()
    hold = pool.submit_job(minipool.CustomJob(handler=lambda: (inside.set(), gate.wait(30))))
    assert inside.wait(30)
    return pool, gate, hold


def _outcome(f):
    try:
        return f.result(600)
    except Exception as e:      # noqa
        return e


def test_one_invalid_request_in_a_drained_queue_fails_alone(worker):
    minipool = _minipool()
    mk = lambda s, d=0.5: _Req(prompt=f"iso {s}", size="64x64", seed=s, num_inference_steps=2, denoise_strength=d)
    solo = {s: worker.run_job(_Job(mk(s))) for s in range(8) if s != 3}
    pool, gate, hold = _held_pool(worker, minipool)
    try:
        n0 = len(worker._engine.batcher.batches)
        futs = [pool.submit_job(minipool.GenerationJob(req=mk(s, 7.0 if s == 3 else 0.5))) for s in range(8)]
        gate.set()
        hold.result(60)
        res = [_outcome(f) for f in futs]
        pool.q.join()
        for s in range(8):
            if s == 3:
                assert isinstance(res[s], RuntimeError) and "denoise_strength" in str(res[s])
            else:
                assert res[s] == solo[s], s
        assert sum(worker._engine.batcher.batches[n0:]) == 7 and len(worker._engine.batcher.batches[n0:]) < 7
    finally:
        worker.bind_queue(None)
        pool._worker = None
        pool.shutdown()


def test_mixed_plain_and_refinement_jobs_keep_their_solo_bytes(worker):
    minipool = _minipool()

    def mk(s):
        extra = [dict(), dict(denoise_strength=0.5), dict(denoise_strength=0.5, pass_number=2), dict(denoise_strength=1.0)][s % 4]
        return _Req(prompt=f"mixed {s // 4}", size="64x64", seed=s // 4, num_inference_steps=2, **extra)
    solo = {s: worker.run_job(_Job(mk(s))) for s in range(12)}
    assert solo[0] == solo[3] and solo[0] != solo[1] and solo[1] != solo[2]
    worker._engine.refine_cache.clear()
    pool, gate, hold = _held_pool(worker, minipool)
    try:
        futs = [pool.submit_job(minipool.GenerationJob(req=mk(s))) for s in range(12)]
        gate.set()
        hold.result(60)
        res = [_outcome(f) for f in futs]
        pool.q.join()
        assert res == [solo[s] for s in range(12)]
    finally:
        worker.bind_queue(None)
        pool._worker = None
        pool.shutdown()


@pytest.mark.parametrize("model,steps,guidance", [("synthetic-sd2", 4, 1.0), ("synthetic-sdxl", 2, 5.0)])
def test_other_families_refine(monkeypatch, model, steps, guidance):
    """SD 2.x (v-prediction) and SDXL (classifier-free guidance: both halves of the state handed over), 256x256 as their worker
    tests: a refinement runs, repeats byte for byte -- cold and from the cache -- and differs from the plain request."""
    monkeypatch.setenv("MODEL", model)
    monkeypatch.setenv("MODEL_ROOT", "/nonexistent")
    from sdlcm_amd.backends.worker_factory import create_hip_worker
    w = create_hip_worker(worker_id=1)
    try:
        eng = w._engine
        base = dict(prompt="a lighthouse at dusk", size="256x256", seed=7, num_inference_steps=steps, guidance_scale=guidance)
        plain, _ = w.run_job(_Job(_Req(**base)))
        a, _ = w.run_job(_Job(_Req(**base, denoise_strength=0.6, pass_number=2)))
        n0 = eng.stats["unet_evals"]
        b, _ = w.run_job(_Job(_Req(**base, denoise_strength=0.6, pass_number=2)))          # from the cached x^1
        assert eng.stats["unet_evals"] - n0 == steps
        eng.refine_cache.clear()
        c, _ = w.run_job(_Job(_Req(**base, denoise_strength=0.6, pass_number=2)))          # cold again
        assert a[:8] == b"\x89PNG\r\n\x1a\n" and a == b == c and a != plain
        assert np.abs(_dec(a) - _dec(plain)).mean() > 0.5
    finally:
        w.close()
