"""sampler_name on the MI355X: the lcm_sampler_step kernel against fp64 within a bound counted from its stated operation order,
its independence of the batch, fractional timesteps in the time embedding, the sampler pass of LcmHipPipeline against
tests/sampler_reference.py's chain oracle in the cells whose wiring mutants tests/test_samplers_cpu.py tells apart, and the
worker's requests.  Tolerances of the chain cells are chain_reference.IMG_TOL and latent_bound, unchanged."""
import os
import types

import numpy as np
import pytest
import torch

import chain_reference as cr
import sampler_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -24            # one rounding to fp32 (round to nearest): relative to the magnitude of the rounded result


# ---- the kernel -------------------------------------------------------------------------------------------------------------------
def _f32(*vals):
    return tuple(float(np.float32(v)) for v in vals)


def _fp64_step(m, mu, g, x, x0p, noise, row, pred):
    """The step in float64 on the kernel's own fp32 operands -> (x', x0, bound of x', bound of x0).  The bounds count one rounding
    of 2^-24 of the result's magnitude per operation of the order include/lcm_hip.h states, carried through what follows:
      guidance  d = m - mu (1), mg = fma(g, d, mu) (1)                    E_m  = U (|g| |d| + |mg|)
      epsilon   n = fma(-sb, mg, x) (1), x0 = n / sa (1)                  E_x0 = (sb E_m + U |n|) / sa + U |x0|   (the 1 / sa amplification)
      v         p = sa x (1), x0 = fma(-sb, mg, p) (1)                    E_x0 = sb E_m + U |p| + U |x0|
      sample    x0 = mg                                                   E_x0 = E_m
      q = c0 x0 (1), r = fma(cx, x, q) (1), [fma(c1, x0_prev, r) (1)], [fma(cn, noise, r) (1)]
    and 0.1 % on top for the products of two roundings."""
    sa, sb, cx, c0, c1, cn = row
    E_m = 0.0
    if mu is not None:
        d = m - mu
        mg = g * d + mu
        E_m = U * (abs(g) * np.abs(d) + np.abs(mg))
    else:
        mg = m
    if pred == "epsilon":
        n = x - sb * mg
        x0 = n / sa
        E_x0 = (sb * E_m + U * np.abs(n)) / sa + U * np.abs(x0)
    elif pred == "v_prediction":
        p = sa * x
        x0 = p - sb * mg
        E_x0 = sb * E_m + U * np.abs(p) + U * np.abs(x0)
    else:
        x0, E_x0 = mg, E_m + 0.0 * x
    q = c0 * x0
    E = abs(c0) * E_x0 + U * np.abs(q)
    r = cx * x + q
    E = E + U * np.abs(r)
    if c1 != 0.0:
        r = r + c1 * x0p
        E = E + U * np.abs(r)
    if cn != 0.0:
        r = r + cn * noise
        E = E + U * np.abs(r)
    return r, x0, 1.001 * E, 1.001 * E_x0


ROWS = {  # (sa, sb, cx, c0, c1, cn) as float32 values: a first DPM++ 2M step, a later one, an Euler a step, a last step
    "first": _f32(0.068264848, 0.99766723, 0.78848246, 0.56358234, 0.0, 0.0),
    "history": _f32(0.61740797, 0.78664312, 0.03706272, 1.73268458, -0.75599250, 0.0),
    "ancestral": _f32(0.068264848, 0.99766723, 0.06873991, 0.61271545, 0.0, 0.78364803),
    "both": _f32(0.52630841, 0.85029375, 0.67128142, 0.46779753, -0.31, 0.42),
    "last": _f32(0.99957490, 0.029155134, 0.0, 1.0, 0.0, 0.0),
}


def _operands(B, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)
    return dict(m=r(B, h, w, 4) * 1.3, mu=r(B, h, w, 4) * 1.1 + 0.2, x=r(B, 4, h, w) * 2.0, x0p=r(B, 4, h, w) * 0.9, noise=r(B, 4, h, w))


def _launch(op, row, pred, guided, dup, B, h, w):
    """One launch on fresh device copies -> (lat [B or 2B,4,h,w], x0_prev) on the host."""
    from sdlcm_amd import ops
    dev = lambda t: t.to(DEV).contiguous()
    lat = dev(torch.cat([torch.full_like(op["x"], 7.0), op["x"]]) if dup else op["x"].clone())
    state = lat[B:] if dup else lat
    x0p, m, mu, noise = dev(op["x0p"].clone()), dev(op["m"]), dev(op["mu"]), dev(op["noise"])
    ops.sampler_step(m, state, x0p, noise if row[5] != 0.0 else None, *row, B, h, w, pred=pred, dup=dup,
                     **(dict(eps_uncond=mu, guidance=2.5) if guided else {}))
    torch.cuda.synchronize()
    return lat.cpu(), x0p.cpu()


@pytest.mark.parametrize("pred", ["epsilon", "v_prediction", "sample"])
@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (8, 8), (33, 17)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("B", [1, 3])
def test_kernel_against_fp64(B, shape, pred):
    h, w = shape
    op = _operands(B, h, w, 100 * B + h)
    nhwc = lambda t: t.double().permute(0, 3, 1, 2).numpy()          # the model output as NCHW float64
    m64, mu64 = nhwc(op["m"]), nhwc(op["mu"])
    x64, x0p64, n64 = (op[k].double().numpy() for k in ("x", "x0p", "noise"))
    worst = 0.0
    for name, row in ROWS.items():
        for guided in (False, True):
            for dup in (False, True):
                lat, x0p = _launch(op, row, pred, guided, dup, B, h, w)
                want, want_x0, E, E0 = _fp64_step(m64, mu64 if guided else None, 2.5, x64, x0p64, n64, row, pred)
                got = lat[B:] if dup else lat
                err, err0 = np.abs(got.double().numpy() - want), np.abs(x0p.double().numpy() - want_x0)
                worst = max(worst, float((err / np.maximum(E, 1e-300)).max()))
                assert (err <= E).all(), f"{name} guided={guided} dup={dup}: x' off by {float((err / E).max()):.3g} bounds"
                assert (err0 <= E0).all(), f"{name} guided={guided}: x0_prev off"
                if pred == "sample" and not guided:
                    assert np.array_equal(x0p.numpy(), op["m"].permute(0, 3, 1, 2).numpy())      # x0 = m, bit for bit
                if dup:                                              # both classifier-free halves carry the new state
                    assert np.array_equal(lat[:B].numpy().view(np.int32), lat[B:].numpy().view(np.int32))
    print(f"[samplers] kernel B={B} {h}x{w} {pred}: worst |error| / bound = {worst:.3g}")


@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
def test_a_row_keeps_its_bits_at_every_batch_position(pred):
    h, w = 33, 17
    one = _operands(1, h, w, 5)
    others = _operands(3, h, w, 6)
    for row in (ROWS["history"], ROWS["both"]):
        for guided in (False, True):
            solo_lat, solo_x0 = _launch(one, row, pred, guided, guided, 1, h, w)
            for pos in range(3):
                op = {k: v.clone() for k, v in others.items()}
                for k in op:
                    op[k][pos] = one[k][0]
                lat, x0 = _launch(op, row, pred, guided, guided, 3, h, w)
                state = lat[3:] if guided else lat
                assert np.array_equal(state[pos].numpy().view(np.int32), solo_lat[-1].numpy().view(np.int32)), (pos, guided)
                assert np.array_equal(x0[pos].numpy().view(np.int32), solo_x0[0].numpy().view(np.int32)), (pos, guided)


def test_time_embedding_takes_fractional_timesteps():
    from sdlcm_amd import ops
    ts, B, dim = [716.5, 0.25, 998.75], 2, 320
    out = torch.zeros(len(ts) * B, dim, dtype=torch.float16, device=DEV)
    ops.timestep_embedding_steps(ts, out, B, dim)
    torch.cuda.synchronize()
    got = out.float().cpu().numpy().reshape(len(ts), B, dim).astype(np.float64)
    half = dim // 2
    f = np.exp(-np.log(10000.0) * np.arange(half, dtype=np.float64) / half)
    for i, t in enumerate(ts):
        want = np.concatenate([np.cos(t * f), np.sin(t * f)])
        err = np.abs(got[i] - want[None]).max()
        trunc = np.abs(np.concatenate([np.cos(int(t) * f), np.sin(int(t) * f)]) - want)
        print(f"[samplers] time embedding at t = {t}: max|d| = {err:.3g} (bound 2^-10); truncation would move column 0 by {trunc[0]:.3g}")
        assert err <= 2.0 ** -10, (t, err)
    one = torch.zeros(B, dim, dtype=torch.float16, device=DEV)
    ops.timestep_embedding(716.5, one, B, dim)
    torch.cuda.synchronize()
    assert torch.equal(one.cpu(), out[:B].cpu())


# ---- the chain cells --------------------------------------------------------------------------------------------------------------
def _build(form):
    from sdlcm_amd import weights
    from sdlcm_amd.pipeline import LcmHipPipeline
    from sdlcm_amd.scheduler import LCMSchedule
    usd, pipe_cfg, cfg, sch = cr.form_weights(form)
    vsd, esd = weights.synthetic_vae(), weights.synthetic_vae_encoder()
    hip = LcmHipPipeline(usd, vsd, unet_cfg=pipe_cfg, device=DEV, schedule=LCMSchedule(**sch) if sch else None)
    hip.set_vae_encoder_source(esd)
    cn_sd = None
    if form == "a":
        cn_sd = weights.synthetic_controlnet()
        hip.set_controlnet(cn_sd)
    ora = R.SamplerChainOracle(usd, vsd, cfg, enc_sd=esd, cn_sd=cn_sd, schedule=sch)
    return dict(hip=hip, ora=ora)


@pytest.fixture(scope="module")
def form_a():
    s = _build("a")
    yield s
    s["hip"].close()


@pytest.fixture(scope="module")
def form_b():
    s = _build("b")
    yield s
    s["hip"].close()


@pytest.fixture(scope="module")
def form_c(form_b):
    s = _build("c")
    s["ora"] = form_b["ora"]          # the same weights and schedule: one oracle serves both
    yield s
    s["hip"].close()


def _run(hip, cell, inp, rows=(0, 1), sampler=True, **kw):
    cid, form, name, kind_s, steps, kind, size = cell[:7]
    rows = list(rows)
    W, H, g = inp["width"], inp["height"], inp["guidance"]
    pe, seeds = inp["pe"][rows], [inp["seeds"][b] for b in rows]
    if sampler:
        kw["sampler"] = (name, kind_s)
    if inp["ne"] is not None:
        kw["negative_embeds"] = inp["ne"][rows]
    if kind == "img2img":
        return hip.generate_img2img(pe, seeds, inp["pics"][rows], W, H, steps, R.STRENGTH[cid], g, **kw)
    if kind == "control":
        kw["control"] = (inp["hints"][rows], R.CONTROL_SCALE)
    if kind == "variation":
        kw["variation"] = [inp["variations"][b] for b in rows]
    return hip.generate(pe, seeds, W, H, steps, g, **kw)


@pytest.mark.parametrize("cell", R.CELLS, ids=[c[0] for c in R.CELLS])
def test_cell(request, cell):
    """The pair of requests of a cell on the pipeline: the cell's request against the oracle's B = 1 run (image within IMG_TOL on
    [0,1], final latents within latent_bound); the captured replay equals the eager run and request 1 its solo run, bit for bit;
    the sampler changed the result."""
    cid, form, name, kind_s, steps, kind, size = cell[:7]
    st = request.getfixturevalue("form_" + form)
    hip, ora = st["hip"], st["ora"]
    ora.forget()
    inp = R.cell_inputs(cell)
    g = inp["guidance"]
    assert hip.sched.prediction_type == cr.FORMS[form][1] == ora.pred and ora.do_cfg(g) == (form != "b")
    eager = _run(hip, cell, inp, want_float=True)
    b = cell[7]
    ref = R.oracle_run(ora, cell, inp, b)
    ora.forget()
    e_img = float(np.abs(cr.image01(eager["image"][b:b + 1].transpose(0, 3, 1, 2)) - cr.image01(ref["image"])).max())
    e_lat = float(np.abs(eager["latents"][b] - ref["latents"][0]).max())
    bound = cr.latent_bound(g, ref["latents"])
    print(f"[samplers] {cid} request {b}: image[0,1] max|d| = {e_img:.4g} (bound {cr.IMG_TOL:g}), latents max|d| = {e_lat:.4g} "
          f"(bound {bound:.4g} = {cr.LATENT_REL_TOL:g} x {max(1.0, g):g} x std {np.std(ref['latents']):.3g})")
    cap = _run(hip, cell, inp)
    solo = _run(hip, cell, inp, rows=(1,))
    for k in ("rgb", "latents", "pool8"):
        assert np.array_equal(cap[k], eager[k]), f"captured {k} differs from the eager run"
        assert np.array_equal(solo[k][0], cap[k][1]), f"request 1's {k} depends on its batch"
    if kind == "img2img":
        n_eval = len(ref["ts"])
        assert eager["unet_evals"] == n_eval * (2 if form != "b" else 1)
        assert n_eval == (min(int(steps * R.STRENGTH[cid]), steps) if name == R.DDIM else int(min(R.STRENGTH[cid], 0.999) * steps) + 1)
    elif steps <= 3 or kind != "plain":      # the LCM pass of the same request is another picture
        lcm = _run(hip, cell, inp, sampler=False)
        assert not np.array_equal(lcm["rgb"], cap["rgb"])
    assert e_img < cr.IMG_TOL, f"image off by {e_img:.4g}"
    assert e_lat < bound, f"latents off by {e_lat:.4g}, bound {bound:.4g}"


def test_pipeline_refuses_what_is_not_served(form_b):
    from sdlcm_amd.lib import LcmHipError
    hip = form_b["hip"]
    inp = cr.cell_inputs(("img2img", "b", 0))
    pe = inp["pe"][:1]
    with pytest.raises(LcmHipError, match="not combined with hires fix or refinement"):
        hip.generate(pe, [1], 64, 64, 2, 1.0, sampler=("Euler", "normal"), strength=0.5, passes=1)
    with pytest.raises(LcmHipError, match="outside 1..50"):
        hip.generate(pe, [1], 64, 64, 51, 1.0, sampler=("Euler", "normal"))
    with pytest.raises(LcmHipError, match="unknown sampler"):
        hip.generate(pe, [1], 64, 64, 2, 1.0, sampler=("Heun", "normal"))
    with pytest.raises(LcmHipError, match="number of pipeline steps is 0"):
        hip.generate_img2img(pe, [1], inp["pics"][:1], 64, 64, 3, 0.2, 1.0, sampler=("DDIM", "normal"))


# ---- through the worker -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def worker():
    old = {k: os.environ.get(k) for k in ("MODEL", "MODEL_ROOT")}
    os.environ["MODEL"], os.environ["MODEL_ROOT"] = "synthetic-sd2", "/nonexistent"
    from sdlcm_amd.backends.worker_factory import create_hip_worker
    try:
        w = create_hip_worker(worker_id=5)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    yield w
    w.close()


def _req(s, **kw):
    d = dict(prompt=f"a lighthouse {s}", size="64x64", num_inference_steps=3, guidance_scale=2.0, seed=900 + s, style_lora=None,
             negative_prompt="fog and rain")
    d.update(kw)
    return types.SimpleNamespace(**d)


def _job(req):
    return types.SimpleNamespace(req=req)


def test_worker_lcm_names_are_todays_request(worker):
    eng = worker._engine
    n0 = eng.stats["sampler_requests"]
    plans0 = {k for L in eng.pipe.lanes for k in L.plans}
    a = worker.run_job(_job(_req(0)))
    plans = {k for L in eng.pipe.lanes for k in L.plans}
    assert worker.run_job(_job(_req(0, sampler_name=None))) == a
    assert worker.run_job(_job(_req(0, sampler_name="LCM"))) == a
    assert worker.run_job(_job(_req(0, sampler_name="lcm", scheduler="Automatic"))) == a
    assert {k for L in eng.pipe.lanes for k in L.plans} == plans and not any("sampler" in k for k in plans - plans0)
    assert eng.stats["sampler_requests"] == n0
    e = worker.run_job(_job(_req(0, sampler_name="Euler a")))
    assert e[1] == a[1] and e[0] != a[0] and e[0][:8] == b"\x89PNG\r\n\x1a\n"
    assert eng.stats["sampler_requests"] == n0 + 1
    assert any(k[-3:] == ("sampler", "Euler a", "normal") for L in eng.pipe.lanes for k in L.plans)
    assert worker.run_job(_job(_req(0))) == a                           # ... and the LCM request after it


@pytest.mark.parametrize("fields", [dict(sampler_name="Euler a"), dict(sampler_name="Euler a", scheduler="Karras", init_image="pic",
                                                                         denoising_strength=0.6)], ids=["plain", "img2img"])
def test_worker_euler_a_solo_and_in_a_batch_of_3(worker, fields):
    from sdlcm_amd.backends.hip_worker import encode_png
    eng = worker._engine
    mk = lambda s: _req(s, **{k: (cr.picture(64, 64, 40 + s) if v == "pic" else v) for k, v in fields.items()})
    solo = [worker.run_job(_job(mk(s)))[0] for s in range(3)]
    assert len(set(solo)) == 3
    reqs = [mk(s) for s in range(3)]
    key = worker._job_key(reqs[0])
    assert all(worker._job_key(r) == key for r in reqs) and "sampler" in key
    n0 = eng.stats["sampler_requests"]
    res = eng.run_batch(key, [worker._prepare(r, key) for r in reqs])
    assert [encode_png(r[0]) for r in res] == solo
    assert eng.stats["sampler_requests"] == n0 + 3


@pytest.mark.parametrize("name", ["Euler", "DDIM", "DPM++ 2M Karras"])
def test_worker_deterministic_samplers_ignore_the_step_noise(worker, name):
    from sdlcm_amd.backends.hip_worker import encode_png
    eng = worker._engine
    r = _req(1, sampler_name=name)
    key = worker._job_key(r)
    want = worker.run_job(_job(r))[0]
    it = worker._prepare(r, key)
    lat, extra = it[2]
    assert len(extra) == 2
    other = [torch.randn(e.shape, generator=torch.Generator().manual_seed(77 + i)) for i, e in enumerate(extra)]
    assert encode_png(eng.run_batch(key, [(it[0], it[1], (lat, other))])[0][0]) == want
    # ... while Euler a reads them
    ra = _req(1, sampler_name="Euler a")
    ka = worker._job_key(ra)
    ia = worker._prepare(ra, ka)
    assert encode_png(eng.run_batch(ka, [(ia[0], ia[1], (ia[2][0], other))])[0][0]) != worker.run_job(_job(ra))[0]


def test_worker_errors_belong_to_their_job_inside_a_drained_batch(worker):
    from test_refine_gpu import _held_pool, _minipool, _outcome
    minipool = _minipool()
    mk = lambda s, **kw: _req(s, **dict(dict(sampler_name="DPM++ 2M"), **kw))
    solo = {s: worker.run_job(_job(mk(s))) for s in range(4)}
    bad = [mk(10, sampler_name="Heun"), mk(11, scheduler="Karras", sampler_name="DDIM"), mk(12, enable_hr=True, hr_scale=1.5),
           mk(13, num_inference_steps=60), mk(14, denoise_strength=0.5)]
    words = ["'Heun' is not served", "is not served with sampler_name 'DDIM'", "sampler_name is not combined with enable_hr",
             "outside 1..50", "sampler_name is not combined with refinement"]
    pool, gate, hold = _held_pool(worker, minipool)
    try:
        n0 = len(worker._engine.batcher.batches)
        futs, bads = [], []
        for s in range(4):
            futs.append(pool.submit_job(minipool.GenerationJob(req=mk(s))))
            bads.append(pool.submit_job(minipool.GenerationJob(req=bad[s])))
        bads.append(pool.submit_job(minipool.GenerationJob(req=bad[4])))
        gate.set()
        hold.result(60)
        assert [_outcome(f) for f in futs] == [solo[s] for s in range(4)]
        for f, word in zip(bads, words):
            e = _outcome(f)
            assert isinstance(e, RuntimeError) and word in str(e), (word, e)
        pool.q.join()
        assert len(worker._engine.batcher.batches[n0:]) < 4                # the good ones were coalesced
    finally:
        worker.bind_queue(None)
        pool._worker = None
        pool.shutdown()
