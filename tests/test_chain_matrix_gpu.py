"""Chain parity of every request kind under classifier-free guidance and v-prediction: LcmHipPipeline against
tests/chain_reference.py's ChainOracle in the cells of the (kind x guidance form x prediction type) matrix that no chain-level
test reached, and the worker's request kinds under classifier-free guidance.  tests/test_chain_matrix_cpu.py shows on the CPU
that the oracle equals the trusted chain oracles where they overlap and that every wiring mutant lies at least ten bounds away
at these very inputs.

Per cell (two requests that differ in seed, picture, mask, prompt and negative embeddings): every request against the oracle's
B = 1 run -- the pre-overlay image within 1e-2 on [0,1], the final latents within 5e-3 max(1, g) std(oracle latents); the
captured replay equals the eager run bit for bit; request 1 equals its solo run bit for bit; unet_evals as documented."""
import os
import types

import numpy as np
import pytest

import chain_reference as cr
import inpaint_reference as ir

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


# ---- the three pipelines ----------------------------------------------------------------------------------------------------------
def _build(form):
    from sdlcm_amd import weights
    from sdlcm_amd.pipeline import LcmHipPipeline
    from sdlcm_amd.scheduler import LCMSchedule
    usd, pipe_cfg, cfg, sch = cr.form_weights(form)
    vsd, esd = weights.synthetic_vae(), weights.synthetic_vae_encoder()
    hip = LcmHipPipeline(usd, vsd, unet_cfg=pipe_cfg, device=DEV, schedule=LCMSchedule(**sch) if sch else None)
    hip.set_vae_encoder_source(esd)
    return dict(hip=hip, ora=cr.ChainOracle(usd, vsd, cfg, enc_sd=esd, schedule=sch), form=form)


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


@pytest.fixture
def forms(request):
    return lambda f: request.getfixturevalue("form_" + f)


# ---- one cell ---------------------------------------------------------------------------------------------------------------------
def _run(hip, cell, inp, rows=(0, 1), **kw):
    """The cell's request pair (or the rows of it) on the pipeline."""
    kind = cell[0]
    rows = list(rows)
    W, H, g, steps = inp["width"], inp["height"], inp["guidance"], inp["steps"]
    pe, seeds = inp["pe"][rows], [inp["seeds"][b] for b in rows]
    if inp["ne"] is not None:
        kw["negative_embeds"] = inp["ne"][rows]
    if kind == "refine":
        return hip.generate(pe, seeds, W, H, steps, g, strength=cr.REFINE[0], passes=cr.REFINE[1], **kw)
    if kind == "hires":
        return hip.generate(pe, seeds, W, H, steps, g, hires=cr.oracle_kind(cell, inp, 0)[1:], **kw)
    if kind == "img2img":
        return hip.generate_img2img(pe, seeds, inp["pics"][rows], W, H, steps, cr.STRENGTH, g, **kw)
    if kind == "inpaint":
        return hip.generate_inpaint(pe, seeds, inp["pics"][rows], inp["masks"][rows], W, H, steps, cr.STRENGTH,
                                    mask_blur=cr.MASK_BLUR, guidance_scale=g, **kw)
    assert kind == "variation"
    return hip.generate(pe, seeds, W, H, steps, g, variation=[inp["variations"][b] for b in rows], **kw)


KEYS = {"refine": ("rgb", "latents", "pool8"), "hires": ("rgb", "latents", "pool8", "lowres_latents"),
        "img2img": ("rgb", "latents", "pool8", "init_latents"), "variation": ("rgb", "latents", "pool8"),
        "inpaint": ("rgb", "latents", "pool8", "init_latents", "alpha", "latent_mask")}


@pytest.mark.parametrize("cell", cr.CELLS, ids=cr.cell_id)
def test_cell(forms, cell):
    kind, form, _ = cell
    st = forms(form)
    hip, ora = st["hip"], st["ora"]
    ora.forget()
    inp = cr.cell_inputs(cell)
    g, cfg = inp["guidance"], ora.do_cfg(inp["guidance"])
    assert cfg == (form != "b") and hip.sched.prediction_type == cr.FORMS[form][1] == ora.pred
    eager = _run(hip, cell, inp, want_float=True)
    M = None
    if kind == "inpaint":
        # integer path: both sides select the same cells, and what is kept is the init picture's latents bit for bit
        M = ir.latent_mask(ir.blur(inp["masks"], cr.MASK_BLUR))
        assert np.array_equal(eager["latent_mask"], M) and all(0 < m.sum() < m.size for m in M)
        keep4 = np.broadcast_to((M == 0)[:, None], eager["latents"].shape)
        assert np.array_equal(eager["latents"][keep4].view(np.int32), eager["init_latents"][keep4].view(np.int32))
        assert (eager["latents"][~keep4] != eager["init_latents"][~keep4]).any()
    # ---- every request against the oracle's B = 1 run
    errs = []
    for b in range(2):
        ref = cr.oracle_run(ora, cell, inp, b, None if M is None else M[b])
        e_img = float(np.abs(cr.image01(eager["image"][b:b + 1].transpose(0, 3, 1, 2)) - cr.image01(ref["image"])).max())
        e_lat = float(np.abs(eager["latents"][b] - ref["latents"][0]).max())
        bound = cr.latent_bound(g, ref["latents"])
        print(f"[chain-matrix] {cr.cell_id(cell)} request {b}: image[0,1] max|d| = {e_img:.4g} (bound {cr.IMG_TOL:g}), latents max|d| = "
              f"{e_lat:.4g} (bound {bound:.4g} = {cr.LATENT_REL_TOL:g} x {max(1.0, g):g} x std {np.std(ref['latents']):.3g})")
        errs.append((b, e_img, e_lat, bound))
    # ---- the documented evaluation counts
    steps = inp["steps"]
    if kind == "refine":                  # counted in passes of the chain, whatever the guidance form (tests/test_refine_gpu.py)
        assert eager["unet_evals"] == steps * (cr.REFINE[1] + 1)
    elif kind == "hires":
        assert eager["unet_evals"] == (steps + cr.HIRES[0]) * (2 if cfg else 1)
    elif kind in ("img2img", "inpaint"):
        assert eager["unet_evals"] == steps * (2 if cfg else 1)
    else:                                 # a variation is a plain request: generate() reports no evaluation count for those
        assert kind == "variation" and "unet_evals" not in eager
    # ---- captured replay and the solo run, bit for bit
    cap = _run(hip, cell, inp)
    rep = _run(hip, cell, inp)
    solo = _run(hip, cell, inp, rows=(1,))
    for k in KEYS[kind]:
        assert np.array_equal(cap[k], eager[k]), f"captured {k} differs from the eager run"
        assert np.array_equal(rep[k], eager[k]), f"replayed {k} differs from the eager run"
        assert np.array_equal(solo[k][0], cap[k][1]), f"request 1's {k} depends on its batch"
    if kind == "hires":                   # stage 1 is the plain request, bit for bit
        kw = dict(negative_embeds=inp["ne"]) if inp["ne"] is not None else {}
        plain = hip.generate(inp["pe"], inp["seeds"], inp["width"], inp["height"], steps, g, **kw)
        assert np.array_equal(cap["lowres_latents"], plain["latents"])
    for b, e_img, e_lat, bound in errs:
        assert e_img < cr.IMG_TOL, f"request {b}: image off by {e_img:.4g}"
        assert e_lat < bound, f"request {b}: latents off by {e_lat:.4g}, bound {bound:.4g}"


# ---- the worker under classifier-free guidance ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def worker():
    old = {k: os.environ.get(k) for k in ("MODEL", "MODEL_ROOT")}
    os.environ["MODEL"], os.environ["MODEL_ROOT"] = "synthetic-sd2", "/nonexistent"
    from sdlcm_amd.backends.worker_factory import create_hip_worker
    try:
        w = create_hip_worker(worker_id=3)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    yield w
    w.close()


def _wmask(s):
    m = np.zeros((64, 64), np.uint8)
    m[12 + s:44 + s, 20:52] = 255
    return m


WORKER_KINDS = {
    "init_image": (lambda s: dict(init_image=cr.picture(64, 64, 40 + s), denoising_strength=0.5), "img2img_batch_cap"),
    "mask": (lambda s: dict(init_image=cr.picture(64, 64, 40 + s), denoising_strength=0.5, mask=_wmask(s)), "inpaint_batch_cap"),
    "enable_hr": (lambda s: dict(enable_hr=True, hr_scale=1.5, denoising_strength=0.7), "hires_batch_cap"),
    "refine": (lambda s: dict(denoise_strength=0.6, pass_number=2), None),
    "variation": (lambda s: dict(subseed=500 + s, subseed_strength=0.4), None),
}
NEGATIVES = ("fog and rain", "a crowd of people", "(smoke:1.3)")      # two plain texts and a weighted one
# (tag, the requests' negative prompts, does one encoded row serve the batch?)  _conditioning encodes the unconditional half once
# and expands it to the batch when every request carries the same unweighted text; otherwise per request.
BATCHES = (("three negative prompts", NEGATIVES, False),
           ("one shared negative prompt", (NEGATIVES[0],) * 3, True),
           ("no negative prompt at all", ("",) * 3, True),
           ("one shared weighted negative prompt", (NEGATIVES[2],) * 3, False),
           ("one negative prompt differs", (NEGATIVES[0], NEGATIVES[0], NEGATIVES[1]), False),
           ("no negative prompt but one", ("", NEGATIVES[1], ""), False))


def _req(kind, s, negative):
    d = dict(prompt=f"a lighthouse {s}", size="64x64", num_inference_steps=2, guidance_scale=2.0, seed=900 + s, style_lora=None,
             negative_prompt=negative)
    d.update(WORKER_KINDS[kind][0](s))
    return types.SimpleNamespace(**d)


@pytest.mark.parametrize("kind", list(WORKER_KINDS))
def test_worker_kind_under_classifier_free_guidance(worker, monkeypatch, kind):
    """Guidance 2.0 on the synthetic SD 2.x worker: the negative prompt reaches the picture of every request kind, and a request
    keeps its solo bytes in a batch whether the negative prompts all differ (encoded per request), are one unweighted text (one
    encoded row expanded to the batch -- that this branch of _conditioning ran is read off the count of encoded chunks: B + 1, not
    2 B), are one weighted text or differ in one request only.  The kinds with a batch cap run three requests: a padded tail of
    _run_capped and, under a cap of 2, two passes; a refinement batch of three is split by _run_refine into 2 + 1, cold and from
    the cached latents; the variation kind, whose pass takes the whole batch, runs four.  The batches go through
    _Engine.run_batch, the call every drained or coalesced batch ends in (as tests/test_inpaint_gpu.py's batch tests do)."""
    from sdlcm_amd.backends.hip_worker import encode_png
    eng = worker._engine
    assert not eng.pipe.unet.has_cond and eng.pipe.sched.prediction_type == "v_prediction"
    n_req = 4 if kind == "variation" else 3
    cap = WORKER_KINDS[kind][1]
    solos = {}

    def solo(s, neg):
        if (s, neg) not in solos:
            eng.refine_cache.clear()
            solos[s, neg] = worker.run_job(types.SimpleNamespace(req=_req(kind, s, neg)))[0]
        return solos[s, neg]

    def batch(negs, expanded, warm=False):
        reqs = [_req(kind, s, neg) for s, neg in enumerate(negs)]
        key = worker._job_key(reqs[0])
        assert all(worker._job_key(r) == key for r in reqs)
        if not warm:
            eng.refine_cache.clear()          # a refinement batch runs its whole chain, not only what the solo runs left over
        items = [worker._prepare(r, key) for r in reqs]
        n0 = eng.stats["prompt_chunks"]
        res = eng.run_batch(key, items)
        # the prompts' rows, and the unconditional half as one row or as one per request
        assert eng.stats["prompt_chunks"] - n0 == len(reqs) + (1 if expanded else len(reqs)), "the other branch of _conditioning ran"
        return [encode_png(r[0]) for r in res]

    assert solo(0, NEGATIVES[0]) != solo(0, ""), "the negative prompt did not reach the picture"
    assert solo(0, NEGATIVES[0]) != solo(0, NEGATIVES[1])
    for tag, negs, expanded in BATCHES:
        negs = tuple(negs[i % 3] for i in range(n_req))
        want = [solo(s, neg) for s, neg in enumerate(negs)]
        assert batch(negs, expanded) == want, f"{kind}, {tag}: a request's bytes depend on its batch"
        if kind == "refine":
            assert batch(negs, expanded, warm=True) == want, f"{kind}, {tag}: from the cached latents"
        if cap is not None:
            with monkeypatch.context() as mp:
                mp.setattr(eng.pipe, cap, lambda *a, **kw: 2)
                assert batch(negs, expanded) == want, f"{kind}, {tag}, passes of at most 2: a request's bytes depend on its batch"
