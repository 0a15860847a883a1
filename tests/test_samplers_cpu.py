"""sampler_name without a GPU: the standing of tests/sampler_reference.py on the Gaussian closed form, samplers.py against it,
parsing and batch keys, the C entry's argument checks, the fractional timesteps a pass hands to the time embeddings, and the
wiring mutants of the chain oracle in the cells tests/test_samplers_gpu.py compares on the GPU."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import chain_reference as cr  # noqa: E402
import sampler_reference as R  # noqa: E402
from sdlcm_amd import samplers as S  # noqa: E402
from sdlcm_amd.backends import sampler as sb  # noqa: E402
from sdlcm_amd.backends.hip_worker import HipLcmSDXLWorker, HipLcmWorker, samplers as sampler_list  # noqa: E402
from sdlcm_amd.scheduler import LCMSchedule, SD21_768_SCHEDULE  # noqa: E402

ABAR = R.alphas_cumprod()
COMBOS = [(R.EULER, "normal"), (R.EULER, "karras"), (R.EULER_A, "normal"), (R.EULER_A, "karras"), (R.DPMPP_2M, "normal"),
          (R.DPMPP_2M, "karras"), (R.DDIM, "normal")]


# ---- the oracle's own standing ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["normal", "karras"])
def test_reference_ddim_on_eulers_sigmas_is_euler(kind):
    for n in (5, 10, 20):
        sig = R.schedule(ABAR, kind, n)[0]
        a = R.gaussian_run(lambda s: R.sigma_steps(R.EULER, s), sig, state=True)
        b = R.gaussian_run(R.ddim_on_sigmas, sig, state=True)
        assert np.abs(a - b).max() < 1e-12


@pytest.mark.parametrize("kind", ["normal", "karras"])
def test_reference_euler_is_first_order(kind):
    errs = [R.gaussian_run(lambda s: R.sigma_steps(R.EULER, s), R.schedule(ABAR, kind, n)[0]) for n in (5, 10, 20, 40)]
    ratios = [errs[i] / errs[i + 1] for i in range(3)]
    print(f"[samplers] Euler on {kind} sigmas, end error at n = 5, 10, 20, 40: {errs}, ratios {ratios}")
    assert all(1.7 <= r <= 2.3 for r in ratios), ratios


def test_reference_dpmpp_2m_gains_more_than_first_order():
    errs = [R.gaussian_run(lambda s: R.sigma_steps(R.DPMPP_2M, s), R.schedule(ABAR, "karras", n)[0]) for n in (20, 40)]
    print(f"[samplers] DPM++ 2M on Karras sigmas, end error at n = 20, 40: {errs}")
    assert errs[0] / errs[1] > 3.0


@pytest.mark.parametrize("kind", ["normal", "karras"])
def test_reference_euler_a_splits_the_variance(kind):
    for n in (2, 3, 7, 50):
        sig = R.schedule(ABAR, kind, n)[0]
        for (sa, _, cx, c0, _, cn), s, s2 in zip(R.sigma_steps(R.EULER_A, sig), sig[:-1], sig[1:]):
            up = cn / R.S(s2)
            dn = cx * sa * s / R.S(s2)
            assert abs(dn * dn + up * up - s2 * s2) <= 1e-12 * max(1.0, s2 * s2)
            assert abs(c0 - R.S(s2) * (1 - dn / s)) < 1e-12
        assert R.sigma_steps(R.EULER_A, sig)[-1][2:] == (0.0, 1.0, 0.0, 0.0)          # the last step is x' = x0, no noise


# ---- samplers.py against the reference --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sched_kw", [{}, SD21_768_SCHEDULE], ids=["sd15", "sd21-768"])
def test_tables_agree_with_the_reference(sched_kw):
    sc = LCMSchedule(**sched_kw)
    abar = R.alphas_cumprod(**sched_kw)
    final = 1.0 if sched_kw.get("set_alpha_to_one", True) else float(abar[0])
    assert np.array_equal(abar, np.asarray(sc.alphas_cumprod, dtype=np.float64)) and final == sc.final_alpha_cumprod
    for name, kind in COMBOS:
        for n in (1, 2, 3, 7, 50):
            T, Q = S.tables(sc, name, kind, n), R.tables(abar, final, name, kind, n)
            assert len(T.coefs) == len(Q["rows"]) == n
            assert np.abs(np.array(T.coefs) - np.array(Q["rows"])).max() < 1e-12
            assert np.abs(T.ts - Q["ts"]).max() < 1e-12 * 1000
            assert (T.init_scale is None) == (Q["init_scale"] is None) == (name == R.DDIM)
            if name != R.DDIM:
                assert abs(T.init_scale - Q["init_scale"]) < 1e-12
                assert np.abs(T.sigmas - Q["sigmas"]).max() < 1e-12 * T.sigmas[0]
            for strength in (0.05, 0.3, 0.5, 0.75, 0.999, 1.0):
                try:
                    Q = R.img2img_tables(abar, final, name, kind, n, strength)
                except ValueError:
                    with pytest.raises(ValueError, match="number of pipeline steps is 0"):
                        S.img2img_tables(sc, name, kind, n, strength)
                    assert name == R.DDIM
                    continue
                T = S.img2img_tables(sc, name, kind, n, strength)
                assert len(T.coefs) == len(Q["rows"]) == len(T.ts)
                if name != R.DDIM:
                    assert len(T.ts) == int(min(strength, 0.999) * n) + 1
                else:
                    assert len(T.ts) == min(int(n * strength), n)
                assert np.abs(np.array(T.coefs) - np.array(Q["rows"])).max() < 1e-12
                assert np.abs(T.ts - Q["ts"]).max() < 1e-9 and np.abs(np.array(T.start) - np.array(Q["start"])).max() < 1e-12


def test_sigma_round_trip_and_schedule_ends():
    sc = LCMSchedule()
    t = np.concatenate([np.array([0.0, 0.25, 716.5, 998.75, 999.0]), np.random.default_rng(0).uniform(0, 999, 200)])
    assert np.abs(S.sigma_to_t(sc, S.t_to_sigma(sc, t)) - t).max() < 1e-9
    assert all(abs(R.sigma_to_t(ABAR, R.t_to_sigma(ABAR, float(v))) - v) < 1e-9 for v in t)
    tab = S.sigma_table(sc)
    assert S.sigma_to_t(sc, tab[0] / 2) == 0.0 and S.sigma_to_t(sc, tab[-1] * 2) == 999.0       # the weight is clipped
    for kind in ("normal", "karras"):
        sig, ts = S.schedule_sigmas(sc, kind, 1)
        assert abs(sig[0] - tab[-1]) < 1e-12 * tab[-1] and sig[1] == 0.0 and abs(ts[0] - 999.0) < 1e-9
        sig, ts = S.schedule_sigmas(sc, kind, 7)
        assert abs(sig[0] - tab[-1]) < 1e-12 * tab[-1] and abs(sig[-2] - tab[0]) < 1e-12 and sig[-1] == 0.0
        assert np.all(np.diff(sig) < 0) and np.all(np.diff(ts) < 0)
    assert np.any(S.schedule_sigmas(sc, "karras", 7)[1] % 1 != 0)                               # fractional timesteps
    with pytest.raises(ValueError):
        S.tables(sc, R.DDIM, "karras", 4)
    for n in (0, 51):
        with pytest.raises(ValueError, match="outside 1..50"):
            S.tables(sc, R.EULER, "normal", n)


# ---- parsing and keys -------------------------------------------------------------------------------------------------------------
def _req(**kw):
    d = dict(prompt="a cat", size="512x512", num_inference_steps=4, guidance_scale=1.0, seed=7, style_lora=None)
    d.update(kw)
    return types.SimpleNamespace(**d)


PIC = np.zeros((8, 8, 3), np.uint8)
KINDS = {"plain": {}, "refine": dict(denoise_strength=0.6, pass_number=2), "hires": dict(enable_hr=True, hr_scale=1.5, denoising_strength=0.7),
         "control": dict(controlnet_image=np.zeros((512, 512, 3), np.uint8)),
         "canny": dict(controlnet_image=np.zeros((512, 512, 3), np.uint8), controlnet_module="canny"),
         "img2img": dict(init_image=PIC, denoising_strength=0.5),
         "inpaint": dict(init_image=PIC, denoising_strength=0.5, mask=np.zeros((8, 8), np.uint8)),
         "long": dict(prompt="a cat " * 60)}


@pytest.mark.parametrize("kind", list(KINDS))
def test_the_lcm_names_give_todays_key(kind):
    today = HipLcmWorker._job_key(_req(**KINDS[kind]))
    for fields in (dict(sampler_name=None), dict(sampler_name=""), dict(sampler_name="LCM"), dict(sampler_name="lcm"), dict(sampler_name=" Lcm "),
                   dict(sampler_name=None, scheduler="Karras"), dict(scheduler="Automatic")):
        assert HipLcmWorker._job_key(_req(**KINDS[kind], **fields)) == today
        assert sb.parse_sampler(_req(**fields)) is None
    if kind in ("plain", "long"):
        assert HipLcmSDXLWorker._job_key(_req(sampler_name="LCM")) == HipLcmSDXLWorker._job_key(_req())


NAMES = [("Euler", None, (R.EULER, "normal")), ("euler", "Automatic", (R.EULER, "normal")), ("EULER", "karras", (R.EULER, "karras")),
         ("Euler a", None, (R.EULER_A, "normal")), ("euler A", "Karras", (R.EULER_A, "karras")), ("Euler  a", "normal", (R.EULER_A, "normal")),
         ("DDIM", None, (R.DDIM, "normal")), ("ddim", "Normal", (R.DDIM, "normal")), ("DPM++ 2M", None, (R.DPMPP_2M, "normal")),
         ("dpm++ 2m", "KARRAS", (R.DPMPP_2M, "karras")), ("DPM++ 2M Karras", None, (R.DPMPP_2M, "karras")),
         ("dpm++ 2m karras", "Automatic", (R.DPMPP_2M, "karras")), ("DPM++ 2M Karras", "Karras", (R.DPMPP_2M, "karras"))]


@pytest.mark.parametrize("name,scheduler,want", NAMES, ids=[f"{n}-{s}" for n, s, _ in NAMES])
def test_served_names_and_their_keys(name, scheduler, want):
    fields = dict(sampler_name=name) if scheduler is None else dict(sampler_name=name, scheduler=scheduler)
    assert sb.parse_sampler(_req(**fields)) == want
    tail = ("sampler",) + want
    for kind in ("plain", "control", "canny", "img2img"):
        today = HipLcmWorker._job_key(_req(**KINDS[kind]))
        key = HipLcmWorker._job_key(_req(**KINDS[kind], **fields))
        assert key == today + tail and sb.split_key(key) == (today, want)
    # a long prompt: the sampler's ending, then ("ctx", n)
    today = HipLcmWorker._job_key(_req(**KINDS["long"]))
    key = HipLcmWorker._job_key(_req(**KINDS["long"], **fields))
    assert today[-2] == "ctx" and key == today[:-2] + tail + today[-2:]
    # the per-image fields stay out of the key
    assert HipLcmWorker._job_key(_req(subseed=5, subseed_strength=0.25, negative_prompt="fog", clip_skip=2, **fields)) == \
        HipLcmWorker._job_key(_req(**fields))


def test_split_key_leaves_every_other_key_alone():
    for kind, fields in KINDS.items():
        key = HipLcmWorker._kind_key(_req(**fields))
        assert sb.split_key(key) == (key, None), kind
    assert sb.split_key((512, 512, 4, 1.0, "sampler", 3)) == ((512, 512, 4, 1.0, "sampler", 3), None)    # a style of that name


ERRORS = [(dict(sampler_name="Heun"), r"sampler_name 'Heun' is not served \(served: LCM, Euler, Euler a, DDIM, DPM\+\+ 2M, DPM\+\+ 2M Karras"),
          (dict(sampler_name="DPM++ SDE"), r"sampler_name 'DPM\+\+ SDE' is not served"), (dict(sampler_name="UniPC"), r"is not served"),
          (dict(sampler_name=3), r"sampler_name 3 is not a string \(served: LCM, Euler"),
          (dict(sampler_name=["Euler"]), r"is not a string"),
          (dict(sampler_name="DDIM", scheduler="Karras"), r"scheduler 'Karras' is not served with sampler_name 'DDIM' \(served"),
          (dict(sampler_name="Euler", scheduler="Exponential"), r"scheduler 'Exponential' is not served \(served"),
          (dict(sampler_name="Euler", scheduler=7), r"scheduler 7 is not a string"),
          (dict(sampler_name="Euler", num_inference_steps=0), r"num_inference_steps=0 outside 1\.\.50 with sampler_name 'Euler'"),
          (dict(sampler_name="Euler a", num_inference_steps=51), r"num_inference_steps=51 outside 1\.\.50"),
          (dict(sampler_name="Euler", **KINDS["inpaint"]), r"sampler_name is not combined with mask"),
          (dict(sampler_name="Euler", **KINDS["hires"]), r"sampler_name is not combined with enable_hr"),
          (dict(sampler_name="Euler", **KINDS["refine"]), r"sampler_name is not combined with refinement"),
          (dict(sampler_name="Euler", denoise_strength=0.5), r"sampler_name is not combined with refinement")]


@pytest.mark.parametrize("fields,msg", ERRORS, ids=[str(i) for i in range(len(ERRORS))])
def test_errors_and_their_messages(fields, msg):
    with pytest.raises(RuntimeError, match=msg):
        HipLcmWorker._job_key(_req(**fields))


def test_the_sdxl_worker_refuses_a_sampler():
    with pytest.raises(RuntimeError, match=r"sampler_name: samplers are not served by the SDXL worker"):
        HipLcmSDXLWorker._job_key(_req(sampler_name="Euler a"))
    with pytest.raises(RuntimeError, match=r"sampler_name 'Heun' is not served"):
        HipLcmSDXLWorker._job_key(_req(sampler_name="Heun"))


def test_lcm_samplers_switch(monkeypatch):
    names = [s["name"] for s in sampler_list()]
    assert names == ["LCM", "Euler", "Euler a", "DDIM", "DPM++ 2M", "DPM++ 2M Karras"]
    assert all(set(s) == {"name", "aliases", "options"} for s in sampler_list())
    assert sampler_list()[0] == {"name": "LCM", "aliases": ["lcm"], "options": {}}
    monkeypatch.setenv("LCM_SAMPLERS", "lcm")

    class Untouchable:                                 # the fields are not read at all
        prompt, size, num_inference_steps, guidance_scale, seed, style_lora = "a cat", "512x512", 4, 1.0, 7, None

        def __getattr__(self, name):
            if name in ("sampler_name", "scheduler"):
                raise AssertionError(f"{name} was read")
            raise AttributeError(name)
    assert sb.parse_sampler(Untouchable()) is None
    assert HipLcmWorker._job_key(Untouchable()) == HipLcmWorker._job_key(_req())
    assert HipLcmWorker._job_key(_req(sampler_name="Heun")) == HipLcmWorker._job_key(_req())
    assert HipLcmSDXLWorker._job_key(_req(sampler_name="Euler")) == HipLcmSDXLWorker._job_key(_req())
    assert [s["name"] for s in sampler_list()] == ["LCM"]
    monkeypatch.setenv("LCM_SAMPLERS", "request")
    assert sb.parse_sampler(_req(sampler_name="ddim")) == (R.DDIM, "normal")
    monkeypatch.setenv("LCM_SAMPLERS", "all")
    monkeypatch.setenv("MODEL", "synthetic")
    with pytest.raises(RuntimeError, match=r"Unknown LCM_SAMPLERS=all, expected one of request, lcm"):
        HipLcmWorker(0)


def test_prepare_draws_what_the_lcm_request_draws():
    """A request with a sampler draws exactly the tensors it draws without one, on the caller's thread; the LCM bound on
    steps x strength does not apply to an image-to-image request with a sampler, DDIM with no timestep left is that job's error."""
    from sdlcm_amd.backends import hip_worker
    from sdlcm_amd.backends import prompt_syntax as ps
    from sdlcm_amd.clip import HashTokenizer
    pipe = types.SimpleNamespace(sched=LCMSchedule(), unet=types.SimpleNamespace(has_cond=False))
    enc = types.SimpleNamespace(chunker=ps.PromptChunker(HashTokenizer()), enc=types.SimpleNamespace(L=12))
    eng = types.SimpleNamespace(pipe=pipe, batch_sizes=(1, 2, 4, 8), encode=enc, ensure_vae_encoder=lambda: None, batcher=None)
    w = object.__new__(hip_worker.HipLcmWorker)
    w.worker_id, w._engine = 0, eng
    w._bind_prompt_ctx()
    try:
        for fields in (dict(), dict(subseed=21, subseed_strength=0.25)):
            plain = w._prepare(_req(size="64x64", **fields), w._job_key(_req(size="64x64", **fields)))
            for name in ("Euler", "Euler a", "DDIM", "DPM++ 2M Karras"):
                r = _req(size="64x64", sampler_name=name, **fields)
                it = w._prepare(r, w._job_key(r))
                assert len(it) == len(plain) == 3 and it[1] == plain[1] == 7
                assert torch.equal(it[2][0], plain[2][0]) and len(it[2][1]) == len(plain[2][1]) == 3
                assert all(torch.equal(a, b) for a, b in zip(it[2][1], plain[2][1]))
        i2i = dict(size="64x64", init_image=np.zeros((64, 64, 3), np.uint8), num_inference_steps=30)
        with pytest.raises(Exception, match="smaller than num_inference_steps"):          # the LCM sampler's own bound
            w._prepare(_req(denoising_strength=0.5, **i2i), w._job_key(_req(denoising_strength=0.5, **i2i)))
        r = _req(denoising_strength=0.5, sampler_name="Euler", **i2i)
        it = w._prepare(r, w._job_key(r))
        lcm = w._prepare(_req(denoising_strength=0.9, **i2i), w._job_key(_req(denoising_strength=0.9, **i2i)))
        assert torch.equal(it[2][0], lcm[2][0]) and len(it[2][1]) == len(lcm[2][1]) == 30
        r = _req(denoising_strength=0.05, sampler_name="DDIM", **dict(i2i, num_inference_steps=10))      # int(10 x 0.05) = 0
        with pytest.raises(RuntimeError, match="number of pipeline steps is 0"):
            w._prepare(r, w._job_key(r))
    finally:
        w._engine = None


# ---- the C entry's argument checks ------------------------------------------------------------------------------------------------
def test_sampler_step_argument_errors_without_a_gpu():
    from sdlcm_amd import lib
    assert "lcm_sampler_step" in lib.EXPORTS
    L = lib.load()
    buf = C.create_string_buffer(4096 + 64)
    base = (C.addressof(buf) + 63) // 64 * 64
    p = lambda off=0: C.c_void_p(base + off)

    def call(eps=p(), eps_u=None, lat=p(1024), x0p=p(2048), noise=None, cn=0.0, pred=0, B=1, h=2, w=2, sa=0.5):
        rc = L.lcm_sampler_step(eps, eps_u, 1.0, lat, x0p, noise, sa, 0.5, 1.0, 1.0, 0.0, cn, pred, B, h, w, 0, None)
        return rc, L.lcm_last_error()
    for kw in (dict(eps=None), dict(lat=None), dict(x0p=None)):
        rc, msg = call(**kw)
        assert rc == -1 and b"sampler_step: null pointer" in msg, (kw, msg)
    for kw in (dict(eps=p(4)), dict(eps_u=p(8))):
        rc, msg = call(**kw)
        assert rc == -1 and b"16-byte aligned" in msg, (kw, msg)
    for kw in (dict(lat=p(1026)), dict(x0p=p(2049)), dict(noise=p(3073), cn=0.5)):
        rc, msg = call(**kw)
        assert rc == -1 and b"4-byte aligned" in msg, (kw, msg)
    rc, msg = call(cn=0.25)
    assert rc == -1 and b"cn = 0.25 needs a noise tensor" in msg
    for pred in (-1, 3):
        rc, msg = call(pred=pred)
        assert rc == -1 and b"unknown prediction type" in msg
    for kw in (dict(B=0), dict(h=0), dict(w=-1), dict(B=1 << 14, h=1 << 8, w=1 << 8)):
        rc, msg = call(**kw)
        assert rc == -1 and b"bad shape" in msg
    rc, msg = call(sa=0.0)
    assert rc == -1 and b"sa = 0" in msg


# ---- fractional timesteps reach the time embeddings ---------------------------------------------------------------------------------
class _Net:
    MAX_HOISTED_STEPS = 64
    has_cond = has_added = False

    def __init__(self):
        self.embedded, self.forwarded = [], []

    def encode_context(self, ehs, UB):
        return "kv"

    def time_embed_all(self, ts, wemb, UB, aug=None):
        self.embedded.append(list(ts))
        return torch.zeros(len(ts) * UB, 1)

    def embed_hint(self, *a):
        pass

    def forward(self, lat, t, *a, **kw):
        self.forwarded.append(t)
        assert kw["ta"] is not None
        return [], None


@pytest.mark.parametrize("control", [False, True])
def test_a_karras_plan_hands_fractional_timesteps_to_the_time_embeddings(monkeypatch, control):
    from sdlcm_amd import ops, pipeline
    sc = LCMSchedule()
    T = S.tables(sc, R.DPMPP_2M, "karras", 5)
    want = [float(t) for t in T.ts]
    assert sum(abs(t - round(t)) > 1e-3 for t in want) >= 3 and any(abs(t - int(t)) > 0.4 for t in want)
    assert np.abs(np.array(want) - [R.sigma_to_t(ABAR, s) for s in R.schedule(ABAR, "karras", 5)[0][:-1]]).max() < 1e-9
    unet, cn, steps, scaled = _Net(), _Net(), [], []
    monkeypatch.setattr(ops, "sampler_step", lambda eps, lat, x0p, noise, *c, **kw: steps.append((c[:6], noise, kw)))
    monkeypatch.setattr(ops, "latents_renoise", lambda x0, n, a, b, lat, *r, **kw: scaled.append((x0, n, a, b, kw)))
    B, h, w = 1, 2, 2
    z = lambda *s: torch.zeros(*s)
    P = types.SimpleNamespace(sampler=T, B=B, UB=B, h=h, w=w, do_cfg=False, kind=None, FROM_STATE=("from-state", "inpaint"), xk=None,
                              lane=types.SimpleNamespace(unet=unet), control=0.8 if control else None, lat0=z(B, 4, h, w), lat=z(B, 4, h, w),
                              eps=z(B, h, w, 4), ehs=z(77, 8), wemb=None, noise=z(4, B, 4, h, w), x0_prev=z(B, 4, h, w), hint=z(B, 16, 16, 3),
                              hint_emb=z(B * h * w, 4))
    me = types.SimpleNamespace(sched=sc, lane_controlnet=lambda L: cn, device="cpu")
    me._control_setup = lambda P, taps=None: pipeline.LcmHipPipeline._control_setup(me, P, taps)
    pipeline.LcmHipPipeline._sampler_pass(me, P, 1.0)
    assert unet.embedded == [want] and unet.forwarded == want
    assert (cn.embedded == [want] and cn.forwarded == want) if control else (cn.embedded == [] and cn.forwarded == [])
    assert len(steps) == 5 and all(n is None for _, n, _ in steps)
    assert [tuple(np.float64(v) for v in c) for c, _, _ in steps] == [tuple(np.float64(v) for v in row) for row in T.coefs]
    # the initial scale is one launch on the device, from lat0 (i.e. behind a variation's blend into it)
    assert len(scaled) == 1 and scaled[0][0] is P.lat0 and scaled[0][2] == T.init_scale == float(S.sb(T.sigmas[0])) and scaled[0][3] == 0.0
    # Euler a reads the step noises in draw order, none on the last step
    steps.clear()
    P.sampler = S.tables(sc, R.EULER_A, "normal", 5)
    pipeline.LcmHipPipeline._sampler_pass(me, P, 1.0)
    assert [None if n is None else n.data_ptr() for _, n, _ in steps] == [P.noise[i].data_ptr() for i in range(4)] + [None]


# ---- the wiring mutants, on the oracle alone ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracles():
    made = {}

    def get(form):
        f = "b" if form == "c" else form
        if f not in made:
            made[f] = R.build_oracle(f, with_controlnet=f == "a")
        return made[f]
    return get


def test_every_mutant_is_assigned_to_a_cell():
    assigned = [m for c in R.CELLS for m in c[8]]
    assert sorted(assigned) == sorted(R.MUTANTS)


@pytest.mark.parametrize("cell", [c for c in R.CELLS if c[8]], ids=[c[0] for c in R.CELLS if c[8]])
def test_mutants_leave_the_chain_bound(oracles, cell):
    """Every mutant assigned to the cell moves the final latents of the cell's request by more than the bound the GPU test holds
    the pipeline to (chain_reference.latent_bound)."""
    ora = oracles(cell[1])
    ora.forget()
    inp = R.cell_inputs(cell)
    b = cell[7]
    ref = R.oracle_run(ora, cell, inp, b, decode=False)
    bound = cr.latent_bound(inp["guidance"], ref["latents"])
    moved = {}
    for m in cell[8]:
        out = R.oracle_run(ora, cell, inp, b, mutate=m, decode=False)
        moved[m] = float(np.abs(out["latents"] - ref["latents"]).max())
        print(f"[samplers] {cell[0]}: {m} moves the final latents by {moved[m]:.4g} = {moved[m] / bound:.3g} bounds ({bound:.4g})")
    ora.forget()
    assert all(v > bound for v in moved.values()), (moved, bound)
