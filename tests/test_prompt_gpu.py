"""Weighted, long and negative prompts with clip_skip on the GPU: the emphasis kernel against float64, cross-attention over 154 / 231 /
308 context rows, CLIP with a stop layer, the chain against the CPU oracle, the worker's behaviour and invariants, and the launch audit
of the new launches inside a real pass.  All end-to-end cases: 64 x 64, 2 steps, synthetic weights."""
import os
import sys
import types

import numpy as np
import pytest
import torch

import attention_cases as ac
import launch_audit as la
import prompt_reference as pr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -7.0
WEIGHTS = [0.0, 1 / 1.1, 1.0, 1.1, 1.21, 1.5]


# ---------------------------------------------------------------------------------------------------------------------------
# lcm_prompt_emphasis_f16 against float64
# ---------------------------------------------------------------------------------------------------------------------------
def _emphasis_case(n, D, seed):
    g = np.random.default_rng(seed)
    z = torch.from_numpy(g.normal(0.3, 1.0, (n, 77, D))).half()
    w = g.choice(WEIGHTS, (n, 77)).astype(np.float32)
    w[:, 0] = 1.0
    return z, w


def _launch_emphasis(z, w, pad=16):
    """one launch into a sentinel-framed destination of leading dimension D + pad -> (the [n * 77, D] view, the frame intact?)"""
    from sdlcm_amd import ops
    n, _, D = z.shape
    rows, ldo = n * 77, D + pad
    buf = torch.full((rows + 2, ldo), SENTINEL, dtype=torch.float16, device=DEV)
    out = buf[1:rows + 1]
    zd, wd = z.reshape(rows, D).to(DEV), torch.from_numpy(w.reshape(-1)).to(DEV)
    zk, wk = zd.clone(), wd.clone()
    ops.prompt_emphasis(zd, wd, out, n, 77, D)
    torch.cuda.synchronize()
    intact = bool((buf[0] == SENTINEL).all() and (buf[-1] == SENTINEL).all() and (buf[1:rows + 1, D:] == SENTINEL).all())
    assert torch.equal(zd, zk) and torch.equal(wd, wk), "an operand was written"
    return out[:, :D].clone(), intact


@pytest.mark.parametrize("D", [768, 1024, 1280])
@pytest.mark.parametrize("n", [1, 3])
def test_emphasis_kernel_fp64(n, D):
    """Tolerance (prompt_reference.emphasis_bound): one fp16 rounding of the result, 2^-10 |ref| (2^-25 where the result is an fp16
    subnormal), plus the fp32 reduction bound of the order fixed in include/lcm_hip.h.  That order: a thread adds 8 ceil(77 D / 4096)
    elements (120 / 160 / 200 for D = 768 / 1024 / 1280), a wave combines 64 thread sums in 6 butterfly steps, 8 wave sums are added in
    order: a longest path of k = 134 / 174 / 214 additions.  A sum along a path of k fp32 additions is within k U sum|terms| (U = 2^-24),
    so each of S0 = sum z and S1 = sum z w is relatively off by k U A / |S| with A the sum of magnitudes; the inputs are offset so that
    |S| >= 0.1 A before and after weighting (asserted below on the fp64 side), hence <= 10 k U each.  r = S0 / S1 adds one rounding, the
    two products of the scaling two more: the result is relatively off by at most 1.01 ((20 k + 1) U + 2 U) <= 2.6e-4 before its fp16
    rounding (1.01 covers the second-order terms)."""
    z, w = _emphasis_case(n, D, 100 * n + D)
    z64 = z.double().numpy()
    cond = pr.conditioning(z64, w)
    assert cond >= 0.1, cond
    ref, bnd = pr.emphasis_fp64(z64, w), pr.emphasis_bound(z64, w)
    got, intact = _launch_emphasis(z, w)
    assert intact, "written outside the [n * 77, D] output: columns past D or the guard rows"
    err = np.abs(got.double().cpu().numpy().reshape(n, 77, D) - ref)
    print(f"\n[emphasis] n={n} D={D}: conditioning {cond:.3f}, worst |err| / bound = {(err / bnd).max():.3f}, max rel err = "
          f"{(err / np.maximum(np.abs(ref), 1e-3)).max():.3g}")
    assert (err <= bnd).all()
    assert np.abs(got.double().cpu().numpy().reshape(n, 77, D) - z64).max() > 0.05        # the weights did something


@pytest.mark.parametrize("D", [768, 1024, 1280])
def test_emphasis_bits_do_not_depend_on_the_launch(D):
    z, w = _emphasis_case(3, D, 7 + D)
    w[2] = 1.0                                             # chunk 2: all weights exactly 1.0
    three, ok3 = _launch_emphasis(z, w)
    solo, ok1 = _launch_emphasis(z[1:2], w[1:2], pad=8)
    assert ok3 and ok1
    assert torch.equal(three[77:154], solo), "chunk 1 of three differs from the same chunk launched alone"
    assert torch.equal(three[154:], z[2].to(DEV)), "a chunk with all weights 1.0 is not its input bit for bit"
    assert not torch.equal(three[:77], z[0].to(DEV))


def test_emphasis_refuses_other_shapes():
    from sdlcm_amd import ops
    from sdlcm_amd.lib import LcmHipError
    z = torch.zeros(2 * 77, 768, dtype=torch.float16, device=DEV)
    w = torch.ones(2 * 77, dtype=torch.float32, device=DEV)
    out = torch.zeros(2 * 77, 768, dtype=torch.float16, device=DEV)
    for kw, what in ((dict(S=76), "77 tokens"), (dict(S=154), "77 tokens"), (dict(D=512), "D = 512"), (dict(D=760), "D = 760"),
                     (dict(n=0), "n_chunks"), (dict(ldo=760), "ldo"), (dict(ldo=772), "ldo")):
        a = dict(n=2, S=77, D=768, ldo=768)
        a.update(kw)
        with pytest.raises(LcmHipError, match=r"rc=-1.*" + what):
            ops.prompt_emphasis(z, w, out, a["n"], a["S"], a["D"], ldo=a["ldo"])
    torch.cuda.synchronize()
    assert not out.any()


# ---------------------------------------------------------------------------------------------------------------------------
# cross-attention over the context of 2, 3 and 4 chunks
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [40, 64, 80, 160])          # 64: the heads of SD 2.x
@pytest.mark.parametrize("Sq", [64, 1024])
@pytest.mark.parametrize("Sk", [154, 231, 308])
def test_cross_attention_over_long_contexts(Sk, Sq, d):
    """The UNet's call: K and V are column windows of one wide [B * Sk, ld] buffer (ldk = ldv > heads * d), Q carries the scale;
    designed logits and the bound of tests/attention_cases.py / launch_audit.attention_check; image 1 of 2 bit-equal to it alone."""
    from sdlcm_amd import ops
    heads, B = 2, 2
    C = heads * d
    ld = 2 * C + 24
    for case in ac._shape_cases(f"x{d}-{Sq}x{Sk}", d, heads, Sq, Sk, False, kinds_of=("steps", "spikes")):
        q, k, v = case.operands()
        g = torch.Generator().manual_seed(13)
        q2 = torch.cat([torch.randn(Sq, C, generator=g).half(), q]).to(DEV)
        kv = torch.full((B * Sk, ld), 3.0, dtype=torch.float16)
        kv[:, 8:8 + C] = torch.cat([torch.randn(Sk, C, generator=g).half(), k])
        kv[:, 16 + C:16 + 2 * C] = torch.cat([torch.randn(Sk, C, generator=g).half(), v])
        kv = kv.to(DEV)
        k2, v2 = kv[:, 8:8 + C], kv[:, 16 + C:16 + 2 * C]
        kept = kv.clone()

        def launch(nb, qq, kk, vv):
            buf = torch.full((nb * Sq + 2, C + 16), SENTINEL, dtype=torch.float16, device=DEV)
            out = buf[1:nb * Sq + 1, 8:8 + C]
            ops.attention(qq, kk, vv, out, nb, heads, Sq, Sk, d, ldq=C, ldk=ld, ldv=ld, ldo=C + 16, scale=case.scale)
            torch.cuda.synchronize()
            frame = buf.clone()
            frame[1:nb * Sq + 1, 8:8 + C] = SENTINEL
            assert (frame == SENTINEL).all(), "written outside the logical output"
            return out.clone()
        out2 = launch(B, q2, k2, v2)
        assert torch.equal(kv, kept) and torch.isfinite(out2).all()
        r = la.attention_check(out2, q2, k2, v2, B, heads, Sq, Sk, d, scale=case.scale)
        print(f"\n[cross-attention] {case.form} | {case.name} | worst ratio {r:.4f}")
        assert r <= 1.0, (case.name, r)
        solo = launch(1, q2[Sq:], k2[Sk:], v2[Sk:])
        assert torch.equal(solo, out2[Sq:]), "an image alone differs from the same image second of two"


# ---------------------------------------------------------------------------------------------------------------------------
# CLIP with a stop layer
# ---------------------------------------------------------------------------------------------------------------------------
def test_clip_stop_layer():
    from sdlcm_amd.clip import CLIP_L, ClipTextHip, HashTokenizer, synthetic_clip
    cfg = dict(CLIP_L, num_hidden_layers=4)
    sd = synthetic_clip(cfg, seed=9)
    ids = HashTokenizer()(["a photo of an astronaut riding a horse", "", "x " * 100])
    enc = ClipTextHip(sd, cfg, device=DEV)
    today = enc.forward(ids)
    for skip in (1, 2):
        stop = cfg["num_hidden_layers"] - (skip - 1)
        ref = pr.clip_text_cpu(sd, cfg, ids, stop=stop).numpy()
        got = enc.forward(ids, stop=stop)
        e = np.abs(got.float().cpu().numpy() - ref).max()
        print(f"\n[clip] clip_skip={skip}: max|d| = {e:.3g}, max|ref| = {np.abs(ref).max():.3g}")
        assert e < 2e-2 * max(1.0, np.abs(ref).max())              # the project's bound for the text encoder
        if skip == 1:
            assert torch.equal(got, today)
        else:
            assert np.abs(got.float().cpu().numpy() - today.float().cpu().numpy()).max() > 1e-2
    s = torch.cuda.Stream(device=DEV)                              # on a stream of its own the call replays a graph per (B, S, stop)
    with torch.cuda.stream(s):
        a, b, c = enc.forward(ids), enc.forward(ids, stop=3), enc.forward(ids, stop=4)
        s.synchronize()
    assert torch.equal(a, today) and torch.equal(c, today) and torch.equal(b, enc.forward(ids, stop=3))
    assert set(enc._graphs) == {(3, 77, 4), (3, 77, 3)}
    with pytest.raises(ValueError, match="stop layer"):
        enc.forward(ids, stop=5)


# ---------------------------------------------------------------------------------------------------------------------------
# the worker
# ---------------------------------------------------------------------------------------------------------------------------
def _req(prompt, seed=11, **kw):
    d = dict(prompt=prompt, size="64x64", num_inference_steps=2, guidance_scale=1.0, seed=seed, style_lora=None)
    d.update(kw)
    return types.SimpleNamespace(**d)


def _job(*a, **kw):
    return types.SimpleNamespace(req=_req(*a, **kw))


def _words(n, tag="w"):
    return " ".join(f"{tag}{i}" for i in range(n))


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
def clip_ref():
    """(state dict, config) of the synthetic worker's text encoder, for the CPU side"""
    from sdlcm_amd.clip import CLIP_L, synthetic_clip
    return synthetic_clip(None), dict(CLIP_L)


@pytest.fixture(scope="module")
def offset_clip(worker):
    """(prompt encoder, state dict, config): the worker's prompt encoder over a text encoder whose final LayerNorm bias is raised by
    0.3.  The synthetic encoder's output has a chunk mean of ~1e-3 against mean|z| ~ 0.8 (its LayerNorm bias averages to zero), which
    leaves mean(z) / mean(z w) ill-conditioned: any two correct implementations disagree on it.  With the offset the ratio is
    well conditioned (asserted on the fp64 side where it is used), as for the inputs of the kernel test."""
    import copy
    from sdlcm_amd.clip import CLIP_L, ClipTextHip, synthetic_clip
    sd = dict(synthetic_clip(None))
    sd["final_layer_norm.bias"] = (sd["final_layer_norm.bias"].float() + 0.3).half()
    enc = copy.copy(worker._engine.encode)
    enc.enc = ClipTextHip(sd, None, device=DEV)
    return enc, sd, dict(CLIP_L)


def _well_conditioned(sd, cfg, ch, clip=None):
    z = np.concatenate([(clip or (lambda ids: pr.clip_text_cpu(sd, cfg, ids)))(torch.tensor([ids])).double().numpy() for ids in ch.ids])
    c = pr.conditioning(z, np.asarray(ch.weights))
    assert c >= 0.1, c
    return c


def test_tokens_past_the_75th_reach_the_picture(worker):
    eng = worker._engine
    head = _words(79)
    n0 = eng.stats["prompt_chunks"]
    a = worker.run_job(_job(head + " alpha tail"))[0]
    assert eng.stats["prompt_chunks"] == n0 + 2
    b = worker.run_job(_job(head + " beta tail"))[0]
    assert a != b, "two prompts that differ only in their 80th token gave the same picture"
    assert worker.run_job(_job(head + " alpha tail"))[0] == a
    assert worker._job_key(_req(head + " alpha tail"))[-2:] == ("ctx", 2)


def test_emphasis_reaches_the_picture_and_matches_the_reference(worker, clip_ref):
    eng = worker._engine
    n0 = eng.stats["weighted_prompts"]
    plain = worker.run_job(_job("a cat"))[0]
    assert worker.run_job(_job("a (cat:1.4)"))[0] != plain
    assert eng.stats["weighted_prompts"] == n0 + 1
    assert worker.run_job(_job("a (cat:1.0)"))[0] == plain                 # byte-equal: the brackets vanish in the parse
    assert worker.run_job(_job("a cat", negative_prompt="blurry, (ugly:1.3)"))[0] == plain        # guidance 1.0: never read
    assert worker.run_job(_job("a cat", clip_skip=1))[0] == plain
    assert worker.run_job(_job("a cat", clip_skip=2))[0] != plain
    assert worker.run_job(_job("a cat", override_settings={"CLIP_stop_at_last_layers": 2})) == worker.run_job(_job("a cat", clip_skip=2))
    # the embeddings: the reference's (CPU CLIP, fp64 emphasis), not those of the brackets as literal text
    sd, cfg = clip_ref
    ck = eng.encode.chunker
    got, n = eng.encode.encode_chunked([ck.chunk("a (cat:1.4)")])
    got = got.float().cpu().numpy()
    ref = pr.embed_prompt_cpu(sd, cfg, ck.chunk("a (cat:1.4)"))
    tol = 2e-2 * max(1.0, np.abs(ref).max())
    literal = eng.encode(["a (cat:1.4)"]).float().cpu().numpy()
    print(f"\n[worker] 'a (cat:1.4)': max|d| vs reference {np.abs(got - ref).max():.3g} (tol {tol:.3g}), literal tokenisation "
          f"{np.abs(literal - ref).max():.3g}")
    assert n == 1 and np.abs(got - ref).max() < tol < np.abs(literal - ref).max()
    assert np.abs(ref - pr.embed_prompt_cpu(sd, cfg, ck.chunk("a cat"))).max() > tol


def test_a_long_prompt_keeps_its_bytes_in_any_batch_on_any_lane(worker):
    from sdlcm_amd.backends.hip_worker import encode_png
    eng = worker._engine
    reqs = [_req(_words(90, f"k{s}") + " (bright:1.2)", seed=40 + s) for s in range(4)]
    key = worker._job_key(reqs[0])
    assert key == (64, 64, 2, 1.0, None, 0, "ctx", 2) and all(worker._job_key(r) == key for r in reqs)

    def batch(rs, lane=0, pick=0):
        return encode_png(eng.run_batch(key, [worker._prepare(r, key) for r in rs], lane)[pick][0])
    solo = worker.run_job(types.SimpleNamespace(req=reqs[0]))[0]
    pngs = {"batch of 2": batch(reqs[:2]), "third of 4": batch([reqs[1], reqs[2], reqs[0], reqs[3]], pick=2)}
    if eng.n_lanes > 1:
        pngs["lane 1"] = batch(reqs[:1], lane=1)
    worker.run_job(_job("a plain request"))
    pngs["after a plain request"] = worker.run_job(types.SimpleNamespace(req=reqs[0]))[0]
    for tag, png in pngs.items():
        assert png == solo, tag
    assert batch(reqs[:2], pick=1) != solo
    # drained queues of 2 and of 4 long prompts with a plain job among them: the long prompts are taken from the pool's queue
    # together, the plain one keeps its own key, and everyone gets the bytes of a solo run
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import threading
    from tools import minipool
    solo_all = [worker.run_job(types.SimpleNamespace(req=r)) for r in reqs]
    plain = worker.run_job(_job("a plain request"))
    pool = minipool.MiniPool(lambda worker_id: worker, {"m": "synthetic"}, "m")
    worker.bind_queue(pool.q)
    try:
        for n in (2, 4):
            gate, inside = threading.Event(), threading.Event()
            hold = pool.submit_job(minipool.CustomJob(handler=lambda: (inside.set(), gate.wait(30))))
            assert inside.wait(30)
            n0 = len(eng.batcher.batches)
            futs = [pool.submit_job(minipool.GenerationJob(req=r)) for r in reqs[:1] + [_req("a plain request")] + reqs[1:n]]
            gate.set()
            hold.result(60)
            assert [f.result(600) for f in futs] == solo_all[:1] + [plain] + solo_all[1:n], n
            pool.q.join()
            sizes = sorted(eng.batcher.batches[n0:])
            print(f"\n[worker] drained queue of {n} long prompts and a plain job: passes of {sizes}")
            assert sizes == [1, n], sizes
    finally:
        worker.bind_queue(None)
        pool._worker = None
        pool.shutdown()


KINDS = {"init_image": lambda: dict(init_image=_pic(3), denoising_strength=0.5),
         "mask": lambda: dict(init_image=_pic(3), denoising_strength=0.6, mask=np.pad(np.full((32, 32), 255, np.uint8), 16)),
         "enable_hr": lambda: dict(enable_hr=True, hr_scale=1.5, denoising_strength=0.7),
         "controlnet_image": lambda: dict(controlnet_image=_pic(5))}


@pytest.mark.parametrize("kind", list(KINDS))
def test_a_two_chunk_prompt_runs_with_every_request_kind(worker, kind):
    long, cut = _words(75) + " (sunset:1.3) over the sea", _words(75)
    assert worker._engine.encode.chunker.chunk(long).n == 2 and worker._engine.encode.chunker.chunk(cut).n == 1
    key = worker._job_key(_req(long, **KINDS[kind]()))
    assert key[-2:] == ("ctx", 2) and key[:-2] == worker._job_key(_req(cut, **KINDS[kind]()))
    a = worker.run_job(_job(long, **KINDS[kind]()))[0]
    b = worker.run_job(_job(cut, **KINDS[kind]()))[0]
    assert a[:8] == b"\x89PNG\r\n\x1a\n" and a != b, "the second chunk did not reach the picture"
    assert worker.run_job(_job(long, **KINDS[kind]()))[0] == a


def test_errors_are_the_jobs_own(worker):
    with pytest.raises(RuntimeError, match=r"301 tokens.*cap of 4"):
        worker.run_job(_job(_words(301)))
    L = worker._engine.encode.enc.L
    for bad in (0, L + 1):
        with pytest.raises(RuntimeError, match="clip_skip"):
            worker.run_job(_job("a cat", clip_skip=bad))
    assert worker.run_job(_job("a cat", clip_skip=L))[0][:4] == b"\x89PNG"


def test_negative_prompt_under_classifier_free_guidance(monkeypatch):
    """MODEL=synthetic-sd2: a UNet without a guidance embedding, so guidance 2.0 is classifier-free guidance and the negative prompt
    is the unconditional half."""
    monkeypatch.setenv("MODEL", "synthetic-sd2")
    monkeypatch.setenv("MODEL_ROOT", "/nonexistent")
    from sdlcm_amd.backends.worker_factory import create_hip_worker
    w = create_hip_worker(worker_id=2)
    try:
        eng = w._engine
        assert not eng.pipe.unet.has_cond
        base = w.run_job(_job("a lighthouse", guidance_scale=2.0))[0]
        assert w.run_job(_job("a lighthouse", guidance_scale=2.0, negative_prompt=""))[0] == base
        neg = w.run_job(_job("a lighthouse", guidance_scale=2.0, negative_prompt="fog, (rain:1.3)"))[0]
        assert neg != base, "the negative prompt did not reach the picture"
        assert w.run_job(_job("a lighthouse", guidance_scale=2.0, negative_prompt="fog, (rain:1.3)"))[0] == neg
        plain = w.run_job(_job("a lighthouse"))[0]
        assert w.run_job(_job("a lighthouse", negative_prompt="fog, (rain:1.3)"))[0] == plain          # guidance 1.0: never read
        # a negative prompt of two chunks: the prompt is filled with an empty-prompt chunk, the pass has 154 context rows
        r = _req("a lighthouse", guidance_scale=2.0, negative_prompt=_words(80))
        assert w._job_key(r) == (64, 64, 2, 2.0, None, 0, "ctx", 2)
        long_neg = w.run_job(types.SimpleNamespace(req=r))[0]
        assert long_neg not in (base, neg) and w.run_job(types.SimpleNamespace(req=r))[0] == long_neg
    finally:
        w.close()


# ---------------------------------------------------------------------------------------------------------------------------
# the chain against the CPU oracle, and the audit of the new launches inside a real pass
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,prompt", [(2, _words(70) + ", (a red fox:1.3) in the [snow] at dawn, ((mist))"),
                                      (3, _words(60) + " BREAK (b:1.5) " + _words(80, "v") + " [c]")], ids=["2 chunks", "3 chunks"])
def test_chain_against_the_cpu_oracle(worker, offset_clip, n, prompt):
    from oracle.clip import clip_text_oracle
    from oracle.pipeline import LCMPipelineOracle
    from sdlcm_amd import weights
    eng = worker._engine
    encode, sd, cfg = offset_clip
    ch = encode.chunker.chunk(prompt)
    assert ch.n == n and ch.weighted
    oracle_clip = lambda ids: clip_text_oracle(sd, cfg, ids)
    _well_conditioned(sd, cfg, ch, oracle_clip)
    pe_ref = pr.embed_prompt_cpu(sd, cfg, ch, clip=oracle_clip)                                          # [1, 77 n, 768] float64
    ref = LCMPipelineOracle(weights.synthetic_unet(), weights.synthetic_vae())(pe_ref.astype(np.float32), 64, 64, 2, 1.0, 42)
    pe, chunks = encode.encode_chunked([ch])
    torch.cuda.synchronize()                               # encoded on the default stream, used on the lane's
    assert chunks == n and tuple(pe.shape) == (1, 77 * n, 768)
    with eng.lane_locks[0]:
        out = eng.pipe.generate(pe, [42], 64, 64, 2, 1.0, want_float=True)
        rep = eng.pipe.generate(pe, [42], 64, 64, 2, 1.0)
    a = np.clip(out["image"].transpose(0, 3, 1, 2) / 2 + 0.5, 0, 1)
    err = float(np.abs(a - np.clip(ref["image"] / 2 + 0.5, 0, 1)).max())
    print(f"\n[chain] {n} chunks: embeddings max|d| = {np.abs(pe.float().cpu().numpy() - pe_ref).max():.3g}, image max|d| = {err:.3g}")
    assert err < 1e-2
    assert np.array_equal(out["rgb"], rep["rgb"]), "graph replay differs from eager"


def test_new_launches_audited_inside_a_real_pass(worker, offset_clip, monkeypatch):
    """tests/launch_audit.py's hook, extended by the emphasis entry point: the prompt is encoded and the pass runs eagerly under
    the audit.  The emphasis launch -- fed by the real text encoder, feeding the real pass -- is compared with float64 under its
    derived bound and must write nothing but its rows; the cross-attention launches over 154 context rows are checked like every
    attention launch of an audited pass."""
    eng = worker._engine
    monkeypatch.setitem(la.CHECKED, "prompt_emphasis", ("out",))

    class Audit(la.Audit):
        def _ref_prompt_emphasis(self, B, A, r):
            n, D = A["n_chunks"], A["D"]
            z = B["z"][:n * 77].double().cpu().numpy().reshape(n, 77, D)
            w = B["w"][:n * 77].double().cpu().numpy().reshape(n, 77)
            assert pr.conditioning(z, w) >= 0.1
            got = A["out"][:n * 77, :D].double().cpu().numpy().reshape(n, 77, D)
            # the bound of test_emphasis_kernel_fp64 with the conditioning these activations have (emphasis_bound reads it off z)
            return float((np.abs(got - pr.emphasis_fp64(z, w)) / pr.emphasis_bound(z, w)).max()), None

    encode, sd, cfg = offset_clip
    ch = encode.chunker.chunk(_words(72) + ", (a red fox:1.4) in the [snow], ((mist)) at dawn")
    assert ch.n == 2 and not ch.plain(0) and not ch.plain(1)
    plans = eng.pipe.lanes[0].plans
    before = set(plans)
    with eng.lane_locks[0], Audit() as au:
        pe, _ = encode.encode_chunked([ch])
        out = eng.pipe.generate(pe, [7], 64, 64, 2, 1.0, want_float=True)
    for k in set(plans) - before:
        plans.pop(k)
    bad = la.failures(au.checks)
    per = la.entry_table(au.checks)
    print(f"\n[audit] 2-chunk weighted prompt, 64x64: {len(au.checks)} launches checked, {la.summary_line(au.checks)}")
    assert not bad, bad
    assert per["prompt_emphasis"][0] == 1 and per["prompt_emphasis"][1] <= 1.0
    cross = [c for c in au.checks if c["op"] == "attention" and c["args"]["Sk"] == 154]
    assert cross and all(c["ratio"] <= 1.0 for c in cross), cross
    assert {c["args"]["Sq"] for c in cross} >= {64} and not [c for c in au.checks if c["op"] == "attention" and c["args"]["Sk"] == 77 and not c["args"]["causal"]]
    assert np.isfinite(out["latents"]).all()
