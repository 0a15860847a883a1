"""Prompt grammar, chunking, job keys and per-job errors of weighted / long / negative prompts (backends/prompt_syntax.py) -- CPU
tests; the fp64 emphasis and the CPU CLIP with a stop layer of tests/prompt_reference.py are checked against their definitions."""
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
import prompt_reference as pr  # noqa: E402
import tinytok  # noqa: E402
from sdlcm_amd.backends import prompt_syntax as ps  # noqa: E402
from sdlcm_amd.backends.hip_worker import HipLcmSDXLWorker, HipLcmWorker  # noqa: E402
from sdlcm_amd.clip import HashTokenizer  # noqa: E402
from tools import minipool  # noqa: E402

R, Q = 1.1, 1 / 1.1
B = ps.BREAK

GRAMMAR = [
    ("a cat", [("a cat", 1.0)]),
    ("", [("", 1.0)]),
    ("(x)", [("x", R)]),
    ("[x]", [("x", Q)]),
    ("(x:1.3)", [("x", 1.3)]),
    ("(x: 1.3 )", [("x", 1.3)]),
    ("(x:.5)", [("x", 0.5)]),
    ("(x:0)", [("x", 0.0)]),
    ("a (x:1.0) b", [("a x b", 1.0)]),                       # equal weights merge: the brackets vanish
    ("((x))", [("x", R * R)]),
    ("[[x]]", [("x", Q * Q)]),
    ("([x])", [("x", Q * R)]),
    ("(a (b:2) c:1.5)", [("a ", 1.5), ("b", 3.0), (" c", 1.5)]),
    ("a (b) [c] d", [("a ", 1.0), ("b", R), (" ", 1.0), ("c", Q), (" d", 1.0)]),
    (r"\(x\)", [("(x)", 1.0)]),
    (r"\[x\] \\", [("[x] \\", 1.0)]),
    (r"(a \) b)", [("a ) b", R)]),
    ("a (b c", [("a ", 1.0), ("b c", R)]),                   # unclosed: x 1.1 to the end
    ("a [b (c", [("a ", 1.0), ("b ", Q), ("c", Q * R)]),
    ("a) b] c", [("a) b] c", 1.0)]),                         # closers nothing opened are text
    ("a:1.3) b", [("a:1.3) b", 1.0)]),
    ("x: y", [("x: y", 1.0)]),
    ("a AND b", [("a AND b", 1.0)]),                         # not recognised: text
    ("<lora:foo:0.8>", [("<lora:foo:0.8>", 1.0)]),
    ("[a|b]", [("a|b", Q)]),
    ("[a:b:0.5]", [("a:b:0.5", Q)]),
    ("a BREAK b", [("a ", 1.0), B, (" b", 1.0)]),
    ("BREAK a", [B, (" a", 1.0)]),
    ("a BREAK", [("a ", 1.0), B]),
    ("a BREAK BREAK b", [("a ", 1.0), B, (" ", 1.0), B, (" b", 1.0)]),
    ("aBREAK BREAKb", [("aBREAK BREAKb", 1.0)]),             # only as a whitespace-delimited word
    ("(a BREAK b:1.2)", [("a ", 1.2), B, (" b", 1.2)]),
    ("(a)BREAK b", [("a", R), ("BREAK b", 1.0)]),           # a bracket or an escaped character next to it: not whitespace-delimited
    (r"a\(BREAK b", [("a(BREAK b", 1.0)]),
    ("a BREAK(b)", [("a BREAK", 1.0), ("b", R)]),
    ("BREAK", [B]),
    ("a\nBREAK\nb", [("a\n", 1.0), B, ("\nb", 1.0)]),
]


@pytest.mark.parametrize("text,want", GRAMMAR, ids=[repr(t) for t, _ in GRAMMAR])
def test_grammar(text, want):
    got = ps.parse(text)
    assert len(got) == len(want), got
    for g, w in zip(got, want):
        if w is B:
            assert g is B
        else:
            assert g is not B and g[0] == w[0] and g[1] == pytest.approx(w[1], rel=1e-12), (g, w)


# ---- chunking --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bpe(tmp_path_factory):
    from sdlcm_amd.prompt import _BpeTokenizer
    return _BpeTokenizer(tinytok.write(str(tmp_path_factory.mktemp("tok"))))


def _toks(kind, bpe):
    """(tokenizer, a word that is one token, a comma that is one token)"""
    return (bpe, "cat", ",") if kind == "bpe" else (HashTokenizer(), "cat", ",")


@pytest.mark.parametrize("kind", ["bpe", "hash"])
def test_chunk_boundaries_and_weights(kind, bpe, monkeypatch):
    tok, word, comma = _toks(kind, bpe)
    ck = ps.PromptChunker(tok)
    assert len(tok.encode_text(word)) == 1 and tok.encode_text(comma) == [tok.comma]
    wid = tok.encode_text(word)[0]
    c = ck.chunk(" ".join([word] * 75))
    assert c.n == 1 and c.n_tokens == 75 and c.ids[0] == [tok.bos] + [wid] * 75 + [tok.eos] and not c.weighted
    c = ck.chunk(" ".join([word] * 76))
    assert c.n == 2 and c.ids[0] == [tok.bos] + [wid] * 75 + [tok.eos]
    assert c.ids[1] == [tok.bos, wid, tok.eos] + [tok.pad] * 74
    assert ck.count(" ".join([word] * 76)) == 2 and ck.count("x") == 1
    e = ck.chunk("")
    assert e.n == 1 and (e.ids[0], e.weights[0]) == ck.empty_chunk() and e.ids[0][:2] == [tok.bos, tok.eos]
    # a comma with 20 tokens behind it in the full chunk: those 20 move on; with 21 behind it nothing moves
    for behind, moved in ((20, True), (21, False), (0, True)):
        words = [word] * (74 - behind) + [comma] + [word] * behind + ["dog"]
        c = ck.chunk(" ".join(words))
        dog = tok.encode_text("dog")
        assert c.n == 2 and c.n_tokens == 75 + len(dog)
        if moved:
            assert c.ids[0] == [tok.bos] + [wid] * (74 - behind) + [tok.comma, tok.eos] + [tok.pad] * behind
            assert c.ids[1][:1 + behind + len(dog)] == [tok.bos] + [wid] * behind + dog
        else:
            assert c.ids[0] == [tok.bos] + [wid] * (74 - behind) + [tok.comma] + [wid] * behind + [tok.eos]
            assert c.ids[1][:1 + len(dog)] == [tok.bos] + dog
    # a comma arriving at a full chunk just opens the next one
    c = ck.chunk(" ".join([word] * 75 + [comma, word]))
    assert c.n == 2 and c.ids[1][:3] == [tok.bos, tok.comma, wid]
    # weights: the run's weight on its tokens, 1.0 at BOS, EOS and padding; the moved tail keeps its weights
    c = ck.chunk(f"{word} ({word} {word}:1.5) [{word}]")
    assert c.weights[0] == [1.0, 1.0, 1.5, 1.5, Q, 1.0] + [1.0] * 71 and c.weighted and not c.plain(0)
    c = ck.chunk(" ".join([word] * 60 + [comma] + [f"({word}:1.3)"] * 14 + [word]))
    assert c.n == 2 and c.plain(0) and c.weights[1] == [1.0] + [1.3] * 14 + [1.0] * 62 and c.weights[1][0] == c.weights[1][16] == 1.0
    for ch in (ck.chunk(" ".join([word] * 100)), ck.chunk(f"({word}:0)")):
        for ids, w in zip(ch.ids, ch.weights):
            assert len(ids) == len(w) == 77 and w[0] == 1.0
            assert all(x == 1.0 for i, x in zip(ids, w) if i in (tok.bos, tok.eos, tok.pad) and i != wid)
    # BREAK: closes the chunk whatever it holds; no empty chunk at the end
    did = tok.encode_text("dog")[0]
    assert [x[:3] for x in ck.chunk(f"{word} BREAK dog").ids] == [[tok.bos, wid, tok.eos], [tok.bos, did, tok.eos]]
    assert ck.chunk(f"BREAK {word}").n == 2 and ck.chunk(f"BREAK {word}").ids[0] == ck.empty_chunk()[0]
    assert ck.chunk(f"{word} BREAK").n == 1
    assert ck.chunk(f"{word} BREAK BREAK {word}").n == 3 and ck.chunk(f"{word} BREAK BREAK {word}").ids[1] == ck.empty_chunk()[0]
    # the cap: an error that names the token count and the cap
    assert ck.chunk(" ".join([word] * 300)).n == 4
    with pytest.raises(RuntimeError, match=r"301 tokens.*cap of 4 chunks"):
        ck.chunk(" ".join([word] * 301))
    with pytest.raises(RuntimeError, match=r"301 tokens.*cap of 4 chunks"):          # the cached verdict raises again
        ck.count(" ".join([word] * 301))
    monkeypatch.setenv("LCM_MAX_PROMPT_CHUNKS", "2")
    with pytest.raises(RuntimeError, match=r"151 tokens.*cap of 2 chunks"):
        ps.PromptChunker(tok).chunk(" ".join([word] * 151))


@pytest.mark.parametrize("kind", ["bpe", "hash"])
def test_plain_prompts_get_the_ids_of_the_tokenizer_call(kind, bpe):
    tok, word, _ = _toks(kind, bpe)
    ck = ps.PromptChunker(tok)
    for text in ("", "a cat", "a cat, a dog. zebra!", "  A  Cat  ", " ".join([word] * 75), "a (cat:1.0) dog" if kind == "hash" else "cat dog"):
        want = tok([text.replace("(cat:1.0)", "cat")])[0].tolist()
        got = ck.chunk(text)
        assert got.n == 1 and got.ids[0] == want and not got.weighted, text
    if kind == "bpe":                                    # the directory's own pad id (SDXL's second tokenizer pads with id 0)
        import tempfile
        from sdlcm_amd.prompt import _BpeTokenizer
        t0 = _BpeTokenizer(tinytok.write(tempfile.mkdtemp(), pad="!"))
        assert t0.pad == 0 and ps.PromptChunker(t0).chunk("a cat").ids[0] == t0(["a cat"])[0].tolist()


# ---- job keys ----------------------------------------------------------------------------------------------------------------------
def _req(**kw):
    d = dict(prompt="a cat", size="512x512", num_inference_steps=4, guidance_scale=1.0, seed=1)
    d.update(kw)
    return types.SimpleNamespace(**d)


LONG = " ".join(["word"] * 100)


def test_job_keys():
    today = (512, 512, 4, 1.0, None, 0)
    assert HipLcmWorker._job_key(_req()) == today
    assert HipLcmWorker._job_key(_req(prompt="a (cat:1.4) [dog]")) == today
    assert HipLcmWorker._job_key(_req(negative_prompt="blurry, " + LONG)) == today          # guidance 1.0: never read
    assert HipLcmWorker._job_key(_req(clip_skip=2)) == today
    assert HipLcmWorker._job_key(_req(prompt=LONG)) == today + ("ctx", 2)
    assert HipLcmWorker._job_key(_req(prompt="a BREAK b BREAK c")) == today + ("ctx", 3)
    i2i = HipLcmWorker._job_key(_req(init_image=np.zeros((8, 8, 3), np.uint8), denoising_strength=0.5))
    assert HipLcmWorker._job_key(_req(prompt=LONG, init_image=np.zeros((8, 8, 3), np.uint8), denoising_strength=0.5)) == i2i + ("ctx", 2)
    assert ps.split_ctx(i2i + ("ctx", 2)) == (i2i, 2) and ps.split_ctx(i2i) == (i2i, 1) and ps.split_ctx(today) == (today, 1)
    assert HipLcmSDXLWorker._job_key(_req(prompt=LONG)) == today                              # out of scope: truncated as ever


class _Enc:
    """what a worker reads of its engine's prompt encoder"""

    def __init__(self, L=12, tok=None):
        self.chunker = ps.PromptChunker(tok or HashTokenizer())
        self.enc = types.SimpleNamespace(L=L)


def _fake_worker(has_cond, run_pass=lambda key, items: None, tok=None):
    from sdlcm_amd.backends import hip_worker
    from sdlcm_amd.backends.batching import MicroBatcher
    pipe = types.SimpleNamespace(sched=types.SimpleNamespace(init_noise_sigma=1.0), unet=types.SimpleNamespace(has_cond=has_cond))
    eng = types.SimpleNamespace(pipe=pipe, batch_sizes=(1, 2, 4, 8), passes=[], encode=_Enc(tok=tok))

    def run_batch(key, items, lane=0):
        eng.passes.append((key, [it[0].prompt for it in items]))
        run_pass(key, items)
        return [(np.full((8, 8, 3), it[1] % 251, np.uint8), np.zeros((1, 4, 8, 8), np.float16)) for it in items]

    eng.batcher = MicroBatcher(run_batch, max_batch=8, lanes=1)
    w = object.__new__(hip_worker.HipLcmWorker)
    w.worker_id, w._engine = 0, eng
    w._bind_prompt_ctx()
    return w


def test_a_workers_key_counts_the_negative_prompt_only_under_classifier_free_guidance():
    today = (512, 512, 4, 2.0, None, 0)
    lcm, cfg = _fake_worker(True), _fake_worker(False)
    try:
        r = _req(guidance_scale=2.0, negative_prompt=LONG)
        assert lcm._job_key(r) == today                   # a guidance embedding: no unconditional half, the text is not read
        assert cfg._job_key(r) == today + ("ctx", 2)
        assert cfg._job_key(_req(guidance_scale=2.0, negative_prompt="blurry")) == today
        assert cfg._job_key(_req(guidance_scale=1.0, negative_prompt=LONG)) == (512, 512, 4, 1.0, None, 0)
        assert cfg._job_key(_req(guidance_scale=2.0, prompt=" ".join(["w"] * 160), negative_prompt=LONG)) == today + ("ctx", 3)
        assert cfg._job_key(_req(override_settings={"CLIP_stop_at_last_layers": 2})) == (512, 512, 4, 1.0, None, 0)
        for bad in (0, 13, -1, "two", 1.5):
            with pytest.raises(RuntimeError, match="clip_skip"):
                cfg._job_key(_req(clip_skip=bad))
        with pytest.raises(RuntimeError, match="clip_skip"):
            cfg._job_key(_req(override_settings={"CLIP_stop_at_last_layers": 13}))
        assert ps.parse_clip_skip(_req(clip_skip=12), 12) == 12 and ps.parse_clip_skip(_req(), 12) == 1
    finally:
        lcm._engine.batcher.close()
        cfg._engine.batcher.close()


MULTIBYTE = [("\u732b" * 40, 2), ("\U0001f600" * 40, 3), ("\u00e9" * 70, 2), ("\u732b" * 20, 1), ("a cat \u00e9", 1)]


def test_the_count_is_the_chunkers_own_on_multibyte_text(bpe):
    """One character of a byte-level vocabulary can be several tokens (here: one per UTF-8 byte): a short text can be a long prompt.
    The key's count is chunk()'s count, on the first sight of a text as on every later one."""
    today = (512, 512, 4, 1.0, None, 0)
    for text, n in MULTIBYTE:
        fresh = ps.PromptChunker(bpe)
        first = fresh.count(text)
        assert first == fresh.chunk(text).n == fresh.count(text) == n, (text, first)
        assert fresh.chunk(text).n_tokens == len(bpe.encode_text(text))
        w = _fake_worker(True, tok=bpe)
        try:
            want = today if n == 1 else today + ("ctx", n)
            assert w._job_key(_req(prompt=text)) == want == w._job_key(_req(prompt=text)), text
        finally:
            w._engine.batcher.close()


def test_the_cache_is_shared_by_threads_and_bounded(monkeypatch):
    ck = ps.PromptChunker(HashTokenizer())
    monkeypatch.setattr(ps.PromptChunker, "CACHE", 8)
    errors = []

    def worker(t):
        try:
            for i in range(300):
                text = f"t{t} w{i % 23} " + "x " * (i % 90)
                assert ck.count(text) == (1 if i % 90 + 2 <= 75 else 2)
        except BaseException as e:      # noqa
            errors.append(e)
    th = [threading.Thread(target=worker, args=(t,)) for t in range(6)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert not errors, errors[:2]
    assert len(ck._cache) <= 8


def test_errors_reach_only_their_own_job():
    w = _fake_worker(True)
    pool = minipool.MiniPool(lambda worker_id: w, {"m": "synthetic"}, "m", queue_max=64)
    w.bind_queue(pool.q)
    bad = {1: (dict(prompt=" ".join(["w"] * 301)), "301 tokens"), 3: (dict(clip_skip=0), "clip_skip"), 5: (dict(clip_skip=13), "clip_skip")}
    try:
        gate, inside = threading.Event(), threading.Event()
        hold = pool.submit_job(minipool.CustomJob(handler=lambda: (inside.set(), gate.wait(10))))
        assert inside.wait(10)
        futs = [pool.submit_job(minipool.GenerationJob(req=_req(size="64x64", seed=100 + i, **bad.get(i, ({}, ""))[0]))) for i in range(8)]
        gate.set()
        hold.result(10)
        for i, f in enumerate(futs):
            if i in bad:
                with pytest.raises(RuntimeError, match=bad[i][1]):
                    f.result(10)
            else:
                assert f.result(10)[1] == 100 + i
        pool.q.join()
        assert sorted(len(p[1]) for p in w._engine.passes) == [1, 4]         # the five good jobs were drained together: plan sizes 4 + 1
    finally:
        pool._worker = None
        pool.shutdown()


# ---- the references against their definitions ---------------------------------------------------------------------------------------
def test_reference_emphasis_restores_the_chunk_mean():
    g = np.random.default_rng(0)
    z = g.normal(0.3, 1.0, (3, 77, 64))
    w = g.choice([0, 1 / 1.1, 1, 1.1, 1.21, 1.5], (3, 77))
    out = pr.emphasis_fp64(z, w)
    assert np.allclose(out.mean(axis=(1, 2)), z.mean(axis=(1, 2)), rtol=1e-12)
    assert np.array_equal(pr.emphasis_fp64(z, np.ones((3, 77))), z * 1.0)
    assert np.allclose(out[1] / out[1].mean(), (z[1] * w[1][:, None]) / (z[1] * w[1][:, None]).mean(), rtol=1e-12)
    assert pr.reduction_depth(768) == 8 * 15 + 14 and pr.reduction_depth(1280) == 8 * 25 + 14


def test_reference_clip_is_transformers_clip_and_stops_where_asked():
    from oracle.clip import clip_text_oracle
    from sdlcm_amd.clip import CLIP_L, synthetic_clip
    cfg = dict(CLIP_L, num_hidden_layers=3, hidden_size=64, intermediate_size=128, num_attention_heads=2, vocab_size=1000)
    sd = synthetic_clip(cfg)
    ids = torch.tensor([[998] + list(range(5, 80))[:75] + [999], [998, 7, 999] + [999] * 74])
    full = pr.clip_text_cpu(sd, cfg, ids)
    assert (full - clip_text_oracle(sd, cfg, ids)).abs().max() < 1e-4
    assert torch.equal(pr.clip_text_cpu(sd, cfg, ids, stop=3), full)
    # clip_skip 2: transformers' hidden_states[-2] through the final LayerNorm
    from transformers import CLIPTextConfig, CLIPTextModel
    m = CLIPTextModel(CLIPTextConfig(**cfg)).eval().float()
    strip = lambda k: k[len("text_model."):] if k.startswith("text_model.") else k
    m.load_state_dict({k: sd[strip(k)].float() for k in m.state_dict() if "position_ids" not in k}, strict=False)
    with torch.inference_mode():
        o = m(input_ids=ids, output_hidden_states=True)
        want = getattr(m, "text_model", m).final_layer_norm(o.hidden_states[-2])
    assert (pr.clip_text_cpu(sd, cfg, ids, stop=2) - want).abs().max() < 1e-4
