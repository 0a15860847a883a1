"""The style-LoRA path on the GPU, per weight and per picture (tests/lora_reference.py states the comparison; tests/test_lora_cpu.py
shows on the CPU that it tells every packing mistake from the truth):

1. ``lcm_ln_fold_refresh`` and ``lcm_axpy_f16`` against fp64 at the sizes a merge launches them with;
2. the per-tensor comparison on the device: the full-width synthetic SD1.5 UNet with a LoRA on one module of every target kind
   at every level it occurs, and the synthetic SD 2.x UNet with transformer targets at every level, each against the same class
   built from the merged checkpoint; weight 0 restores every tensor bit for bit;
3. a graph captured BEFORE the merge replays the merged weights: replay == eager bit for bit, both within the chain oracle's
   bounds of the oracle on the merged checkpoint, at a size whose odd skip sizes read the upsamplers' plain ``.w3`` copy (form (a))
   and on SD 2.x under v-prediction (form (c)); the LoRA moves the oracle's picture by SEPARATION x IMG_TOL at least;
4. ``ClipLora`` on the synthetic CLIP-H tower and on a projected second encoder (index 1) against transformers' CLIP on merged weights;
5. the worker switching between two styles with overlapping targets, directly and on two lanes: every PNG is the one a worker
   gives that has served nothing else."""
import os
import threading
import types

import numpy as np
import pytest
import torch

import chain_reference as cr
import launch_audit as la
import lora_reference as lr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
WT = 0.75


def _rnd(*shape, seed, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(torch.float16)


# ---- 1. the two kernels -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", [(6, 8), (5, 520), (3, 512), (960, 320), (10240, 1280)])
def test_ln_fold_refresh_fp64(N, K):
    """One wave per row, four rows per workgroup: N below, at and off a multiple of 4, K below one sweep of the wave (8), one sweep
    exactly (512), one and a bit (520) and several.  g against the fp64 row sums of the fp16 weight; c = c_base + alpha c_delta with
    two fp32 roundings; rows past N of larger g / c buffers untouched; without c_out nothing but g is written."""
    from sdlcm_amd import ops
    w = _rnd(N, K, seed=N + K, scale=K ** -0.5)
    w[0, : K // 2] = w[0, : K // 2].abs()                    # one row that does not cancel
    wd = w.to(DEV)
    W = wd.double()
    ref_g = W.sum(1)
    bound_g = la.acc_err(K, W.abs().sum(1)) + la.U * ref_g.abs() + 1e-30
    cb = torch.randn(N + 5, generator=torch.Generator().manual_seed(1)).to(DEV)
    cd = (torch.randn(N + 5, generator=torch.Generator().manual_seed(2)) * 0.3).to(DEV)
    worst_g = worst_c = 0.0
    for c_out, c_delta, alpha in ((False, False, 0.0), (True, False, -0.5), (True, True, 0.0), (True, True, -0.5)):
        g = torch.full((N + 5,), 7.5, device=DEV)
        c = torch.full((N + 5,), -3.25, device=DEV)
        g0, c0 = g.clone(), c.clone()
        ops.ln_fold_refresh(wd, g, cb if c_out else None, cd if c_delta else None, alpha, c if c_out else None)
        torch.cuda.synchronize()
        worst_g = max(worst_g, la.worst_ratio(g[:N], ref_g, bound_g))
        assert la.tail_same(g, g0, N), "rows past N of the g buffer were written"
        if not c_out:
            assert la.same_bits(c, c0)
            continue
        assert la.tail_same(c, c0, N), "rows past N of the c buffer were written"
        a32 = float(np.float32(alpha)) if c_delta else 0.0
        ref_c = cb[:N].double() + a32 * cd[:N].double()
        bound_c = 2 * la.U * (cb[:N].double().abs() + abs(a32) * cd[:N].double().abs()) + 1e-38
        worst_c = max(worst_c, la.worst_ratio(c[:N], ref_c, bound_c))
        if a32 == 0.0:
            assert la.same_bits(c[:N], cb[:N]), "weight 0 must hand c_base through"
    print(f"[lora] ln_fold_refresh N={N} K={K}: worst error/bound g {worst_g:.4g}, c {worst_c:.4g}")
    assert worst_g <= 1.0 and worst_c <= 1.0


@pytest.mark.parametrize("shape", [(320, 36), (4, 2880)], ids=["conv_in", "conv_out"])
def test_axpy_at_the_conv_in_and_conv_out_sizes_fp64(shape):
    """11520 elements (45 workgroups' worth of one sweep, far below the grid-stride span tests/test_ops_gpu.py covers): within
    H |ref| + SUB + 2 U s of fp64, into a copy of the base as the merge does; the weights 0.75 and -0.5 of the comparison."""
    from sdlcm_amd import ops
    base, delta = _rnd(*shape, seed=5, scale=0.2), _rnd(*shape, seed=6, scale=0.1)
    b, d = base.to(DEV), delta.to(DEV)
    worst = 0.0
    for alpha in (0.75, -0.5):
        live = b.clone()
        ops.axpy(b, d, alpha, live)
        torch.cuda.synchronize()
        ref = b.double() + alpha * d.double()
        s = b.double().abs() + abs(alpha) * d.double().abs()
        worst = max(worst, la.worst_ratio(live, ref, la.H * ref.abs() + la.SUB + 2 * la.U * s))
    print(f"[lora] axpy {shape}: worst error/bound {worst:.4g}")
    assert worst <= 1.0


# ---- the two pipelines, each with one LoRA ----------------------------------------------------------------------------------------
_TF_KINDS = ("proj_in", "proj_out") + tuple(f"transformer_blocks.0.{s}" for s in (
    "attn1.to_q", "attn1.to_k", "attn1.to_v", "attn1.to_out.0", "attn2.to_q", "attn2.to_k", "attn2.to_v", "attn2.to_out.0",
    "ff.net.0.proj", "ff.net.2"))
# one Transformer2DModel per block that has them (320 / 640 / 1280 wide on the way down, 1280 in the middle, 1280 / 640 / 320 up)
_TF_SITES = ("down_blocks.0.attentions.0", "down_blocks.1.attentions.1", "down_blocks.2.attentions.0", "mid_block.attentions.0",
             "up_blocks.1.attentions.2", "up_blocks.2.attentions.0", "up_blocks.3.attentions.1")
_RES_SITES = ("down_blocks.0.resnets.1", "down_blocks.1.resnets.0", "down_blocks.2.resnets.0", "down_blocks.3.resnets.1",
              "mid_block.resnets.0", "up_blocks.0.resnets.2", "up_blocks.1.resnets.0", "up_blocks.2.resnets.1", "up_blocks.3.resnets.0")

# LoRA strength per form, chosen on the oracle alone so that the merged picture lies SEPARATION x IMG_TOL = 0.1 from the unmerged one
# (the oracle's two images differ by 0.36 under form (a) and by 0.37 under form (c); half the strength gives 0.16 under (c))
GAIN = {"a": 0.25, "c": 2.0}
SIZE = {"a": (72, 40), "c": (64, 96)}          # 72x40: latents 9x5 -> 5x3 -> 3x2 -> 2x1, every upsampler targets an odd size


def modules_of(form, sd):
    if form == "a":
        mods = [f"{p}.{k}" for p in _TF_SITES for k in _TF_KINDS]
        for p in _RES_SITES:
            mods += [f"{p}.{k}" for k in ("conv1", "conv2", "time_emb_proj", "conv_shortcut") if f"{p}.{k}.weight" in sd]
        mods += [f"down_blocks.{i}.downsamplers.0.conv" for i in range(3)] + [f"up_blocks.{i}.upsamplers.0.conv" for i in range(3)]
        return sorted(mods + ["conv_in", "conv_out"])
    # SD 2.x: the to_q factor differs per level (5 / 10 / 20 / 20 heads), the context is 1024 wide, the projections are linear
    return sorted(f"{p}.{k}" for p in _TF_SITES[:4] + _TF_SITES[4:5] for k in
                  ("proj_in", "transformer_blocks.0.attn1.to_q", "transformer_blocks.0.attn2.to_q", "transformer_blocks.0.attn2.to_k",
                   "transformer_blocks.0.ff.net.0.proj"))


def _build(form):
    from sdlcm_amd import weights
    from sdlcm_amd.lora import LoraStyle
    from sdlcm_amd.pipeline import LcmHipPipeline
    from sdlcm_amd.scheduler import LCMSchedule
    usd, pipe_cfg, cfg, sch = cr.form_weights(form)
    vsd = weights.synthetic_vae()
    hip = LcmHipPipeline(usd, vsd, unet_cfg=pipe_cfg, device=DEV, schedule=LCMSchedule(**sch) if sch else None)
    mods = modules_of(form, usd)
    raw, deltas = lr.make_lora(cfg, usd, mods, r=4, alpha=2.0, seed=23, key_style="mixed", gain=GAIN[form])
    before = lr.snapshot(hip.unet.w)
    with torch.cuda.stream(hip.stream):
        style = LoraStyle(hip.unet, raw)
        hip.stream.synchronize()
    assert style.modules == mods and not style.skipped
    return types.SimpleNamespace(form=form, hip=hip, usd=usd, vsd=vsd, cfg=cfg, pipe_cfg=pipe_cfg, sch=sch, mods=mods, raw=raw,
                                 deltas=deltas, style=style, before=before)


def _apply(st, wt):
    with torch.cuda.stream(st.hip.stream):
        st.style.apply(wt)
        st.hip.stream.synchronize()


@pytest.fixture(scope="module")
def form_a():
    st = _build("a")
    yield st
    st.hip.close()


@pytest.fixture(scope="module")
def form_c():
    st = _build("c")
    yield st
    st.hip.close()


@pytest.fixture
def forms(request):
    return lambda f: request.getfixturevalue("form_" + f)


# ---- 2. per tensor, on the device -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["a", "c"])
def test_merge_per_tensor_on_the_device(forms, form):
    from sdlcm_amd.model import UNetHip
    st = forms(form)
    live = st.hip.unet.w
    expected = lr.expected_touched(st.mods)
    if form == "a":
        # beside the kinds tests/test_pipeline_gpu.py merges: attn1.to_k, a proj_in given as a plain matrix, an up block's time_emb_proj
        assert any(m.endswith("attn1.to_k") for m in st.mods) and any(m.startswith("up_blocks") and m.endswith(".time_emb_proj") for m in st.mods)
        assert any(v.dim() == 2 for k, v in st.raw.items() if "proj_in.lora_" in k and ("lora_down" in k or "lora_A" in k))
        assert {n for n in expected if n.endswith(".w3")} == {f"up_blocks.{i}.upsamplers.0.conv.w3" for i in range(3)}
    ref = UNetHip(lr.merged_checkpoint(st.usd, st.deltas, WT), st.pipe_cfg, DEV).w
    c64 = lr.fold_constants64(st.usd, st.cfg, st.deltas, WT, sorted(n[:-2] for n in expected if n.endswith(".c")))
    _apply(st, WT)
    try:
        m = lr.measure(live, ref, st.before, expected, st.style.delta, WT, c64)
        rg, n_g = lr.g_ratio(live)
        print(f"[lora] form ({form}): {len(st.mods)} modules, {len(expected)} packed tensors; {n_g} row-sum vectors worst error/bound {rg:.4g}")
        lr.check(m, expected, f"form ({form}) on the device wt={WT:g}")
        assert rg <= 1.0
    finally:
        _apply(st, 0.0)
    torch.cuda.synchronize()
    bad = [n for n in live if not la.same_bits(live[n], st.before[n])]
    assert not bad, f"weight 0 does not restore {bad[:6]}"
    # the touched weights hold negative zeros, which base + 0 * delta would not keep: weight 0 must copy the base
    assert any(((st.before[n] == 0) & torch.signbit(st.before[n])).any() for n in expected if n.endswith(".w"))


# ---- 3. a graph captured before the merge, and the odd path -----------------------------------------------------------------------
def _cell_inputs(form):
    W, H = SIZE[form]
    D = 768 if form == "a" else 1024
    gen = torch.Generator().manual_seed(5200 + ord(form))
    pe, ne = ((torch.randn(1, 77, D, generator=gen) + cr.EMBED_OFFSET * torch.sign(torch.randn(1, 1, D, generator=gen))).to(torch.float16)
              for _ in range(2))
    return dict(W=W, H=H, pe=pe, ne=ne, g=cr.FORMS[form][2], steps=cr.STEPS[form], seed=8100)


def _odd_upsamples(recs):
    """Recorded conv3x3 launches of the loader-fused upsampling form with an explicit (odd) target size."""
    n = 0
    for rec in recs:
        for cell in getattr(rec[2], "__closure__", None) or ():
            v = cell.cell_contents
            if isinstance(v, dict) and v.get("ups") == 1 and v.get("out_hw") is not None:
                n += 1
    return n


KEYS = ("rgb", "latents", "pool8")


@pytest.mark.parametrize("form", ["a", "c"])
def test_replay_of_a_graph_captured_before_the_merge(forms, form):
    from sdlcm_amd import ops
    st = forms(form)
    hip, inp = st.hip, _cell_inputs(form)
    assert hip.sched.prediction_type == cr.FORMS[form][1] and not hip.unet.has_cond
    run = lambda **kw: hip.generate(inp["pe"], [inp["seed"]], inp["W"], inp["H"], inp["steps"], inp["g"], negative_embeds=inp["ne"], **kw)
    # the oracle on the unmerged and on the merged checkpoint (fp32 tensors are taken as they are: one conversion serves both)
    f32 = {k: v.float() for k, v in st.usd.items()}
    merged = dict(f32, **{m + ".weight": v for m in st.deltas for v in [lr.merged_checkpoint(st.usd, {m: st.deltas[m]}, WT)[m + ".weight"]]})
    refs = []
    for sd in (f32, merged):
        ora = cr.ChainOracle(sd, st.vsd, st.cfg, schedule=st.sch)
        refs.append(ora(inp["pe"].float(), inp["W"], inp["H"], inp["steps"], inp["g"], inp["seed"], negative_embeds=inp["ne"].float()))
    sep = float(np.abs(cr.image01(refs[1]["image"]) - cr.image01(refs[0]["image"])).max())
    print(f"[lora] form ({form}) {inp['W']}x{inp['H']}: the LoRA moves the oracle's image by {sep:.3g} on [0,1] "
          f"(condition: {cr.SEPARATION * cr.IMG_TOL:g})")
    assert sep >= cr.SEPARATION * cr.IMG_TOL
    first = run()                                   # captures the plan
    again = run()
    assert all(np.array_equal(first[k], again[k]) for k in KEYS)
    _apply(st, WT)
    try:
        rep = run()
        with ops.recording() as recs:
            eager = run(want_float=True)
        if form == "a":
            n_odd = _odd_upsamples(recs)
            print(f"[lora] form (a): {n_odd} upsampling launches read the plain .w3 weights")
            assert n_odd >= 3 * inp["steps"]
        for k in KEYS:
            assert np.array_equal(rep[k], eager[k]), f"the replay of the graph captured before the merge differs from the eager run in {k}"
        assert not np.array_equal(rep["rgb"], first["rgb"])
        ref = refs[1]
        e_img = float(np.abs(cr.image01(eager["image"].transpose(0, 3, 1, 2)) - cr.image01(ref["image"])).max())
        e_lat = float(np.abs(eager["latents"][0] - ref["latents"][0]).max())
        bound = cr.latent_bound(inp["g"], ref["latents"])
        print(f"[lora] form ({form}) merged: image[0,1] max|d| = {e_img:.4g} (bound {cr.IMG_TOL:g}, ratio {e_img / cr.IMG_TOL:.3g}), "
              f"latents max|d| = {e_lat:.4g} (bound {bound:.4g}, ratio {e_lat / bound:.3g})")
    finally:
        _apply(st, 0.0)
    back = run()
    for k in KEYS:
        assert np.array_equal(back[k], first[k]), f"after weight 0 the replay's {k} is not the first run's"
    assert e_img < cr.IMG_TOL, f"image off by {e_img:.4g}"
    assert e_lat < bound, f"latents off by {e_lat:.4g}, bound {bound:.4g}"


# ---- 4. text encoders -------------------------------------------------------------------------------------------------------------
TE_GAIN = 1.0          # on the oracle alone: the merge moves every output by 30 tolerances and more


@pytest.mark.parametrize("tag", ["clip-h", "projected"])
def test_text_encoder_lora_against_transformers(tag):
    from sdlcm_amd.clip import CLIP_BIGG, CLIP_H, ClipTextHip, HashTokenizer, synthetic_clip
    from sdlcm_amd.lora import ClipLora
    from oracle.clip import clip_text_oracle, clip_text_oracle_sdxl
    cfg, index = (dict(CLIP_H), 0) if tag == "clip-h" else (dict(CLIP_BIGG, num_hidden_layers=4), 1)
    L = cfg["num_hidden_layers"]
    sd = synthetic_clip(cfg, seed=7)
    targets = [(i, sub) for i in sorted({0, L // 2, L - 2}) for sub in lr.TE_SUBS]
    mine, deltas = lr.make_te_lora(sd, targets, index=index, r=4, alpha=2.0, seed=47, gain=TE_GAIN)
    other, _ = lr.make_te_lora(sd, targets, index=1 - index, r=4, alpha=2.0, seed=49, gain=TE_GAIN)
    ids = HashTokenizer()(["a papercut illustration of a fox", ""])
    enc = ClipTextHip(sd, cfg, device=DEV)
    before = lr.snapshot(enc.w)

    def fwd():
        if index:
            h, p = enc.forward(ids, output="penultimate", pooled=True)
            return [h.clone(), p.clone()]
        return [enc.forward(ids).clone()]

    base = fwd()
    style = ClipLora(enc, {**other, **mine}, index)
    assert sorted(style.used) == sorted(k for k in mine if not k.endswith(".alpha")) and len(style.modules) == len(targets)
    merged = lr.merged_checkpoint(sd, deltas, WT)
    refs = [t for t in clip_text_oracle_sdxl(merged, cfg, ids)] if index else [clip_text_oracle(merged, cfg, ids)]
    expected = lr.expected_touched_te(targets)
    style.apply(WT)
    torch.cuda.synchronize()
    lr.check(lr.measure(enc.w, ClipTextHip(merged, cfg, device=DEV).w, before, expected, style.delta, WT), expected, f"{tag} on the device")
    got = fwd()
    for name, g, r, b in zip(("hidden", "pooled"), got, refs, base):
        g, r, b = g.float().cpu().numpy(), r.numpy(), b.float().cpu().numpy()
        tol = 2e-2 * max(1.0, np.abs(r).max())
        e, moved = np.abs(g - r).max(), np.abs(g - b).max()
        print(f"[lora] {tag} {name}: max|d| vs transformers on merged weights {e:.4g} (tolerance {tol:.4g}, ratio {e / tol:.3g}); "
              f"the merge moves the output by {moved:.4g} ({moved / tol:.3g} tolerances)")
        assert e < tol
        assert moved > 10 * tol
    style.apply(0.0)
    torch.cuda.synchronize()
    assert all(la.same_bits(enc.w[n], before[n]) for n in enc.w)
    assert all(torch.equal(a, b) for a, b in zip(fwd(), base))


# ---- 5. the worker: two styles with overlapping targets ---------------------------------------------------------------------------
STYLE_TARGETS = {
    "lora_a": ("down_blocks.1.attentions.0.transformer_blocks.0.attn1.to_q", "mid_block.attentions.0.transformer_blocks.0.ff.net.0.proj",
               "up_blocks.2.resnets.1.conv1"),
    "lora_b": ("down_blocks.1.attentions.0.transformer_blocks.0.attn1.to_q", "up_blocks.3.attentions.2.transformer_blocks.0.attn2.to_v",
               "up_blocks.1.upsamplers.0.conv"),
}
STYLE_LEVELS = {"lora_a": [0.5, 1.0], "lora_b": [0.6, 0.9]}


def _wreq(style=None, level=0, seed=5):
    return types.SimpleNamespace(prompt="a paper boat", size="64x64", num_inference_steps=2, guidance_scale=1.0, seed=seed,
                                 style_lora=types.SimpleNamespace(style=style, level=level))


@pytest.fixture(scope="module")
def styled(tmp_path_factory):
    """Two style files on disk and in the registry; MODEL=synthetic, engines not shared between workers."""
    from safetensors.torch import save_file
    from sdlcm_amd import weights
    from sdlcm_amd.backends import styles
    usd = weights.synthetic_unet()
    d = tmp_path_factory.mktemp("styles")
    old = {k: os.environ.get(k) for k in ("MODEL", "MODEL_ROOT", "LCM_SHARE_ENGINE")}
    os.environ.update(MODEL="synthetic", MODEL_ROOT="/nonexistent", LCM_SHARE_ENGINE="0")
    for i, (sid, mods) in enumerate(STYLE_TARGETS.items()):
        raw, _ = lr.make_lora(None, usd, list(mods), r=4, alpha=4.0, seed=61 + i, key_style="kohya", gain=2.0)
        path = str(d / f"{sid}.safetensors")
        save_file({k: v.contiguous() for k, v in raw.items()}, path)
        styles.register_style(styles.StyleDef(id=sid, title=sid, lora_path=path, adapter_name="style_" + sid, levels=STYLE_LEVELS[sid],
                                             required_cross_attention_dim=768))
    yield
    for sid in STYLE_TARGETS:
        styles.STYLE_REGISTRY.pop(sid, None)
    for k, v in old.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def _solo(req):
    """The request's PNG from a worker that serves nothing else."""
    from sdlcm_amd.backends.worker_factory import create_hip_worker
    w = create_hip_worker(worker_id=0)
    try:
        return w.run_job(types.SimpleNamespace(req=req))[0]
    finally:
        w.close()


SEQUENCE = ((None, 0), ("lora_a", 1), ("lora_b", 2), ("lora_a", 2), ("lora_b", 1), (None, 0))


@pytest.fixture(scope="module")
def solos(styled):
    return {sl: _solo(_wreq(*sl)) for sl in dict.fromkeys(SEQUENCE)}


def test_worker_switches_between_overlapping_styles(styled, solos):
    """plain, A1, B2, A2, B1, plain in one worker: A -> B directly (both write the same to_q rows), a level change within a style,
    and back to plain; every PNG is the solo worker's, and the five kinds differ."""
    from sdlcm_amd.backends.worker_factory import create_hip_worker
    assert len(set(solos.values())) == len(solos), "two of plain, A1, A2, B1, B2 give the same picture"
    w = create_hip_worker(worker_id=0)
    try:
        assert set(STYLE_TARGETS) <= set(w._styles)
        for i, sl in enumerate(SEQUENCE):
            png = w.run_job(types.SimpleNamespace(req=_wreq(*sl)))[0]
            assert png == solos[sl], f"request {i} {sl}: the PNG depends on what the worker served before"
    finally:
        w.close()


def test_two_lanes_interleaved_styles_keep_their_solo_bytes(styled, solos):
    """A2 and B1 jobs interleaved in a held queue, drained by a worker with two lanes: the merged weights are shared by the lanes,
    so a lane must never replay while the other style is merged."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from tools import minipool
    from sdlcm_amd.backends.worker_factory import create_hip_worker
    w = create_hip_worker(worker_id=0)
    pool = None
    try:
        assert w._engine.n_lanes >= 2
        order = [("lora_a", 2), ("lora_b", 1)] * 4
        pool = minipool.MiniPool(lambda worker_id: w, {"m": "synthetic"}, "m")
        w.bind_queue(pool.q)
        gate, inside = threading.Event(), threading.Event()
        hold = pool.submit_job(minipool.CustomJob(handler=lambda: (inside.set(), gate.wait(30))))
        assert inside.wait(30)
        futs = [pool.submit_job(minipool.GenerationJob(req=_wreq(*sl))) for sl in order]
        gate.set()
        hold.result(60)
        res = [f.result(300) for f in futs]
        pool.q.join()
        for i, (sl, r) in enumerate(zip(order, res)):
            assert (r[0] if isinstance(r, tuple) else r) == solos[sl], f"job {i} {sl}: not its solo bytes"
    finally:
        w.bind_queue(None)
        if pool is not None:
            pool._worker = None
            pool.shutdown()
        w.close()
