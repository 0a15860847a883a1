"""Parity at the BASELINE.json configurations themselves (the sizes the reference's own live-GPU suite sweeps,
tests/test_sdxl_worker.py:230-256: 512, 768, 1024), against the CPU oracle on identical seeds.

Tolerance: north_star -- per-pixel |delta| < 1e-2 on the decoded image in [0,1].  Parity tests come first in the
file; self-comparison (determinism) checks last, so a parity regression is never masked by them.
The oracle restates diffusers' published algorithm (parity unpinned at that boundary: oracle/__init__.py)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# The oracle outputs of the BASELINE-size cases are committed fixtures (tests/golden/oracle_*.npz, computed by
# tests/golden/make_oracle_golden.py in the build container: final latents, the FULL u8 image, the float image on a stride-4 grid):
# minutes of CPU oracle time per run otherwise (round 2: 718 s of the driver's 900 s limit).  LCM_LIVE_ORACLE=1 runs the
# oracle live on the full image instead.  Small sizes keep a live oracle run (tests/test_pipeline_gpu.py).
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _golden(case):
    """The committed fixture of a case -- a missing file is an ERROR (a silent fall-back to a live run would hide a fixture that
    was never committed); LCM_LIVE_ORACLE=1 asks for the live oracle on purpose."""
    if os.environ.get("LCM_LIVE_ORACLE", "0") == "1":
        return None
    p = os.path.join(GOLD, f"oracle_{case}.npz")
    assert os.path.exists(p), f"{p} missing: run tests/golden/make_oracle_golden.py {case} in the build container"
    return np.load(p)


# The final latents: fp16-operand kernels against the fp32 oracle.  North_star's tolerance is stated on the decoded image; the
# latents of the synthetic weights have a standard deviation of 16-24 (|max| 65-105), so their bound is relative to that scale:
# max |delta| < 5e-3 x std(oracle latents) -- five fp16 steps at the scale of the data (measured: 1.8e-3 x std at 768^2 / 8 steps,
# the largest of the guidance-1 cases) -- times the guidance scale under classifier-free guidance (SDXL, g = 5: 1.2e-2 x std).  A wrong tile border, a skipped step or a mis-scaled sigma shows up at >= 5e-2 x std.
LATENT_REL_TOL = 5e-3
U8_HALF_STEP = 0.5 / 255.0


def _err_vs(out, gold, ref_fn, req=0, guidance=1.0):
    """Per-pixel error of request ``req`` on the decoded [0,1] image, EVERY pixel.  With a fixture: (a) the float image against
    the oracle's full u8 image -- |x - u8/255| + 0.5/255 bounds |x - x_oracle| for every pixel, returned as the error; (b) the
    float image against the fixture's exact fp16 values on the stride-4 grid; (c) the final latents in full.  Live: everything
    in float.  -> (error array over all pixels, u8 max diff over all pixels)."""
    img = out["image"][req:req + 1].transpose(0, 3, 1, 2)
    if gold is not None:
        st = int(gold["stride"])
        eg = np.abs(_img01(img[0][:, ::st, ::st]) - _img01(gold["image_grid"].astype(np.float32)))
        assert eg.max() < 1e-2, f"stride-{st} grid: max|d|={eg.max():.4g}"
        full = gold["u8_full"]                                              # [H, W, 3]
        assert full.shape == out["rgb"][req].shape
        e = np.abs(_img01(img[0]).transpose(1, 2, 0) - full.astype(np.float32) / 255.0) + U8_HALF_STEP
        u8 = int(np.abs(out["rgb"][req].astype(int) - full.astype(int)).max())
        gl = gold["latents"][0].astype(np.float32)
        lat = np.abs(out["latents"][req].astype(np.float32) - gl)
        print(f"[parity] latents max|d|={lat.max():.4g} = {lat.max() / gl.std():.3g} x std ({gl.std():.3g}), mean|d|={lat.mean():.3g}; "
              f"grid max|d|={eg.max():.4g}; all pixels: u8 max diff {u8}")
        # classifier-free guidance extrapolates: eps = eps_u + g (eps_t - eps_u) carries g times the rounding of its two inputs
        assert lat.max() < LATENT_REL_TOL * max(1.0, guidance) * gl.std(), f"final latents: max|d|={lat.max():.4g} against std {gl.std():.4g}"
        return e, u8
    ref = ref_fn()
    e = np.abs(_img01(img) - _img01(ref["image"]))
    gl = ref["latents"][0].astype(np.float32)
    lat = np.abs(out["latents"][req].astype(np.float32) - gl)
    assert lat.max() < LATENT_REL_TOL * max(1.0, guidance) * gl.std(), f"final latents: max|d|={lat.max():.4g} against std {gl.std():.4g}"
    return e, int(np.abs(out["rgb"][req:req + 1].astype(int) - ref["image_u8"].astype(int)).max())


def _embeds(B, D=768, seed=5):
    return torch.randn(B, 77, D, generator=torch.Generator().manual_seed(seed)).to(torch.float16)


def _img01(x_nchw):
    return np.clip(x_nchw / 2 + 0.5, 0, 1)


@pytest.fixture(scope="module")
def sd15():
    from sdlcm_amd import weights
    from sdlcm_amd.pipeline import LcmHipPipeline
    from oracle.pipeline import LCMPipelineOracle
    usd, vsd = weights.synthetic_unet(), weights.synthetic_vae()
    hip = LcmHipPipeline(usd, vsd, device="cuda:0")
    cache = {}

    def ora():                     # built only when a case has no fixture (or LCM_LIVE_ORACLE=1)
        if "o" not in cache:
            cache["o"] = LCMPipelineOracle(usd, vsd)
        return cache["o"]
    yield dict(hip=hip, ora=ora)
    hip.close()


def test_config1_512_4step_batch1_parity(sd15):
    """BASELINE configs[1]: SD1.5 LCM 512x512, 4 steps, batch 1 -- eager pass vs oracle, and the hipGraph replay of the
    same request is bit-identical to the eager pass."""
    hip, ora = sd15["hip"], sd15["ora"]
    pe = _embeds(1, seed=42)
    out = hip.generate(pe, [42], 512, 512, 4, 1.0, want_float=True)
    e, u8 = _err_vs(out, _golden("sd15_512_4step"), lambda: ora()(pe.float(), 512, 512, 4, 1.0, 42))
    print(f"[parity] 512x512 4-step batch 1: max|d|={e.max():.4g} mean|d|={e.mean():.3g} u8 max diff {u8}")
    assert e.max() < 1e-2
    assert u8 <= 3
    rep = hip.generate(pe, [42], 512, 512, 4, 1.0)
    assert np.array_equal(rep["rgb"], out["rgb"]) and np.array_equal(rep["latents"], out["latents"])


def test_config2_512_batch8_parity_per_request(sd15):
    """BASELINE configs[2] per-GPU shard: batch 8 at 512x512 (1 step keeps the CPU side affordable): requests 0 and 7
    of the batch against the oracle run per request, and every request bit-identical to its solo run."""
    hip, ora = sd15["hip"], sd15["ora"]
    B = 8
    pe = _embeds(B, seed=77)
    seeds = [500 + i for i in range(B)]
    out = hip.generate(pe, seeds, 512, 512, 1, 1.0, want_float=True)
    for i in (0, 7):
        e, _ = _err_vs(out, _golden(f"sd15_512_b8_1step_req{i}"), lambda: ora()(pe[i:i + 1].float(), 512, 512, 1, 1.0, seeds[i]), req=i)
        print(f"[parity] 512x512 batch 8, request {i}: max|d|={e.max():.4g}")
        assert e.max() < 1e-2
    graph = hip.generate(pe, seeds, 512, 512, 1, 1.0)
    assert np.array_equal(graph["rgb"], out["rgb"])
    for i in (1, 6):
        solo = hip.generate(pe[i:i + 1], [seeds[i]], 512, 512, 1, 1.0)
        assert np.array_equal(solo["rgb"][0], graph["rgb"][i]) and np.array_equal(solo["latents"][0], graph["latents"][i])


def test_config3_768_8step_parity(sd15):
    """BASELINE configs[3] geometry and step count: 768x768, 8 steps (batch 1 on the CPU side).  The SD1.5 VAE has
    sample_size 512, so the 96x96 latent takes diffusers' overlapping-tile decode (vae.enable_tiling(),
    backends/cuda_worker.py:91) on both sides; the S = 9216 self-attention is the long-sequence case."""
    hip, ora = sd15["hip"], sd15["ora"]
    pe = _embeds(1, seed=9)
    out = hip.generate(pe, [31], 768, 768, 8, 1.0, want_float=True)
    assert out["rgb"].shape == (1, 768, 768, 3)
    e, _ = _err_vs(out, _golden("sd15_768_8step"), lambda: ora()(pe.float(), 768, 768, 8, 1.0, 31))
    print(f"[parity] 768x768 8-step: max|d|={e.max():.4g} mean|d|={e.mean():.3g}")
    assert e.max() < 1e-2


@pytest.fixture(scope="module")
def sdxl():
    from sdlcm_amd import weights
    from sdlcm_amd.config import SDXL_UNET, unet_config, vae_config
    from sdlcm_amd.pipeline import LcmHipPipeline
    from oracle.pipeline import LCMPipelineOracle
    ucfg = unet_config(SDXL_UNET)
    vcfg = vae_config(dict(scaling_factor=0.13025, sample_size=1024, force_upcast=True))
    usd = weights.synthetic_state_dict(weights.unet_param_spec(ucfg), 0)
    vsd = weights.synthetic_state_dict(weights.vae_param_spec(vcfg), 1)
    hip = LcmHipPipeline(usd, vsd, ucfg, vcfg, device="cuda:0")
    cache = {}

    def ora():
        if "o" not in cache:
            cache["o"] = LCMPipelineOracle(usd, vsd, ucfg, vcfg)
        return cache["o"]
    yield dict(hip=hip, ora=ora)
    hip.close()


def _sdxl_inputs():
    g = torch.Generator().manual_seed(8)
    pe = torch.randn(1, 77, 2048, generator=g).half()
    pooled = torch.randn(1, 1280, generator=g).half()
    tids = torch.tensor([[1024.0, 1024.0, 0, 0, 1024.0, 1024.0]])
    return pe, pooled, tids


@pytest.mark.parametrize("guidance,steps", [(1.0, 1), (5.0, 1)])
def test_config4_sdxl_1024_parity(sdxl, guidance, steps):
    """BASELINE configs[4] architecture and geometry: SDXL-base (full width, 2.57 B-parameter UNet, cross_attention_dim
    2048, text_time embedding) at 1024x1024 against the oracle; guidance 1 (no CFG) and guidance 5 (classifier-free
    guidance, negative conditioning = zeros).  The 30 steps of the config are not affordable on the CPU (~6.8 TFLOP per
    UNet forward): 1 step here (multi-step sampling is covered against the oracle on SD1.5 at 512 and 768 px and on the
    narrow SDXL-family configuration in test_pipeline_gpu.py), the 30-step run by the GPU-only determinism check below."""
    hip, ora = sdxl["hip"], sdxl["ora"]
    pe, pooled, tids = _sdxl_inputs()
    kw = dict(added=(pooled, tids))
    okw = dict(added=(pooled.float(), tids))
    if guidance > 1:
        kw.update(negative_embeds=torch.zeros_like(pe), negative_added=(torch.zeros_like(pooled), tids))
        okw.update(negative_embeds=torch.zeros_like(pe).float(), negative_added=(torch.zeros_like(pooled).float(), tids))
    out = hip.generate(pe, [21], 1024, 1024, steps, guidance, want_float=True, **kw)
    assert out["rgb"].shape == (1, 1024, 1024, 3)
    e, _ = _err_vs(out, _golden(f"sdxl_1024_g{int(guidance)}_{steps}step"), lambda: ora()(pe.float(), 1024, 1024, steps, guidance, 21, **okw),
                   guidance=guidance)
    print(f"[parity] SDXL 1024x1024 g={guidance} {steps}-step: max|d|={e.max():.4g} mean|d|={e.mean():.3g}")
    assert e.max() < 1e-2
    rep = hip.generate(pe, [21], 1024, 1024, steps, guidance, **kw)             # captured graph == the eager pass
    assert np.array_equal(rep["rgb"], out["rgb"]) and np.array_equal(rep["latents"], out["latents"])


# ---- launch audit: every contraction / attention launch of the tuned passes against fp64 (tests/launch_audit.py) ------------
# The passes tools/make_plans.py tunes, run eagerly (generate(want_float=True) -> pipe._enqueue on the lane stream) with the
# shipped plan table -- never pipe.tune() -- and inputs filled the way generate() fills them.  The first launch of each distinct
# shape is checked in full, every image of the batch.
SD15_TUNED_PASSES = [(1, 512), (1, 768), (1, 256), (1, 128), (1, 192), (1, 64), (2, 512), (4, 512), (8, 512), (2, 256), (3, 128),
                     (8, 768)]
TUNED_STEPS = 4
_AUDITED = {}                   # pass name -> (Audit.checks, plan keys the pass launched), for the coverage report


def _audit_pass(hip, name, B, size, guidance=1.0, **kw):
    from launch_audit import Audit
    plans = hip.lanes[0].plans
    before = set(plans)
    with Audit() as au:
        hip.generate(kw.pop("pe"), [300 + i for i in range(B)], size, size, TUNED_STEPS, guidance, want_float=True, **kw)
    for k in set(plans) - before:          # the eager pass's plan is not kept (no graph was captured for it)
        plans.pop(k)
    torch.cuda.empty_cache()
    launched = au.record_keys()
    _AUDITED[name] = (au.checks, launched)
    assert au.checked_keys() == launched, f"{name}: hook saw {len(au.checked_keys())} of {len(launched)} plan keys"
    _audit_verdict(name, au, f"{len(launched)} plan keys ({sum(k in au.table for k in launched)} in the table), ")
    return au


def _audit_verdict(name, au, extra=""):
    from launch_audit import failures, summary_line
    bad = failures(au.checks)
    print(f"[audit] {name}: {len(au.checks)} launches checked, {extra}{summary_line(au.checks)}")
    for c in bad:
        print(f"[audit] {name} FAIL {c}")
    assert not bad, f"{name}: {len(bad)} launches outside their fp64 error bound (or past the GroupNorm kappa tripwire)"


def _audit_report(table):
    from launch_audit import CHECKED, REFINE_ENTRIES, config_table, entry_table
    checks = [c for name in _AUDITED for c in _AUDITED[name][0]]
    per = entry_table(checks)
    for op in sorted(per):
        n, r, k = per[op]
        print(f"[audit] entry {op:>28}: {n:>5} launches checked, worst ratio {r:.3f}" + (f", worst kappa {k:.4g}" if k else ""))
    # every entry point the audit checks was reached by a real pass: a refactor that routes around ops.X fails here
    # (the two entry points of refinement chains are held to the same by tests/test_audit_ragged_gpu.py, whose passes run them)
    missing = sorted(set(CHECKED) - set(REFINE_ENTRIES) - set(per))
    assert not missing, f"audited entry points no pass reached: {missing}"
    reached = set().union(*(v[1] for v in _AUDITED.values()))
    rows = config_table(checks)
    table_cfgs = {(k[0],) + tuple(int(x) for x in v[:4]) for k, v in table.items()}
    reached_cfgs = {(k[0],) + tuple(int(x) for x in table[k][:4]) for k in reached if k in table}
    print(f"[audit] passes: {', '.join(_AUDITED)}")
    print(f"[audit] {'kind':>4} {'bm':>4} {'bn':>4} {'splits':>6} {'variant':>7} {'checked':>7} {'worst':>7} {'stats':>7}")
    for cfg in sorted(rows):
        n, r, sr = rows[cfg]
        print(f"[audit] {cfg[0]:>4} {cfg[1]:>4} {cfg[2]:>4} {cfg[3]:>6} {cfg[4]:>7} {n:>7} {r:>7.3f} {sr:>7.3f}")
    print(f"[audit] table configurations reached: {len(reached_cfgs)} of {len(table_cfgs)}; "
          f"table entries reached: {len(reached & set(table))} of {len(table)}")
    for k in sorted(set(table) - reached):
        print(f"[audit] unreached table entry {','.join(map(str, k))}: {list(table[k][:4])}")


def test_audit_sd15_tuned_passes_fp64(sd15):
    """The 12 SD1.5 passes tools/make_plans.py tunes: every launch shape within its fp64 bound, every plan key checked."""
    hip = sd15["hip"]
    for B, size in SD15_TUNED_PASSES:
        _audit_pass(hip, f"sd15 B{B} {size}px", B, size, pe=_embeds(B, seed=60 + B))


def test_audit_sd15_text_encoder_and_unfused_paths_fp64(monkeypatch):
    """The SD1.5 text encoder (CLIP-L, last hidden state) under the audit, and a small SD1.5 pass through the paths the tuned
    passes do not take: the VAE mid attention on the MFMA GEMMs (scores + softmax_rows + transpose; the flash kernel is the
    default for 512-wide VAEs) and the time embedding computed per step (time_embed, not time_embed_all)."""
    from launch_audit import Audit
    from sdlcm_amd import model, weights
    from sdlcm_amd.clip import CLIP_L, ClipTextHip, HashTokenizer, synthetic_clip
    from sdlcm_amd.pipeline import LcmHipPipeline
    enc = ClipTextHip(synthetic_clip(CLIP_L), CLIP_L, device="cuda:0")
    with Audit() as au:
        enc.forward(HashTokenizer()(["a red fox in the snow", "a lighthouse"]))
    _AUDITED["clip-l"] = (au.checks, set())
    _audit_verdict("clip-l", au)
    del enc
    monkeypatch.setattr(model, "VAE_FLASH_ATTN", False)
    hip = LcmHipPipeline(weights.synthetic_unet(), weights.synthetic_vae(), device="cuda:0")
    try:
        assert not hip.vae.flash_attn
        monkeypatch.setattr(hip.unet, "MAX_HOISTED_STEPS", 0)
        _audit_pass(hip, "sd15 B2 128px unfused", 2, 128, pe=_embeds(2, seed=70))
    finally:
        hip.close()
    torch.cuda.empty_cache()


def test_audit_sdxl_1024_passes_fp64(sdxl):
    """SDXL 1024x1024 without and with classifier-free guidance (the two SDXL passes of tools/make_plans.py)."""
    hip = sdxl["hip"]
    pe, pooled, tids = _sdxl_inputs()
    _audit_pass(hip, "sdxl B1 1024px", 1, 1024, pe=pe, added=(pooled, tids))
    g = torch.Generator().manual_seed(9)
    neg, neg_pooled = torch.randn(1, 77, 2048, generator=g).half(), torch.randn(1, 1280, generator=g).half()
    _audit_pass(hip, "sdxl B1 1024px cfg", 1, 1024, 5.0, pe=pe, added=(pooled, tids), negative_embeds=neg,
                negative_added=(neg_pooled, tids))
    # the SDXL text encoders: CLIP-L and OpenCLIP-bigG penultimate hidden states, bigG's pooled projection
    from launch_audit import Audit
    from sdlcm_amd.clip import CLIP_BIGG, CLIP_L, ClipTextHip, HashTokenizer, synthetic_clip
    ids = HashTokenizer()(["an astronaut riding a horse on the moon"])
    for cname, cfg, pooled in (("sdxl clip-l", CLIP_L, False), ("sdxl clip-bigg", CLIP_BIGG, True)):
        enc = ClipTextHip(synthetic_clip(cfg), cfg, device="cuda:0")
        with Audit() as au:
            out = enc.forward(ids, output="penultimate", pooled=pooled)
        assert (out[1].shape == (1, cfg["projection_dim"])) if pooled else (out.shape == (1, 77, cfg["hidden_size"]))
        _AUDITED[cname] = (au.checks, set())
        _audit_verdict(cname, au)
        del enc, out
        torch.cuda.empty_cache()
    from sdlcm_amd import lib
    _audit_report(lib.known_plans())


# ---- self-comparison checks (kept last) ----------------------------------------------------------------------------
def test_config4_sdxl_1024_30step_is_deterministic(sdxl):
    """The full configs[4] run (30 steps) on the GPU only: two graph replays of the same request give identical bytes (graph
    replay == eager pass is checked at 1024x1024 by the parity test above and at 512 by test_config1), another seed gives
    another image."""
    hip = sdxl["hip"]
    pe, pooled, tids = _sdxl_inputs()
    kw = dict(added=(pooled, tids))
    a = hip.generate(pe, [5], 1024, 1024, 30, 1.0, **kw)
    b = hip.generate(pe, [5], 1024, 1024, 30, 1.0, **kw)
    c = hip.generate(pe, [6], 1024, 1024, 30, 1.0, **kw)
    assert np.isfinite(a["latents"]).all() and a["rgb"].std() > 1.0
    assert np.array_equal(a["rgb"], b["rgb"]) and np.array_equal(a["latents"], b["latents"])
    assert not np.array_equal(a["rgb"], c["rgb"])


def test_config3_768_batch8_requests_match_solo(sd15):
    """configs[3] at its batch size (8) on the GPU only: each request of the batch is bit-identical to its solo run."""
    hip = sd15["hip"]
    B = 8
    pe = _embeds(B, seed=13)
    seeds = [900 + i for i in range(B)]
    out = hip.generate(pe, seeds, 768, 768, 2, 1.0)
    for i in (0, 5):
        solo = hip.generate(pe[i:i + 1], [seeds[i]], 768, 768, 2, 1.0)
        assert np.array_equal(solo["rgb"][0], out["rgb"][i])
