"""The launch audit (tests/launch_audit.py) on the geometry the tuned passes never have: sizes that are multiples of 8 but not of
64 (odd latent extents at every level, ragged key tiles, tiles straddling the images of a batch, no fused GroupNorm statistics,
4x8 patches), ControlNet-conditioned passes, multi-pass refinement and a tiled VAE decode with ragged last tiles.

Every pass runs eagerly with the shipped plan table under ``Audit()`` (every image of a batch checked): the first launch of each
distinct shape against its fp64 reference under the derived bound, what a launch must not write unchanged, every plan key the
pass launched checked.  The file ends with a reach check built from the recorded arguments of the checked launches."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
STEPS = 2
_AUDITED = {}                   # pass name -> Audit.checks (in launch order), for the reach check


def _embeds(B, D=768, seed=5):
    return torch.randn(B, 77, D, generator=torch.Generator().manual_seed(seed)).to(torch.float16)


def _verdict(name, au, extra=""):
    from launch_audit import failures, summary_line
    bad = failures(au.checks)
    print(f"[audit] {name}: {len(au.checks)} launches checked, {extra}{summary_line(au.checks)}")
    for c in bad:
        print(f"[audit] {name} FAIL {c}")
    _AUDITED[name] = au.checks
    assert au.checks and not bad, f"{name}: {len(bad)} launches outside their fp64 error bound, past the GroupNorm kappa tripwire " \
                                  f"or writing outside their output"


def _audit_pass(hip, name, B, width, height, guidance=1.0, steps=STEPS, **kw):
    """tests/test_configs_gpu.py::_audit_pass with width and height of their own: one eager pass under the audit; every plan key
    the pass launched was checked, no check failed."""
    from launch_audit import Audit
    plans = hip.lanes[0].plans
    before = set(plans)
    with Audit() as au:
        out = hip.generate(kw.pop("pe"), [300 + i for i in range(B)], width, height, steps, guidance, want_float=True, **kw)
    for k in set(plans) - before:          # the eager pass's plan is not kept (no graph was captured for it)
        plans.pop(k)
    torch.cuda.empty_cache()
    launched = au.record_keys()
    assert au.checked_keys() == launched, f"{name}: hook saw {len(au.checked_keys())} of {len(launched)} plan keys"
    _verdict(name, au, f"{len(launched)} plan keys ({sum(k in au.table for k in launched)} in the table), ")
    assert np.isfinite(out["latents"]).all()
    return au, out


@pytest.fixture(scope="module")
def nets():
    from sdlcm_amd import weights
    nocond = dict(time_cond_proj_dim=None)
    return dict(unet=weights.synthetic_unet(), vae=weights.synthetic_vae(), cn=weights.synthetic_controlnet(),
                nocond=nocond, unet_nocond=weights.synthetic_unet(nocond))


@pytest.fixture(scope="module")
def sd15(nets):
    from sdlcm_amd.pipeline import LcmHipPipeline
    hip = LcmHipPipeline(nets["unet"], nets["vae"], device=DEV)
    yield hip
    hip.close()


@pytest.fixture(scope="module")
def sd15_cfg(nets):
    """SD1.5 without the guidance embedding: guidance > 1 is classifier-free guidance on doubled rows."""
    from sdlcm_amd.pipeline import LcmHipPipeline
    hip = LcmHipPipeline(nets["unet_nocond"], nets["vae"], unet_cfg=nets["nocond"], device=DEV)
    yield hip
    hip.close()


def _hints(B, width, height, seed=0):
    """controlnet_reference.test_hint images with 0 and 255 in the corners (tests/test_controlnet_gpu.py::_hint_images)."""
    import controlnet_reference as cr
    imgs = np.stack([cr.test_hint(width, height, seed + b) for b in range(B)])
    imgs[0, :4, :4] = 0
    imgs[0, -4:, -4:] = 255
    return imgs


# ---- plain passes ----------------------------------------------------------------------------------------------------------
def test_audit_sd15_b1_520x392(sd15):
    """Latents 65x49 -> 33x25 -> 17x13 -> 9x7: odd at every level; Sk = 3185 (key-split, an odd tile count), 825, 221, 63;
    the VAE mid attention at S = 3185, d = 512."""
    _audit_pass(sd15, "sd15 B1 520x392", 1, 520, 392, pe=_embeds(1, seed=61))


def test_audit_sd15_b3_136x72(sd15):
    """Latents 17x9 -> 9x5 -> 5x3 -> 3x2, 153 / 45 / 15 / 6 rows per image: every tile straddles images, 4x8 patches."""
    _audit_pass(sd15, "sd15 B3 136x72", 3, 136, 72, pe=_embeds(3, seed=62))


def test_audit_sd15_one_side_odd(sd15):
    """Upsample targets odd in one direction only: latents 17x16 (height only) and 16x17 (width only) -- the passes above
    are odd in both at every level."""
    _audit_pass(sd15, "sd15 B1 128x136", 1, 128, 136, pe=_embeds(1, seed=63))
    _audit_pass(sd15, "sd15 B1 136x128", 1, 136, 128, pe=_embeds(1, seed=64))


def test_audit_sd15_cfg_b2_264x136(sd15_cfg):
    """Classifier-free guidance: doubled rows at 33x17 latents."""
    _audit_pass(sd15_cfg, "sd15 B2 264x136 cfg", 2, 264, 136, 5.0, pe=_embeds(2, seed=65), negative_embeds=_embeds(2, seed=66))


def test_audit_sdxl_style_b1_264x136():
    """The narrow SDXL-family configuration of tests/test_pipeline_gpu.py: d = 64 heads, text_time embedding, deeper
    transformers."""
    from sdlcm_amd import weights
    from sdlcm_amd.config import SDXL_UNET, unet_config, vae_config
    from sdlcm_amd.pipeline import LcmHipPipeline
    ucfg = unet_config(dict(SDXL_UNET, block_out_channels=(64, 128, 256), attention_head_dim=(1, 2, 4), cross_attention_dim=128,
                            transformer_layers_per_block=(1, 2, 2), addition_time_embed_dim=32,
                            projection_class_embeddings_input_dim=64 + 6 * 32))
    vcfg = vae_config(dict(block_out_channels=(64, 64, 128, 128), scaling_factor=0.13025))
    hip = LcmHipPipeline(weights.synthetic_state_dict(weights.unet_param_spec(ucfg), 0),
                         weights.synthetic_state_dict(weights.vae_param_spec(vcfg), 1), ucfg, vcfg, device=DEV)
    try:
        g = torch.Generator().manual_seed(8)
        pe = torch.randn(1, 77, 128, generator=g).half()
        pooled = torch.randn(1, 64, generator=g).half()
        tids = torch.tensor([[136.0, 264.0, 0, 0, 136.0, 264.0]])
        _audit_pass(hip, "sdxl-style B1 264x136", 1, 264, 136, pe=pe, added=(pooled, tids))
    finally:
        hip.close()
    torch.cuda.empty_cache()


def test_audit_sd2_b1_136x72(nets):
    """SD 2.x as tests/test_sd2_gpu.py audits it: v-prediction, linear projections, 64-wide heads."""
    from sdlcm_amd import weights
    from sdlcm_amd.config import SD2_UNET, unet_config
    from sdlcm_amd.pipeline import LcmHipPipeline
    from sdlcm_amd.scheduler import LCMSchedule, SD21_768_SCHEDULE
    hip = LcmHipPipeline(weights.synthetic_sd2_unet(), nets["vae"], unet_config(SD2_UNET), device=DEV,
                         schedule=LCMSchedule(**SD21_768_SCHEDULE))
    try:
        au, _ = _audit_pass(hip, "sd2 B1 136x72", 1, 136, 72, pe=_embeds(1, D=1024, seed=67))
        assert any(c["op"] == "scheduler_step" and c["args"]["pred"] == "v_prediction" for c in au.checks)
    finally:
        hip.close()
    torch.cuda.empty_cache()


def test_audit_clip_text_encoder():
    """The causal attention of a pass: the CLIP-L text encoder (S = 77: one ragged key tile)."""
    from launch_audit import Audit
    from sdlcm_amd.clip import CLIP_L, ClipTextHip, HashTokenizer, synthetic_clip
    enc = ClipTextHip(synthetic_clip(CLIP_L), CLIP_L, device=DEV)
    with Audit() as au:
        enc.forward(HashTokenizer()(["a red fox in the snow", "a lighthouse"]))
    _verdict("clip-l", au)
    del enc
    torch.cuda.empty_cache()


# ---- ControlNet ------------------------------------------------------------------------------------------------------------
def test_audit_controlnet_b1_520x392(sd15, nets):
    sd15.set_controlnet(nets["cn"])
    try:
        au, out = _audit_pass(sd15, "controlnet B1 520x392", 1, 520, 392, pe=_embeds(1, seed=68),
                              control=(_hints(1, 520, 392), 1.0))
    finally:
        sd15.set_controlnet(None)
    assert out["controlnet_evals"] == STEPS
    assert {"hint_conv_u8", "hint_conv", "conv3x3_c4_res"} <= {c["op"] for c in au.checks}


def test_audit_controlnet_cfg_b2_136x72(sd15_cfg, nets):
    """Classifier-free guidance: the ControlNet runs on both halves, the hint embedding is repeated for the negative half."""
    sd15_cfg.set_controlnet(nets["cn"])
    try:
        au, _ = _audit_pass(sd15_cfg, "controlnet B2 136x72 cfg", 2, 136, 72, 5.0, pe=_embeds(2, seed=69),
                            negative_embeds=_embeds(2, seed=70), control=(_hints(2, 136, 72, seed=3), 0.75))
    finally:
        sd15_cfg.set_controlnet(None)
    assert any(c["op"] == "conv3x3_c4_res" and c["args"]["B"] == 4 for c in au.checks)


# ---- multi-pass refinement -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("guidance", [1.0, 5.0])
def test_audit_refinement_b2_136x72(sd15, sd15_cfg, guidance):
    """passes = 2 at strength 0.5: the hand-over step between the passes (with guidance 5 the dup form: both halves of the
    [2B] state), then the same chain from cached x^0, which latents_renoise opens."""
    hip = sd15_cfg if guidance > 1 else sd15
    kw = dict(negative_embeds=_embeds(2, seed=72)) if guidance > 1 else {}
    tag = "refine B2 136x72" + (" cfg" if guidance > 1 else "")
    au, out = _audit_pass(hip, tag, 2, 136, 72, guidance, pe=_embeds(2, seed=71), strength=0.5, passes=2, **kw)
    ho = [c for c in au.checks if c["op"] == "scheduler_step_handover"]
    assert ho and all(c["args"]["dup"] == (guidance > 1) for c in ho)
    start = (0, [out["xk"][0, b].clone() for b in range(2)])
    au2, part = _audit_pass(hip, tag + " cached", 2, 136, 72, guidance, pe=_embeds(2, seed=71), strength=0.5, passes=2,
                            start=start, **kw)
    rn = [c for c in au2.checks if c["op"] == "latents_renoise"]
    assert rn and all(c["args"]["dup"] == (guidance > 1) for c in rn)
    assert np.array_equal(part["latents"], out["latents"]), "the chain from cached x^0 differs from the chain that ran through"


# ---- tiled VAE decode at an odd latent size --------------------------------------------------------------------------------
def test_audit_tiled_vae_decode_49x65(sd15):
    """sample_size 256 (as tests/test_pipeline_gpu.py::test_vae_tiled_decode_parity lowers it): 32-latent tiles at stride 24 over
    49x65 latents: ragged last tiles, the blend and place launches under the audit."""
    from launch_audit import Audit
    hip = sd15
    B, h, w = 1, 49, 65
    lat = (torch.randn(B, 4, h, w, generator=torch.Generator().manual_seed(73)) * 0.9).to(DEV)
    old = hip.vae.cfg.get("sample_size", 512)
    hip.vae.cfg["sample_size"] = 256
    try:
        with torch.inference_mode(), torch.cuda.stream(hip.stream), Audit() as au:
            rgb = torch.zeros(B, 8 * h, 8 * w, 3, dtype=torch.uint8, device=DEV)
            img = torch.zeros(B, 8 * h, 8 * w, 3, dtype=torch.float32, device=DEV)
            hip.vae.decode(lat, B, h, w, rgb, img_f32=img)
            hip.stream.synchronize()
    finally:
        hip.vae.cfg["sample_size"] = old
    assert au.checked_keys() == au.record_keys()
    _verdict("tiled vae 49x65", au)
    ops = {c["op"] for c in au.checks}
    assert {"vae_blend", "vae_place_tile"} <= ops, ops
    assert torch.isfinite(img).all() and float(img.std()) > 0
    torch.cuda.empty_cache()


# ---- reach (kept last) -----------------------------------------------------------------------------------------------------
def _reach(checks_by_pass):
    """item -> the passes whose checked launches reached it, from the recorded arguments (Audit.checks: args, stats_P, m_img,
    config)."""
    items = {}

    def hit(item, name):
        items.setdefault(item, set()).add(name)
    want = ["conv3x3 odd out_hw in height only", "conv3x3 odd out_hw in width only", "conv3x3 odd out_hw in both",
            "stride-2 conv odd H", "stride-2 conv odd W", "attention d=40 Sk<128 ragged", "attention d=80 Sk<128 ragged",
            "attention d=160 Sk<128 ragged", "attention 128<=Sk<1024 ragged", "attention 1024<=Sk<=4096 ragged",
            "attention d=512 ragged", "attention causal", "stats requested, P == 0, then a checked standalone groupnorm",
            "K partition > 1 part at rows per image % 64 != 0"]
    for name, checks in checks_by_pass.items():
        for i, c in enumerate(checks):
            a, op = c["args"], c["op"]
            hit("entry " + op, name)
            if op == "conv3x3" and a["ups"] == 1 and a["out_hw"] is not None:
                oh, ow = a["out_hw"][0] == 2 * a["H"] - 1, a["out_hw"][1] == 2 * a["W"] - 1
                if oh or ow:
                    hit("conv3x3 odd out_hw in " + ("both" if oh and ow else "height only" if oh else "width only"), name)
            if op == "conv3x3" and a["stride"] == 2:
                if a["H"] % 2:
                    hit("stride-2 conv odd H", name)
                if a["W"] % 2:
                    hit("stride-2 conv odd W", name)
            if op == "attention":
                if a["causal"]:
                    hit("attention causal", name)
                if a["Sk"] % 64:
                    if a["d"] == 512:
                        hit("attention d=512 ragged", name)
                    elif a["Sk"] < 128:
                        hit(f"attention d={a['d']} Sk<128 ragged", name)
                    elif a["Sk"] < 1024:
                        hit("attention 128<=Sk<1024 ragged", name)
                    elif a["Sk"] <= 4096:
                        hit("attention 1024<=Sk<=4096 ragged", name)
            if c.get("stats_P") == 0 and any(d["op"] == "groupnorm" for d in checks[i + 1:]):
                hit("stats requested, P == 0, then a checked standalone groupnorm", name)
            if c.get("config") is not None and c["config"][3] > 1 and c.get("m_img") and c["m_img"] % 64:
                hit("K partition > 1 part at rows per image % 64 != 0", name)
    return want, items


def test_reach_of_the_ragged_audits():
    """Across this file's passes every path the issue names was launched AND checked at least once, and every entry point the
    audit hooks or checks since this file exists was reached by a real pass."""
    from launch_audit import entry_table
    assert len(_AUDITED) >= 15, f"the audits of this file did not run before the reach check: {sorted(_AUDITED)}"
    want, items = _reach(_AUDITED)
    per = entry_table([c for checks in _AUDITED.values() for c in checks])
    for op in sorted(per):
        n, r, k = per[op]
        print(f"[audit] entry {op:>28}: {n:>5} launches checked, worst ratio {r:.3f}" + (f", worst kappa {k:.4g}" if k else ""))
    want += ["entry " + op for op in ("hint_conv_u8", "hint_conv", "conv3x3_c4_res", "latents_renoise", "scheduler_step_handover")]
    for item in want:
        print(f"[reach] {item}: {', '.join(sorted(items.get(item, ()))) or 'NOT REACHED'}")
    missing = [item for item in want if not items.get(item)]
    assert not missing, f"paths no audited pass of this file reached: {missing}"
