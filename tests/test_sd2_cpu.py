"""SD 2.x on the host side: the schedule's prediction type, the three step forms against diffusers' LCMScheduler.step in
float64, SD 2.x single files (OpenCLIP-H text tower, 64-wide heads, linear projections, v-prediction), SD 2.x diffusers
directories and the worker factory's routing.  Tiny checkpoints written on the fly; no GPU."""
import json
import os

import numpy as np
import pytest
import torch

import sd2_reference as R

SD2_TINY = dict(block_out_channels=(64, 128, 256, 256), cross_attention_dim=128, attention_head_dim=(1, 2, 4, 4),
                use_linear_projection=True, time_cond_proj_dim=None)
VCFG = dict(block_out_channels=(64, 64, 128, 128), norm_num_groups=32)
TOWER_W, TOWER_L = 128, 3


# ---- schedule ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pred", R.PREDS)
def test_schedule_reads_prediction_type_from_scheduler_config(tmp_path, pred):
    from sdlcm_amd.scheduler import LCMSchedule
    p = tmp_path / "scheduler_config.json"
    p.write_text(json.dumps({"_class_name": "DDIMScheduler", "beta_start": 0.00085, "beta_end": 0.012,
                             "beta_schedule": "scaled_linear", "set_alpha_to_one": False, "prediction_type": pred,
                             "clip_sample": False, "steps_offset": 1}))
    s = LCMSchedule.from_config_file(str(p))
    assert s.prediction_type == pred
    assert LCMSchedule(prediction_type=pred).prediction_type == pred
    assert LCMSchedule().prediction_type == "epsilon"


def test_schedule_rejects_unknown_prediction_type(tmp_path):
    from sdlcm_amd.scheduler import LCMSchedule
    with pytest.raises(ValueError, match="flow_prediction"):
        LCMSchedule(prediction_type="flow_prediction")
    p = tmp_path / "scheduler_config.json"
    p.write_text(json.dumps({"prediction_type": "x_start"}))
    with pytest.raises(ValueError, match="x_start"):
        LCMSchedule.from_config_file(str(p))


# ---- the step, every prediction type ------------------------------------------------------------------------------------
@pytest.mark.parametrize("pred", R.PREDS)
@pytest.mark.parametrize("cfg", [False, True])
def test_host_coefficients_agree_with_fp64_step(pred, cfg):
    """The kernel's form (six host coefficients) and diffusers' form (from alphas_cumprod) of LCMScheduler.step agree in
    float64 at every step of a 4-step SD 2.1-768 schedule, with and without CFG."""
    from sdlcm_amd.scheduler import LCMSchedule, SD21_768_SCHEDULE
    s = LCMSchedule(**SD21_768_SCHEDULE)
    ts = s.timesteps(4)
    rng = np.random.default_rng(3)
    m, mu, x, n = (rng.standard_normal((2, 4, 5, 7)) for _ in range(4))
    g = 7.5 if cfg else 1.0
    for i in range(len(ts)):
        coef, last = s.step_coefficients(ts, i)
        tp = int(ts[i]) if last else int(ts[i + 1])
        want = R.lcm_step_diffusers_fp64(m, x, n, s.alphas_cumprod, int(ts[i]), tp, pred, last, mu if cfg else None, g,
                                         s.final_alpha_cumprod)
        got, _ = R.lcm_step_coef_fp64(coef, last, m, x, n, pred, mu if cfg else None, g)
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


def test_step_forms_differ():
    """The three readings of one model output are different samples (so a dropped prediction type cannot pass unnoticed)."""
    from sdlcm_amd.scheduler import LCMSchedule, SD21_768_SCHEDULE
    s = LCMSchedule(**SD21_768_SCHEDULE)
    ts = s.timesteps(4)
    coef, last = s.step_coefficients(ts, 0)
    rng = np.random.default_rng(4)
    m, x, n = (rng.standard_normal((1, 4, 8, 8)) for _ in range(3))
    outs = [R.lcm_step_coef_fp64(coef, last, m, x, n, p)[0] for p in R.PREDS]
    for a in range(3):
        for b in range(a + 1, 3):
            assert np.abs(outs[a] - outs[b]).max() > 0.1


# ---- SD 2.x single file ------------------------------------------------------------------------------------------------
def _sd2_file(tmp_path, name="sd2.safetensors"):
    import tinytok
    from sdlcm_amd import weights
    from sdlcm_amd.config import unet_config
    ucfg = unet_config(SD2_TINY)
    usd = weights.synthetic_state_dict(weights.unet_param_spec(ucfg), 0)
    vsd = weights.synthetic_state_dict(weights.vae_param_spec(VCFG), 1)
    tower = R.openclip_tower(TOWER_W, TOWER_L, len(tinytok.vocab()))
    path = str(tmp_path / name)
    R.write_sd2_single_file(path, usd, vsd, tower)
    return path, usd, vsd, tower


def test_sd2_single_file_unet_and_vae(tmp_path, monkeypatch):
    from sdlcm_amd import weights
    monkeypatch.delenv("LCM_PREDICTION_TYPE", raising=False)
    path, usd, vsd, _ = _sd2_file(tmp_path)
    assert usd["down_blocks.0.attentions.0.proj_in.weight"].dim() == 2                 # linear proj_in in the file
    lu, lucfg, lv, lvcfg, lc, meta = weights.load_single_file(path, with_meta=True)
    assert lucfg["attention_head_dim"] == (1, 2, 4, 4)
    assert lucfg["use_linear_projection"] is True
    assert lucfg["cross_attention_dim"] == TOWER_W and lucfg["time_cond_proj_dim"] is None
    assert set(lu) == set(usd) and all(torch.equal(lu[k], usd[k]) for k in usd)
    assert set(lv) == set(vsd) and all(torch.equal(lv[k], vsd[k]) for k in vsd)
    assert meta["family"] == "sd2" and meta["prediction_type"] == "v_prediction"
    assert meta["text_config"]["hidden_act"] == "gelu"
    # the 5-tuple form is unchanged
    assert len(weights.load_single_file(path)) == 5


def test_sd2_single_file_prediction_type_override(tmp_path, monkeypatch):
    from sdlcm_amd import weights
    path = _sd2_file(tmp_path)[0]
    monkeypatch.setenv("LCM_PREDICTION_TYPE", "epsilon")
    assert weights.load_single_file(path, with_meta=True)[5]["prediction_type"] == "epsilon"
    monkeypatch.setenv("LCM_PREDICTION_TYPE", "v-pred")
    with pytest.raises(ValueError, match="v-pred"):
        weights.load_single_file(path, with_meta=True)


def test_sd2_single_file_text_tower_is_penultimate_block_plus_ln_final(tmp_path, monkeypatch):
    from sdlcm_amd import weights
    monkeypatch.delenv("LCM_PREDICTION_TYPE", raising=False)
    path, _, _, tower = _sd2_file(tmp_path)
    lc = weights.load_single_file(path)[4]
    layers = {int(k.split(".")[2]) for k in lc if k.startswith("encoder.layers.")}
    assert layers == set(range(TOWER_L - 1))                                           # resblocks 0 .. n-2
    assert "text_projection.weight" not in lc
    for i in range(TOWER_L - 1):
        w = tower[f"transformer.resblocks.{i}.attn.in_proj_weight"]
        b = tower[f"transformer.resblocks.{i}.attn.in_proj_bias"]
        for j, n in enumerate("qkv"):
            assert torch.equal(lc[f"encoder.layers.{i}.self_attn.{n}_proj.weight"], w[j * TOWER_W:(j + 1) * TOWER_W])
            assert torch.equal(lc[f"encoder.layers.{i}.self_attn.{n}_proj.bias"], b[j * TOWER_W:(j + 1) * TOWER_W])
    assert torch.equal(lc["final_layer_norm.weight"], tower["ln_final.weight"])
    # transformers.CLIPTextModel from the mapped dict == the OpenCLIP tower run to its penultimate block + ln_final
    from oracle.clip import clip_text_oracle
    cfg = dict(vocab_size=tower["token_embedding.weight"].shape[0], hidden_size=TOWER_W, intermediate_size=4 * TOWER_W,
               num_hidden_layers=TOWER_L - 1, num_attention_heads=TOWER_W // 64, max_position_embeddings=77,
               hidden_act="gelu", layer_norm_eps=1e-5)
    ids = torch.randint(0, cfg["vocab_size"] - 1, (2, 77), generator=torch.Generator().manual_seed(1))
    ids[:, -1] = cfg["vocab_size"] - 1
    got = clip_text_oracle(lc, cfg, ids)
    want = R.openclip_penultimate_ln_final(tower, ids, TOWER_W // 64)
    err = (got - want).abs().max().item()
    assert err < 1e-4 * max(1.0, want.abs().max().item()), err
    # quick_gelu (the CLIP-L default) would be a different encoder: the activation must come through
    wrong = clip_text_oracle(lc, dict(cfg, hidden_act="quick_gelu"), ids)
    assert (wrong - want).abs().max().item() > 100 * err


def test_sd2_single_file_prompt_encoder_config(tmp_path, monkeypatch):
    """HipPromptEncoder's single-file branch carries the loader's text config (gelu) into ClipTextHip; the tokenizer is the
    SD2 vocabulary from LCM_TOKENIZER_DIR (a real tower without one is refused)."""
    import tinytok
    from sdlcm_amd import weights
    from sdlcm_amd.prompt import HipPromptEncoder
    path = _sd2_file(tmp_path)[0]
    *_, lc, meta = weights.load_single_file(path, with_meta=True)
    monkeypatch.delenv("LCM_TOKENIZER_DIR", raising=False)
    with pytest.raises(RuntimeError, match="LCM_TOKENIZER_DIR"):
        HipPromptEncoder("cpu", None, lc, meta["text_config"])
    tinytok.write(str(tmp_path / "vocab" / "tokenizer"), pad="!")
    monkeypatch.setenv("LCM_TOKENIZER_DIR", str(tmp_path / "vocab"))
    pe = HipPromptEncoder("cpu", None, lc, meta["text_config"])
    c = pe.enc.cfg
    assert c["hidden_act"] == "gelu" and pe.enc.L == TOWER_L - 1 and pe.enc.D == TOWER_W and pe.enc.heads == TOWER_W // 64
    ids = pe.tokenize(["a cat"])
    assert ids.shape == (1, 77) and int(ids[0, -1]) == 0                          # SD2's own pad id ("!")


# ---- SD 2.x diffusers directory ----------------------------------------------------------------------------------------
def test_sd2_diffusers_dir(tmp_path):
    from safetensors.torch import save_file
    from sdlcm_amd import weights
    from sdlcm_amd.clip import ClipTextHip, load_clip_dir, synthetic_clip
    from sdlcm_amd.config import unet_config
    from sdlcm_amd.scheduler import LCMSchedule
    root = tmp_path / "sd21"
    for d in ("unet", "vae", "scheduler", "text_encoder"):
        (root / d).mkdir(parents=True)
    ucfg = unet_config(SD2_TINY)
    usd = weights.synthetic_state_dict(weights.unet_param_spec(ucfg), 0)
    vsd = weights.synthetic_state_dict(weights.vae_param_spec(VCFG), 1)
    save_file(usd, str(root / "unet" / "diffusion_pytorch_model.safetensors"))
    save_file(vsd, str(root / "vae" / "diffusion_pytorch_model.safetensors"))
    (root / "unet" / "config.json").write_text(json.dumps({
        "_class_name": "UNet2DConditionModel", "block_out_channels": list(SD2_TINY["block_out_channels"]),
        "attention_head_dim": list(SD2_TINY["attention_head_dim"]), "cross_attention_dim": TOWER_W, "use_linear_projection": True,
        "upcast_attention": True, "layers_per_block": 2, "in_channels": 4, "out_channels": 4, "norm_num_groups": 32,
        "down_block_types": ["CrossAttnDownBlock2D"] * 3 + ["DownBlock2D"]}))
    (root / "vae" / "config.json").write_text(json.dumps({"block_out_channels": list(VCFG["block_out_channels"]),
                                                          "norm_num_groups": 32, "scaling_factor": 0.18215}))
    (root / "scheduler" / "scheduler_config.json").write_text(json.dumps({
        "_class_name": "DDIMScheduler", "beta_start": 0.00085, "beta_end": 0.012, "beta_schedule": "scaled_linear",
        "set_alpha_to_one": False, "prediction_type": "v_prediction", "steps_offset": 1}))
    (root / "model_index.json").write_text(json.dumps({"_class_name": "StableDiffusionPipeline"}))
    tcfg = dict(vocab_size=65, hidden_size=TOWER_W, intermediate_size=4 * TOWER_W, num_hidden_layers=2,
                num_attention_heads=TOWER_W // 64, max_position_embeddings=77, hidden_act="gelu", layer_norm_eps=1e-5)
    csd = synthetic_clip(tcfg)
    save_file({"text_model." + k: v for k, v in csd.items()}, str(root / "text_encoder" / "model.safetensors"))
    (root / "text_encoder" / "config.json").write_text(json.dumps(dict(tcfg, architectures=["CLIPTextModel"], projection_dim=512)))

    lu, lucfg, lv, _ = weights.load_diffusers_dir(str(root))
    assert lucfg["attention_head_dim"] == (1, 2, 4, 4) and lucfg["use_linear_projection"] is True
    assert lucfg["upcast_attention"] is True and lucfg["time_cond_proj_dim"] is None
    assert set(lu) == set(usd) and all(torch.equal(lu[k], usd[k]) for k in usd)
    s = LCMSchedule.from_config_file(str(root / "scheduler" / "scheduler_config.json"))
    assert s.prediction_type == "v_prediction" and s.final_alpha_cumprod == float(s.alphas_cumprod[0])
    sd, cfg = load_clip_dir(str(root / "text_encoder"))
    enc = ClipTextHip(sd, cfg, device="cpu")                 # construction only: weights placed, config resolved
    assert enc.cfg["hidden_act"] == "gelu" and enc.L == 2 and enc.heads == 2 and enc.act == 3


# ---- constants, factory ------------------------------------------------------------------------------------------------
def test_sd2_constants():
    from sdlcm_amd import weights
    from sdlcm_amd.clip import CLIP_H, clip_param_spec
    from sdlcm_amd.config import SD2_UNET, heads_at, unet_config
    c = unet_config(SD2_UNET)
    assert [heads_at(c, i) for i in range(4)] == [5, 10, 20, 20]
    assert all(ch // heads_at(c, i) == 64 for i, ch in enumerate(c["block_out_channels"]))
    assert c["cross_attention_dim"] == 1024 and c["use_linear_projection"] and not c["time_cond_proj_dim"]
    assert round(weights.count_params(weights.unet_param_spec(c)) / 1e6) == 866                # SD 2.x UNet: 865.9 M
    assert CLIP_H["hidden_size"] == 1024 and CLIP_H["num_hidden_layers"] == 23 and CLIP_H["hidden_act"] == "gelu"
    assert CLIP_H["hidden_size"] // CLIP_H["num_attention_heads"] == 64 and CLIP_H["intermediate_size"] == 4096
    assert round(weights.count_params(clip_param_spec(CLIP_H)) / 1e6) == 340


def test_factory_routes_sd2(tmp_path, monkeypatch):
    from safetensors.torch import save_file
    from sdlcm_amd.backends import worker_factory
    save_file({"model.diffusion_model.input_blocks.1.1.transformer_blocks.0.attn2.to_k.weight": torch.zeros(320, 1024, dtype=torch.float16)},
              str(tmp_path / "v2-1_768.safetensors"))
    monkeypatch.setenv("MODEL_ROOT", str(tmp_path))
    monkeypatch.setenv("MODEL", "v2-1_768.safetensors")
    assert worker_factory.detect_worker_type() == "sd15"
    monkeypatch.setenv("MODEL", "synthetic-sd2")
    assert worker_factory.detect_worker_type() == "sd15"


def test_sd15_single_file_loads_as_before(tmp_path, monkeypatch):
    from sdlcm_amd import weights
    from sdlcm_amd.clip import synthetic_clip
    from sdlcm_amd.config import unet_config
    monkeypatch.delenv("LCM_PREDICTION_TYPE", raising=False)
    ucfg = unet_config(dict(block_out_channels=(64, 128, 192, 192)))
    usd = weights.synthetic_state_dict(weights.unet_param_spec(ucfg), 0)
    vsd = weights.synthetic_state_dict(weights.vae_param_spec(VCFG), 1)
    csd = synthetic_clip(dict(num_hidden_layers=2, hidden_size=128, intermediate_size=256, num_attention_heads=2, vocab_size=1000))
    raw = R.ldm_unet_names(usd)
    raw.update(R.ldm_vae_names(vsd))
    raw.update({"cond_stage_model.transformer.text_model." + k: v for k, v in csd.items()})
    from safetensors.torch import save_file
    path = str(tmp_path / "sd15.safetensors")
    save_file({k: v.contiguous() for k, v in raw.items()}, path)
    lu, lucfg, lv, lvcfg, lc, meta = weights.load_single_file(path, with_meta=True)
    assert lucfg == ucfg                                             # 8 heads, 1x1-conv projections, cond_proj 256
    assert meta == dict(family="sd15", prediction_type="epsilon", text_config={})
    assert set(lc) == set(csd) and all(torch.equal(lc[k], csd[k]) for k in csd)
    plain = weights.load_single_file(path)
    assert len(plain) == 5 and plain[1] == lucfg
