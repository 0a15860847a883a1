"""Host side of ControlNet-conditioned generation: the parameter spec, synthetic weights and the loader, the CPU reference's own
sanity (tests/controlnet_reference.py), request parsing, batch keys and the error cases.  No GPU."""
import io
import json
import os
from dataclasses import dataclass, field
from typing import Optional

import numpy as np
import pytest
import torch

from sdlcm_amd import weights
from sdlcm_amd.backends import controlnet as cnb
from sdlcm_amd.config import SD2_UNET, SDXL_UNET, unet_config

import controlnet_reference as cr

TOL = 1e-2          # the parity tolerance of the GPU tests


# ---- spec, synthetic weights, loader ----------------------------------------------------------------------------------------
def test_spec_is_the_sd15_controlnet():
    spec = list(weights.controlnet_param_spec())
    names = [n for n, _, _ in spec]
    assert len(names) == len(set(names))
    assert weights.count_params(spec) == 361_279_120                 # diffusers' ControlNetModel for SD1.5
    shapes = {n: s for n, s, _ in spec}
    e = "controlnet_cond_embedding"
    assert shapes[e + ".conv_in.weight"] == (16, 3, 3, 3)
    assert [shapes[f"{e}.blocks.{i}.weight"][:2] for i in range(6)] == [(16, 16), (32, 16), (32, 32), (96, 32), (96, 96), (256, 96)]
    assert shapes[e + ".conv_out.weight"] == (320, 256, 3, 3)
    assert [shapes[f"controlnet_down_blocks.{i}.weight"][0] for i in range(12)] == [320] * 4 + [640] * 3 + [1280] * 5
    assert shapes["controlnet_mid_block.weight"] == (1280, 1280, 1, 1)
    assert "time_embedding.cond_proj.weight" not in shapes and not any(n.startswith("up_blocks") for n in names)
    # the encoder half carries the UNet's own names and shapes
    ushapes = {n: s for n, s, _ in weights.unet_param_spec()}
    for n, s in shapes.items():
        if n.startswith(("down_blocks.", "mid_block.", "conv_in.", "time_embedding.linear")):
            assert ushapes[n] == s, n


def test_synthetic_weights_are_seeded_and_the_zero_convs_are_not_zero():
    a, b = weights.synthetic_controlnet(), weights.synthetic_controlnet()
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert not torch.equal(a["conv_in.weight"], weights.synthetic_controlnet(seed=8)["conv_in.weight"])
    z = weights.synthetic_controlnet(zero=True)
    for k in a:
        if k.startswith(("controlnet_down_blocks", "controlnet_mid_block")):
            assert float(a[k].float().abs().max()) > 0 and float(z[k].float().abs().max()) == 0
        else:
            assert torch.equal(a[k], z[k]), k
    w = a["controlnet_down_blocks.0.weight"].float()
    assert abs(float(w.std()) - weights.SYNTHETIC_ZERO_CONV_SCALE * 320 ** -0.5) < 0.05 * 320 ** -0.5


def _small_cfg():
    return dict(block_out_channels=(32, 64, 64, 64), cross_attention_dim=32, attention_head_dim=4)


def _write_dir(tmp_path, sd, cfg_json):
    from safetensors.torch import save_file
    d = tmp_path / "cn"
    d.mkdir()
    save_file({k: v.contiguous() for k, v in sd.items()}, str(d / "diffusion_pytorch_model.safetensors"))
    (d / "config.json").write_text(json.dumps(cfg_json))
    return str(d)


def test_loader_round_trip_directory_and_single_file(tmp_path):
    from safetensors.torch import save_file
    ucfg = unet_config(_small_cfg())
    ccfg = weights.controlnet_config(ucfg)
    sd = weights.synthetic_controlnet(ccfg)
    j = dict(block_out_channels=[32, 64, 64, 64], cross_attention_dim=32, attention_head_dim=4, layers_per_block=2,
             conditioning_embedding_out_channels=[16, 32, 96, 256],
             down_block_types=["CrossAttnDownBlock2D"] * 3 + ["DownBlock2D"])
    got, gcfg = weights.load_controlnet(_write_dir(tmp_path, sd, j))
    assert set(got) >= set(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    weights.check_controlnet_matches(gcfg, ucfg)
    f = tmp_path / "cn.safetensors"
    save_file({k: v.contiguous() for k, v in sd.items()}, str(f))
    got2, gcfg2 = weights.load_controlnet(str(f))
    assert all(torch.equal(got2[k], sd[k]) for k in sd)
    assert tuple(gcfg2["block_out_channels"]) == (32, 64, 64, 64) and gcfg2["cross_attention_dim"] == 32
    # a missing tensor is named
    bad = dict(sd)
    del bad["controlnet_mid_block.bias"]
    f2 = tmp_path / "bad.safetensors"
    save_file({k: v.contiguous() for k, v in bad.items()}, str(f2))
    with pytest.raises(RuntimeError, match="controlnet_mid_block.bias"):
        weights.load_controlnet(str(f2))


@pytest.mark.parametrize("name", ["cn.ckpt", "cn.bin", "cn.pt"])
def test_pickles_are_refused(tmp_path, name):
    p = tmp_path / name
    p.write_bytes(b"\x80\x04not really a pickle")
    with pytest.raises(RuntimeError, match="safetensors"):
        weights.load_controlnet(str(p))
    d = tmp_path / "dir"
    d.mkdir()
    (d / "config.json").write_text("{}")
    (d / "diffusion_pytorch_model.bin").write_bytes(b"x")
    with pytest.raises(RuntimeError, match="pickled"):
        weights.load_controlnet(str(d))


def test_mismatched_configs_raise_naming_both_values():
    sd15 = unet_config()
    with pytest.raises(RuntimeError, match=r"cross_attention_dim is 1024 in the ControlNet and 768 in the UNet"):
        weights.check_controlnet_matches(weights.controlnet_config(SD2_UNET), sd15)
    with pytest.raises(RuntimeError, match=r"block_out_channels is \(32, 64, 64, 64\) in the ControlNet and \(320, 640, 1280, 1280\)"):
        weights.check_controlnet_matches(weights.controlnet_config(_small_cfg()), sd15)
    with pytest.raises(RuntimeError, match="layers_per_block is 1 in the ControlNet and 2 in the UNet"):
        weights.check_controlnet_matches(weights.controlnet_config(dict(layers_per_block=1)), sd15)
    with pytest.raises(RuntimeError, match="attention_head_dim"):
        weights.check_controlnet_matches(weights.controlnet_config(dict(attention_head_dim=(5, 10, 20, 20))), sd15)
    with pytest.raises(RuntimeError, match="conditioning_embedding_out_channels"):
        weights.check_controlnet_matches(weights.controlnet_config(None, dict(conditioning_embedding_out_channels=(16, 32, 64, 128))), sd15)
    with pytest.raises(RuntimeError, match="SDXL"):
        weights.check_controlnet_matches(weights.controlnet_config(), unet_config(SDXL_UNET))
    weights.check_controlnet_matches(weights.controlnet_config(SD2_UNET), unet_config(SD2_UNET))
    weights.check_controlnet_matches(weights.controlnet_config(), sd15)
    weights.check_controlnet_matches(weights.controlnet_config(dict(attention_head_dim=(8, 8, 8, 8))), sd15)     # one layout, two spellings


def test_sdxl_controlnet_directory_is_refused(tmp_path):
    d = tmp_path / "xl"
    d.mkdir()
    from safetensors.torch import save_file
    save_file({"add_embedding.linear_1.weight": torch.zeros(4, 4)}, str(d / "diffusion_pytorch_model.safetensors"))
    (d / "config.json").write_text(json.dumps(dict(addition_embed_type="text_time", addition_time_embed_dim=256)))
    with pytest.raises(RuntimeError, match="SDXL"):
        weights.load_controlnet(str(d))


# ---- the CPU reference itself ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nets():
    return dict(unet=weights.synthetic_unet(), vae=weights.synthetic_vae(), cn=weights.synthetic_controlnet(),
                cn_zero=weights.synthetic_controlnet(zero=True))


@pytest.fixture(scope="module")
def pe():
    return torch.randn(1, 77, 768, generator=torch.Generator().manual_seed(5)).to(torch.float16).float()


def test_reference_with_all_zero_zero_convs_is_the_plain_oracle_exactly(nets, pe):
    from oracle.pipeline import LCMPipelineOracle
    plain = LCMPipelineOracle(nets["unet"], nets["vae"])(pe, 64, 64, 4, 1.0, 42)
    z = cr.ControlNetPipelineOracle(nets["unet"], nets["vae"], nets["cn_zero"])(pe, 64, 64, 4, 1.0, 42, cr.test_hint(64, 64))
    assert np.array_equal(z["image"], plain["image"]) and np.array_equal(z["latents"], plain["latents"])
    # ... and without a hint it IS the plain oracle
    n = cr.ControlNetPipelineOracle(nets["unet"], nets["vae"], nets["cn"])(pe, 64, 64, 4, 1.0, 42, None)
    assert np.array_equal(n["image"], plain["image"])


@pytest.mark.parametrize("size", [64, 128, 256])
def test_the_hint_moves_the_picture_by_ten_tolerances(nets, pe, size):
    """What makes the GPU parity test mean something: with the standard synthetic ControlNet and the test hint the decoded
    [0, 1] image differs from the plain oracle's by a mean |d| of at least 10 x 1e-2.  Measured while choosing
    weights.SYNTHETIC_ZERO_CONV_SCALE (4 steps, seed 42): scale 0.5 -> 0.0561 / 0.0600 / 0.0600 at 64^2 / 128^2 / 256^2 (too
    little), 1.0 -> 0.0992 / 0.1003 / 0.1011 (no margin), 1.5 -> 0.1247 / 0.1234 / 0.1246 (chosen; max |d| 0.82 / 0.73 / 0.92)."""
    from oracle.pipeline import LCMPipelineOracle
    a = LCMPipelineOracle(nets["unet"], nets["vae"])(pe, size, size, 4, 1.0, 42)["image"]
    b = cr.ControlNetPipelineOracle(nets["unet"], nets["vae"], nets["cn"])(pe, size, size, 4, 1.0, 42, cr.test_hint(size, size))["image"]
    d = float(np.abs(np.clip(a / 2 + 0.5, 0, 1) - np.clip(b / 2 + 0.5, 0, 1)).mean())
    print(f"mean |d| of the hint's effect at {size}x{size}: {d:.4f}")
    assert d >= 10 * TOL, d


def test_reference_scale_is_linear_in_the_residuals(nets):
    cn = cr.ControlNetOracle(nets["cn"])
    g = torch.Generator().manual_seed(3)
    lat, ehs = torch.randn(1, 4, 8, 8, generator=g), torch.randn(1, 77, 768, generator=g)
    hint = cr.test_hint(64, 64)[None]
    d1, m1 = cn.forward(lat, 999, ehs, hint, 1.0)
    d2, m2 = cn.forward(lat, 999, ehs, hint, 0.5)
    assert len(d1) == 12 and [tuple(t.shape[1:]) for t in d1] == [(320, 8, 8)] * 3 + [(320, 4, 4)] + [(640, 4, 4)] * 2 + \
        [(640, 2, 2)] + [(1280, 2, 2)] * 2 + [(1280, 1, 1)] * 3
    assert all(torch.allclose(a * 0.5, b, atol=1e-6) for a, b in zip(d1 + [m1], d2 + [m2]))
    assert cn.embed_hint(cr.test_hint(72, 40)[None].transpose(0, 2, 1, 3)).shape == (1, 320, 9, 5)      # odd latent extents


# ---- request parsing, batch keys, errors -----------------------------------------------------------------------------------
@dataclass
class _Style:
    style: Optional[str] = None
    level: int = 0


@dataclass
class _Req:
    prompt: str = "p"
    size: str = "64x64"
    num_inference_steps: int = 4
    guidance_scale: float = 1.0
    seed: Optional[int] = 1
    style_lora: _Style = field(default_factory=_Style)


def _req(**extra):
    r = _Req()
    for k, v in extra.items():
        setattr(r, k, v)
    return r


def _png(arr):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(arr, "RGB").save(b, "PNG")
    return b.getvalue()


def test_parse_control_inputs():
    from PIL import Image
    hint = cr.test_hint(64, 64)
    assert cnb.parse_control(_req()) is None and cnb.parse_control(_req(controlnet_image=None, controlnet_conditioning_scale=0.5)) is None
    for src in (hint, _png(hint), Image.fromarray(hint, "RGB"), bytearray(_png(hint))):
        s, h = cnb.parse_control(_req(controlnet_image=src))
        assert s == 1.0 and h.dtype == np.uint8 and np.array_equal(h, hint)
    b = io.BytesIO()
    Image.fromarray(hint, "RGB").save(b, "JPEG", quality=100, subsampling=0)
    s, h = cnb.parse_control(_req(controlnet_image=b.getvalue(), controlnet_conditioning_scale="0.5"))
    assert s == 0.5 and h.shape == (64, 64, 3) and np.abs(h.astype(int) - hint.astype(int)).mean() < 8
    g = np.asarray(Image.fromarray(hint[..., 0], "L"))
    s, h = cnb.parse_control(_req(controlnet_image=_png(hint)[:0] + _gray_png(g)))
    assert h.shape == (64, 64, 3) and np.array_equal(h[..., 0], g) and np.array_equal(h[..., 1], g)     # grey -> RGB
    r = _req(controlnet_image=_png(hint))
    assert cnb.parse_control(r)[1] is cnb.parse_control(r)[1]                                      # decoded once per request


def _gray_png(g):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(g, "L").save(b, "PNG")
    return b.getvalue()


@pytest.mark.parametrize("extra,word", [
    (dict(controlnet_image=b"not an image"), "controlnet_image"), (dict(controlnet_image=b""), "controlnet_image"),
    (dict(controlnet_image=np.zeros((8, 8), np.uint8)), "controlnet_image"),
    (dict(controlnet_image=np.zeros((8, 8, 3), np.float32)), "controlnet_image"), (dict(controlnet_image=12), "controlnet_image"),
    (dict(controlnet_image=np.zeros((8, 8, 3), np.uint8), controlnet_conditioning_scale=2.01), "controlnet_conditioning_scale"),
    (dict(controlnet_image=np.zeros((8, 8, 3), np.uint8), controlnet_conditioning_scale=-0.1), "controlnet_conditioning_scale"),
    (dict(controlnet_image=np.zeros((8, 8, 3), np.uint8), controlnet_conditioning_scale=float("nan")), "controlnet_conditioning_scale"),
    (dict(controlnet_image=np.zeros((8, 8, 3), np.uint8), controlnet_conditioning_scale="lots"), "controlnet_conditioning_scale")])
def test_validation_errors_name_the_field(extra, word):
    with pytest.raises(RuntimeError, match=word):
        cnb.parse_control(_req(**extra))


def test_hint_is_resized_to_width_by_height_with_lanczos():
    from PIL import Image
    hint = cr.test_hint(96, 48)                       # H = 48, W = 96
    assert cnb.fit_hint(hint, 96, 48) is hint
    out = cnb.fit_hint(hint, 128, 64)
    assert out.shape == (64, 128, 3)
    assert np.array_equal(out, np.asarray(Image.fromarray(hint, "RGB").resize((128, 64), Image.LANCZOS)))


def test_batch_keys():
    from sdlcm_amd.backends.hip_worker import HipLcmWorker
    hint = cr.test_hint(64, 64)
    plain = (64, 64, 4, 1.0, None, 0)
    assert HipLcmWorker._job_key(_req()) == plain
    assert HipLcmWorker._job_key(_req(controlnet_conditioning_scale=0.5)) == plain          # a scale without a hint is a plain request
    k1 = HipLcmWorker._job_key(_req(controlnet_image=hint))
    k2 = HipLcmWorker._job_key(_req(controlnet_image=cr.test_hint(64, 64, 3)))
    k3 = HipLcmWorker._job_key(_req(controlnet_image=hint, controlnet_conditioning_scale=0.5))
    assert k1 == plain + ("controlnet", 1.0) == k2 and k3 == plain + ("controlnet", 0.5)      # the hint is per image, not in the key
    assert cnb.is_control_key(k1) and not cnb.is_control_key(plain)
    assert not cnb.is_control_key(HipLcmWorker._job_key(_req(denoise_strength=0.5, pass_number=2)))
    with pytest.raises(RuntimeError, match="refinement"):
        HipLcmWorker._job_key(_req(controlnet_image=hint, denoise_strength=0.5))
    with pytest.raises(RuntimeError, match="refinement"):
        HipLcmWorker._job_key(_req(controlnet_image=hint, pass_number=2))
    assert HipLcmWorker._job_key(_req(controlnet_image=hint, denoise_strength=1.0, pass_number=1)) == k1
    with pytest.raises(RuntimeError, match="controlnet_conditioning_scale"):
        HipLcmWorker._job_key(_req(controlnet_image=hint, controlnet_conditioning_scale=3))


def test_controlnet_jobs_coalesce_among_themselves_only():
    import threading
    from sdlcm_amd.backends.batching import MicroBatcher
    from sdlcm_amd.backends.hip_worker import HipLcmWorker
    gate, seen = threading.Event(), []

    def run(key, items):
        gate.wait(10)
        seen.append((key, list(items)))
        return items
    mb = MicroBatcher(run, max_batch=8)
    try:
        h = cr.test_hint(64, 64)
        reqs = [_req(), _req(controlnet_image=h), _req(), _req(controlnet_image=cr.test_hint(64, 64, 1)),
                _req(controlnet_image=h, controlnet_conditioning_scale=0.5), _req(denoise_strength=0.5)]
        futs = [mb.submit(HipLcmWorker._job_key(r), i) for i, r in enumerate(reqs)]
        gate.set()
        assert [f.result(10) for f in futs] == list(range(6))
        for key, items in seen:
            assert {HipLcmWorker._job_key(reqs[i]) for i in items} == {key}
        assert any(items == [1, 3] for _, items in seen)            # same scale, different hints: one pass
        assert any(items == [4] for _, items in seen)               # another scale: a pass of its own
    finally:
        mb.close()


class _Pipe:
    def __init__(self):
        from sdlcm_amd.scheduler import LCMSchedule
        self.controlnet, self.sched, self.calls = None, LCMSchedule(), []

        class _U:
            cfg = unet_config()
        self.unet = _U()

    def set_controlnet(self, sd, cfg):
        weights.check_controlnet_matches(cfg, self.unet.cfg)
        self.controlnet = ("loaded", len(sd))


def _stub_worker(cls, src=None, loader=None, monkeypatch=None):
    from sdlcm_amd.backends import hip_worker
    eng = hip_worker._Engine(cls)
    eng.pipe, eng.controlnet_src, eng.synthetic_model = _Pipe(), src, True
    w = object.__new__(cls)
    w.worker_id, w._engine = 0, eng
    return w, eng


def test_worker_errors_and_lazy_load_with_a_stubbed_engine(monkeypatch):
    from sdlcm_amd.backends.hip_worker import HipLcmSDXLWorker, HipLcmWorker
    hint = cr.test_hint(64, 64)
    loads = []
    monkeypatch.setattr(cnb, "load_controlnet_source",
                        lambda src, ucfg, synth: (loads.append(src), ({"w": 0}, weights.controlnet_config(ucfg)))[1])
    # no ControlNet configured: the job that carries the hint raises, a plain one is prepared as ever
    w, eng = _stub_worker(HipLcmWorker)
    r = _req(controlnet_image=hint)
    with pytest.raises(RuntimeError, match="no ControlNet is loaded"):
        w._prepare(r, w._job_key(r))
    assert len(w._prepare(_req(), w._job_key(_req()))) == 3 and not loads
    # configured: loaded on the first request that needs it, once; the hint travels with the item, resized to the request
    w, eng = _stub_worker(HipLcmWorker, "synthetic")
    assert len(w._prepare(_req(), w._job_key(_req()))) == 3 and eng.pipe.controlnet is None and not loads
    r = _req(controlnet_image=cr.test_hint(32, 32), size="64x64")
    item = w._prepare(r, w._job_key(r))
    assert loads == ["synthetic"] and eng.pipe.controlnet is not None
    assert len(item) == 4 and item[3].shape == (64, 64, 3) and item[3].dtype == np.uint8 and item[1] == 1
    assert len(item[2][1]) == 3                                          # the plain request's RNG stream: steps - 1 step noises
    w._prepare(r, w._job_key(r))
    assert loads == ["synthetic"]
    # SDXL: refused for the job
    w, eng = _stub_worker(HipLcmSDXLWorker, "synthetic")
    with pytest.raises(RuntimeError, match="SDXL"):
        w._prepare(r, w._job_key(r))
    # a ControlNet that does not fit the UNet raises when it is constructed, naming both values
    monkeypatch.setattr(cnb, "load_controlnet_source", lambda src, ucfg, synth: ({"w": 0}, weights.controlnet_config(SD2_UNET)))
    w, eng = _stub_worker(HipLcmWorker, "/some/dir")
    with pytest.raises(RuntimeError, match="1024 in the ControlNet and 768 in the UNet"):
        w._prepare(r, w._job_key(r))
    assert "controlnet_evals" in eng.stats


def test_controlnet_source():
    with pytest.raises(RuntimeError, match="synthetic"):
        cnb.load_controlnet_source("synthetic", unet_config(), False)
    with pytest.raises(RuntimeError, match="no such file"):
        cnb.load_controlnet_source("/nonexistent/controlnet", unet_config(), False)
