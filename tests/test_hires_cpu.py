"""Host side of hires fix (enable_hr / hr_scale / hr_resize_x,y / hr_second_pass_steps / denoising_strength / hr_upscaler): the
exact-coordinate reference of the three latent upscalers against torch, request parsing and validation, batch keys and the draw
order.  No GPU."""
from dataclasses import dataclass, field
from typing import Optional

import numpy as np
import pytest
import torch

from sdlcm_amd.backends import hires
from sdlcm_amd.backends.hip_worker import HipLcmSDXLWorker, HipLcmWorker
from sdlcm_amd.scheduler import LCMSchedule

import hires_reference as hr


@dataclass
class _Style:
    style: Optional[str] = None
    level: int = 0


@dataclass
class _Req:
    prompt: str = "p"
    size: str = "512x512"
    num_inference_steps: int = 4
    guidance_scale: float = 1.0
    seed: Optional[int] = 1
    style_lora: _Style = field(default_factory=_Style)


def _req(**extra):
    r = _Req()
    for k, v in extra.items():
        setattr(r, k, v)
    return r


# ---- the reference against torch -------------------------------------------------------------------------------------------
# Nearest-exact against torch needs shape pairs without an exact integer tie: torch evaluates floor((d + 0.5) * scale) with a
# rounded scale, which may fall on either side of a coordinate that is exactly an integer.  Of the GPU tests' pairs, 8 -> 12 and
# 64 -> 96 (ratio 2/3, like 6 -> 9) tie at d = 1, 4, 7, ...; they are compared for the other two modes, and for nearest-exact
# test_nearest_exact_at_ties_takes_the_exact_floor pins what the reference (and the kernel) do there.
NEAREST_TORCH_SHAPES = tuple(s for s in hr.SHAPES if not (hr.nearest_ties(s[0][0], s[1][0]) or hr.nearest_ties(s[0][1], s[1][1]))) \
    + (((7, 11), (9, 13)), ((15, 17), (24, 40)))


def _x(h, w, seed=0, B=2):
    return torch.randn(B, 4, h, w, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).numpy() * 1.3


def test_nearest_shape_list_has_no_exact_integer_tie():
    assert len(NEAREST_TORCH_SHAPES) >= 4
    for (h, w), (H, W) in NEAREST_TORCH_SHAPES:
        assert hr.nearest_ties(h, H) == [] and hr.nearest_ties(w, W) == [], ((h, w), (H, W))
    assert hr.nearest_ties(6, 9) == [1, 4, 7] and hr.nearest_ties(8, 12)[0] == 1          # the ties the list must avoid


@pytest.mark.parametrize("shape", NEAREST_TORCH_SHAPES)
def test_nearest_exact_reference_equals_torch(shape):
    (h, w), (H, W) = shape
    x = _x(h, w)
    assert np.array_equal(hr.upscale_fp64(x, H, W, hr.NEAREST_EXACT), hr.torch_upscale(x, H, W, hr.NEAREST_EXACT))


def test_nearest_exact_reference_equals_torch_on_every_gpu_pair():
    """All six pairs of the GPU operator test, the two with ties included: torch's fp32 scale for 2/3 rounds up, so at a tie its
    floor lands where the exact rational's does and the comparison holds there too."""
    for (h, w), (H, W) in hr.SHAPES:
        x = _x(h, w, seed=2)
        assert np.array_equal(hr.upscale_fp64(x, H, W, hr.NEAREST_EXACT), hr.torch_upscale(x, H, W, hr.NEAREST_EXACT)), ((h, w), (H, W))


@pytest.mark.parametrize("mode", [hr.BILINEAR, hr.BICUBIC])
@pytest.mark.parametrize("shape", hr.SHAPES + (((7, 10), (9, 13)), ((5, 5), (5, 5)), ((4, 6), (16, 6))))
def test_interpolating_reference_agrees_with_torch(shape, mode):
    (h, w), (H, W) = shape
    x = _x(h, w, seed=3)
    e = np.abs(hr.upscale_fp64(x, H, W, mode) - hr.torch_upscale(x, H, W, mode)).max()
    assert e <= 1e-12, e


def test_nearest_exact_at_ties_takes_the_exact_floor():
    """(d + 0.5) 8 / 12 = 1 exactly at d = 1: the source index is 1, from integers -- whatever a rounded 8 / 12 would give."""
    for n_in, n_out in ((8, 12), (64, 96), (6, 9)):
        idx, _ = hr.axis_taps(hr.NEAREST_EXACT, n_in, n_out)
        for d in hr.nearest_ties(n_in, n_out):
            assert idx[d, 0] == (2 * d + 1) * n_in // (2 * n_out) == ((2 * d + 1) * n_in) / (2 * n_out)


def test_identity_size_is_the_identity_and_weights_sum_to_one():
    x = _x(5, 7, seed=4)
    for mode in hr.MODES:
        assert np.array_equal(hr.upscale_fp64(x, 5, 7, mode), x)
        for n_in, n_out in ((8, 12), (9, 17), (3, 12), (1, 3)):
            idx, wt = hr.axis_taps(mode, n_in, n_out)
            assert np.abs(wt.sum(1) - 1).max() < 1e-15 and idx.min() >= 0 and idx.max() <= n_in - 1
            assert np.abs(wt).sum(1).max() <= 1.375 + 1e-15


def test_renoise_reference():
    x, n = _x(3, 2, seed=5, B=1), _x(12, 8, seed=6, B=1)
    up, lat = hr.upscale_renoise_fp64(x, n, 0.6, 0.8, 12, 8, hr.BICUBIC)
    assert np.allclose(lat, float(np.float32(0.6)) * up + float(np.float32(0.8)) * n, rtol=0, atol=1e-15)


# ---- fields ------------------------------------------------------------------------------------------------------------------
def test_defaults():
    assert hires.parse_hires(_req(), 512, 512, 4) is None
    assert hires.parse_hires(_req(enable_hr=False, hr_scale=3.0, hr_upscaler="ESRGAN_4x"), 512, 512, 4) is None
    assert hires.parse_hires(_req(enable_hr=True), 512, 512, 4) == (1024, 1024, 4, 0.7, 0)
    assert hires.parse_hires(_req(enable_hr=True, hr_second_pass_steps=0), 512, 384, 6) == (1024, 768, 6, 0.7, 0)
    got = hires.parse_hires(_req(enable_hr=True, hr_second_pass_steps=3, denoising_strength=0.5, hr_upscaler="Latent (bicubic)"), 512, 512, 4)
    assert got == (1024, 1024, 3, 0.5, 1)
    assert hires.parse_hires(_req(enable_hr=True, hr_upscaler="Latent (nearest-exact)", hr_scale=1), 512, 512, 4) == (512, 512, 4, 0.7, 2)


def test_a1111_size_rule():
    assert hires.parse_hires(_req(enable_hr=True, hr_scale=1.5), 520, 392, 4)[:2] == (776, 584)
    assert hires.parse_hires(_req(enable_hr=True, hr_scale=4), 64, 72, 4)[:2] == (256, 288)
    assert hires.parse_hires(_req(enable_hr=True, hr_scale=1.26), 64, 64, 4)[:2] == (80, 80)
    # both hr_resize_* > 0 override the scale; one alone does not
    assert hires.parse_hires(_req(enable_hr=True, hr_scale=3.0, hr_resize_x=768, hr_resize_y=640), 512, 512, 4)[:2] == (768, 640)
    assert hires.parse_hires(_req(enable_hr=True, hr_scale=1.5, hr_resize_x=768, hr_resize_y=0), 512, 512, 4)[:2] == (768, 768)


@pytest.mark.parametrize("extra,name", [
    (dict(hr_scale=0.5), "hr_scale"), (dict(hr_scale=4.5), "hr_scale"), (dict(hr_scale="big"), "hr_scale"),
    (dict(hr_scale=float("nan")), "hr_scale"),
    (dict(denoising_strength=0.01), "denoising_strength"), (dict(denoising_strength=1.5), "denoising_strength"),
    (dict(denoising_strength="x"), "denoising_strength"),
    (dict(hr_resize_x=772, hr_resize_y=768), "hr_resize_x"), (dict(hr_resize_x=768, hr_resize_y=504), "hr_resize_y"),
    (dict(hr_resize_x=2056, hr_resize_y=768), "hr_resize_x"), (dict(hr_resize_x=-8, hr_resize_y=768), "hr_resize_x"),
    (dict(hr_resize_x=768.5, hr_resize_y=768), "hr_resize_x"),
    (dict(hr_second_pass_steps=-1), "hr_second_pass_steps"), (dict(hr_second_pass_steps=2.5), "hr_second_pass_steps"),
])
def test_out_of_range_values_name_the_field(extra, name):
    with pytest.raises(RuntimeError, match=name):
        hires.parse_hires(_req(enable_hr=True, **extra), 512, 512, 4)


@pytest.mark.parametrize("up", ["ESRGAN_4x", "Lanczos", "latent", "Latent (antialiased)", 3])
def test_other_upscalers_list_the_three_served(up):
    with pytest.raises(RuntimeError) as e:
        hires.parse_hires(_req(enable_hr=True, hr_upscaler=up), 512, 512, 4)
    for name in ("'Latent'", "'Latent (bicubic)'", "'Latent (nearest-exact)'"):
        assert name in str(e.value)


def test_too_many_second_pass_steps_raise_diffusers_message():
    sched = LCMSchedule()
    hires.check_schedule(sched, 35, 0.7)
    with pytest.raises(RuntimeError, match=r"The combined original_steps x strength: 35 is smaller than num_inference_steps: 36"):
        hires.check_schedule(sched, 36, 0.7)
    with pytest.raises(RuntimeError, match=r"The combined original_steps x strength"):
        hires.check_schedule(sched, 4, 0.05)


def test_job_keys():
    plain = HipLcmWorker._job_key(_req())
    assert plain == (512, 512, 4, 1.0, None, 0)
    # no enable_hr (or a false one): the plain key, whatever the other hr_* fields say
    for extra in (dict(enable_hr=False), dict(enable_hr=None, hr_scale=9.0), dict(hr_upscaler="nope", denoising_strength=7),
                  dict(enable_hr=0, hr_resize_x=3)):
        assert HipLcmWorker._job_key(_req(**extra)) == plain
    key = HipLcmWorker._job_key(_req(enable_hr=True, hr_scale=1.5, hr_second_pass_steps=3, denoising_strength=0.6))
    assert key == plain + ("hires", 768, 768, 3, 0.6, 0) and hires.is_hires_key(key) and not hires.is_hires_key(plain)
    # every hires field is part of the key: such jobs never share a pass with another kind or another target
    others = [dict(hr_scale=2.0), dict(hr_second_pass_steps=4), dict(denoising_strength=0.7), dict(hr_upscaler="Latent (bicubic)")]
    base = dict(enable_hr=True, hr_scale=1.5, hr_second_pass_steps=3, denoising_strength=0.6)
    assert len({HipLcmWorker._job_key(_req(**dict(base, **o))) for o in others} | {key}) == 5
    # the refinement and ControlNet keys are what they were
    assert HipLcmWorker._job_key(_req(denoise_strength=0.5)) == plain + (0.5, 1)
    assert not hires.is_hires_key(HipLcmWorker._job_key(_req(denoise_strength=0.5, pass_number=2)))


def test_not_combined_and_not_for_sdxl():
    with pytest.raises(RuntimeError, match="enable_hr is not combined with refinement"):
        HipLcmWorker._job_key(_req(enable_hr=True, denoise_strength=0.5))
    with pytest.raises(RuntimeError, match="enable_hr is not combined with refinement"):
        HipLcmWorker._job_key(_req(enable_hr=True, pass_number=2))
    with pytest.raises(RuntimeError, match="enable_hr is not combined with controlnet_image"):
        HipLcmWorker._job_key(_req(enable_hr=True, controlnet_image=np.zeros((512, 512, 3), np.uint8)))
    with pytest.raises(RuntimeError, match="SDXL"):
        HipLcmSDXLWorker._job_key(_req(enable_hr=True))
    assert HipLcmSDXLWorker._job_key(_req(enable_hr=False)) == (512, 512, 4, 1.0, None, 0)
    # denoise_strength 1.0 is a plain request for refinement, so it combines
    assert hires.is_hires_key(HipLcmWorker._job_key(_req(enable_hr=True, denoise_strength=1.0)))


# ---- RNG draw order ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("steps,hr_steps", [(4, 4), (1, 3), (3, 1)])
def test_draw_order(steps, hr_steps):
    from sdlcm_amd.pipeline import draw_noise, draw_noise_hires
    seed, h, w, h2, w2 = 91, 8, 6, 12, 9
    lat, lo, hi = draw_noise_hires(seed, h, w, steps, h2, w2, hr_steps)
    plat, pextra = draw_noise(seed, h, w, steps - 1)
    assert torch.equal(lat, plat) and len(lo) == steps - 1 and all(torch.equal(a, b) for a, b in zip(lo, pextra))
    assert len(hi) == hr_steps and all(t.shape == (1, 4, h2, w2) for t in hi)
    # one generator: the target-shape tensors continue the stream where the plain request's draws ended
    g = torch.Generator().manual_seed(seed)
    for _ in range(steps):
        torch.randn((1, 4, h, w), generator=g)
    assert all(torch.equal(t, torch.randn((1, 4, h2, w2), generator=g)) for t in hi)
    rlo, rhi = hr.draw_hires(seed, h, w, steps, h2, w2, hr_steps)
    assert all(torch.equal(a, b) for a, b in zip([lat] + lo, rlo)) and all(torch.equal(a, b) for a, b in zip(hi, rhi))
