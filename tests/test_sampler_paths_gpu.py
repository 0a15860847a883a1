"""The sampler's host sequencing against a recording of itself: every kind of plan LcmHipPipeline._enqueue serves, and both
chained request kinds around it (hires fix, image-to-image), must give the bytes (SHA-256 of rgb / latents / pool8 / xk /
lowres_latents / init_latents of the graph-replayed call), the counters and the ordered kernel instantiations of one eager call
that tests/golden/sampler_paths.json holds.  The file was recorded by tests/golden/make_sampler_paths_golden.py: the first twelve
cases on the commit before the two sampler loops were merged into one, the hires_* and img2img_* cases on the commit before the
three request paths were; the cases are run by that module's ``run_cases`` (one definition for the recording and the test).
64x64-class requests, synthetic weights, 2 steps unless stated, fixed seeds:

  plain_b1_4step                SD1.5 LCM (guidance embedding), B = 1, 4 steps
  plain_b3_1step                B = 3, 1 step: the final step reads the dummy noise tensor
  plain_cfg_sd2_b2              classifier-free guidance 5 on synthetic SD 2.x (v-prediction), B = 2, 2 steps
  plain_unhoisted_b1_2step      MAX_HOISTED_STEPS = 0: time_embed per step inside forward
  controlnet_b2                 SD1.5 ControlNet, scale 0.75, B = 2, 2 steps
  controlnet_cfg_sd2_b1         ControlNet under guidance 5 on SD 2.x, scale 1.0, B = 1, 2 steps
  refine_scratch_p2_b2          strength 0.5, passes = 2, B = 2, 2 steps
  refine_scratch_cfg_sd2_p1_b1  passes = 1 under guidance 5 on SD 2.x, B = 1, 2 steps
  refine_scratch_p3_b2          passes = 3 from scratch: gives the x^1 and the rgb of the next case
  refine_cached_p3_from1_b2     passes = 3 from cached x^1 (run_cases asserts its rgb equals the from-scratch run's)
  sdxl_plain_b1                 SDXL-style added embeddings, B = 1, 2 steps
  sdxl_refine_p1_b1             the same with passes = 1
  hires_bilinear_b2             hires fix 64x64 -> 96x96 (a non-integer scale), hr_steps 2, strength 0.7, bilinear, B = 2
  hires_bicubic_cfg_sd2_b1      guidance 5 on SD 2.x, 64x64 -> 128x128, bicubic, B = 1: the `dup` hand-over, CFG rows in two plans
  hires_nearest_1step_b3        steps = hr_steps = 1, 64x64 -> 64x64, nearest-exact, B = 3: no low-res step noise, identity size
  img2img_b2                    image-to-image 64x64, strength 0.5, B = 2: encoder stage, hand-over, the strength-cut pass
  img2img_cfg_sd2_b1            the same under guidance 5 on SD 2.x, B = 1
  img2img_odd_b2                width 72, height 40, B = 2: non-square, the encoder's ragged tiles
"""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

pytestmark = pytest.mark.gpu

CASES = ("plain_b1_4step", "plain_b3_1step", "plain_cfg_sd2_b2", "plain_unhoisted_b1_2step", "controlnet_b2",
         "controlnet_cfg_sd2_b1", "refine_scratch_p2_b2", "refine_scratch_cfg_sd2_p1_b1", "refine_scratch_p3_b2",
         "refine_cached_p3_from1_b2", "sdxl_plain_b1", "sdxl_refine_p1_b1", "hires_bilinear_b2", "hires_bicubic_cfg_sd2_b1",
         "hires_nearest_1step_b3", "img2img_b2", "img2img_cfg_sd2_b1", "img2img_odd_b2")


@pytest.fixture(scope="module")
def got():
    import make_sampler_paths_golden as mk
    with mk.pipelines() as pipes:
        return mk.run_cases(pipes)


@pytest.fixture(scope="module")
def golden():
    import make_sampler_paths_golden as mk
    with open(mk.PATH) as f:
        return mk.unpack(json.load(f))


def test_every_case_is_run_and_recorded(got, golden):
    assert set(got) == set(CASES)
    assert set(golden) == set(CASES), "tests/golden/sampler_paths.json does not hold exactly the cases of this test"


@pytest.mark.parametrize("case", CASES)
def test_bytes_counters_and_launches_match_the_recording(got, golden, case):
    assert case in golden, f"{case} is missing from tests/golden/sampler_paths.json"
    g, ref = dict(got[case]), dict(golden[case])
    gl, rl = g.pop("launches"), ref.pop("launches")
    assert g == ref                       # hashes and counters, and the same set of keys (xk / lowres_latents / init_latents only where there is one)
    first = next((i for i, (a, b) in enumerate(zip(gl, rl)) if a != b), min(len(gl), len(rl)))
    assert gl == rl, f"{len(gl)} launches against {len(rl)} recorded; first difference at launch {first}: {gl[first:first + 3]} vs {rl[first:first + 3]}"
