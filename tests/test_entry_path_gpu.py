"""The kernels whose path to the first load was shortened (host-derived constants, multiply-shift divisions, ring-issue
counters, one batch of argument loads, the zero page's address fetched once) compute the parent commit's bytes.

tests/golden/parent_bits_entry_path.json was recorded on a build of the parent commit by
tests/golden/make_parent_bits_entry_path.py; tests/entry_path_cases.py holds the launches: tail rows, uneven k-tile bounds,
several n-tiles per workgroup, strided batches, the stride-2 row gather, halo convs on ragged images with 1 and 5 parts, phase and
cropped upsampling, skip concat, the GroupNorm-staged and staged-epilogue forms, the reduce on all three slab geometries, the
single-launch GroupNorm, attention.  Outputs AND statistics slabs are compared.  A 128x128 2-step request, captured in a graph
and replayed twice, equals its eager bytes and the parent's."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import entry_path_cases

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(__file__), "golden", "parent_bits_entry_path.json")) as _f:
    DOC = json.load(_f)


@pytest.fixture(scope="module")
def got():
    return entry_path_cases.run_cases()


def test_the_case_list_is_the_recorded_one(got):
    assert sorted(got) == sorted(DOC["cases"])


@pytest.mark.parametrize("name", sorted(DOC["cases"]))
def test_launch_gives_the_parent_commits_bytes(got, name):
    assert got[name] == DOC["cases"][name], f"{name}: output or statistics differ from commit {DOC['parent_commit'][:12]}"


def _bytes(a):
    return np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a).tobytes()


def test_graph_replays_of_a_request_equal_eager_and_the_parent():
    from sdlcm_amd import weights
    from sdlcm_amd.pipeline import LcmHipPipeline
    r = DOC["request"]
    pipe = LcmHipPipeline(weights.synthetic_unet(), weights.synthetic_vae(), device="cuda:0")
    pe = torch.randn(1, 77, 768, generator=torch.Generator().manual_seed(r["prompt_seed"])).to(torch.float16)
    args = (pe, r["seeds"], r["width"], r["height"], r["steps"], r["guidance_scale"])
    first = pipe.generate(*args)                          # captured, replayed
    second = pipe.generate(*args)                         # replayed again: the arguments baked into the graph's nodes
    eager = pipe.generate(*args, want_float=True)         # eager, same plans
    for k in ("rgb", "latents", "pool8"):
        assert _bytes(first[k]) == _bytes(second[k]), f"{k}: second replay differs from the first"
        assert _bytes(first[k]) == _bytes(eager[k]), f"{k}: graph replay differs from eager"
        assert hashlib.sha256(_bytes(first[k])).hexdigest() == r["sha256"][k], f"{k} differs from commit {DOC['parent_commit'][:12]}"
