"""Host side of multi-pass refinement (denoise_strength / pass_number / total_passes): the strength-cut schedule, request
parsing and validation, batch keys, the latent cache and the draw order.  No GPU."""
from dataclasses import dataclass, field
from typing import Optional

import numpy as np
import pytest
import torch

from sdlcm_amd.backends import refine
from sdlcm_amd.scheduler import LCMSchedule

import refine_reference as rr


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


TABLE = [(4, 1.0, [999, 759, 499, 259]), (4, 0.5, [499, 379, 259, 139]), (4, 0.55, [539, 419, 279, 139]),
         (10, 0.7, [699, 639, 559, 499, 419, 359, 279, 219, 139, 79]), (7, 0.5, [499, 439, 359, 299, 219, 159, 79]),
         (8, 0.8, [799, 699, 599, 499, 399, 299, 199, 99]), (1, 0.3, [299])]


@pytest.mark.parametrize("n,d,want", TABLE)
def test_strength_cut_schedule_table(n, d, want):
    s = LCMSchedule()
    assert s.timesteps(n, d).tolist() == want
    assert s.timesteps(n, strength=d).tolist() == rr.strength_timesteps(n, d).tolist()


def test_strength_cut_schedule_too_short_raises_diffusers_message():
    with pytest.raises(ValueError, match=r"The combined original_steps x strength.*is smaller than num_inference_steps"):
        LCMSchedule().timesteps(7, 0.1)


def test_default_schedule_is_unchanged():
    s = LCMSchedule()
    for n in range(1, 51):
        a, b = s.timesteps(n), s.timesteps(n, 1.0)
        assert a.dtype == b.dtype == np.int64 and np.array_equal(a, b)
        k = 1000 // 50
        origin = (np.arange(1, 51) * k - 1)[::-1]
        assert np.array_equal(a, origin[np.floor(np.linspace(0, 50, num=n, endpoint=False)).astype(np.int64)])
    with pytest.raises(ValueError, match="exceeds original_inference_steps"):
        s.timesteps(51)


def test_renoise_coefficients():
    s = LCMSchedule()
    sa, sb = s.renoise_coefficients(499)
    assert sa == float(s.alphas_cumprod[499]) ** 0.5 and abs(sa * sa + sb * sb - 1) < 1e-12


def test_parse_plain_requests():
    assert refine.parse_refine(_req()) is None
    assert refine.parse_refine(_req(denoise_strength=1.0)) is None
    assert refine.parse_refine(_req(denoise_strength=1.0, pass_number=1, total_passes=3)) is None
    assert refine.parse_refine(_req(pass_number=1)) is None
    assert refine.parse_refine(_req(pass_number=0)) is None
    assert refine.parse_refine(_req(denoise_strength=None, pass_number=None, total_passes=None)) is None


def test_parse_refinement_requests():
    assert refine.parse_refine(_req(denoise_strength=0.5)) == (0.5, 1)
    assert refine.parse_refine(_req(denoise_strength=0.05)) == (0.05, 1)
    assert refine.parse_refine(_req(pass_number=2)) == (1.0, 2)
    assert refine.parse_refine(_req(denoise_strength=1.0, pass_number=3, total_passes=3)) == (1.0, 3)
    assert refine.parse_refine(_req(denoise_strength=0.3, pass_number=8)) == (0.3, 8)
    assert refine.parse_refine(_req(denoise_strength="0.25", pass_number=2.0)) == (0.25, 2)


@pytest.mark.parametrize("extra,field_name", [
    (dict(denoise_strength=0.04), "denoise_strength"), (dict(denoise_strength=1.01), "denoise_strength"),
    (dict(denoise_strength=0.0), "denoise_strength"), (dict(denoise_strength=-0.5), "denoise_strength"),
    (dict(denoise_strength=float("nan")), "denoise_strength"), (dict(denoise_strength="much"), "denoise_strength"),
    (dict(denoise_strength=0.5, pass_number=0), "pass_number"), (dict(denoise_strength=0.5, pass_number=-1), "pass_number"),
    (dict(pass_number=9), "pass_number"), (dict(pass_number=2.5), "pass_number"), (dict(pass_number="two"), "pass_number"),
    (dict(denoise_strength=0.5, pass_number=3, total_passes=2), "total_passes"),
    (dict(pass_number=2, total_passes=1), "total_passes"), (dict(pass_number=2, total_passes="x"), "total_passes")])
def test_validation_errors_name_the_field(extra, field_name):
    with pytest.raises(RuntimeError, match=field_name):
        refine.parse_refine(_req(**extra))


def test_batch_keys():
    from sdlcm_amd.backends.hip_worker import HipLcmWorker
    plain = (512, 512, 4, 1.0, None, 0)
    assert HipLcmWorker._job_key(_req()) == plain
    assert HipLcmWorker._job_key(_req(denoise_strength=1.0)) == plain
    assert HipLcmWorker._job_key(_req(denoise_strength=1.0, pass_number=1, total_passes=3)) == plain
    k1 = HipLcmWorker._job_key(_req(denoise_strength=0.5))
    k2 = HipLcmWorker._job_key(_req(denoise_strength=0.5, pass_number=2))
    k3 = HipLcmWorker._job_key(_req(denoise_strength=0.6))
    k4 = HipLcmWorker._job_key(_req(pass_number=2))
    assert k1 == plain + (0.5, 1) and k2 == plain + (0.5, 2) and k3 == plain + (0.6, 1) and k4 == plain + (1.0, 2)
    assert len({plain, k1, k2, k3, k4}) == 5
    assert HipLcmWorker._job_key(_req(denoise_strength=0.5, pass_number=1)) == k1
    with pytest.raises(RuntimeError, match="denoise_strength"):
        HipLcmWorker._job_key(_req(denoise_strength=2.0))
    with pytest.raises(RuntimeError, match="Invalid size"):
        HipLcmWorker._job_key(_req(size="bogus", denoise_strength=0.5))


def test_refinement_jobs_never_coalesce_with_plain_ones_in_the_batcher():
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
        reqs = [_req(), _req(denoise_strength=0.5), _req(), _req(denoise_strength=0.5), _req(denoise_strength=0.5, pass_number=2)]
        futs = [mb.submit(HipLcmWorker._job_key(r), i) for i, r in enumerate(reqs)]
        gate.set()
        assert [f.result(10) for f in futs] == list(range(5))
        for key, items in seen:
            assert len({HipLcmWorker._job_key(reqs[i]) for i in items}) == 1 and HipLcmWorker._job_key(reqs[items[0]]) == key
        assert sorted(i for _, it in seen for i in it) == list(range(5))
        assert any(items == [1, 3] for _, items in seen)            # the two (0.5, 1) jobs, queued behind the held pass, share one
    finally:
        mb.close()


def test_cache_lru_and_cap():
    t = lambda v: torch.full((4, 8, 8), float(v))          # 1 KiB each
    c = refine.RefineCache(3 * 1024)
    for k in range(3):
        assert c.put(("a", k), t(k))
    assert len(c) == 3 and c.bytes == 3072
    assert c.get(("a", 0)) is not None                      # touch: 0 is now the most recent
    assert c.put(("a", 3), t(3))
    assert ("a", 1) not in c and ("a", 0) in c and ("a", 2) in c and ("a", 3) in c and c.bytes == 3072
    assert c.put(("a", 0), t(9)) and c.bytes == 3072 and float(c.get(("a", 0))[0, 0, 0]) == 9.0     # replace, not grow
    assert not c.put(("big",), torch.zeros(4, 32, 32)) and ("big",) not in c and len(c) == 3          # larger than the cap
    assert c.evict(("a", 2)) and not c.evict(("a", 2)) and c.bytes == 2048
    c.clear()
    assert len(c) == 0 and c.bytes == 0
    off = refine.RefineCache(0)
    assert not off.put(("a", 0), t(0)) and len(off) == 0 and off.deepest(("a",), 0.5, 3) == (None, None)


def test_cache_size_from_env(monkeypatch):
    monkeypatch.delenv("LCM_REFINE_CACHE_MB", raising=False)
    assert refine.cache_bytes_from_env() == 64 << 20
    monkeypatch.setenv("LCM_REFINE_CACHE_MB", "0")
    assert refine.cache_bytes_from_env() == 0
    monkeypatch.setenv("LCM_REFINE_CACHE_MB", "1.5")
    assert refine.cache_bytes_from_env() == 3 << 19


class _FakeEngine:
    """The engine's use of the cache without a GPU: 'running' pass k of a request stores a tensor that names (ident, k)."""

    def __init__(self, cap):
        self.cache = refine.RefineCache(cap)
        self.passes_run = []

    def serve(self, ident, d, p):
        k0, _ = self.cache.deepest(ident, d, p)
        first = 0 if k0 is None else k0 + 1
        for k in range(first, p + 1):
            self.passes_run.append((ident, k))
            self.cache.put(ident + (d, k), torch.full((4, 8, 8), float(k)))
        return k0


def test_start_depth_choice_against_a_fake_engine():
    e = _FakeEngine(1 << 20)
    a, b = ("prompt a", 1), ("prompt b", 1)
    assert e.serve(a, 0.5, 2) is None and e.passes_run == [(a, 0), (a, 1), (a, 2)]            # cold: x^0, x^1, x^2
    e.passes_run.clear()
    assert e.serve(a, 0.5, 3) == 2 and e.passes_run == [(a, 3)]                                  # warm: one pass
    e.passes_run.clear()
    assert e.serve(a, 0.5, 2) == 1 and e.passes_run == [(a, 2)]                                  # the same pass again: from x^1
    assert e.serve(b, 0.5, 1) is None                                                            # another request: nothing shared
    assert e.serve(a, 0.6, 1) is None                                                            # another strength: a chain of its own
    e.cache.evict(a + (0.5, 1))
    e.cache.evict(a + (0.5, 2))
    e.passes_run.clear()
    assert e.serve(a, 0.5, 3) == 0 and e.passes_run == [(a, 1), (a, 2), (a, 3)]                # from the deepest that is left
    assert e.cache.deepest(a, 0.5, 1)[0] == 0 and e.cache.deepest(a, 0.5, 9)[0] == 3


def test_items_of_one_pass_share_a_start_depth():
    g = refine.group_by_start([None, 1, None, 1, 1, 0, None], (1, 2, 4, 8))
    assert g == [(None, [0, 2]), (None, [6]), (1, [1, 3]), (1, [4]), (0, [5])]
    assert refine.group_by_start([2] * 8, (1, 2, 4, 8)) == [(2, list(range(8)))]
    assert refine.group_by_start([None] * 3, (1,)) == [(None, [0]), (None, [1]), (None, [2])]


def test_noise_draw_order():
    from sdlcm_amd.pipeline import draw_noise
    steps, p, h, w = 4, 2, 8, 8
    assert refine.noise_draws(steps, p) == 12 and refine.noise_draws(steps, 0) == steps
    lat, extra = draw_noise(7, h, w, steps - 1)
    lat2, extra2 = draw_noise(7, h, w, refine.noise_draws(steps, p) - 1)
    assert torch.equal(lat, lat2) and len(extra2) == 11
    for a, b in zip(extra, extra2):
        assert torch.equal(a, b)                           # the first `steps` tensors are the plain request's
    ref = rr.draw_all(7, h, w, 12)
    for a, b in zip([lat2] + extra2, ref):
        assert torch.equal(a, b)                           # pass k: tensors [steps k, steps (k + 1)) of the one stream
