"""Multi-pass refinement in latent space: the request fields the UI sends with ``/generate`` (``denoise_strength``,
``pass_number``, ``total_passes``; lcm-sr-ui/src/utils/api.js:177-186), and the engine's device-resident cache of the denoised
latents x^k that lets pass p start from pass p - 1.  No GPU code here: the chain itself is
``LcmHipPipeline.generate(..., strength=, passes=, start=)``.
"""
from __future__ import annotations

import os
import threading
from collections import OrderedDict

MIN_STRENGTH, MAX_STRENGTH = 0.05, 1.0
MAX_PASSES = 8


def parse_refine(req):
    """-> None for a plain request (no ``denoise_strength`` or 1.0, and no ``pass_number`` or <= 1), else (d, p).
    Raises RuntimeError naming the offending field."""
    d = getattr(req, "denoise_strength", None)
    p = getattr(req, "pass_number", None)
    total = getattr(req, "total_passes", None)
    if d is not None:
        try:
            d = float(d)
        except (TypeError, ValueError):
            raise RuntimeError(f"Invalid denoise_strength {d!r}, expected a number in [{MIN_STRENGTH}, {MAX_STRENGTH}]")
        if not MIN_STRENGTH <= d <= MAX_STRENGTH:         # NaN fails both comparisons
            raise RuntimeError(f"Invalid denoise_strength {d!r}, expected a number in [{MIN_STRENGTH}, {MAX_STRENGTH}]")
    if p is not None:
        try:
            if isinstance(p, bool) or int(p) != p:
                raise ValueError
            p = int(p)
        except (TypeError, ValueError):
            raise RuntimeError(f"Invalid pass_number {p!r}, expected an integer in 1..{MAX_PASSES}")
    if (d is None or d == 1.0) and (p is None or p <= 1):
        # plain -- whatever total_passes says: today's path, key and bytes.  pass_number <= 0 without a strength was ignored
        # before these fields were served, and still is.
        return None
    p = 1 if p is None else p
    if not 1 <= p <= MAX_PASSES:
        raise RuntimeError(f"Invalid pass_number {p!r}, expected an integer in 1..{MAX_PASSES}")
    if total is not None:
        try:
            if isinstance(total, bool) or int(total) != total:
                raise ValueError
            total = int(total)
        except (TypeError, ValueError):
            raise RuntimeError(f"Invalid total_passes {total!r}, expected an integer >= pass_number")
        if p > total:
            raise RuntimeError(f"Invalid pass_number {p}: larger than total_passes {total}")
    return (1.0 if d is None else d, p)


def noise_draws(steps: int, passes: int) -> int:
    """Tensors a request's generator yields: the plain request's ``steps`` (initial latents + steps - 1), then ``steps`` per
    refinement pass (its re-noise draw, then its steps - 1 step noises)."""
    return int(steps) * (int(passes) + 1)


def check_schedule(sched, steps: int, strength: float):
    """diffusers' own error for steps > int(original_inference_steps x strength), as a RuntimeError of the job: the one check
    of refinement, hires (its hr_steps) and image-to-image requests."""
    try:
        sched.timesteps(int(steps), float(strength))
    except ValueError as e:
        raise RuntimeError(str(e))


def cache_bytes_from_env() -> int:
    try:
        mb = float(os.environ.get("LCM_REFINE_CACHE_MB", "64") or 0)
    except ValueError:
        mb = 64.0
    return max(0, int(mb * (1 << 20)))


class RefineCache:
    """LRU of fp32 [4,h,w] tensors under a byte cap.  Key: (request identity ..., d, k); value: x^k.  Thread-safe."""

    def __init__(self, cap_bytes: int):
        self.cap = max(0, int(cap_bytes))
        self.bytes = 0
        self._d: OrderedDict = OrderedDict()
        self._lock = threading.Lock()

    @staticmethod
    def _size(t) -> int:
        return int(t.numel()) * int(t.element_size())

    def __len__(self):
        return len(self._d)

    def __contains__(self, key):
        with self._lock:
            return key in self._d

    def get(self, key):
        with self._lock:
            t = self._d.get(key)
            if t is not None:
                self._d.move_to_end(key)
            return t

    def put(self, key, t) -> bool:
        n = self._size(t)
        if self.cap <= 0 or n > self.cap:
            return False
        with self._lock:
            old = self._d.pop(key, None)
            if old is not None:
                self.bytes -= self._size(old)
            self._d[key] = t
            self.bytes += n
            while self.bytes > self.cap:
                _, ev = self._d.popitem(last=False)
                self.bytes -= self._size(ev)
        return True

    def evict(self, key) -> bool:
        with self._lock:
            t = self._d.pop(key, None)
            if t is not None:
                self.bytes -= self._size(t)
            return t is not None

    def clear(self):
        with self._lock:
            self._d.clear()
            self.bytes = 0

    def deepest(self, ident, d, p):
        """The deepest cached x^k of request ``ident`` with k < p: (k, tensor), or (None, None) when the chain starts from
        scratch.  x^0 does not depend on d; it is still kept per d, as the key is stated."""
        for k in range(int(p) - 1, -1, -1):
            t = self.get(ident + (d, k))
            if t is not None:
                return k, t
        return None, None


def request_ident(req, key, seed, variation=None):
    """What x^k of a request depends on besides (d, k): prompt, seed, size, steps, guidance, style, level -- and, for a request
    with an active variation (backends/variation.py), the resolved (subseed, strength, hs, ws) its initial latents were blended
    with: without it pass 2 of a varied request would start from the unvaried request's cached x^1."""
    # (a negative prompt or a clip_skip other than 1 changes x^k too; requests without them keep the identity of always)
    ov = getattr(req, "override_settings", None)
    more = (getattr(req, "negative_prompt", None) or "", getattr(req, "clip_skip", None) or 1,
            (ov.get("CLIP_stop_at_last_layers") if isinstance(ov, dict) else None) or 1)
    ident = (req.prompt, int(seed)) + tuple(key[:6]) + (more if more != ("", 1, 1) else ())
    return ident if variation is None else ident + (("variation",) + tuple(variation),)


def group_by_start(starts, sizes):
    """starts: per item its start depth (None: from scratch).  -> [(depth, [item indices])]: items of one pass share a start
    depth; every group is cut to the plan batch sizes.  Order: first appearance."""
    groups: OrderedDict = OrderedDict()
    for i, s in enumerate(starts):
        groups.setdefault(s, []).append(i)
    out = []
    sizes = sorted(sizes)
    for s, idx in groups.items():
        while idx:
            n = max(x for x in sizes if x <= len(idx))
            out.append((s, idx[:n]))
            idx = idx[n:]
    return out
