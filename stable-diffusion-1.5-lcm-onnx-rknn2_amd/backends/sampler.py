"""A1111's ``sampler_name`` / ``scheduler`` fields of a request: which sampler steps it (samplers.py holds the tables, the
``lcm_sampler_step`` kernel the arithmetic).  Absent, None, "" or "LCM" is the LCM sampler of always: the request's batch key,
plan, launches and bytes are untouched.

LCM_SAMPLERS=request (default): the fields are read.  LCM_SAMPLERS=lcm: they are not read at all, every request is stepped
by the LCM sampler (the worker before it knew the fields).  Anything else is a RuntimeError when a worker is constructed."""
from __future__ import annotations

import os

from .. import samplers as _s

KEY_TAG = "sampler"               # batch / plan keys of a sampler pass carry (KEY_TAG, canonical name, "karras" | "normal")
MODES = ("request", "lcm")
SDXL_ERROR = "sampler_name: samplers are not served by the SDXL worker"
NOT_COMBINED = "sampler_name is not combined with "


def mode() -> str:
    m = (os.environ.get("LCM_SAMPLERS") or "request").strip().lower()
    if m not in MODES:
        raise RuntimeError(f"Unknown LCM_SAMPLERS={m}, expected one of {', '.join(MODES)}")
    return m


def _served() -> str:
    return ("served: LCM, " + ", ".join(_s.SERVED) + "; scheduler Automatic, Normal, or Karras with "
            + ", ".join(_s.KARRAS_OK))


def parse_sampler(req):
    """-> None (the LCM sampler) | (canonical name, "normal" | "karras").  RuntimeError for anything that is not served."""
    if mode() == "lcm":
        return None
    name = getattr(req, "sampler_name", None)
    if name is None:
        return None
    if not isinstance(name, str):
        raise RuntimeError(f"sampler_name {name!r} is not a string ({_served()})")
    key = " ".join(name.split()).lower()
    if key in ("", "lcm"):
        return None
    if key not in _s.NAMES:
        raise RuntimeError(f"sampler_name {name!r} is not served ({_served()})")
    canon, schedule = _s.NAMES[key]
    sch = getattr(req, "scheduler", None)
    if sch is not None:
        if not isinstance(sch, str):
            raise RuntimeError(f"scheduler {sch!r} is not a string ({_served()})")
        k = sch.strip().lower()
        if k == "karras":
            if canon not in _s.KARRAS_OK:
                raise RuntimeError(f"scheduler {sch!r} is not served with sampler_name {name!r} ({_served()})")
            schedule = _s.KARRAS
        elif k not in ("", "automatic", "normal"):
            raise RuntimeError(f"scheduler {sch!r} is not served ({_served()})")
    steps = int(req.num_inference_steps)
    if not 1 <= steps <= _s.MAX_STEPS:
        raise RuntimeError(f"num_inference_steps={steps} outside 1..{_s.MAX_STEPS} with sampler_name {name!r}")
    return canon, schedule


def check_img2img(sched, smp, steps, strength):
    """Raise for an image-to-image request whose strength leaves the sampler no step (DDIM), before any GPU work."""
    try:
        _s.img2img_tables(sched, smp[0], smp[1], steps, strength)
    except ValueError as e:
        raise RuntimeError(str(e))


def tail(smp) -> tuple:
    """The ending a sampler puts on a batch key; () for the LCM sampler."""
    return () if smp is None else (KEY_TAG,) + tuple(smp)


def split_key(key):
    """A batch key without its ("ctx", n) ending -> (the key without its sampler ending, None | (name, schedule))."""
    if len(key) >= 3 and key[-3] == KEY_TAG:
        return tuple(key[:-3]), (key[-2], key[-1])
    return key, None
