"""Host-side tables of the ordinary samplers -- Euler, Euler a, DDIM, DPM++ 2M -- for checkpoints that were never
LCM-distilled (the per-step arithmetic itself is the ``lcm_sampler_step`` kernel; include/lcm_hip.h, samplers, holds the
definitions).  Pure numpy float64 on ``LCMSchedule.alphas_cumprod`` / ``final_alpha_cumprod``; the kernel gets float32.

The state is the variance-preserving one the UNet reads: with k-diffusion's state X at noise level s, x = sa(s) X where
sa(s) = 1 / sqrt(1 + s^2) and sb(s) = s sa(s).  Every step is x' = cx x + c0 x0 + c1 x0_prev + cn noise.

Written after the published formulas of k-diffusion (sample_euler, sample_euler_ancestral, sample_dpmpp_2m, get_sigmas_karras,
DiscreteSchedule.t_to_sigma / sigma_to_t), A1111 (sample_img2img) and diffusers (DDIMScheduler, the img2img pipeline's
get_timesteps).  None of them was at hand to compare with: equality with any of them is unverified."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

EULER, EULER_A, DDIM, DPMPP_2M = "Euler", "Euler a", "DDIM", "DPM++ 2M"
NORMAL, KARRAS = "normal", "karras"
MAX_STEPS = 50

# request name (lower case) -> (canonical name, the name's own sigmas)
NAMES = {"euler": (EULER, NORMAL), "euler a": (EULER_A, NORMAL), "ddim": (DDIM, NORMAL), "dpm++ 2m": (DPMPP_2M, NORMAL),
         "dpm++ 2m karras": (DPMPP_2M, KARRAS)}
SERVED = ("Euler", "Euler a", "DDIM", "DPM++ 2M", "DPM++ 2M Karras")
KARRAS_OK = (EULER, EULER_A, DPMPP_2M)

# One pass: ts -- the (fractional) timestep of every UNet evaluation; coefs -- per step (sa, sb, cx, c0, c1, cn); init_scale -- what
# the initial noise is multiplied by (None: nothing, DDIM); start -- (sqrt_a, sqrt_b) of an image-to-image pass's first state
# sqrt_a z + sqrt_b e1 (None for text-to-image); sigmas -- the pass's noise levels with the final 0 (None for DDIM, which steps over timesteps)
Tables = namedtuple("Tables", "name schedule ts coefs init_scale start sigmas")


def sa(s):
    return 1.0 / np.sqrt(1.0 + np.asarray(s, dtype=np.float64) ** 2)


def sb(s):
    return np.asarray(s, dtype=np.float64) * sa(s)


def _abar(sched):
    return np.asarray(sched.alphas_cumprod, dtype=np.float64)


def sigma_table(sched) -> np.ndarray:
    a = _abar(sched)
    return np.sqrt((1.0 - a) / a)


def t_to_sigma(sched, t):
    """Fractional t -> sigma: linear in log sigma between floor(t) and ceil(t)."""
    ls = np.log(sigma_table(sched))
    t = np.asarray(t, dtype=np.float64)
    lo, hi = np.floor(t).astype(np.int64), np.ceil(t).astype(np.int64)
    w = t - lo
    return np.exp((1.0 - w) * ls[lo] + w * ls[hi])


def sigma_to_t(sched, s):
    """The inverse of t_to_sigma on the same table; the weight is clipped to [0, 1]."""
    ls = np.log(sigma_table(sched))
    x = np.log(np.atleast_1d(np.asarray(s, dtype=np.float64)))
    lo = np.clip(np.searchsorted(ls, x, side="right") - 1, 0, len(ls) - 2)
    hi = lo + 1
    w = np.clip((ls[lo] - x) / (ls[lo] - ls[hi]), 0.0, 1.0)
    t = (1.0 - w) * lo + w * hi
    return t if np.ndim(s) else float(t[0])


def schedule_sigmas(sched, schedule: str, n: int):
    """-> (sigmas [n + 1] with the final 0, the n timesteps the UNet is evaluated at)."""
    n = int(n)
    if n < 1:
        raise ValueError("num_inference_steps must be >= 1")
    tab = sigma_table(sched)
    if schedule == NORMAL:
        ts = np.linspace(len(tab) - 1, 0, n)
        sig = t_to_sigma(sched, ts)
    elif schedule == KARRAS:
        smax, smin, rho = tab[-1], tab[0], 7.0
        ramp = np.linspace(0.0, 1.0, n) if n > 1 else np.zeros(1)
        sig = (smax ** (1 / rho) + ramp * (smin ** (1 / rho) - smax ** (1 / rho))) ** rho
        ts = sigma_to_t(sched, sig)
    else:
        raise ValueError(f"unknown sigma schedule {schedule!r}")
    return np.append(sig, 0.0), np.asarray(ts, dtype=np.float64)


def sigma_coefficients(name: str, sig) -> list:
    """The steps of Euler / Euler a / DPM++ 2M over the noise levels sig (the last one may be 0) -> [(sa, sb, cx, c0, c1, cn)]."""
    out, h_prev = [], None
    for i in range(len(sig) - 1):
        s, s2 = float(sig[i]), float(sig[i + 1])
        S, S2 = float(sa(s)), float(sa(s2))
        c1 = cn = 0.0
        if name == EULER:
            cx, c0 = S2 * s2 / (S * s), S2 * (1.0 - s2 / s)
        elif name == EULER_A:
            up = min(s2, np.sqrt(s2 * s2 * (s * s - s2 * s2) / (s * s)))
            dn = np.sqrt(s2 * s2 - up * up)
            cx, c0, cn = S2 * dn / (S * s), S2 * (1.0 - dn / s), S2 * up
        elif name == DPMPP_2M:
            if s2 == 0.0:
                cx, c0 = 0.0, 1.0
            else:
                h = np.log(s) - np.log(s2)
                e = -np.expm1(-h)
                cx = S2 * s2 / (S * s)
                if h_prev is None:
                    c0 = S2 * e
                else:
                    r = h_prev / h
                    c0, c1 = S2 * e * (1.0 + 1.0 / (2.0 * r)), -S2 * e / (2.0 * r)
                h_prev = h
        else:
            raise ValueError(f"{name!r} does not step over sigmas")
        out.append((S, float(sb(s)), float(cx), float(c0), float(c1), float(cn)))
    return out


def ddim_timesteps(sched, n: int) -> np.ndarray:
    """diffusers' DDIMScheduler.set_timesteps(n), "leading" spacing, steps_offset 1."""
    n = int(n)
    if n < 1:
        raise ValueError("num_inference_steps must be >= 1")
    return (np.arange(n)[::-1] * (sched.num_train_timesteps // n) + 1).astype(np.int64)


def ddim_coefficients(sched, ts, n: int) -> list:
    """DDIM (eta 0) at the integer timesteps ts of an n-step schedule."""
    a, k = _abar(sched), sched.num_train_timesteps // int(n)
    out = []
    for t in ts:
        p = int(t) - k
        a_t, a_p = a[int(t)], (a[p] if p >= 0 else float(sched.final_alpha_cumprod))
        sa_t, sb_t, sa_p, sb_p = np.sqrt(a_t), np.sqrt(1.0 - a_t), np.sqrt(a_p), np.sqrt(1.0 - a_p)
        out.append((float(sa_t), float(sb_t), float(sb_p / sb_t), float(sa_p - sb_p * sa_t / sb_t), 0.0, 0.0))
    return out


def _check(name, schedule, n):
    if name not in (EULER, EULER_A, DDIM, DPMPP_2M):
        raise ValueError(f"unknown sampler {name!r}")
    if schedule not in (NORMAL, KARRAS) or (schedule == KARRAS and name not in KARRAS_OK):
        raise ValueError(f"sampler {name!r} has no {schedule!r} sigmas")
    if not 1 <= int(n) <= MAX_STEPS:
        raise ValueError(f"num_inference_steps={n} outside 1..{MAX_STEPS} with sampler_name")


def tables(sched, name: str, schedule: str, n: int) -> Tables:
    """The text-to-image pass of n steps."""
    _check(name, schedule, n)
    if name == DDIM:
        ts = ddim_timesteps(sched, n)
        return Tables(name, schedule, ts.astype(np.float64), ddim_coefficients(sched, ts, n), None, None, None)
    sig, ts = schedule_sigmas(sched, schedule, n)
    return Tables(name, schedule, ts, sigma_coefficients(name, sig), float(sb(sig[0])), None, sig)


def img2img_tables(sched, name: str, schedule: str, n: int, strength: float) -> Tables:
    """The image-to-image tail of an n-step schedule.  Euler, Euler a, DPM++ 2M (after A1111's sample_img2img):
    t_enc = int(min(strength, 0.999) n), the pass runs over sigmas[n - t_enc - 1:] -- t_enc + 1 evaluations -- from
    sa(s) z + sb(s) e1 at its first sigma s.  DDIM (diffusers' img2img): the last min(int(n strength), n) timesteps, from
    add_noise at the first of them; none left is a ValueError."""
    _check(name, schedule, n)
    n, strength = int(n), float(strength)
    if name == DDIM:
        full = ddim_timesteps(sched, n)
        ts = full[max(n - min(int(n * strength), n), 0):]
        if len(ts) == 0:
            raise ValueError(f"After adjusting the num_inference_steps by strength parameter: {strength}, the number of pipeline "
                             f"steps is 0 which is < 1 and not appropriate for this pipeline.")
        a0 = float(_abar(sched)[int(ts[0])])
        return Tables(name, schedule, ts.astype(np.float64), ddim_coefficients(sched, ts, n), None, (a0 ** 0.5, (1.0 - a0) ** 0.5), None)
    sig, ts = schedule_sigmas(sched, schedule, n)
    first = n - int(min(strength, 0.999) * n) - 1
    sig, ts = sig[first:], ts[first:]
    return Tables(name, schedule, ts, sigma_coefficients(name, sig), None, (float(sa(sig[0])), float(sb(sig[0]))), sig)


def sampler_list():
    """The answer of ``/sdapi/v1/samplers``: LCM first, then what ``sampler_name`` serves."""
    out = [{"name": "LCM", "aliases": ["lcm"], "options": {}}]
    for n in SERVED:
        canon, schedule = NAMES[n.lower()]
        out.append({"name": n, "aliases": [n.lower().replace("+", "p").replace(" ", "_")],
                    "options": {"scheduler": schedule} if schedule == KARRAS else {}})
    return out
