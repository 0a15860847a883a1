"""fp64 numpy restatement of the ordinary samplers (include/lcm_hip.h, samplers): the sigma schedules, the per-step coefficients
and the step, written from the definitions and importing nothing from sdlcm_amd.samplers; and a chain oracle in the manner of
tests/chain_reference.py, built on oracle.unet.UNetOracle (which takes fractional timesteps), tests/controlnet_reference.py,
tests/vae_encoder_reference.py and oracle.vae.

The state is the variance-preserving one: x = sa(s) X for k-diffusion's X at noise level s, sa(s) = 1 / sqrt(1 + s^2),
sb(s) = s sa(s).  Every step is x' = cx x + c0 x0 + c1 x0_prev + cn noise.

``mutate=`` names one wiring mistake, stated on the oracle's side (MUTANTS)."""
from __future__ import annotations

import math

import numpy as np
import torch

EULER, EULER_A, DDIM, DPMPP_2M = "Euler", "Euler a", "DDIM", "DPM++ 2M"


# ---- tables ---------------------------------------------------------------------------------------------------------------------
def alphas_cumprod(beta_start=0.00085, beta_end=0.012, n=1000, **_):
    """The product's alphas_cumprod (scaled-linear betas, accumulated in float32 as LCMSchedule does), as float64."""
    betas = np.linspace(beta_start ** 0.5, beta_end ** 0.5, n, dtype=np.float32) ** 2
    return np.cumprod((1.0 - betas).astype(np.float32), dtype=np.float32).astype(np.float64)


def S(s):
    return 1.0 / math.sqrt(1.0 + s * s)


def log_sigmas(abar):
    return 0.5 * (np.log1p(-abar) - np.log(abar))


def t_to_sigma(abar, t):
    ls = log_sigmas(abar)
    lo, hi = int(math.floor(t)), int(math.ceil(t))
    w = t - lo
    return math.exp((1.0 - w) * ls[lo] + w * ls[hi])


def sigma_to_t(abar, s):
    """k-diffusion's DiscreteSchedule.sigma_to_t, entry by entry: the last table entry not above log s (at most the last but
    one), the weight between it and the next clipped to [0, 1]."""
    ls = log_sigmas(abar)
    x = math.log(s)
    lo = min(max(int(np.cumsum(x - ls >= 0).argmax()), 0), len(ls) - 2)
    hi = lo + 1
    w = min(max((ls[lo] - x) / (ls[lo] - ls[hi]), 0.0), 1.0)
    return (1.0 - w) * lo + w * hi


def schedule(abar, kind, n):
    """-> (n + 1 sigmas, the last one 0; the n timesteps of the UNet)."""
    N = len(abar)
    if kind == "normal":
        ts = [float(N - 1)] if n == 1 else [(N - 1) * (1.0 - i / (n - 1)) for i in range(n)]
        sig = [t_to_sigma(abar, t) for t in ts]
    else:
        assert kind == "karras"
        smax, smin = t_to_sigma(abar, N - 1), t_to_sigma(abar, 0)
        a, b = smax ** (1.0 / 7.0), smin ** (1.0 / 7.0)
        sig = [smax] if n == 1 else [(a + i / (n - 1) * (b - a)) ** 7 for i in range(n)]
        ts = [sigma_to_t(abar, s) for s in sig]
    return np.array(sig + [0.0]), np.array(ts)


def sigma_steps(name, sig):
    """[(sa, sb, cx, c0, c1, cn)] of Euler / Euler a / DPM++ 2M over the sigmas."""
    rows, h_prev = [], None
    for s, s2 in zip(sig[:-1], sig[1:]):
        s, s2 = float(s), float(s2)
        c1 = cn = 0.0
        if name == EULER:
            cx, c0 = S(s2) * s2 / (S(s) * s), S(s2) * (1.0 - s2 / s)
        elif name == EULER_A:
            up = min(s2, math.sqrt(s2 ** 2 * (s ** 2 - s2 ** 2) / s ** 2))
            dn = math.sqrt(s2 ** 2 - up ** 2)
            cx, c0, cn = S(s2) * dn / (S(s) * s), S(s2) * (1.0 - dn / s), S(s2) * up
        else:
            assert name == DPMPP_2M
            if s2 == 0.0:
                cx, c0 = 0.0, 1.0
            else:
                h = math.log(s) - math.log(s2)
                e = -math.expm1(-h)
                cx, c0 = S(s2) * s2 / (S(s) * s), S(s2) * e
                if h_prev is not None:
                    r = h_prev / h
                    c0, c1 = S(s2) * e * (1.0 + 1.0 / (2.0 * r)), -S(s2) * e / (2.0 * r)
                h_prev = h
        rows.append((S(s), s * S(s), cx, c0, c1, cn))
    return rows


def ddim_on_sigmas(sig):
    """DDIM's update (eta 0) between arbitrary noise levels: sa_t = sa(s), sb_t = sb(s)."""
    rows = []
    for s, s2 in zip(sig[:-1], sig[1:]):
        sa_t, sb_t, sa_p, sb_p = S(s), s * S(s), S(s2), s2 * S(s2)
        rows.append((sa_t, sb_t, sb_p / sb_t, sa_p - sb_p * sa_t / sb_t, 0.0, 0.0))
    return rows


def ddim_steps(abar, final, n, ts=None):
    """diffusers' DDIMScheduler (eta 0, leading spacing, steps_offset 1) -> (integer timesteps, rows)."""
    k = len(abar) // n
    full = [(n - 1 - i) * k + 1 for i in range(n)]
    ts = full if ts is None else ts
    rows = []
    for t in ts:
        p = t - k
        a_t, a_p = abar[t], abar[p] if p >= 0 else final
        rows.append((math.sqrt(a_t), math.sqrt(1 - a_t), math.sqrt(1 - a_p) / math.sqrt(1 - a_t),
                     math.sqrt(a_p) - math.sqrt(1 - a_p) * math.sqrt(a_t) / math.sqrt(1 - a_t), 0.0, 0.0))
    return np.array(ts, dtype=np.float64), rows


def tables(abar, final, name, kind, n):
    """-> dict(ts, rows, init_scale | None) of the text-to-image pass."""
    if name == DDIM:
        ts, rows = ddim_steps(abar, final, n)
        return dict(ts=ts, rows=rows, init_scale=None)
    sig, ts = schedule(abar, kind, n)
    return dict(ts=ts, rows=sigma_steps(name, sig), init_scale=sig[0] * S(sig[0]), sigmas=sig)


def img2img_tables(abar, final, name, kind, n, strength, off_by_one=False):
    """-> dict(ts, rows, start = (sqrt_a, sqrt_b)) of the image-to-image tail (off_by_one: the tail one entry short)."""
    if name == DDIM:
        full, _ = ddim_steps(abar, final, n)
        keep = min(int(n * strength), n) - (1 if off_by_one else 0)
        ts = [int(t) for t in full[n - keep:]] if keep > 0 else []
        if not ts:
            raise ValueError("no timestep left")
        ts, rows = ddim_steps(abar, final, n, ts)
        return dict(ts=ts, rows=rows, start=(math.sqrt(abar[int(ts[0])]), math.sqrt(1 - abar[int(ts[0])])))
    sig, ts = schedule(abar, kind, n)
    t_enc = int(min(strength, 0.999) * n)
    first = n - t_enc - 1 + (1 if off_by_one else 0)
    sig, ts = sig[first:], ts[first:]
    return dict(ts=ts, rows=sigma_steps(name, sig), start=(S(sig[0]), sig[0] * S(sig[0])), sigmas=sig)


# ---- the step -------------------------------------------------------------------------------------------------------------------
def x0_of(x, m, sa, sb, pred):
    if pred == "epsilon":
        return (x - sb * m) / sa
    if pred == "v_prediction":
        return sa * x - sb * m
    assert pred == "sample"
    return m


def step(x, m, x0_prev, noise, row, pred):
    """-> (x', x0) in the dtype of the operands (float64 arrays for the kernel check, fp32 torch tensors in the chain)."""
    sa, sb, cx, c0, c1, cn = row
    x0 = x0_of(x, m, sa, sb, pred)
    out = cx * x + c0 * x0
    if c1 != 0.0:
        out = out + c1 * x0_prev
    if cn != 0.0:
        out = out + cn * noise
    return out, x0


# ---- the Gaussian closed form ---------------------------------------------------------------------------------------------------
def gaussian_run(rows_of, sig, mu=0.7, c=0.5, n_points=64, seed=0, state=False):
    """Data N(mu, c^2) per coordinate: the optimal denoiser of X = x0 + s n is mu + c^2 / (c^2 + s^2) (X - mu), and the
    probability-flow solution from X_0 at s_0 to s = 0 is mu + (X_0 - mu) c / sqrt(c^2 + s_0^2).  Runs the steps rows_of(sig) with
    that denoiser as a "sample" prediction from X_0 = s_0 e -> the RMS end error against the closed form (state: the end state)."""
    e = np.random.default_rng(seed).standard_normal(n_points)
    X0 = sig[0] * e
    x = S(sig[0]) * X0
    x0_prev = np.zeros_like(x)
    for s, row in zip(sig[:-1], rows_of(sig)):
        X = x / S(s)
        m = mu + c * c / (c * c + s * s) * (X - mu)
        x, x0_prev = step(x, m, x0_prev, None, row, "sample")
    if state:
        return x
    exact = mu + (X0 - mu) * c / math.sqrt(c * c + sig[0] ** 2)
    return float(np.sqrt(np.mean((x - exact) ** 2)))


# ---- the chain ------------------------------------------------------------------------------------------------------------------
MUTANTS = ("wrong_prediction", "init_unscaled", "blend_after_scale", "history_stale", "noise_on_last", "noise_shift", "cfg_swapped",
           "tail_off_by_one")


class SamplerChainOracle:
    """One request (B = 1) through a sampler pass in fp32 torch: plain, ControlNet (hint, scale) or image-to-image
    (picture, strength); the guidance form follows the UNet config as in chain_reference.ChainOracle."""

    def __init__(self, unet_sd, vae_sd, unet_cfg=None, enc_sd=None, cn_sd=None, schedule=None, prediction_type=None):
        import controlnet_reference as cnr
        from oracle.vae import VAEDecoderOracle
        sch = dict(schedule or {})
        self.unet = cnr.UNetWithResiduals(unet_sd, unet_cfg)
        self.cn = cnr.ControlNetOracle(cn_sd, unet_cfg) if cn_sd is not None else None
        self.vae = VAEDecoderOracle(vae_sd)
        self.abar = alphas_cumprod(**{k: sch[k] for k in ("beta_start", "beta_end") if k in sch})
        self.final = 1.0 if sch.get("set_alpha_to_one", True) else float(self.abar[0])
        self.pred = prediction_type or sch.get("prediction_type", "epsilon")
        self.enc_sd = enc_sd
        self._evals, self._z = {}, {}

    def forget(self):
        self._evals.clear()
        self._z.clear()

    def do_cfg(self, guidance):
        return guidance > 1.0 and not self.unet.cfg.get("time_cond_proj_dim")

    def _eval(self, x, t, ctx, hint_emb, scale):
        key = (float(t), x.numpy().tobytes(), ctx.numpy().tobytes(), scale)
        if key not in self._evals:
            kw = {}
            if hint_emb is not None:
                d, m = self.cn.forward(x, float(t), ctx, None, scale, hint_emb=hint_emb.expand(x.shape[0], -1, -1, -1))
                kw = dict(down_residuals=d, mid_residual=m)
            self._evals[key] = self.unet.forward(x, float(t), ctx, None, **kw)
        return self._evals[key]

    @torch.inference_mode()
    def __call__(self, prompt_embeds, width, height, steps, guidance, seed, sampler, kind=("plain",), negative_embeds=None,
                 variation=None, mutate=None, decode=True):
        """sampler = (name, "normal" | "karras"); kind ("plain",) | ("control", hint uint8 [H,W,3], scale) |
        ("img2img", picture uint8 [H,W,3], strength); variation = (t, sub, base | None) as generate(variation=) takes it.
        -> dict(latents [1,4,h,w], image NCHW float, ts: the timesteps the UNet saw, trace: the state after every step)."""
        import variation_reference as vr
        import vae_encoder_reference as ver
        from sdlcm_amd.pipeline import draw_noise, draw_noise_img2img
        assert mutate is None or mutate in MUTANTS
        name, sched_kind = sampler
        f32 = lambda a: None if a is None else torch.as_tensor(np.asarray(a), dtype=torch.float32)
        pe, ne, g = f32(prompt_embeds), f32(negative_embeds), float(guidance)
        cfg = self.do_cfg(g)
        assert self.unet.cfg.get("time_cond_proj_dim") is None, "samplers serve UNets without a guidance embedding"
        h, w = height // 8, width // 8
        pred = self.pred
        if mutate == "wrong_prediction":
            pred = "v_prediction" if pred == "epsilon" else "epsilon"
        hint_emb, scale = None, None
        if kind[0] == "control":
            hint_emb, scale = self.cn.embed_hint(np.asarray(kind[1])[None]), float(kind[2])
        if kind[0] == "img2img":
            T = img2img_tables(self.abar, self.final, name, sched_kind, steps, kind[2], off_by_one=mutate == "tail_off_by_one")
            e0, rest = draw_noise_img2img(seed, h, w, steps)
            key = np.asarray(kind[1]).tobytes()
            if key not in self._z:
                self._z[key] = ver.EncoderReference(self.enc_sd).moments(torch.from_numpy(np.ascontiguousarray(kind[1])[None]))
            z = ver.sample(self._z[key], e0, self.vae.cfg["scaling_factor"])
            x = (T["start"][0] * z + T["start"][1] * rest[0]).float()
            noises = rest[1:] if mutate != "noise_shift" else rest[:-1]          # noise_shift: the first step reads e1 again
        else:
            T = tables(self.abar, self.final, name, sched_kind, steps)
            l0, extra = draw_noise(seed, h, w, steps - 1, 1.0)
            scale0 = 1.0 if (T["init_scale"] is None or mutate == "init_unscaled") else T["init_scale"]
            if variation is not None:
                t, sub, base = variation
                vary = lambda a: torch.from_numpy(vr.vary_fp64(a[0].numpy(), None if base is None else np.asarray(base)[0],
                                                               None if sub is None else np.asarray(sub)[0], t).astype(np.float32))[None]
                x = vary((l0 * scale0).float()) if mutate == "blend_after_scale" else (vary(l0) * scale0).float()
            else:
                x = (l0 * scale0).float()
            noises = extra if mutate != "noise_shift" else extra[1:] + extra[:1]     # noise_shift: every step reads the next draw
        rows, ts = T["rows"], T["ts"]
        x0_prev = torch.zeros_like(x)
        trace = []
        for i, (t, row) in enumerate(zip(ts, rows)):
            if cfg:
                eu, et = self._eval(torch.cat([x, x]), t, torch.cat([ne, pe]), hint_emb, scale).chunk(2)
                m = eu + g * (et - eu) if mutate != "cfg_swapped" else et + g * (eu - et)
            else:
                m = self._eval(x, t, pe, hint_emb, scale)
            noise = noises[i] if row[5] != 0.0 else None
            if mutate == "noise_on_last" and i == len(rows) - 1 and i > 0:
                row = row[:5] + (rows[i - 1][5],)                                # the last step re-noises like the one before it
                noise = noises[i - 1]
            x, x0 = step(x, m, x0_prev, noise, tuple(float(np.float32(v)) for v in row), pred)
            x = x.float()
            if mutate != "history_stale":
                x0_prev = x0.float()
            trace.append(x.numpy().copy())
        out = dict(latents=x.numpy(), ts=np.asarray(ts, dtype=np.float64), trace=trace)
        if decode:
            out["image"] = self.vae.decode(x).numpy()
        return out


# ---- the cells that tests/test_samplers_cpu.py (mutants, on the oracle alone) and tests/test_samplers_gpu.py (parity) share ---------
# (id, form of chain_reference.FORMS, sampler, sigmas, steps, kind, size index of chain_reference.SIZES, the request of the pair the
#  oracle runs, the mutants assigned to the cell).  Forms: (a) epsilon under classifier-free guidance 3 with a negative prompt,
# (b) v-prediction without guidance, (c) v-prediction under classifier-free guidance 2.  Kinds: plain | long (a two-chunk prompt) |
# variation | control | img2img.  The two mutants of the initial scale move the state by 1 - sb(sigma_0) = 0.23 % only; they pass
# the bound where there is no guidance factor in it and five steps of the second-order sampler carry the difference.
STRENGTH = {"img2img-dpm": 0.5, "img2img-ddim": 0.7, "img2img-euler-a": 0.6}
CONTROL_SCALE = 0.8
CELLS = [
    ("euler-a-plain", "a", EULER, "normal", 3, "plain", 0, 1, ("cfg_swapped",)),
    ("euler-a-control", "a", EULER_A, "normal", 3, "control", 0, 1, ("noise_shift",)),
    ("euler-b-plain", "b", EULER, "normal", 3, "plain", 0, 1, ("wrong_prediction",)),
    ("euler-karras-b-1step", "b", EULER, "karras", 1, "plain", 0, 1, ()),
    ("dpm-b-variation", "b", DPMPP_2M, "normal", 5, "variation", 0, 0, ("blend_after_scale", "init_unscaled")),
    ("img2img-dpm", "b", DPMPP_2M, "karras", 5, "img2img", 0, 1, ("tail_off_by_one", "history_stale")),
    ("euler-a-karras-c-long", "c", EULER_A, "karras", 3, "long", 1, 1, ("noise_on_last",)),
    ("img2img-ddim", "c", DDIM, "normal", 3, "img2img", 1, 1, ()),
    ("ddim-c-plain", "c", DDIM, "normal", 5, "plain", 0, 1, ()),
    ("img2img-euler-a", "c", EULER_A, "normal", 5, "img2img", 0, 1, ()),
]


def cell_inputs(cell):
    """chain_reference.cell_inputs of the cell's form and size, plus per kind: hints uint8 [2,H,W,3] (control) and, for a long
    prompt, a second chunk of its own on the prompt and the negative embeddings ([2,154,D])."""
    import chain_reference as cr
    import controlnet_reference as cnr
    cid, form, name, kind_s, steps, kind, size = cell[:7]
    inp = cr.cell_inputs(("variation" if kind == "variation" else "img2img", form, size))
    inp["steps"] = steps
    if kind == "control":
        inp["hints"] = np.stack([cnr.test_hint(inp["width"], inp["height"], s) for s in (0, 1)])
    if kind == "long":
        more = cr.cell_inputs(("img2img", form, 1 - size))
        inp["pe"] = torch.cat([inp["pe"], more["pe"]], dim=1)
        if inp["ne"] is not None:
            inp["ne"] = torch.cat([inp["ne"], more["ne"]], dim=1)
    return inp


def oracle_run(ora, cell, inp, b, mutate=None, decode=True):
    """Request b of a cell on the oracle (its B = 1 run)."""
    cid, form, name, kind_s, steps, kind, size = cell[:7]
    k = ("plain",)
    if kind == "img2img":
        k = ("img2img", inp["pics"][b], STRENGTH[cid])
    elif kind == "control":
        k = ("control", inp["hints"][b], CONTROL_SCALE)
    ne = inp["ne"]
    return ora(inp["pe"][b:b + 1].float(), inp["width"], inp["height"], steps, inp["guidance"], inp["seeds"][b], (name, kind_s), kind=k,
               negative_embeds=None if ne is None else ne[b:b + 1].float(),
               variation=inp["variations"][b] if kind == "variation" else None, mutate=mutate, decode=decode)


def build_oracle(form, with_controlnet=False):
    """The oracle of a form on the synthetic weights tests/test_chain_matrix_gpu.py uses (forms (b) and (c) share theirs)."""
    import chain_reference as cr
    from sdlcm_amd import weights
    usd, pipe_cfg, cfg, sch = cr.form_weights(form)
    return SamplerChainOracle(usd, weights.synthetic_vae(), cfg, enc_sd=weights.synthetic_vae_encoder(),
                              cn_sd=weights.synthetic_controlnet() if with_controlnet else None, schedule=sch)
