"""One CPU oracle of the sampler chain for every request kind, guidance form and prediction type (a plain module, like
tests/refine_reference.py), and the matrix of cells that tests/test_chain_matrix_cpu.py and tests/test_chain_matrix_gpu.py share.

The oracle composes the fp32 torch parts the suite already trusts and copies none of them: oracle.unet.UNetOracle,
oracle.vae.VAEDecoderOracle, oracle.scheduler.LCMSchedulerOracle (its coefficients and its epsilon step),
vae_encoder_reference.EncoderReference / sample / add_noise, hires_reference.upscale_fp64, variation_reference.vary_fp64 and
refine_reference.strength_timesteps.  The RNG streams are the product's own (draw_noise, draw_noise_img2img, draw_noise_hires;
a variation's tensors come from draw_variation_sources, drawn by the caller).  Where a trusted chain oracle exists
(RefineChainOracle, HiresChainOracle, inpaint_reference.cpu_chain, LCMPipelineOracle) this one gives its final latents bit for
bit: the arithmetic is written in the same order on purpose (tests/test_chain_matrix_cpu.py holds it to that).

``mutate=`` names one wiring mistake, stated on the oracle's side; MUTANTS lists which apply where.  A variation applied after
the initial sigma scaling instead of before ("blend_after_sigma") is NOT among them: init_noise_sigma is 1.0 for every LCM
schedule (oracle.scheduler and sdlcm_amd.scheduler both fix it), so the two orders are the same numbers and cannot differ."""
from __future__ import annotations

import numpy as np
import torch

import hires_reference as hr
import refine_reference as rr
import vae_encoder_reference as ver
import variation_reference as vr

PLAIN = ("plain",)


def refine(d, p):
    return ("refine", float(d), int(p))


def hires(tw, th, hr_steps, strength, mode):
    return ("hires", int(tw), int(th), int(hr_steps), float(strength), int(mode))


def img2img(pic, strength):
    return ("img2img", pic, float(strength))


def inpaint(pic, latmask, strength):
    return ("inpaint", pic, latmask, float(strength))


CFG_MUTANTS = ("cfg_swapped", "cfg_dropped", "neg_rows_rotated", "uncond_state_stale")
MUTANTS = {
    "plain": ("wrong_prediction",),
    "refine": ("wrong_prediction", "noise_shift", "renoise_at_next"),
    "hires": ("wrong_prediction", "renoise_at_next"),
    "img2img": ("wrong_prediction", "noise_shift", "renoise_at_next"),
    "inpaint": ("wrong_prediction", "noise_shift", "renoise_at_next", "kept_at_current", "kept_noised_at_end"),
}


def mutants_of(kind, cfg):
    """The mutants that apply to a cell: the kind's own, and under classifier-free guidance the four of the doubled rows."""
    return MUTANTS[kind] + (CFG_MUTANTS if cfg else ())


class ChainOracle:
    """prediction_type "epsilon" | "v_prediction"; schedule: None (the default LCM schedule) or a dict such as
    sdlcm_amd.scheduler.SD21_768_SCHEDULE (its betas and, unless prediction_type is given, its prediction type).  The guidance
    form follows the UNet config: the guidance embedding when it has time_cond_proj_dim, otherwise classifier-free guidance on
    cat([negative, prompt]) rows for guidance above 1."""

    def __init__(self, unet_sd, vae_sd, unet_cfg=None, vae_cfg=None, enc_sd=None, schedule=None, prediction_type=None):
        from oracle.scheduler import LCMSchedulerOracle
        from oracle.unet import UNetOracle
        from oracle.vae import VAEDecoderOracle
        sch = dict(schedule or {})
        self.unet = UNetOracle(unet_sd, unet_cfg)
        self.vae = VAEDecoderOracle(vae_sd, vae_cfg)
        self.sched = LCMSchedulerOracle(**{k: sch[k] for k in ("num_train_timesteps", "beta_start", "beta_end") if k in sch})
        self.pred = prediction_type or sch.get("prediction_type", "epsilon")
        if self.pred not in ("epsilon", "v_prediction"):
            raise ValueError(self.pred)
        self.enc_sd = enc_sd
        self._z = {}
        self._evals = {}              # UNet evaluations by their exact inputs: a mutant shares every one ahead of its mistake

    # ---- the parts ------------------------------------------------------------------------------------------------------------
    def do_cfg(self, guidance):
        return guidance > 1.0 and not self.unet.cfg.get("time_cond_proj_dim")

    def _cond(self, guidance):
        from oracle import glue
        tcd = self.unet.cfg.get("time_cond_proj_dim")
        if not tcd:
            return None
        return torch.from_numpy(glue.guidance_scale_embedding(np.full((1,), guidance - 1.0, dtype=np.float32), tcd, np.float32))

    def _step(self, out, i, x, noise, pred):
        """LCMScheduler.step: the oracle scheduler's own for epsilon; for v_prediction its coefficients with
        x0 = sqrt(a) x - sqrt(1 - a) v, the step tests/test_sd2_gpu.py's _oracle_scheduler restates."""
        if pred == "epsilon":
            return self.sched.step(out, i, x, noise)[0]
        sa, sb, c_skip, c_out, sap, sbp, last = self.sched.coefficients(i)
        den = c_out * (sa * x - sb * out) + c_skip * x
        return den if last else sap * den + sbp * noise

    def _unet(self, x, t, ctx, cond):
        key = (int(t), x.numpy().tobytes(), ctx.numpy().tobytes(), None if cond is None else cond.numpy().tobytes())
        if key not in self._evals:
            self._evals[key] = self.unet.forward(x, int(t), ctx, cond)
        return self._evals[key]

    def forget(self):
        """Drop the remembered UNet evaluations and encoder moments (they are kept per oracle, for the mutants of one cell)."""
        self._evals.clear()
        self._z.clear()

    def renoise(self, x, t):
        return lambda e: ver.add_noise(x, e, float(self.sched.alphas_cumprod[int(t)]))

    def init_latents_of(self, pic, e0):
        """The posterior sample of the reference encoder (fp32), times the VAE's scaling factor; the moments are kept per picture."""
        key = pic.tobytes()
        if key not in self._z:
            self._z[key] = ver.EncoderReference(self.enc_sd).moments(torch.from_numpy(np.ascontiguousarray(pic)[None]))
        return ver.sample(self._z[key], e0, self.vae.cfg["scaling_factor"])

    def _pass(self, c, x, ts, noises, keep=None):
        """The LCM steps over ts from state x with the len(ts) - 1 step noises.  keep = (M, z, e1): after every step the cells
        outside M go back to z re-noised with e1 to the NEXT timestep, z itself after the last step."""
        self.sched.timesteps = np.asarray(ts, dtype=np.int64)
        g, pe, ne, m = c["g"], c["pe"], c["ne"], c["mutate"]
        pred = self.pred
        if m == "wrong_prediction":
            pred = "v_prediction" if pred == "epsilon" else "epsilon"
        xu = x                                            # the unconditional half of the state
        for i, t in enumerate(ts):
            last = i == len(ts) - 1
            if c["cfg"]:
                eu, et = self._unet(torch.cat([xu, x]), t, torch.cat([ne, pe]), None).chunk(2)
                out = eu + g * (et - eu)
                if m == "cfg_swapped":
                    out = et + g * (eu - et)
                elif m == "cfg_dropped":
                    out = et
            else:
                out = self._unet(x, t, pe, c["cond"])
            x = self._step(out, i, x, None if last else noises[i], pred)
            if keep is not None:
                M, z, e1 = keep
                kept = z if last else self.renoise(z, ts[i + 1])(e1)
                if m == "kept_at_current":
                    kept = self.renoise(z, ts[i])(e1)
                elif m == "kept_noised_at_end" and last:
                    kept = self.renoise(z, ts[i])(e1)
                x = torch.where(M, x, kept.to(x.dtype))
            if m != "uncond_state_stale":
                xu = x
            c["trace"].append(x.numpy().copy())
        return x

    # ---- the chains -----------------------------------------------------------------------------------------------------------
    @torch.inference_mode()
    def __call__(self, prompt_embeds, width, height, steps, guidance, seed, kind=PLAIN, negative_embeds=None, variation=None,
                 mutate=None, other_negative_embeds=None, decode=True):
        """One request (B = 1).  kind: PLAIN | refine(d, p) | hires(tw, th, hr_steps, strength, mode) | img2img(pic, strength) |
        inpaint(pic, latmask, strength); pic uint8 [H,W,3], latmask [h,w] of 0 / 1.  variation = (t, sub, base | None), host fp32
        [1,4,hs,ws] as ``generate(variation=)`` takes them: blended into the initial latents (plain, refine, hires).
        other_negative_embeds: the negative embeddings of the OTHER request of a pair, read by mutate="neg_rows_rotated" only.
        -> dict(latents [1,4,h,w]; image NCHW float (before any overlay); latents0; trace: the state after every step, in order;
        per kind lowres / upscaled / xk / z)."""
        from sdlcm_amd.pipeline import draw_noise, draw_noise_hires, draw_noise_img2img
        name = kind[0]
        f32 = lambda a: None if a is None else torch.as_tensor(np.asarray(a), dtype=torch.float32)
        cfg = self.do_cfg(guidance)
        if mutate is not None and mutate not in mutants_of(name, cfg):
            raise ValueError(f"mutant {mutate!r} does not apply to a {name} chain" + (" without classifier-free guidance" if not cfg else ""))
        ne = f32(other_negative_embeds if mutate == "neg_rows_rotated" else negative_embeds) if cfg else None
        c = dict(g=guidance, pe=f32(prompt_embeds), ne=ne, cfg=cfg, cond=self._cond(guidance), mutate=mutate, trace=[])
        h, w, sigma = height // 8, width // 8, self.sched.init_noise_sigma
        first = 1 if mutate == "renoise_at_next" else 0           # the timestep index the front re-noise goes to
        out = {}

        def start(l0):
            if variation is not None:
                if name in ("img2img", "inpaint"):
                    raise ValueError("a variation acts on the initial noise: not combined with a picture")
                t, sub, base = variation
                l0 = torch.from_numpy(vr.vary_fp64(l0[0].numpy(), None if base is None else np.asarray(base)[0],
                                                   None if sub is None else np.asarray(sub)[0], t).astype(np.float32))[None]
            out["latents0"] = l0.numpy().copy()
            return l0

        if name == "plain":
            l0, extra = draw_noise(seed, h, w, steps - 1, sigma)
            x = self._pass(c, start(l0), self.sched.set_timesteps(int(steps)).copy(), extra)
        elif name == "refine":
            _, d, p = kind
            l0, extra = draw_noise(seed, h, w, steps * (p + 1), sigma)       # one more than the chain needs: noise_shift's last read
            draws = [l0] + extra
            x = self._pass(c, start(l0), self.sched.set_timesteps(int(steps)).copy(), draws[1:steps])
            xs = [x]
            ts = rr.strength_timesteps(steps, d)
            for k in range(1, p + 1):
                dk = draws[steps * k: steps * (k + 1)]
                step_noises = dk[1:]
                if mutate == "noise_shift" and step_noises:               # the next pass's first draw in place of this pass's first step noise
                    step_noises = [draws[steps * (k + 1)]] + step_noises[1:]
                x = self._pass(c, self.renoise(x, ts[first])(dk[0]), ts, step_noises)
                xs.append(x)
            out["xk"] = [t.numpy() for t in xs]
        elif name == "hires":
            _, tw, th, hr_steps, strength, mode = kind
            h2, w2 = th // 8, tw // 8
            l0, lo, hi = draw_noise_hires(seed, h, w, steps, h2, w2, hr_steps, sigma)
            low = self._pass(c, start(l0), self.sched.set_timesteps(int(steps)).copy(), lo)
            up = torch.from_numpy(hr.upscale_fp64(low.numpy(), h2, w2, mode).astype(np.float32))
            ts = rr.strength_timesteps(hr_steps, strength)
            x = self._pass(c, self.renoise(up, ts[first])(hi[0]), ts, hi[1:])
            out.update(lowres=low.numpy(), upscaled=up.numpy())
        elif name in ("img2img", "inpaint"):
            pic, strength = kind[1], kind[-1]
            e0, rest = draw_noise_img2img(seed, h, w, steps)
            e1, step_noises = rest[0], rest[1:]
            if mutate == "noise_shift":                                   # the first step reads e1 again
                step_noises = rest[:-1]
            z = self.init_latents_of(pic, e0)
            ts = rr.strength_timesteps(steps, strength)
            keep = None
            if name == "inpaint":
                keep = (torch.from_numpy(np.asarray(kind[2]).astype(bool))[None, None], z, e1)
            x = self._pass(c, self.renoise(z, ts[first])(e1), ts, step_noises, keep)
            out["z"] = z.numpy()
        else:
            raise ValueError(f"unknown kind {name!r}")
        out.update(latents=x.numpy(), trace=c["trace"])
        if decode:
            out["image"] = self.vae.decode(x).numpy()
        return out


def image01(x_nchw):
    """NCHW float in ~[-1,1] -> the [0,1] image the parity bound speaks of."""
    return np.clip(np.asarray(x_nchw) / 2 + 0.5, 0, 1)


# ---- the matrix ---------------------------------------------------------------------------------------------------------------
# The parity bounds of every cell: |delta| < IMG_TOL per pixel of the decoded [0,1] image (the project's parity bound), and on the
# final latents max |delta| < LATENT_REL_TOL x max(1, guidance) x std(oracle latents) -- a few fp16 roundings per step at the scale
# of the data, times the guidance scale under classifier-free guidance since eps_u + g (eps_t - eps_u) carries g times the
# rounding of its two inputs (tests/test_configs_gpu.py, tests/test_sd2_gpu.py).
IMG_TOL = 1e-2
LATENT_REL_TOL = 5e-3
SEPARATION = 10           # a mutant lies at least this many bounds from the true oracle (a condition, not a fit)

# form -> (UNet, prediction type, guidance): (a) SD1.5-shaped UNet without the guidance embedding, epsilon, classifier-free
# guidance; (b) the synthetic SD 2.1-768 UNet on its v-prediction schedule without guidance; (c) the same under classifier-free guidance
FORMS = {"a": ("nocond", "epsilon", 3.0), "b": ("sd2", "v_prediction", 1.0), "c": ("sd2", "v_prediction", 2.0)}
STRENGTH, REFINE, MASK_BLUR = 0.5, (0.6, 2), 4
# Steps per form.  Two where two show the wiring; three under form (a): its latents are large (std ~ 20 against ~ 0.9 under (b) and
# (c)) and the decode saturates, so with two steps a stale unconditional state moved the [0,1] image of the refine and variation
# cells by 0.10 - 0.11 only, at the condition's edge.  With three steps the state is stale for two of them: 0.20 and more.
STEPS = {"a": 3, "b": 2, "c": 2}
HIRES = (2, 0.7)          # hr_steps, strength; the target is 1.5 x the base size
SEEDS = (7100, 7101)
EMBED_OFFSET = 1.5        # the shared direction of an embedding's tokens, per coordinate +- this (cell_inputs)
SIZES = ((64, 64), (64, 96))          # (width, height): 8 x 8 latents, and 12 rows of 8 so that a transposed or mis-pitched state shows

# (kind, form, size index): every cell the chain-level comparison did not reach, the variation under both classifier-free forms,
# and per kind one cell at the non-square size (under form (c): doubled rows and v-prediction at once)
CELLS = [(k, f, 0) for k, fs in (("hires", "bc"), ("refine", "abc"), ("img2img", "abc"), ("inpaint", "abc"), ("variation", "ac"))
         for f in fs] + [(k, "c", 1) for k in ("hires", "refine", "img2img", "inpaint", "variation")]


def cell_id(cell):
    k, f, s = cell
    return f"{k}-{f}-{SIZES[s][0]}x{SIZES[s][1]}"


def picture(h, w, seed):
    """A smooth picture with some texture (seeded), uint8 [h, w, 3]."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([128 + 100 * np.sin(x / 7.0 + seed), 128 + 100 * np.cos(y / 5.0), 128 + 90 * np.sin((x + y) / 9.0)], -1)
    return np.clip(base + rng.normal(0, 12, (h, w, 3)), 0, 255).astype(np.uint8)


def form_weights(form):
    """-> (unet_sd, unet_cfg as the pipeline takes it, full UNet config, schedule dict | None) of a form."""
    from sdlcm_amd import weights
    from sdlcm_amd.config import SD2_UNET, unet_config
    from sdlcm_amd.scheduler import SD21_768_SCHEDULE
    if FORMS[form][0] == "nocond":
        nocond = dict(time_cond_proj_dim=None)
        return weights.synthetic_unet(nocond), nocond, unet_config(nocond), None
    cfg = unet_config(SD2_UNET)
    return weights.synthetic_sd2_unet(), cfg, cfg, dict(SD21_768_SCHEDULE)


def cell_inputs(cell):
    """Everything a cell's two requests consist of -> dict(width, height, guidance, seeds, pe, ne (fp16 [2,77,D]; ne None without
    classifier-free guidance), pics uint8 [2,H,W,3], masks uint8 [2,H,W] (half planes whose edge lies inside a latent cell: the
    right part from x = 28, the lower part from y = 36), variations: per request (t, sub, base | None) -- request 0 blended in
    place, request 1 with a seed-resize from a 10 x 6 source -- with the seeds chosen so that no column is near the blend's
    branch limit)."""
    from sdlcm_amd.pipeline import draw_variation_sources
    kind, form, s = cell
    W, H = SIZES[s]
    g = FORMS[form][2]
    D = 768 if FORMS[form][0] == "nocond" else 1024
    gen = torch.Generator().manual_seed(4300 + 10 * s + ord(form))
    # Every embedding is noise around a direction of its own that all 77 tokens of it share, as the tokens of a real prompt do: a
    # cross-attention over pure noise averages 77 independent rows to almost nothing, the prompt would barely reach the picture
    # and the mutants of the guidance wiring could not be told from the truth.
    pe, ne = ((torch.randn(2, 77, D, generator=gen) + EMBED_OFFSET * torch.sign(torch.randn(2, 1, D, generator=gen))).to(torch.float16)
              for _ in range(2))
    pics = np.stack([picture(H, W, 51), picture(H, W, 52)])
    masks = np.zeros((2, H, W), np.uint8)
    masks[0, :, 28:] = 255
    masks[1, 36:, :] = 255
    seeds, var = list(SEEDS), None
    if kind == "variation":
        h, w = H // 8, W // 8
        s0, sub0, _, _ = vr.seed_pair(h, w, start=7100)
        s1, sub1, _, _ = vr.seed_pair(10, 6, start=7200)
        seeds = [s0, s1]
        var = [(0.5,) + draw_variation_sources(s0, sub0, h, w), (0.3,) + draw_variation_sources(s1, sub1, 10, 6, resized=True)]
    return dict(width=W, height=H, steps=STEPS[form], guidance=g, seeds=seeds, pe=pe, ne=ne if g > 1.0 else None, pics=pics, masks=masks, variations=var)


def oracle_kind(cell, inp, b, latmask=None):
    """The oracle's kind argument of request b of a cell (latmask: the [h,w] mask of an inpaint request)."""
    kind = cell[0]
    W, H = inp["width"], inp["height"]
    if kind == "refine":
        return refine(*REFINE)
    if kind == "hires":
        return hires(W * 3 // 2, H * 3 // 2, HIRES[0], HIRES[1], (hr.BICUBIC, hr.BILINEAR)[cell[2]])
    if kind == "img2img":
        return img2img(inp["pics"][b], STRENGTH)
    if kind == "inpaint":
        return inpaint(inp["pics"][b], latmask, STRENGTH)
    return PLAIN


def oracle_run(ora, cell, inp, b, latmask=None, mutate=None, decode=True):
    """Request b of a cell on the oracle (its B = 1 run)."""
    ne = inp["ne"]
    return ora(inp["pe"][b:b + 1].float(), inp["width"], inp["height"], inp["steps"], inp["guidance"], inp["seeds"][b],
               kind=oracle_kind(cell, inp, b, latmask), negative_embeds=None if ne is None else ne[b:b + 1].float(),
               other_negative_embeds=None if ne is None else ne[1 - b:2 - b].float(),
               variation=inp["variations"][b] if inp["variations"] else None, mutate=mutate, decode=decode)


def latent_bound(guidance, ref_latents):
    return LATENT_REL_TOL * max(1.0, guidance) * float(np.std(ref_latents))
