"""References of the hires-fix tests (a plain module, like tests/refine_reference.py): A1111's three latent upscalers restated
in numpy float64 from EXACT integer source coordinates, the fused re-noise, and the two-stage sampler composed from the CPU
oracle's UNet / VAE / scheduler and tests/refine_reference.py.

Source coordinate of output index d along an axis of `n_in` source and `n_out` output elements (torch's align_corners=False
mapping (d + 0.5) n_in / n_out - 0.5) = ((2 d + 1) n_in - n_out) / (2 n_out): floor and fraction come from integer division, so
the reference never multiplies by a rounded n_in / n_out."""
from __future__ import annotations

import numpy as np
import torch

import refine_reference as rr

U32 = 2.0 ** -24
BILINEAR, BICUBIC, NEAREST_EXACT = 0, 1, 2
MODES = (BILINEAR, BICUBIC, NEAREST_EXACT)
TORCH_MODE = {BILINEAR: "bilinear", BICUBIC: "bicubic", NEAREST_EXACT: "nearest-exact"}
UPSCALER_NAME = {BILINEAR: "Latent", BICUBIC: "Latent (bicubic)", NEAREST_EXACT: "Latent (nearest-exact)"}

# (h, w) -> (H, W) of the operator tests on the GPU (the issue's list)
SHAPES = (((8, 8), (16, 16)), ((8, 8), (12, 12)), ((9, 5), (17, 11)), ((1, 1), (3, 3)), ((3, 2), (12, 8)), ((64, 64), (96, 96)))


def nearest_ties(n_in, n_out):
    """Output indices whose nearest-exact source coordinate (d + 0.5) n_in / n_out is an exact integer: there a floating-point
    evaluation may land on either side of the floor, the exact rational does not."""
    return [d for d in range(n_out) if ((2 * d + 1) * n_in) % (2 * n_out) == 0]


def _cubic(t):
    A = -0.75
    near = lambda x: ((A + 2) * x - (A + 3)) * x * x + 1
    far = lambda x: ((A * x - 5 * A) * x + 8 * A) * x - 4 * A
    return [far(t + 1), near(t), near(1 - t), far(2 - t)]


def axis_taps(mode, n_in, n_out):
    """-> (idx int [n_out, k], wt float64 [n_out, k]): the k source indices (clamped) and weights of every output index."""
    d = np.arange(n_out, dtype=np.int64)
    den = 2 * n_out
    if mode == NEAREST_EXACT:
        return np.minimum(((2 * d + 1) * n_in) // den, n_in - 1)[:, None], np.ones((n_out, 1))
    num = (2 * d + 1) * n_in - n_out
    if mode == BILINEAR:                                   # the coordinate is clamped at 0
        num = np.maximum(num, 0)
        i0 = num // den
        t = (num - i0 * den).astype(np.float64) / den
        return np.stack([np.minimum(i0, n_in - 1), np.minimum(i0 + 1, n_in - 1)], 1), np.stack([1 - t, t], 1)
    fl = np.floor_divide(num, den)                         # bicubic: floor of a possibly negative rational, not clamped
    t = (num - fl * den).astype(np.float64) / den
    idx = np.stack([np.clip(fl - 1 + k, 0, n_in - 1) for k in range(4)], 1)
    return idx, np.stack(_cubic(t), 1)


def upscale_fp64(x, H, W, mode):
    """x [..., h, w] -> float64 [..., H, W]."""
    x = np.asarray(x, np.float64)
    iy, wy = axis_taps(mode, x.shape[-2], H)
    ix, wx = axis_taps(mode, x.shape[-1], W)
    rows = sum(x[..., iy[:, k], :] * wy[:, k][:, None] for k in range(iy.shape[1]))          # [..., H, w]
    return sum(rows[..., :, ix[:, k]] * wx[:, k] for k in range(ix.shape[1]))


def upscale_renoise_fp64(x0, noise, sa, sb, H, W, mode):
    """-> (up(x0), sa up(x0) + sb noise) in float64 from the fp32 operands, coefficients as the kernel receives them."""
    sa, sb = float(np.float32(sa)), float(np.float32(sb))
    up = upscale_fp64(x0, H, W, mode)
    return up, sa * up + sb * np.asarray(noise, np.float64)


def operator_tolerance(x0, noise):
    """The issue's bound on |kernel - fp64|: 64 x 2^-24 x (max|x0| + max|noise|) -- at most 4 x 4 taps with correctly rounded
    weights and sum|w| <= 1.375 per axis (bicubic), then two products and one add."""
    return 64 * U32 * (float(np.abs(x0).max()) + float(np.abs(noise).max()))


def torch_upscale(x, H, W, mode):
    """torch.nn.functional.interpolate in float64, A1111's call (align_corners=False where the mode takes it, antialias=False)."""
    t = torch.as_tensor(np.asarray(x, np.float64))
    if mode == NEAREST_EXACT:
        return torch.nn.functional.interpolate(t, size=(H, W), mode="nearest-exact").numpy()
    return torch.nn.functional.interpolate(t, size=(H, W), mode=TORCH_MODE[mode], align_corners=False, antialias=False).numpy()


def draw_hires(seed, h, w, steps, h2, w2, hr_steps):
    """The request's RNG stream: ``steps`` tensors [1,4,h,w], then ``hr_steps`` tensors [1,4,h2,w2], from one CPU generator."""
    g = torch.Generator(device="cpu").manual_seed(int(seed))
    lo = [torch.randn((1, 4, h, w), generator=g, dtype=torch.float32) for _ in range(steps)]
    hi = [torch.randn((1, 4, h2, w2), generator=g, dtype=torch.float32) for _ in range(hr_steps)]
    return lo, hi


class HiresChainOracle(rr.RefineChainOracle):
    """Stage 1: the plain request at (width, height); hand-over: upscale its final latents (float64 weights, result in fp32),
    re-noise to ts2[0]; stage 2: the LCM steps over ts2 = timesteps(hr_steps, strength) at the target size; one decode."""

    @torch.inference_mode()
    def one_pass(self, pe, lat, ts, noises, guidance, negative=None):
        if self.unet.cfg.get("time_cond_proj_dim") or guidance <= 1.0:
            return super().one_pass(pe, lat, ts, noises, guidance)
        self.sched.timesteps = np.asarray(ts, dtype=np.int64)           # classifier-free guidance (oracle/pipeline.py)
        for i, t in enumerate(ts):
            eu, et = self.unet.forward(torch.cat([lat, lat]), int(t), torch.cat([negative, pe]), None).chunk(2)
            lat, _ = self.sched.step(eu + guidance * (et - eu), i, lat, noises[i] if i < len(noises) else None)
        return lat

    @torch.inference_mode()
    def __call__(self, prompt_embeds, width, height, steps, guidance, seed, hires, negative_embeds=None):
        """hires = (W2, H2, hr_steps, strength, mode) -> dict(lowres, upscaled, latents numpy; image NCHW float; image_u8)."""
        from oracle import glue
        W2, H2, hr_steps, strength, mode = hires
        pe = torch.as_tensor(np.asarray(prompt_embeds), dtype=torch.float32)
        ne = None if negative_embeds is None else torch.as_tensor(np.asarray(negative_embeds), dtype=torch.float32)
        h, w, h2, w2 = height // 8, width // 8, H2 // 8, W2 // 8
        lo, hi = draw_hires(seed, h, w, steps, h2, w2, hr_steps)
        ts1 = self.sched.set_timesteps(int(steps)).copy()
        x = self.one_pass(pe, lo[0] * self.sched.init_noise_sigma, ts1, lo[1:], guidance, ne)
        up = torch.from_numpy(upscale_fp64(x.numpy(), h2, w2, mode).astype(np.float32))
        ts2 = rr.strength_timesteps(hr_steps, strength)
        y = self.one_pass(pe, self.renoise(up, ts2[0], hi[0]), ts2, hi[1:], guidance, ne)
        img = self.vae.decode(y).numpy()
        return dict(lowres=x.numpy(), upscaled=up.numpy(), latents=y.numpy(), image=img, image_u8=glue.postprocess_u8(img),
                    timesteps=ts2)
