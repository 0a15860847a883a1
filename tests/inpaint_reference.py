"""References of the inpainting tests (a plain module, like tests/vae_encoder_reference.py): the integer mask rules of
include/lcm_hip.h restated with numpy -- A1111's Gaussian mask blur as a 16.16 fixed-point separable filter with replicated
edges, the 8 x 8 reduction to the binary latent mask, the integer overlay -- a float64 Gaussian with the same borders to judge
the fixed-point one, and the CPU chain: diffusers' StableDiffusionInpaintPipeline latent loop (4-channel UNet: after every step
the cells outside the mask go back to the init picture's latents, re-noised with the SAME noise to the next timestep) over the
strength-cut LCM schedule, composed from the CPU oracle."""
from __future__ import annotations

import numpy as np
import torch

import refine_reference as rr
import vae_encoder_reference as ver


def blur_radius(sigma: float) -> int:
    """A1111: kernel_size = 2 * int(2.5 * mask_blur + 0.5) + 1."""
    return int(2.5 * float(sigma) + 0.5)


def gaussian(sigma: float) -> np.ndarray:
    """float64 taps g_k / sum g, k = -r .. r (cv2.GaussianBlur's kernel for an explicit sigma)."""
    r = blur_radius(sigma)
    k = np.arange(-r, r + 1, dtype=np.float64)
    g = np.exp(-(k ** 2) / (2.0 * float(sigma) ** 2))
    return g / g.sum()


def blur_weights(sigma: float) -> np.ndarray:
    """int64 [2 r + 1]: floor(65536 g_k / sum g), the remainder on the centre tap -> the sum is 65536 exactly."""
    g = gaussian(sigma)
    w = np.floor(65536.0 * g).astype(np.int64)
    w[len(w) // 2] += 65536 - w.sum()
    return w


def _gather(m, axis, r):
    """[2 r + 1, ...]: m shifted by k = -r .. r along ``axis`` with the index clamped (edge replicated)."""
    n = m.shape[axis]
    idx = np.clip(np.arange(n)[None, :] + np.arange(-r, r + 1)[:, None], 0, n - 1)
    return np.stack([np.take(m, idx[k], axis=axis) for k in range(2 * r + 1)])


def blur_pass(m: np.ndarray, w: np.ndarray, axis: int) -> np.ndarray:
    """uint8 [..] -> uint8: (sum_k w_k m[clamp(i + k)] + 32768) >> 16 along ``axis``."""
    r = len(w) // 2
    acc = np.tensordot(w.astype(np.int64), _gather(m.astype(np.int64), axis, r), axes=(0, 0))
    assert acc.max(initial=0) <= 255 * 65536
    return ((acc + 32768) >> 16).astype(np.uint8)


def blur(m: np.ndarray, sigma: float) -> np.ndarray:
    """mask uint8 [B,H,W] -> alpha uint8 [B,H,W]: horizontal pass, then vertical pass on its uint8 result; sigma 0: the mask."""
    if blur_radius(sigma) == 0:
        return m.copy()
    w = blur_weights(sigma)
    return blur_pass(blur_pass(m, w, axis=2), w, axis=1)


def blur_float64(m: np.ndarray, sigma: float) -> np.ndarray:
    """The same separable Gaussian, clamped borders, in float64 without any rounding -> float64 [B,H,W]."""
    g = gaussian(sigma)
    r = len(g) // 2
    t = np.tensordot(g, _gather(m.astype(np.float64), 2, r), axes=(0, 0))
    return np.tensordot(g, _gather(t, 1, r), axes=(0, 0))


def latent_mask(alpha: np.ndarray) -> np.ndarray:
    """alpha uint8 [B,H,W] (H, W multiples of 8) -> uint8 [B,H/8,W/8]: 1 where the 8 x 8 block mean is >= 127.5."""
    B, H, W = alpha.shape
    s = alpha.astype(np.int64).reshape(B, H // 8, 8, W // 8, 8).sum(axis=(2, 4))
    return (2 * s >= 64 * 255).astype(np.uint8)


def composite(gen: np.ndarray, init: np.ndarray, alpha: np.ndarray) -> np.ndarray:
    """uint8 [B,H,W,3] x 2, alpha uint8 [B,H,W] -> (alpha gen + (255 - alpha) init + 127) // 255."""
    a = alpha.astype(np.int64)[..., None]
    return ((a * gen.astype(np.int64) + (255 - a) * init.astype(np.int64) + 127) // 255).astype(np.uint8)


def cpu_chain(ora: rr.RefineChainOracle, enc_sd, pe, pic, latmask, steps, strength, seed, scaling=0.18215):
    """reference encoder (fp32) -> posterior sample (e0) -> add_noise (e1) at ts[0] -> per step: UNet, LCMScheduler.step, then
    x <- M ? x : (z on the last step, else add_noise(z, e1, ts[i + 1])) -> decode.  pic uint8 [H,W,3]; latmask [h,w] of 0 / 1 (the
    integer mask path is exact, so the caller hands over the mask the GPU used and has verified it against ``latent_mask``).
    -> dict(z, latents, image (NCHW float, before the overlay))."""
    from sdlcm_amd.pipeline import draw_noise_img2img
    h, w = pic.shape[0] // 8, pic.shape[1] // 8
    e0, rest = draw_noise_img2img(seed, h, w, steps)
    e1, step_noises = rest[0], rest[1:]
    z = ver.sample(ver.EncoderReference(enc_sd).moments(torch.from_numpy(pic[None])), e0, scaling)
    ts = rr.strength_timesteps(steps, strength)
    M = torch.from_numpy(np.asarray(latmask).astype(bool))[None, None]
    with torch.inference_mode():
        ora.sched.timesteps = np.asarray(ts, dtype=np.int64)
        cond = ora._cond(1.0)
        x = ora.renoise(z, ts[0], e1)
        for i, t in enumerate(ts):
            eps = ora.unet.forward(x, int(t), pe, cond)
            last = i == len(ts) - 1
            x, _ = ora.sched.step(eps, i, x, None if last else step_noises[i])
            kept = z if last else ora.renoise(z, ts[i + 1], e1)
            x = torch.where(M, x, kept.to(x.dtype))
        img = ora.vae.decode(x).numpy()
    return dict(z=z.numpy(), latents=x.numpy(), image=img)
