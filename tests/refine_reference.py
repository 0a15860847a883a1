"""References of the refinement tests (a plain module, like tests/sd2_reference.py): the strength-cut LCM schedule restated with
numpy, the multi-pass chain composed from the CPU oracle's UNet / VAE / scheduler in torch fp32, and the re-noise and hand-over
step in float64 with their fp32 error bounds."""
from __future__ import annotations

import numpy as np
import torch

U32 = 2.0 ** -24            # fp32 unit roundoff


def strength_timesteps(n, d, num_train_timesteps=1000, original_inference_steps=50):
    """diffusers' LCMScheduler.set_timesteps(n, strength=d)."""
    k = num_train_timesteps // original_inference_steps
    m = int(original_inference_steps * d)
    origin = (np.arange(1, m + 1) * k - 1)[::-1]
    if n > m:
        raise ValueError("The combined original_steps x strength is smaller than num_inference_steps")
    idx = np.floor(np.linspace(0, m, num=n, endpoint=False)).astype(np.int64)
    return origin[idx].astype(np.int64)


def draw_all(seed, h, w, n):
    """The request's RNG stream: n tensors [1,4,h,w] from one CPU generator."""
    g = torch.Generator(device="cpu").manual_seed(int(seed))
    return [torch.randn((1, 4, h, w), generator=g, dtype=torch.float32) for _ in range(n)]


class RefineChainOracle:
    """x^0 = the plain request's final latents; for k = 1..p: re-noise x^{k-1} to ts_k[0], run the LCM steps over ts_k."""

    def __init__(self, unet_sd, vae_sd, unet_cfg=None, vae_cfg=None):
        from oracle.scheduler import LCMSchedulerOracle
        from oracle.unet import UNetOracle
        from oracle.vae import VAEDecoderOracle
        self.unet = UNetOracle(unet_sd, unet_cfg)
        self.vae = VAEDecoderOracle(vae_sd, vae_cfg)
        self.sched = LCMSchedulerOracle()

    def _cond(self, guidance):
        from oracle import glue
        tcd = self.unet.cfg.get("time_cond_proj_dim")
        if not tcd:
            return None
        return torch.from_numpy(glue.guidance_scale_embedding(np.full((1,), guidance - 1.0, dtype=np.float32), tcd, np.float32))

    @torch.inference_mode()
    def one_pass(self, pe, lat, ts, noises, guidance):
        """The LCM steps over ``ts`` from state ``lat`` with len(ts) - 1 step noises -> denoised latents."""
        self.sched.timesteps = np.asarray(ts, dtype=np.int64)
        cond = self._cond(guidance)
        for i, t in enumerate(ts):
            eps = self.unet.forward(lat, int(t), pe, cond)
            lat, _ = self.sched.step(eps, i, lat, noises[i] if i < len(noises) else None)
        return lat

    @torch.inference_mode()
    def renoise(self, x, t0, eps):
        a = float(self.sched.alphas_cumprod[int(t0)])
        return (a ** 0.5) * x + ((1 - a) ** 0.5) * eps

    @torch.inference_mode()
    def __call__(self, prompt_embeds, width, height, steps, guidance, seed, d, p, starts=None):
        """-> dict(xk=[x^0..x^p] numpy, image NCHW float, image_u8 NHWC).  starts: optional {k: x^{k-1} to start pass k from}
        (numpy [1,4,h,w]) -- runs pass k from the given latents instead of this chain's own (isolates one pass)."""
        from oracle import glue
        pe = torch.as_tensor(np.asarray(prompt_embeds), dtype=torch.float32)
        h, w = height // 8, width // 8
        draws = draw_all(seed, h, w, steps * (p + 1))
        ts0 = self.sched.set_timesteps(int(steps)).copy()
        x = self.one_pass(pe, draws[0] * self.sched.init_noise_sigma, ts0, draws[1:steps], guidance)
        xs = [x]
        ts = strength_timesteps(steps, d)
        for k in range(1, p + 1):
            dk = draws[steps * k: steps * (k + 1)]
            src = torch.as_tensor(starts[k]) if starts and k in starts else x
            x = self.one_pass(pe, self.renoise(src, ts[0], dk[0]), ts, dk[1:], guidance)
            xs.append(x)
        img = self.vae.decode(x).numpy()
        return dict(xk=[t.numpy() for t in xs], image=img, image_u8=glue.postprocess_u8(img), timesteps=ts)


def renoise_fp64(x, n, sa, sb):
    """-> (sa x + sb n in float64 from the fp32 operands, the issue's per-element bound 4 U (|sa x| + |sb n|))."""
    sa, sb = float(np.float32(sa)), float(np.float32(sb))
    x, n = np.asarray(x, np.float64), np.asarray(n, np.float64)
    return sa * x + sb * n, 4 * U32 * (np.abs(sa * x) + np.abs(sb * n))
