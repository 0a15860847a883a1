"""References of the ControlNet tests (a plain module, like tests/refine_reference.py): diffusers' ControlNetModel.forward and
UNet2DConditionModel.forward with down_block_additional_residuals / mid_block_additional_residual, restated in torch fp32 from
the architecture, wrapping the CPU oracle's UNet (oracle/unet.py, imported unchanged), and the LCM sampler around them."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from oracle import glue
from oracle.scheduler import LCMSchedulerOracle
from oracle.unet import UNetOracle
from oracle.vae import VAEDecoderOracle

COND_CHANNELS = (16, 32, 96, 256)


def test_hint(width, height, seed=0):
    """A deterministic uint8 [H,W,3] hint with the structure of an edge / depth map: smooth ramps, hard edges, pure 0 and 255."""
    rng = np.random.RandomState(1234 + seed)
    y, x = np.mgrid[0:height, 0:width].astype(np.float32)
    img = np.zeros((height, width, 3), np.float32)
    img[..., 0] = 255.0 * x / max(width - 1, 1)
    img[..., 1] = 127.5 + 127.5 * np.sin(0.11 * y + 0.07 * x + seed)
    img[..., 2] = 255.0 * (((x // 16) + (y // 16)) % 2)
    for _ in range(6):
        cy, cx, r = rng.randint(0, height), rng.randint(0, width), rng.randint(4, max(5, min(width, height) // 3))
        m = (y - cy) ** 2 + (x - cx) ** 2 < r * r
        img[m] = rng.randint(0, 2, size=3) * 255.0
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)
test_hint.__test__ = False


class UNetWithResiduals(UNetOracle):
    """UNetOracle.forward with the ControlNet residuals: added to the skip list AFTER the down blocks (the encoder's own
    forward path sees the unmodified tensors) and to the mid block's output."""

    @torch.inference_mode()
    def forward(self, sample, t, ehs, timestep_cond=None, added=None, down_residuals=None, mid_residual=None):
        if down_residuals is None:
            return super().forward(sample, t, ehs, timestep_cond, added)
        cfg = self.cfg
        B = sample.shape[0]
        t = torch.as_tensor(t).reshape(-1).expand(B) if torch.as_tensor(t).numel() == 1 else torch.as_tensor(t)
        temb = self.time_embed(t, timestep_cond, added)
        x = self.conv("conv_in", sample.float())
        ehs = ehs.float()
        skips = [x]
        nb = len(cfg["block_out_channels"])
        for i in range(nb):
            for j in range(cfg["layers_per_block"]):
                x = self.resnet(f"down_blocks.{i}.resnets.{j}", x, temb)
                if cfg["down_attn"][i]:
                    x = self.transformer(f"down_blocks.{i}.attentions.{j}", x, ehs, i)
                skips.append(x)
            if i < nb - 1:
                x = self.conv(f"down_blocks.{i}.downsamplers.0.conv", x, stride=2)
                skips.append(x)
        assert len(skips) == len(down_residuals)
        skips = [s + r for s, r in zip(skips, down_residuals)]
        for i, s in enumerate(skips):
            self._tap(f"skip_mod.{i}", s)
        x = self.resnet("mid_block.resnets.0", x, temb)
        x = self.transformer("mid_block.attentions.0", x, ehs, nb - 1)
        x = self.resnet("mid_block.resnets.1", x, temb)
        x = x + mid_residual
        self._tap("mid_mod", x)
        up_attn = tuple(reversed(cfg["down_attn"]))
        for i in range(nb):
            for j in range(cfg["layers_per_block"] + 1):
                x = torch.cat([x, skips.pop()], dim=1)
                x = self.resnet(f"up_blocks.{i}.resnets.{j}", x, temb)
                if up_attn[i]:
                    x = self.transformer(f"up_blocks.{i}.attentions.{j}", x, ehs, nb - 1 - i)
            if i < nb - 1:
                tgt = tuple(skips[-1].shape[2:])
                if tgt == (2 * x.shape[2], 2 * x.shape[3]):
                    x = F.interpolate(x, scale_factor=2.0, mode="nearest")
                else:
                    x = F.interpolate(x, size=tgt, mode="nearest")
                x = self.conv(f"up_blocks.{i}.upsamplers.0.conv", x)
        x = F.silu(self.gn("conv_norm_out", x, cfg["norm_eps"]))
        return self.conv("conv_out", x)


class ControlNetOracle(UNetOracle):
    """ControlNetModel.forward: hint embedding, conv_in(sample) + embedding, the down and mid blocks, the zero convolutions,
    everything times conditioning_scale.  cfg: the UNet's config (no guidance embedding here)."""

    def __init__(self, sd, cfg=None):
        super().__init__(sd, cfg)
        self.cfg["time_cond_proj_dim"] = None
        self.cfg["addition_time_embed_dim"] = None

    def embed_hint(self, hint_u8):
        """hint uint8 [B,H,W,3] -> [B, block_out_channels[0], H/8, W/8]."""
        e = "controlnet_cond_embedding"
        x = torch.as_tensor(np.asarray(hint_u8)).permute(0, 3, 1, 2).float() / 255.0
        x = F.silu(self.conv(e + ".conv_in", x))
        self._tap("hint.0", x)
        for i in range(2 * (len(COND_CHANNELS) - 1)):
            x = F.silu(self.conv(f"{e}.blocks.{i}", x, stride=2 if i % 2 else 1))
            self._tap(f"hint.{i + 1}", x)
        x = self.conv(e + ".conv_out", x)
        self._tap("hint.7", x)
        return x

    @torch.inference_mode()
    def forward(self, sample, t, ehs, hint_u8, scale=1.0, hint_emb=None):
        """-> (12 down residuals, mid residual), scaled."""
        cfg = self.cfg
        B = sample.shape[0]
        t = torch.as_tensor(t).reshape(-1).expand(B) if torch.as_tensor(t).numel() == 1 else torch.as_tensor(t)
        temb = self.time_embed(t, None)
        x = self.conv("conv_in", sample.float()) + (self.embed_hint(hint_u8) if hint_emb is None else hint_emb)
        self._tap("cn.conv_in", x)
        ehs = ehs.float()
        feats = [x]
        nb = len(cfg["block_out_channels"])
        for i in range(nb):
            for j in range(cfg["layers_per_block"]):
                x = self.resnet(f"down_blocks.{i}.resnets.{j}", x, temb)
                if cfg["down_attn"][i]:
                    x = self.transformer(f"down_blocks.{i}.attentions.{j}", x, ehs, i)
                feats.append(x)
            if i < nb - 1:
                x = self.conv(f"down_blocks.{i}.downsamplers.0.conv", x, stride=2)
                feats.append(x)
        x = self.resnet("mid_block.resnets.0", x, temb)
        x = self.transformer("mid_block.attentions.0", x, ehs, nb - 1)
        x = self.resnet("mid_block.resnets.1", x, temb)
        down = [self.conv(f"controlnet_down_blocks.{i}", f, padding=0) * scale for i, f in enumerate(feats)]
        mid = self.conv("controlnet_mid_block", x, padding=0) * scale
        for i, (f, r) in enumerate(zip(feats, down)):
            self._tap(f"cn.feat.{i}", f)
            self._tap(f"cn.res.{i}", r)
        self._tap("cn.feat.mid", x)
        self._tap("cn.res.mid", mid)
        return down, mid


class ControlNetPipelineOracle:
    """LCMPipelineOracle with a ControlNet: StableDiffusionControlNetPipeline's loop (guess_mode False: under classifier-free
    guidance the ControlNet runs on both halves with the hint repeated)."""

    def __init__(self, unet_sd, vae_sd, cn_sd, unet_cfg=None, vae_cfg=None):
        self.unet = UNetWithResiduals(unet_sd, unet_cfg)
        self.cn = ControlNetOracle(cn_sd, unet_cfg)
        self.vae = VAEDecoderOracle(vae_sd, vae_cfg)
        self.sched = LCMSchedulerOracle()

    @torch.inference_mode()
    def __call__(self, prompt_embeds, width, height, steps, guidance_scale, seed, hint_u8=None, scale=1.0, negative_embeds=None):
        pe = torch.as_tensor(np.asarray(prompt_embeds), dtype=torch.float32)
        assert pe.shape[0] == 1
        ts = self.sched.set_timesteps(int(steps))
        lat, noises = glue.prepare_latents(seed, height, width, len(ts) - 1, self.sched.init_noise_sigma)
        tcd = self.unet.cfg.get("time_cond_proj_dim")
        cond = None
        if tcd:
            cond = torch.from_numpy(glue.guidance_scale_embedding(np.full((1,), guidance_scale - 1.0, dtype=np.float32), tcd, np.float32))
        do_cfg = guidance_scale > 1.0 and not tcd
        hint = None if hint_u8 is None else np.asarray(hint_u8).reshape(1, height, width, 3)
        emb = None if hint is None else self.cn.embed_hint(hint)
        for i, t in enumerate(ts):
            if do_cfg:
                ne = torch.as_tensor(np.asarray(negative_embeds), dtype=torch.float32)
                x2, e2 = torch.cat([lat, lat]), torch.cat([ne, pe])
                kw = {}
                if hint is not None:
                    d, m = self.cn.forward(x2, int(t), e2, None, scale, hint_emb=torch.cat([emb, emb]))
                    kw = dict(down_residuals=d, mid_residual=m)
                eu, et = self.unet.forward(x2, int(t), e2, None, **kw).chunk(2)
                eps = eu + guidance_scale * (et - eu)
            else:
                kw = {}
                if hint is not None:
                    d, m = self.cn.forward(lat, int(t), pe, None, scale, hint_emb=emb)
                    kw = dict(down_residuals=d, mid_residual=m)
                eps = self.unet.forward(lat, int(t), pe, cond, **kw)
            lat, _ = self.sched.step(eps, i, lat, noises[i] if i < len(noises) else None)
        img = self.vae.decode(lat)
        return dict(image=img.numpy(), image_u8=glue.postprocess_u8(img.numpy()), latents=lat.numpy(), timesteps=ts)
