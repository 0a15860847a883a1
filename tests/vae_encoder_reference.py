"""References of the image-to-image tests (a plain module, like tests/hires_reference.py).

1. A torch-CPU restatement of diffusers' AutoencoderKL ``Encoder`` + ``quant_conv`` + ``DiagonalGaussianDistribution.sample`` +
   ``LCMScheduler.add_noise``, written from the module semantics (diffusers is not installed): conv_in, four down blocks of two
   ResnetBlock2D (GroupNorm 32 groups eps 1e-6 -> SiLU -> conv3x3, twice, 1x1 conv_shortcut where the width changes) with a
   Downsample2D after the first three (F.pad(x, (0, 1, 0, 1)) -> conv3x3 stride 2 padding 0), the mid block (resnet, single-head
   attention over the pixels, resnet), conv_norm_out -> SiLU -> conv_out (8 channels), quant_conv 1x1.  It runs in fp32 or fp64 on
   the fp16-rounded weights; ``round16=True`` rounds the activations to fp16 wherever the HIP kernels store fp16.

2. float64 references of the three new launches computed from their own operands, with bounds DERIVED from the operation from
   tests/launch_audit.py's constants (U fp32 / H fp16 unit roundoff, SUB half the fp16 subnormal step, acc_err(K, S) for an
   fp32 accumulation of K terms bounded by S):

   conv_in   x = 2 u8 / 255 - 1 in fp32: one rounded division (U |2 u8 / 255|), one rounded subtraction (U |x|); carried as
             fp16 hi + lo: the lo part is rounded to fp16 (2^-11 of |x - hi| <= 2^-11 |x|, i.e. 2^-22 |x|) and, below 2^-14,
             to the subnormal grid (SUB).  K = 54 non-zero slots (27 hi + 27 lo), then bias, one fp16 store.
   down      fp16 operands (exact), K = 9 Cin slots, the split-K parts added in fp32 (covered by acc_err's constant, as for
             every contraction of the audit), bias, one fp16 store.
   posterior quant_conv: a chain of 8 fused multiply-adds and one add, each rounded once at a partial sum bounded by
             S = sum |w||x| + |b|: 9 U S.  clamp is 1-Lipschitz.  exp(0.5 lv): the argument's error d gives the factor
             expm1(d); expf itself is accurate to 2 ulp (4 U) at the magnitude it produces.  Then one fma (U |t|), the product
             with scaling_factor (U |z|), and the two roundings of the re-noise (launch_audit.renoise_reference's 4 U form).
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

import launch_audit as la

CONV_IN_K = 54          # non-zero K slots of vae_enc_conv_in_u8: 27 hi + 27 lo
EXP_ULPS = 4 * la.U     # expf: 2 ulp


# ---- 1. the encoder, restated ----------------------------------------------------------------------------------------------
class EncoderReference:
    def __init__(self, sd, cfg=None, dtype=torch.float32):
        from sdlcm_amd.config import vae_config
        self.cfg = vae_config(cfg)
        self.dtype = dtype
        self.w = {k: v.to(torch.float16).to(dtype) for k, v in sd.items() if k.startswith("encoder.") or k.startswith("quant_conv.")}

    def _r(self, t, round16):
        return t.to(torch.float16).to(self.dtype) if round16 else t

    def _gn(self, x, p, silu, round16):
        y = F.group_norm(x, self.cfg.get("norm_num_groups", 32), self.w[p + ".weight"], self.w[p + ".bias"], eps=1e-6)
        return self._r(F.silu(y) if silu else y, round16)

    def _resnet(self, x, p, round16):
        w = self.w
        h = self._gn(x, p + ".norm1", True, round16)
        h = self._r(F.conv2d(h, w[p + ".conv1.weight"], w[p + ".conv1.bias"], padding=1), round16)
        h = self._gn(h, p + ".norm2", True, round16)
        sc = x
        if p + ".conv_shortcut.weight" in w:
            sc = self._r(F.conv2d(x, w[p + ".conv_shortcut.weight"], w[p + ".conv_shortcut.bias"]), round16)
        return self._r(F.conv2d(h, w[p + ".conv2.weight"], w[p + ".conv2.bias"], padding=1) + sc, round16)

    def downsample(self, x, p, round16=False):
        return self._r(F.conv2d(F.pad(x, (0, 1, 0, 1)), self.w[p + ".weight"], self.w[p + ".bias"], stride=2), round16)

    def conv_in(self, img_u8, round16=False):
        x = 2.0 * img_u8.permute(0, 3, 1, 2).to(self.dtype) / 255.0 - 1.0
        return self._r(F.conv2d(x, self.w["encoder.conv_in.weight"], self.w["encoder.conv_in.bias"], padding=1), round16)

    def mid_attention(self, x, round16=False):
        w, a = self.w, "encoder.mid_block.attentions.0"
        B, C, H, W = x.shape
        hn = self._gn(x, a + ".group_norm", False, round16).reshape(B, C, H * W).transpose(1, 2)
        q, k, v = (self._r(hn @ w[f"{a}.{n}.weight"].reshape(C, C).T + w[f"{a}.{n}.bias"], round16) for n in ("to_q", "to_k", "to_v"))
        p = torch.softmax(q @ k.transpose(1, 2) * C ** -0.5, dim=-1)
        o = self._r(p @ v, round16)
        o = o @ w[a + ".to_out.0.weight"].reshape(C, C).T + w[a + ".to_out.0.bias"]
        return self._r(o.transpose(1, 2).reshape(B, C, H, W) + x, round16)

    def mid_block(self, x, round16=False):
        x = self._resnet(x, "encoder.mid_block.resnets.0", round16)
        x = self.mid_attention(x, round16)
        return self._resnet(x, "encoder.mid_block.resnets.1", round16)

    @torch.inference_mode()
    def moments(self, img_u8, round16=False):
        """uint8 [B,H,W,3] -> posterior moments [B,8,h,w] (mean | logvar), in self.dtype."""
        cfg, w = self.cfg, self.w
        x = self.conv_in(img_u8, round16)
        nb = len(cfg["block_out_channels"])
        for i in range(nb):
            for j in range(cfg["layers_per_block"]):
                x = self._resnet(x, f"encoder.down_blocks.{i}.resnets.{j}", round16)
            if i < nb - 1:
                x = self.downsample(x, f"encoder.down_blocks.{i}.downsamplers.0.conv", round16)
        x = self.mid_block(x, round16)
        x = self._gn(x, "encoder.conv_norm_out", True, round16)
        x = F.conv2d(x, w["encoder.conv_out.weight"], w["encoder.conv_out.bias"], padding=1)
        return F.conv2d(x, w["quant_conv.weight"], w["quant_conv.bias"])


def sample(moments, e0, scaling_factor):
    """DiagonalGaussianDistribution(moments).sample() with the draw e0, times scaling_factor."""
    mean, logvar = moments.chunk(2, dim=1)
    return (mean + torch.exp(0.5 * logvar.clamp(-30.0, 20.0)) * e0) * scaling_factor


def add_noise(z, e1, abar):
    """LCMScheduler.add_noise at a timestep whose alphas_cumprod is abar."""
    return abar ** 0.5 * z + (1.0 - abar) ** 0.5 * e1


# ---- 2. the launches against float64 -------------------------------------------------------------------------------------
def conv_in_operand(img_u8, dev=None, lo=True):
    """vae_enc_conv_in_u8's operand -> (x [B,H,W,3] fp64, its error).  lo=False: the error a single fp16 would have (what the
    bound must NOT be: the CPU self-test)."""
    u = img_u8.to(dev if dev is not None else img_u8.device, torch.float64)
    x = 2.0 * u / 255.0 - 1.0
    carry = (2.0 ** -22) * x.abs() + la.SUB if lo else la.H * x.abs()
    return x, carry + la.U * ((2.0 * u / 255.0).abs() + x.abs())


def conv_in_check(got, img_u8, w, bias, B, H, W, images=None):
    """Worst |got - ref| / bound of lcm_vae_enc_conv_in_u8: got fp16 [B*H*W, Cout], w fp16 [Cout][27].  conv_bands pads the
    NORMALISED operand (and its error) with zeros: a border pixel's neighbours are 0."""
    x, e = conv_in_operand(img_u8[:B], got.device)
    return la.hint_layer_check(got, x, e, w, bias, B, H, W, 1, False, CONV_IN_K, images=images)


def down_size(n):
    return (n + 1 - 3) // 2 + 1


def down_reference(x, w, bias, B, H, W):
    """lcm_conv3x3_down_f16 from its stored operands: x fp16 [B*H*W, Cin], w fp16 [Cout][9*Cin] (tap major) -> (ref, bound)
    fp64 [B*Ho*Wo, Cout]."""
    Cin = x.shape[1]
    Ho, Wo = down_size(H), down_size(W)
    x64 = x[:B * H * W].to(torch.float64).reshape(B, H, W, Cin)
    xp = F.pad(x64, (0, 0, 0, 1, 0, 1))                                   # one zero column right, one zero row below
    cols = torch.stack([xp[:, ky:ky + 2 * (Ho - 1) + 1:2, kx:kx + 2 * (Wo - 1) + 1:2] for ky in range(3) for kx in range(3)], 3)
    A = cols.reshape(B * Ho * Wo, 9 * Cin)
    W64 = w.to(x.device, torch.float64)
    Y, S = la._mm(A, W64)
    E = la.acc_err(9 * Cin, S)
    if bias is not None:
        b64 = bias.to(x.device, torch.float64)
        Y = Y + b64
        E = E + la.U * (Y.abs() + b64.abs())
    return Y, la.store_bound(Y, E)


def posterior_reference(pre_m, pre_l, qw, qb, e0, e1, sf, sa, sb):
    """lcm_vae_posterior_renoise from its fp32 operands: pre_m / pre_l [B,h,w,4], qw [8,8], qb [8], e0 / e1 [B,4,h,w]
    -> dict(moments, z, lat: (ref, bound) pairs, NCHW fp64)."""
    f64 = torch.float64
    sf, sa, sb = float(np.float32(sf)), float(np.float32(sa)), float(np.float32(sb))
    pre = torch.cat([pre_m, pre_l], -1).to(f64)                            # [B,h,w,8]
    Wq, bq = qw.to(f64).reshape(8, 8), qb.to(f64)
    mom = pre @ Wq.T + bq
    E_mom = 9 * la.U * (pre.abs() @ Wq.abs().T + bq.abs())
    mom, E_mom = mom.permute(0, 3, 1, 2), E_mom.permute(0, 3, 1, 2)
    mean, E_mean = mom[:, :4], E_mom[:, :4]
    lv, E_lv = mom[:, 4:].clamp(-30.0, 20.0), E_mom[:, 4:]
    sd = torch.exp(0.5 * lv)
    E_sd = sd * (torch.expm1(0.5 * E_lv) + EXP_ULPS)
    E0, E1 = e0.to(f64), e1.to(f64)
    t = mean + sd * E0
    E_t = E_sd * E0.abs() + E_mean + la.U * (t.abs() + (sd * E0).abs())
    z = t * sf
    E_z = abs(sf) * E_t + la.U * z.abs()
    lat, b_lat = la.renoise_reference(z, E1, sa, sb)
    return dict(moments=(mom, E_mom + la.U * mom.abs() + 1e-38), z=(z, E_z + la.U * z.abs() + 1e-38),
                lat=(lat, b_lat + abs(sa) * E_z))


def posterior_check(got_z, got_lat, ref, B, dup, got_moments=None):
    """Worst ratio over z, the state (dup: the second half must equal the first bit for bit) and optionally the moments."""
    dev = got_z.device
    z, bz = ref["z"]
    lat, bl = ref["lat"]
    r = max(la.worst_ratio(got_z[:B], z.to(dev), bz.to(dev)), la._halves_ratio(got_lat, B, lat.to(dev), bl.to(dev), dup))
    if got_moments is not None:
        m, bm = ref["moments"]
        r = max(r, la.worst_ratio(got_moments[:B], m.to(dev), bm.to(dev)))
    return r


# ---- kernel-like CPU emulations (the CPU self-test of the bounds) ------------------------------------------------------------
def conv_in_kernel_like(img_u8, w16, bias16, drop=None, single_fp16=False, pad_minus_one=False):
    """conv_in the way the kernel computes it: x in fp32, hi + lo fp16 parts, fp32 accumulation, fp16 store.  drop = (tap,
    channel): that K term left out; single_fp16: no lo part; pad_minus_one: the border padded BEFORE the normalisation."""
    B, H, W, _ = img_u8.shape
    x = (2.0 * img_u8.to(torch.float32)) / 255.0 - 1.0
    pad_v = -1.0 if pad_minus_one else 0.0
    xp = F.pad(x, (0, 0, 1, 1, 1, 1), value=pad_v)
    cols = torch.stack([xp[:, ky:ky + H, kx:kx + W] for ky in range(3) for kx in range(3)], 3).reshape(B * H * W, 27)
    if drop is not None:
        cols[:, drop[0] * 3 + drop[1]] = 0
    hi = cols.half()
    lo = (cols - hi.float()).half()
    wf = w16.float()
    acc = hi.float() @ wf.T
    if not single_fp16:
        acc = acc + lo.float() @ wf.T
    return (acc + bias16.float()).half()


def posterior_kernel_like(pre_m, pre_l, qw, qb, e0, e1, sf, sa, sb, drop=None, no_clamp=False):
    """The posterior launch in fp32 (torch): drop = (o, k): one term of quant_conv left out."""
    f32 = torch.float32
    Wq = qw.to(f32).reshape(8, 8).clone()
    if drop is not None:
        Wq[drop[0], drop[1]] = 0
    mom = (torch.cat([pre_m, pre_l], -1).to(f32) @ Wq.T + qb.to(f32)).permute(0, 3, 1, 2)
    lv = mom[:, 4:] if no_clamp else mom[:, 4:].clamp(-30.0, 20.0)
    z = (mom[:, :4] + torch.exp(0.5 * lv) * e0) * np.float32(sf)
    return z, np.float32(sa) * z + np.float32(sb) * e1


def pack3x3(w):
    """[Cout, Cin, 3, 3] -> fp16 [Cout, 9 * Cin], tap major / channel minor (packing.pack_conv3x3's layout)."""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).contiguous().to(torch.float16)
