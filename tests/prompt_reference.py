"""CPU restatements for the prompt tests, written in the test tree: the emphasis arithmetic in float64 with the error bound of the
kernel's fixed reduction order, and a torch-CPU CLIP text encoder with a stop layer (``clip_skip``)."""
from __future__ import annotations

import math

import numpy as np
import torch

S = 77
U = 2.0 ** -24          # fp32 unit roundoff
H = 2.0 ** -11          # fp16 unit roundoff


def emphasis_fp64(z, w):
    """z [n, 77, D] (any float), w [n, 77] -> float64 [n, 77, D]: z w mean(z_c) / mean(z_c w) per chunk c."""
    z = np.asarray(z, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    zw = z * w[:, :, None]
    return zw * (z.mean(axis=(1, 2)) / zw.mean(axis=(1, 2)))[:, None, None]


def reduction_depth(D):
    """Additions on the longest path of the kernel's fixed order (include/lcm_hip.h): 8 ceil(77 D / 8 / 512) in a thread, 6
    butterfly steps in a wave, 8 wave sums."""
    return 8 * math.ceil(S * D / 8 / 512) + 6 + 8


def emphasis_bound(z, w):
    """Per-element bound |got - ref| for lcm_prompt_emphasis_f16, [n, 77, D] float64.

    A sum of fp32 additions along a path of depth k is off by at most k U sum|terms| (each term passes through at most k
    roundings, each <= U times a partial sum <= sum|terms|; the fma adds no rounding of the product).  So
        |dS0| <= k U A0,  A0 = sum|z|;   |dS1| <= k U A1,  A1 = sum|z w|
    and r = S0 / S1 (one more rounding) is off relatively by  e_r = k U (A0 / |S0| + A1 / |S1|) + U  to first order; the test's
    conditioning assertion (|mean| >= 0.1 mean|.|) makes A / |S| <= 10, so e_r <= (20 k + 1) U ~ 2.6e-4 at k = 214 and second-order
    terms are below 1e-8: covered by the factor 1.01.  The two fp32 products add 2 U.  The fp16 store of the result is allowed
    2^-10 |ref|, and where the result is an fp16 subnormal one rounding is half the subnormal step, 2^-25, instead."""
    z = np.asarray(z, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    zw = z * w[:, :, None]
    k = reduction_depth(z.shape[2])
    e_r = k * U * (np.abs(z).sum(axis=(1, 2)) / np.abs(z.sum(axis=(1, 2))) + np.abs(zw).sum(axis=(1, 2)) / np.abs(zw.sum(axis=(1, 2)))) + U
    ref = emphasis_fp64(z, w)
    rel = 1.01 * (e_r[:, None, None] + 2 * U)
    return np.abs(ref) * (rel + 2 * H * (1 + rel)) + 2.0 ** -25


def conditioning(z, w):
    """min over chunks of |mean| / mean|.| before and after weighting (float64)."""
    z = np.asarray(z, dtype=np.float64)
    zw = z * np.asarray(w, dtype=np.float64)[:, :, None]
    a = np.abs(z.mean(axis=(1, 2))) / np.abs(z).mean(axis=(1, 2))
    b = np.abs(zw.mean(axis=(1, 2))) / np.abs(zw).mean(axis=(1, 2))
    return float(min(a.min(), b.min()))


def clip_text_cpu(sd, cfg, ids, stop=None):
    """CLIPTextModel's text tower in fp32 on the CPU, from the state dict the HIP path loads: token + position embeddings, ``stop``
    pre-LN layers (None: all) with the causal mask, final_layer_norm.  -> float32 [B, S, D].  clip_skip = k is
    stop = num_hidden_layers - (k - 1)."""
    f = lambda k: sd[k].float()
    D, heads, L = cfg["hidden_size"], cfg["num_attention_heads"], cfg["num_hidden_layers"]
    eps, act = cfg.get("layer_norm_eps", 1e-5), cfg.get("hidden_act", "quick_gelu")
    stop = L if stop is None else stop
    ids = torch.as_tensor(ids).long()
    B, T = ids.shape
    x = f("embeddings.token_embedding.weight")[ids] + f("embeddings.position_embedding.weight")[:T][None]
    mask = torch.full((T, T), float("-inf")).triu(1)
    d = D // heads
    ln = torch.nn.functional.layer_norm
    for i in range(stop):
        p = f"encoder.layers.{i}."
        h = ln(x, (D,), f(p + "layer_norm1.weight"), f(p + "layer_norm1.bias"), eps)
        q, k, v = (torch.nn.functional.linear(h, f(p + f"self_attn.{n}_proj.weight"), f(p + f"self_attn.{n}_proj.bias"))
                   .reshape(B, T, heads, d).transpose(1, 2) for n in "qkv")
        a = torch.softmax(q @ k.transpose(-1, -2) * d ** -0.5 + mask, -1) @ v
        a = a.transpose(1, 2).reshape(B, T, D)
        x = x + torch.nn.functional.linear(a, f(p + "self_attn.out_proj.weight"), f(p + "self_attn.out_proj.bias"))
        h = ln(x, (D,), f(p + "layer_norm2.weight"), f(p + "layer_norm2.bias"), eps)
        h = torch.nn.functional.linear(h, f(p + "mlp.fc1.weight"), f(p + "mlp.fc1.bias"))
        h = h * torch.sigmoid(1.702 * h) if act == "quick_gelu" else torch.nn.functional.gelu(h)
        x = x + torch.nn.functional.linear(h, f(p + "mlp.fc2.weight"), f(p + "mlp.fc2.bias"))
    return ln(x, (D,), f("final_layer_norm.weight"), f("final_layer_norm.bias"), eps)


def embed_prompt_cpu(sd, cfg, chunked, clip=None, stop=None):
    """A ``prompt_syntax.Chunked`` -> float64 [1, 77 n, D]: CLIP per chunk (clip(ids) -> [1, 77, D]; default clip_text_cpu), the
    fp64 emphasis per chunk, the chunks concatenated."""
    clip = clip or (lambda ids: clip_text_cpu(sd, cfg, ids, stop))
    z = np.concatenate([clip(torch.tensor([ids])).double().numpy() for ids in chunked.ids])          # [n, 77, D]
    return emphasis_fp64(z, np.asarray(chunked.weights)).reshape(1, -1, z.shape[2])
