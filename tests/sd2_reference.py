"""References of the SD 2.x tests (a plain module, like tests/sr_reference.py): the LCM step of every prediction type in
float64 with its fp32 error bound, an SD 2.x original-layout (LDM / OpenCLIP) single file written from diffusers-named
tensors, and the OpenCLIP text tower restated on its raw tensors."""
from __future__ import annotations

import numpy as np
import torch

PREDS = ("epsilon", "v_prediction", "sample")
U32 = 2.0 ** -24            # fp32 unit roundoff


# ---------------------------------------------------------------------------------------------------------------------------
# LCMScheduler.step
# ---------------------------------------------------------------------------------------------------------------------------
def lcm_step_diffusers_fp64(m, x, noise, alphas_cumprod, t, t_prev, pred, last, m_u=None, g=1.0, final_alpha=1.0,
                            sigma_data=0.5, timestep_scaling=10.0):
    """diffusers' LCMScheduler.step restated in float64 from the cumulative alphas (not from the host's coefficients):
    CFG on the model output, then x0 by prediction type, the consistency boundary scalings, and the next sample."""
    m, x = np.asarray(m, np.float64), np.asarray(x, np.float64)
    if m_u is not None:
        m_u = np.asarray(m_u, np.float64)
        m = m_u + g * (m - m_u)
    a_t = float(alphas_cumprod[t])
    a_p = float(alphas_cumprod[t_prev]) if t_prev >= 0 else float(final_alpha)
    b_t, b_p = 1.0 - a_t, 1.0 - a_p
    if pred == "epsilon":
        x0 = (x - np.sqrt(b_t) * m) / np.sqrt(a_t)
    elif pred == "v_prediction":
        x0 = np.sqrt(a_t) * x - np.sqrt(b_t) * m
    elif pred == "sample":
        x0 = m
    else:
        raise ValueError(pred)
    s = t * timestep_scaling
    c_skip = sigma_data ** 2 / (s ** 2 + sigma_data ** 2)
    c_out = s / np.sqrt(s ** 2 + sigma_data ** 2)
    den = c_out * x0 + c_skip * x
    if last:
        return den
    return np.sqrt(a_p) * den + np.sqrt(b_p) * np.asarray(noise, np.float64)


def lcm_step_coef_fp64(coef6, last, m, x, noise, pred, m_u=None, g=1.0):
    """The step in the kernel's form, from the six host coefficients, in float64.  -> (value, bound of |fp32 - value|).

    The bound follows the kernel's expression operation by operation.  Inputs and coefficients are exact fp32 values; each fp32
    operation rounds once, to within U = 2^-24 of its result (a fused multiply-add rounds once for two operations, which is
    inside the same bound); the division is allowed 2U.  An operation z = a op b therefore carries the propagated errors of its
    operands (scaled by the factor they are multiplied with) plus U |z|.  Terms of order U^2 are dropped, so the bound is taken
    times 1.01."""
    sa, sb, c_skip, c_out, sap, sbp = (float(c) for c in coef6)
    m, x = np.asarray(m, np.float64), np.asarray(x, np.float64)
    U = U32
    if m_u is not None:
        m_u = np.asarray(m_u, np.float64)
        d = m - m_u
        e_d = U * np.abs(d)
        gd = g * d
        e_gd = abs(g) * e_d + U * np.abs(gd)
        ev = m_u + gd
        e_ev = e_gd + U * np.abs(ev)
    else:
        ev, e_ev = m, np.zeros_like(m)
    if pred == "epsilon":
        p = sb * ev
        e_p = abs(sb) * e_ev + U * np.abs(p)
        q = x - p
        e_q = e_p + U * np.abs(q)
        x0 = q / sa
        e_x0 = e_q / abs(sa) + 2 * U * np.abs(x0)
    elif pred == "v_prediction":
        a1 = sa * x
        p = sb * ev
        x0 = a1 - p
        e_x0 = U * np.abs(a1) + abs(sb) * e_ev + U * np.abs(p) + U * np.abs(x0)
    elif pred == "sample":
        x0, e_x0 = ev, e_ev
    else:
        raise ValueError(pred)
    t1, t2 = c_out * x0, c_skip * x
    den = t1 + t2
    e_den = abs(c_out) * e_x0 + U * np.abs(t1) + U * np.abs(t2) + U * np.abs(den)
    if last:
        return den, 1.01 * e_den
    n = np.asarray(noise, np.float64)
    s1, s2 = sap * den, sbp * n
    out = s1 + s2
    e = abs(sap) * e_den + U * np.abs(s1) + U * np.abs(s2) + U * np.abs(out)
    return out, 1.01 * e


# ---------------------------------------------------------------------------------------------------------------------------
# original-layout SD 2.x single file
# ---------------------------------------------------------------------------------------------------------------------------
_RES = {"norm1": "in_layers.0", "conv1": "in_layers.2", "time_emb_proj": "emb_layers.1", "norm2": "out_layers.0",
        "conv2": "out_layers.3", "conv_shortcut": "skip_connection"}


def _res(rest):
    head, tail = rest.split(".", 1)
    return _RES[head] + "." + tail


def ldm_unet_names(usd, up_attn=(False, True, True, True)):
    """diffusers UNet2DConditionModel names (4 levels, 2 resnets per level) -> 'model.diffusion_model.' names."""
    out = {}
    for k, v in usd.items():
        p = k.split(".")
        if p[0] == "conv_in":
            n = "input_blocks.0.0." + p[1]
        elif p[0] == "time_embedding":
            n = "time_embed.cond_proj.weight" if p[1] == "cond_proj" else f"time_embed.{0 if p[1] == 'linear_1' else 2}.{p[2]}"
        elif p[0] == "down_blocks":
            b = int(p[1])
            if p[2] == "downsamplers":
                n = f"input_blocks.{3 * b + 3}.0.op.{p[-1]}"
            else:
                i = 3 * b + 1 + int(p[3])
                n = f"input_blocks.{i}.0." + _res(".".join(p[4:])) if p[2] == "resnets" else f"input_blocks.{i}.1." + ".".join(p[4:])
        elif p[0] == "mid_block":
            n = f"middle_block.{2 * int(p[2])}." + _res(".".join(p[3:])) if p[1] == "resnets" else "middle_block.1." + ".".join(p[3:])
        elif p[0] == "up_blocks":
            b = int(p[1])
            if p[2] == "upsamplers":
                n = f"output_blocks.{3 * b + 2}.{2 if up_attn[b] else 1}.conv.{p[-1]}"
            else:
                i = 3 * b + int(p[3])
                n = f"output_blocks.{i}.0." + _res(".".join(p[4:])) if p[2] == "resnets" else f"output_blocks.{i}.1." + ".".join(p[4:])
        elif p[0] == "conv_norm_out":
            n = "out.0." + p[1]
        else:
            n = "out.2." + p[1]
        out["model.diffusion_model." + n] = v
    return out


def ldm_vae_names(vsd):
    """diffusers AutoencoderKL decoder names -> 'first_stage_model.' names (attention projections as 1x1 convs)."""
    out = {}
    for k, v in vsd.items():
        if k.startswith("post_quant_conv."):
            n = k
        else:
            p = k.split(".")[1:]
            if p[0] in ("conv_in", "conv_out"):
                n = "decoder." + ".".join(p)
            elif p[0] == "conv_norm_out":
                n = "decoder.norm_out." + p[1]
            elif p[0] == "mid_block" and p[1] == "resnets":
                n = f"decoder.mid.block_{int(p[2]) + 1}." + ".".join(p[3:]).replace("conv_shortcut", "nin_shortcut")
            elif p[0] == "mid_block":
                a = ".".join(p[3:-1])
                n = "decoder.mid.attn_1." + {"group_norm": "norm", "to_q": "q", "to_k": "k", "to_v": "v", "to_out.0": "proj_out"}[a] + "." + p[-1]
                if a != "group_norm" and p[-1] == "weight":
                    v = v.reshape(v.shape[0], v.shape[1], 1, 1)
            elif p[2] == "resnets":
                n = f"decoder.up.{3 - int(p[1])}.block.{p[3]}." + ".".join(p[4:]).replace("conv_shortcut", "nin_shortcut")
            else:
                n = f"decoder.up.{3 - int(p[1])}.upsample.conv.{p[-1]}"
        out["first_stage_model." + n] = v
    return out


def openclip_tower(width, layers, vocab, seed=4, mlp=4):
    """Raw OpenCLIP text-tower tensors (the names SD 2.x files carry under cond_stage_model.model.), fp16, seeded."""
    g = torch.Generator().manual_seed(seed)

    def rn(*shape, std=1.0):
        return (torch.randn(*shape, generator=g) * std).to(torch.float16)

    D, F = width, mlp * width
    t = {"token_embedding.weight": rn(vocab, D, std=0.5), "positional_embedding": rn(77, D, std=0.5),
         "ln_final.weight": 1 + rn(D, std=0.1), "ln_final.bias": rn(D, std=0.1),
         "text_projection": rn(D, D, std=D ** -0.5), "logit_scale": torch.tensor(4.6052)}
    for i in range(layers):
        b = f"transformer.resblocks.{i}."
        t[b + "attn.in_proj_weight"], t[b + "attn.in_proj_bias"] = rn(3 * D, D, std=D ** -0.5), rn(3 * D, std=0.02)
        t[b + "attn.out_proj.weight"], t[b + "attn.out_proj.bias"] = rn(D, D, std=0.25 * D ** -0.5), rn(D, std=0.02)
        for n in ("ln_1", "ln_2"):
            t[b + n + ".weight"], t[b + n + ".bias"] = 1 + rn(D, std=0.1), rn(D, std=0.1)
        t[b + "mlp.c_fc.weight"], t[b + "mlp.c_fc.bias"] = rn(F, D, std=D ** -0.5), rn(F, std=0.02)
        t[b + "mlp.c_proj.weight"], t[b + "mlp.c_proj.bias"] = rn(D, F, std=0.25 * F ** -0.5), rn(D, std=0.02)
    return t


def openclip_penultimate_ln_final(raw, ids, heads, eps=1e-5):
    """SD 2.x conditioning restated on the raw OpenCLIP tensors in fp32: token + position embedding, the pre-LN residual blocks
    up to and including the penultimate one (causal multi-head attention with the fused in_proj, exact-GELU MLP), ln_final."""
    import torch.nn.functional as F
    f = {k: v.float() for k, v in raw.items()}
    n = 1 + max(int(k.split(".")[2]) for k in f if k.startswith("transformer.resblocks."))
    ids = ids.long()
    B, S = ids.shape
    x = f["token_embedding.weight"][ids] + f["positional_embedding"][:S]
    D = x.shape[-1]
    d = D // heads
    mask = torch.full((S, S), float("-inf")).triu(1)
    for i in range(n - 1):
        b = f"transformer.resblocks.{i}."
        h = F.layer_norm(x, (D,), f[b + "ln_1.weight"], f[b + "ln_1.bias"], eps)
        q, k, v = (h @ f[b + "attn.in_proj_weight"].T + f[b + "attn.in_proj_bias"]).split(D, dim=-1)
        q, k, v = (t.reshape(B, S, heads, d).transpose(1, 2) for t in (q, k, v))
        a = torch.softmax(q @ k.transpose(-1, -2) / d ** 0.5 + mask, dim=-1) @ v
        x = x + a.transpose(1, 2).reshape(B, S, D) @ f[b + "attn.out_proj.weight"].T + f[b + "attn.out_proj.bias"]
        h = F.layer_norm(x, (D,), f[b + "ln_2.weight"], f[b + "ln_2.bias"], eps)
        h = F.gelu(h @ f[b + "mlp.c_fc.weight"].T + f[b + "mlp.c_fc.bias"])
        x = x + h @ f[b + "mlp.c_proj.weight"].T + f[b + "mlp.c_proj.bias"]
    return F.layer_norm(x, (D,), f["ln_final.weight"], f["ln_final.bias"], eps)


def write_sd2_single_file(path, usd, vsd, tower):
    """An SD 2.x original-layout .safetensors: UNet + VAE + OpenCLIP tower (cond_stage_model.model.*)."""
    from safetensors.torch import save_file
    raw = ldm_unet_names(usd)
    raw.update(ldm_vae_names(vsd))
    raw.update({"cond_stage_model.model." + k: v for k, v in tower.items()})
    raw["first_stage_model.encoder.conv_in.weight"] = torch.zeros(4, 3, 3, 3, dtype=torch.float16)    # must be ignored
    save_file({k: v.contiguous() for k, v in raw.items()}, path)
