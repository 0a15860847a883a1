"""Per-weight reference of the style-LoRA merge (a plain module, like tests/chain_reference.py): tests/test_lora_cpu.py and
tests/test_lora_gpu.py share it.

The reference of ``LoraStyle.apply(wt)`` / ``ClipLora.apply(wt)`` is the model's own packer run on the merged checkpoint:
``make_lora`` draws a LoRA and states every module's delta (B A) alpha / r in fp64 in the checkpoint's own layout,
``merged_checkpoint`` adds wt times it to the base tensors in fp64 and keeps the sum as fp32 (not rounded to fp16: the packer
rounds once, as it does for the base), and a second network of the same class is built from that.  ``measure`` then takes the
live network's tensors after ``apply(wt)``, the second network's and the live ones from before, and looks at every tensor:

1. a tensor the style does not touch is bit-identical to what it was (weights, biases, norms, ``.lnw`` / ``.lnb``, the ``.g`` /
   ``.c`` of untouched folds) -- and the reference network holds the same bits there;
2. the set of tensors that changed is exactly ``expected_touched``;
3. a touched ``.w`` (``.w3``) obeys, per element,

       |live - ref| <= H (|ref| + s) + 8 U s + 3 SUB          s = |base| + |wt delta16|

   with H, U, SUB those of tests/launch_audit.py.  The two sides differ in the fp16 rounding of the packed base, of the packed
   delta and of the stored result (the reference rounds the packed sum once), each at most H times what it rounds, and in the
   fp32 operations of packer and merge (a few roundings of U each, at the magnitude s).  ``delta16`` is the style's packed fp16
   delta, the operand of the merge kernel; tests/test_lora_cpu.py shows that a delta packed wrongly breaks the comparison
   whatever it does to s;
4. a touched ``.c`` = W' beta + b lies within 4 U (sum_k |W'_k beta_k| + |b|) of its fp64 value (``fold_constants64``, from
   the merged checkpoint in fp64 and this module's own statement of the to_q factor and of the GEGLU row order).

``g_ratio`` checks every live ``.g`` against the fp64 row sums of the live fp16 weight: |g - sum| <= acc_err(K, sum |w|) + U |g|.

LoRA values are dyadic with few bits (``_dyadic``), so that B A and alpha / r are the same numbers in fp32 and in fp64 and the
comparison speaks of the packing alone."""
from __future__ import annotations

import math
import re

import numpy as np
import torch

import launch_audit as la

LOG2E = 1.4426950408889634


# ---- drawing a LoRA ---------------------------------------------------------------------------------------------------------------
def _dyadic(shape, g, scale):
    """N(0, 1) rounded to eighths, times the power of two next to ``scale``: a handful of mantissa bits."""
    p = 2.0 ** round(math.log2(scale))
    return torch.round(torch.randn(shape, generator=g) * 8.0) / 8.0 * p


def make_lora(cfg, sd, modules, r=4, alpha=2.0, seed=0, key_style="mixed", gain=1.0):
    """A LoRA on ``modules`` (paths below the UNet, as lora._target_modules names them) of the checkpoint ``sd``.

    key_style "kohya": ``lora_unet_<path with _>.lora_down.weight`` / ``.lora_up.weight`` and, when alpha is not None, ``.alpha``;
    "peft": ``unet.<path>.lora_A.weight`` / ``.lora_B.weight`` without alpha (scale 1); "mixed": kohya with ``.alpha``, peft, kohya
    without ``.alpha`` in turn, so one file holds both key styles and entries with and without ``.alpha``.  A 3x3 target gets the LoCon pair down [r,Cin,3,3] x up [Cout,r,1,1]; conv_shortcut,
    proj_in and proj_out get their pair in turn as 4-D 1x1 tensors and as plain matrices, whatever the checkpoint's own form.
    -> (raw, {module: fp64 delta in the shape of sd[module + ".weight"]})."""
    g = torch.Generator().manual_seed(seed)
    raw, deltas, n_1x1 = {}, {}, 0
    for i, m in enumerate(modules):
        W = sd[m + ".weight"]
        cout, cin = W.shape[0], W.shape[1]
        three = W.dim() == 4 and W.shape[-1] == 3
        fan_in = cin * (9 if three else 1)
        down = _dyadic((r, cin, 3, 3) if three else (r, cin), g, fan_in ** -0.5)
        up = _dyadic((cout, r), g, 0.5 * gain)
        kohya = key_style == "kohya" or (key_style == "mixed" and i % 3 != 1)
        with_alpha = kohya and alpha is not None and not (key_style == "mixed" and i % 3 == 2)
        scale = (alpha / r) if with_alpha else 1.0
        d = torch.einsum("or,r...->o...", up.double(), down.double()) * scale
        deltas[m] = d.reshape(W.shape)
        if three:
            up = up.reshape(cout, r, 1, 1)
        elif m.endswith((".conv_shortcut", ".proj_in", ".proj_out")):
            if n_1x1 % 2 == 0:
                down, up = down.reshape(r, cin, 1, 1), up.reshape(cout, r, 1, 1)
            n_1x1 += 1
        if kohya:
            k = "lora_unet_" + m.replace(".", "_")
            raw[k + ".lora_down.weight"], raw[k + ".lora_up.weight"] = down, up
            if with_alpha:
                raw[k + ".alpha"] = torch.tensor(float(alpha))
        else:
            raw["unet." + m + ".lora_A.weight"], raw["unet." + m + ".lora_B.weight"] = down, up
    return raw, deltas


def raw_of(raw, modules):
    """The entries of ``raw`` (make_lora's) that belong to ``modules``."""
    stems = {s for m in modules for s in ("lora_unet_" + m.replace(".", "_"), "unet." + m)}
    return {k: v for k, v in raw.items() if (k[:-6] if k.endswith(".alpha") else k.split(".lora_")[0]) in stems}


TE_SUBS = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.out_proj", "mlp.fc1", "mlp.fc2")
_TE_NAME = {"self_attn.q_proj": ("qkv", 0), "self_attn.k_proj": ("qkv", 1), "self_attn.v_proj": ("qkv", 2),
            "self_attn.out_proj": ("o", None), "mlp.fc1": ("fc1", None), "mlp.fc2": ("fc2", None)}


def make_te_lora(sd, targets, index=0, r=4, alpha=2.0, seed=0, gain=1.0):
    """A text-encoder LoRA on ``targets`` = [(layer, sub-module)] of the CLIP checkpoint ``sd`` (names without ``text_model.``),
    for encoder ``index``: kohya ``lora_te_`` / ``lora_te1_`` (in turn) or ``lora_te2_`` keys with alpha, and peft
    ``text_encoder.`` / ``text_encoder_2.`` keys without.  -> (raw, {"encoder.layers.<i>.<sub>": fp64 delta})."""
    g = torch.Generator().manual_seed(seed)
    raw, deltas = {}, {}
    for i, (layer, sub) in enumerate(targets):
        name = f"encoder.layers.{layer}.{sub}"
        W = sd[name + ".weight"]
        down = _dyadic((r, W.shape[1]), g, W.shape[1] ** -0.5)
        up = _dyadic((W.shape[0], r), g, 0.25 * gain)
        path = "text_model." + name
        if i % 2 == 0:
            pre = "lora_te2_" if index else ("lora_te_", "lora_te1_")[(i // 2) % 2]
            k = pre + path.replace(".", "_")
            raw[k + ".lora_down.weight"], raw[k + ".lora_up.weight"], raw[k + ".alpha"] = down, up, torch.tensor(float(alpha))
            scale = alpha / r
        else:
            k = ("text_encoder_2." if index else "text_encoder.") + path
            raw[k + ".lora_A.weight"], raw[k + ".lora_B.weight"] = down, up
            scale = 1.0
        deltas[name] = up.double() @ down.double() * scale
    return raw, deltas


def merged_checkpoint(sd, deltas, wt):
    """W + wt delta in fp64, kept as fp32; every other tensor as it is."""
    out = dict(sd)
    for m, d in deltas.items():
        out[m + ".weight"] = (sd[m + ".weight"].double() + float(wt) * d).float()
    return out


# ---- which packed tensors a module's entry reaches --------------------------------------------------------------------------------
def expected_touched(modules):
    """Names in UNetHip.w that a LoRA on ``modules`` changes."""
    out = set()
    for m in modules:
        a = re.match(r"^(.*\.attentions\.\d+)\.(.*)$", m)
        if a:
            p, rest = a.groups()
            if rest in ("proj_in", "proj_out"):
                out.add(f"{p}.{rest}.w")
                continue
            k, sub = re.match(r"^transformer_blocks\.(\d+)\.(.*)$", rest).groups()
            q = f"{p}.{k}"
            fold = {"attn1.to_q": "qkv", "attn1.to_k": "qkv", "attn1.to_v": "qkv", "attn2.to_q": "q2", "ff.net.0.proj": "ff1"}.get(sub)
            if fold:
                out.update(f"{q}.{fold}.{s}" for s in ("w", "g", "c"))
            elif sub in ("attn2.to_k", "attn2.to_v"):
                out.add("kv_all.w")
            else:
                out.add(q + {"attn1.to_out.0": ".o1.w", "attn2.to_out.0": ".o2.w", "ff.net.2": ".ff2.w"}[sub])
        elif m.endswith(".time_emb_proj"):
            out.add("temb_all.w")
        elif m.endswith(".conv_shortcut"):
            out.add(m[:-len(".conv_shortcut")] + ".sc.w")
        else:
            out.add(m + ".w")
            if ".upsamplers." in m:
                out.add(m + ".w3")
    return out


def expected_touched_te(targets):
    return {f"{layer}.{_TE_NAME[sub][0]}.w" for layer, sub in targets}


# ---- the folded constants in fp64 -------------------------------------------------------------------------------------------------
def _level(p, nb):
    if p.startswith("mid_block"):
        return nb - 1
    i = int(p.split(".")[1])
    return i if p.startswith("down_blocks") else nb - 1 - i


def _geglu_rows(F2):
    """Row of the checkpoint's [value | gate] matrix stored at each row of the packed one: blocks of 16 value rows and the 16
    gate rows of the same channels in turn."""
    Fh = F2 // 2
    o = np.arange(F2)
    blk, half, j = o // 32, (o // 16) % 2, o % 16
    return torch.from_numpy(half * Fh + blk * 16 + j)


def fold_constants64(sd, cfg, deltas, wt, folds):
    """{fold + ".c": (fp64 value of c = W' beta + b in the packed row order, sum_k |W'_k beta_k| + |b| alike)} for ``folds`` = names
    such as "mid_block.attentions.0.0.qkv", with W' = W + wt delta in fp64 and the to_q rows times (C / heads)^-1/2 log2(e)."""
    from sdlcm_amd.config import heads_at, unet_config
    cfg = unet_config(cfg)
    nb = len(cfg["block_out_channels"])

    def W(name):
        w = sd[name + ".weight"].double()
        w = w.reshape(w.shape[0], -1)
        return w + float(wt) * deltas[name].reshape(w.shape) if name in deltas else w

    out = {}
    for f in folds:
        p, k, kind = re.match(r"^(.*\.attentions\.\d+)\.(\d+)\.(qkv|q2|ff1)$", f).groups()
        t = f"{p}.transformer_blocks.{k}"
        b = None
        if kind == "qkv":
            w = [W(f"{t}.attn1.to_{n}") for n in "qkv"]
            qs = (w[0].shape[0] // heads_at(cfg, _level(p, nb))) ** -0.5 * LOG2E
            w, beta = torch.cat([w[0] * qs, w[1], w[2]], 0), sd[f"{t}.norm1.bias"].double()
        elif kind == "q2":
            w = W(f"{t}.attn2.to_q")
            w, beta = w * ((w.shape[0] // heads_at(cfg, _level(p, nb))) ** -0.5 * LOG2E), sd[f"{t}.norm2.bias"].double()
        else:
            w, beta, b = W(f"{t}.ff.net.0.proj"), sd[f"{t}.norm3.bias"].double(), sd[f"{t}.ff.net.0.proj.bias"].double()
        c, mag = w @ beta, w.abs() @ beta.abs()
        if b is not None:
            rows = _geglu_rows(w.shape[0])
            c, mag = (c + b)[rows], (mag + b.abs())[rows]
        out[f + ".c"] = (c, mag)
    return out


# ---- the comparison ---------------------------------------------------------------------------------------------------------------
def snapshot(w):
    return {n: t.clone() for n, t in w.items()}


def w_bound(ref, base, delta16, wt):
    s = base.double().abs()
    if delta16 is not None:
        s = s + (float(wt) * delta16.double()).abs()
    return la.H * (ref.double().abs() + s) + 8.0 * la.U * s + 3.0 * la.SUB


def measure(live, ref, before, expected, delta16, wt, c64=None, only=None):
    """live / ref / before: name -> tensor of the live network after apply(wt), of the network built from the merged checkpoint
    and of the live network before.  expected: the names the style must change.  delta16: name -> the style's packed fp16 delta.
    c64: fold_constants64's result for the touched folds.  only: name endings; the ratios of the other tensors are not computed.
    -> dict(touched: the names that changed, stray: untouched names that changed or that the reference packs differently,
            w: {name: worst |live - ref| / bound}, c: {name: worst ratio})."""
    touched = {n for n in live if not la.same_bits(live[n], before[n])}
    stray = sorted(n for n in live if n not in expected and not (la.same_bits(live[n], before[n]) and la.same_bits(ref[n], before[n])))
    rw, rc = {}, {}
    for n in sorted(expected):
        if only is not None and not n.endswith(only):
            continue
        if n.endswith((".w", ".w3")):
            bound = w_bound(ref[n], before[n], delta16.get(n), wt)
            rw[n] = la.worst_ratio(live[n], ref[n].double(), bound.to(ref[n].device))
        elif n.endswith(".c") and c64 is not None:
            c, mag = (t.to(live[n].device) for t in c64[n])
            rc[n] = la.worst_ratio(live[n], c, 4.0 * la.U * mag)
    return dict(touched=touched, stray=stray, w=rw, c=rc)


def worst(m):
    """The largest error / bound ratio of a measure() result and the tensor it belongs to."""
    items = list(m["w"].items()) + list(m["c"].items())
    return max(items, key=lambda kv: kv[1]) if items else ("", 0.0)


def check(m, expected, tag):
    """Assert the four statements of the comparison on a measure() result; -> (worst .w ratio, worst .c ratio)."""
    assert not m["stray"], f"{tag}: tensors outside the style changed, or the reference packs them differently: {m['stray'][:6]}"
    assert m["touched"] == set(expected), (f"{tag}: touched set differs: missing {sorted(set(expected) - m['touched'])[:6]}, "
                                            f"extra {sorted(m['touched'] - set(expected))[:6]}")
    ww, wc = max(m["w"].values(), default=0.0), max(m["c"].values(), default=0.0)
    print(f"[lora] {tag}: {len(m['w'])} weights worst error/bound {ww:.4g}, {len(m['c'])} fold constants worst error/bound {wc:.4g}")
    bad = [(n, r) for n, r in list(m["w"].items()) + list(m["c"].items()) if not r <= 1.0]
    assert not bad, f"{tag}: outside the bound: {sorted(bad, key=lambda x: -x[1])[:6]}"
    return ww, wc


def g_ratio(w):
    """Worst |g - fp64 row sum of the live fp16 weight| / (acc_err(K, sum |w|) + U |g|) over every fold of a network's tensors."""
    worst_r, n_folds = 0.0, 0
    for n, g in w.items():
        if not n.endswith(".g") or (n[:-2] + ".lnw") not in w:
            continue
        W = w[n[:-2] + ".w"].double()
        ref = W.sum(1)
        bound = la.acc_err(W.shape[1], W.abs().sum(1)) + la.U * ref.abs() + 1e-30
        worst_r = max(worst_r, la.worst_ratio(g, ref, bound))
        n_folds += 1
    return worst_r, n_folds
