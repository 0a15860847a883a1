"""The style-LoRA merge per weight, on the CPU: ``UNetHip(device="cpu")`` / ``ClipTextHip(device="cpu")`` with the two kernels of
the merge (``ops.axpy``, ``ops.ln_fold_refresh``) replaced by torch restatements, against the same class built from the merged
checkpoint (tests/lora_reference.py states the comparison and its bound).

Three reduced UNet configs, the smallest that show each layout, with a LoRA on EVERY module of ``lora._target_modules(cfg)`` at
once -- the comparison is per tensor, so no entry can hide behind another:

    sd15   SD1.5-shaped: block_out_channels (64, 128, 256, 256), cross_attention_dim 96; 1x1-conv proj_in / proj_out
    sd2    SD2_UNET-shaped, the same change: heads per level (5, 10, 20, 20), so the to_q factor is read per level; linear projections
    sdxl   SDXL_UNET-shaped: block_out_channels (64, 128, 256), cross_attention_dim 96, transformer_layers_per_block (1, 2, 3):
           transformer_blocks.k for k > 0, the added embedding beside the targets

Mutants of the code under test, each a monkeypatch on the ``lora`` module or on the stand-in network (never an edit of product
code), measured at weight 0.75.  Condition, not a fit: every mutant breaks the comparison by at least SEPARATION = 10 bounds on some
tensor of every config.  A mutant's style is built from the entries that reach the tensors it can move, and those tensors are
measured (MUTANTS); the true merge of the same entries is measured beside it.  Measured worst error / bound of a tensor (the true
merge of every target: 0.9989 - 0.9991 on the weights -- one fp16 ulp between the two sides at a power of two reaches the bound --,
at most 0.47 on the fold constants, at most 0.0027 on the row sums; weights that carry neither the to_q factor nor a LayerNorm
scale agree bit for bit, the LoRA values being dyadic):

    mutant                                      sd15       sd2        sdxl
    qs taken as 1                               1.2e3      8.4e2      8.4e2
    fold without lnw                            4.8e2      4.2e2      4.6e2
    cdelta dropped                              1.9e6      1.9e6      1.2e6
    pack_geglu as identity                      2.4e6      3.8e6      2.0e6
    pack_ff2_cols as identity                   2.0e3      2.0e3      2.0e3
    to_k and to_v offsets swapped               2.0e3      2.0e3      2.0e3
    temb_off shifted by one resnet              2.0e3      2.0e3      2.0e3
    pack_conv3x3_up2 as zero-padded plain rows  2.0e3      2.0e3      2.0e3
    the .w3 update skipped                      2.0e3      2.0e3      2.0e3
    alpha / r taken as 1                        6.8e2      6.8e2      6.8e2

Found by the restore check: fp16 checkpoints hold negative zeros, and base + 0 * delta turns them into positive ones (the kernel
and its restatement here alike), so weight 0 did not restore the bits; ``apply(0.0)`` now copies the saved base (lora._merge).
"""
import pytest
import torch

import launch_audit as la
import lora_reference as lr

SEPARATION = 10
WEIGHTS = (0.75, -0.5)
R, ALPHA = 4, 2.0          # alpha / r = 0.5: an entry without .alpha (scale 1) and one with it differ by a factor of two


def _unet_cfgs():
    from sdlcm_amd.config import SD2_UNET, SDXL_UNET
    small = dict(block_out_channels=(64, 128, 256, 256), cross_attention_dim=96)
    return {"sd15": dict(small), "sd2": dict(SD2_UNET, **small),
            "sdxl": dict(SDXL_UNET, block_out_channels=(64, 128, 256), cross_attention_dim=96, transformer_layers_per_block=(1, 2, 3))}


# ---- torch restatements of the two kernels (csrc/misc.hip: fp32 math, one fp16 rounding of the result) ------------------------------
def _axpy(base, delta, alpha, out):
    out.copy_((base.float() + torch.tensor(float(alpha), dtype=torch.float32) * delta.float()).to(torch.float16))
    return out


def _ln_fold_refresh(w, g_out, c_base=None, c_delta=None, alpha=0.0, c_out=None):
    g_out.copy_(w.float().sum(1))
    if c_out is not None:
        c_out.copy_(c_base if c_delta is None else c_base + torch.tensor(float(alpha), dtype=torch.float32) * c_delta)


@pytest.fixture(scope="module", autouse=True)
def cpu_kernels():
    from sdlcm_amd import ops
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(ops, "axpy", _axpy)
        mp.setattr(ops, "ln_fold_refresh", _ln_fold_refresh)
        yield


def _copy(sd):
    return {k: v.clone() for k, v in sd.items()}


# ---- one config: the live network, a LoRA on every target, the two reference networks ------------------------------------------------
class _Case:
    def __init__(self, tag, cfg):
        from sdlcm_amd import lora, weights
        from sdlcm_amd.model import UNetHip
        self.tag, self.cfg = tag, cfg
        self.sd = weights.synthetic_unet(cfg, seed=3)
        self.net = UNetHip(_copy(self.sd), cfg, device="cpu")      # on the CPU the packer keeps some of its inputs as they are
        self.before = lr.snapshot(self.net.w)
        self.modules = sorted(lora._target_modules(self.net.cfg))
        self.raw, self.deltas = lr.make_lora(cfg, self.sd, self.modules, r=R, alpha=ALPHA, seed=17, key_style="mixed")
        self.expected = lr.expected_touched(self.modules)
        self.folds = sorted(n[:-2] for n in self.expected if n.endswith(".c"))
        self._ref = {}

    def ref(self, wt):
        """(tensors of the network packed from the merged checkpoint, fp64 fold constants), built once per weight."""
        from sdlcm_amd.model import UNetHip
        if wt not in self._ref:
            net = UNetHip(lr.merged_checkpoint(self.sd, self.deltas, wt), self.cfg, device="cpu")
            self._ref[wt] = (net.w, lr.fold_constants64(self.sd, self.cfg, self.deltas, wt, self.folds))
        return self._ref[wt]

    def restore(self):
        for n, t in self.net.w.items():
            t.copy_(self.before[n])

    def measure(self, style, wt, only=None):
        ref, c64 = self.ref(wt)
        return lr.measure(self.net.w, ref, self.before, self.expected, style.delta, wt, c64, only=only)


@pytest.fixture(scope="module")
def cases():
    built = {}
    cfgs = _unet_cfgs()

    def get(tag):
        if tag not in built:
            built[tag] = _Case(tag, cfgs[tag])
        return built[tag]
    return get


CONFIGS = ("sd15", "sd2", "sdxl")


@pytest.mark.parametrize("tag", CONFIGS)
def test_every_target_merges_like_the_packed_merged_checkpoint(cases, tag):
    from sdlcm_amd.lora import LoraStyle
    c = cases(tag)
    style = LoraStyle(c.net, c.raw)
    assert style.modules == c.modules and not style.skipped
    print(f"[lora] {tag}: {len(c.modules)} target modules, {len(c.expected)} packed tensors")
    try:
        for wt in WEIGHTS:
            style.apply(wt)
            lr.check(c.measure(style, wt), c.expected, f"{tag} wt={wt:g}")
            r, n = lr.g_ratio(c.net.w)
            print(f"[lora] {tag} wt={wt:g}: {n} row-sum vectors worst error/bound {r:.4g}")
            assert n == len([k for k in c.net.w if k.endswith(".lnw")]) and r <= 1.0
        # 0.75 then 0.3 without going through 0 is the fresh 0.3 merge, bit for bit
        style.apply(0.75)
        style.apply(0.3)
        direct = lr.snapshot(c.net.w)
        style.apply(0.0)
        assert all(la.same_bits(c.net.w[n], c.before[n]) for n in c.net.w), "weight 0 does not restore every tensor"
        # not an empty statement: the touched weights do hold negative zeros, which base + 0 * delta does not keep
        assert any(((c.before[n] == 0) & torch.signbit(c.before[n])).any() for n in c.expected if n.endswith(".w"))
        style.apply(0.3)
        assert all(la.same_bits(c.net.w[n], direct[n]) for n in c.net.w), "0.75 -> 0.3 differs from a fresh 0.3 merge"
        assert any(not la.same_bits(direct[n], c.before[n]) for n in direct)
        style.apply(0.0)
        assert all(la.same_bits(c.net.w[n], c.before[n]) for n in c.net.w)
    finally:
        c.restore()


# ---- mutants ----------------------------------------------------------------------------------------------------------------------
class _Lnw1(dict):
    def __getitem__(self, k):
        t = dict.__getitem__(self, k)
        return torch.ones_like(t) if k.endswith(".lnw") else t


class _NoW3(dict):
    def __contains__(self, k):
        return not k.endswith(".w3") and dict.__contains__(self, k)


class _SwapOff(int):
    """The offset of a block's to_k | to_v rows, read as lora.py reads it (off + (Ck if to_v else 0)) with the two exchanged."""
    def __new__(cls, off, ck):
        o = int.__new__(cls, off)
        o.ck = ck
        return o

    def __add__(self, other):
        return int(self) + (self.ck - int(other))


def _zero_padded_plain(w):
    from sdlcm_amd.packing import pack_conv3x3
    plain = pack_conv3x3(w)
    out = torch.zeros(4 * w.shape[0] * 4 * w.shape[1], dtype=plain.dtype)
    out[:plain.numel()] = plain.reshape(-1)
    return out.reshape(4 * w.shape[0], 4 * w.shape[1])


def _shifted_temb(off):
    keys = list(off)
    return {p: (off[keys[(i + 1) % len(keys)]][0] if off[keys[(i + 1) % len(keys)]][0] + off[p][1] <= sum(n for _, n in off.values())
                else off[keys[i - 1]][0], off[p][1]) for i, p in enumerate(keys)}


def _alpha_is_rank(parse):
    def f(raw, cfg):
        out, skipped = parse(raw, cfg)
        return {m: (d, u, float(d.shape[0])) for m, (d, u, _) in out.items()}, skipped
    return f


def _mutate(name, mp, net):
    from sdlcm_amd import lora, ops
    if name == "qs taken as 1":
        mp.setattr(net, "qs", {k: 1.0 for k in net.qs})
    elif name == "fold without lnw":
        mp.setattr(net, "w", _Lnw1(net.w))
    elif name == "cdelta dropped":
        mp.setattr(ops, "ln_fold_refresh", lambda w, g, cb=None, cd=None, a=0.0, co=None: _ln_fold_refresh(w, g, cb, None, a, co))
    elif name == "pack_geglu as identity":
        mp.setattr(lora, "pack_geglu", lambda w, b: (w, b))
    elif name == "pack_ff2_cols as identity":
        mp.setattr(lora, "pack_ff2_cols", lambda w: w)
    elif name == "to_k and to_v offsets swapped":
        mp.setattr(net, "kv_off", {q: (_SwapOff(off, ck), ck) for q, (off, ck) in net.kv_off.items()})
    elif name == "temb_off shifted by one resnet":
        mp.setattr(net, "temb_off", _shifted_temb(net.temb_off))
    elif name == "pack_conv3x3_up2 as zero-padded plain rows":
        mp.setattr(lora, "pack_conv3x3_up2", _zero_padded_plain)
    elif name == "the .w3 update skipped":
        mp.setattr(net, "w", _NoW3(net.w))
    elif name == "alpha / r taken as 1":
        mp.setattr(lora, "parse_lora", _alpha_is_rank(lora.parse_lora))
    else:
        raise ValueError(name)


# mutant -> (endings of the modules whose entries reach the tensors it can move, endings of those tensors): the style of a mutant is
# built from these modules' entries alone and only these tensors are measured -- the other entries reach none of them
_FOLDED = ("attn1.to_q", "attn1.to_k", "attn1.to_v", "attn2.to_q", "ff.net.0.proj")
MUTANTS = {"qs taken as 1": (_FOLDED[:4], (".qkv.w", ".q2.w")),
           "fold without lnw": (_FOLDED, (".qkv.w", ".q2.w", ".ff1.w")),
           "cdelta dropped": (_FOLDED, (".c",)),
           "pack_geglu as identity": (("ff.net.0.proj",), (".ff1.w", ".ff1.c")),
           "pack_ff2_cols as identity": (("ff.net.2",), (".ff2.w",)),
           "to_k and to_v offsets swapped": (("attn2.to_k", "attn2.to_v"), ("kv_all.w",)),
           "temb_off shifted by one resnet": ((".time_emb_proj",), ("temb_all.w",)),
           "pack_conv3x3_up2 as zero-padded plain rows": ((".upsamplers.0.conv",), (".upsamplers.0.conv.w",)),
           "the .w3 update skipped": ((".upsamplers.0.conv",), (".w3",)),
           "alpha / r taken as 1": (("to_out.0", ".proj_in", ".conv_shortcut"), (".o1.w", ".o2.w", ".proj_in.w", ".sc.w"))}


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_mutant_breaks_the_comparison(cases, mutant):
    from sdlcm_amd.lora import LoraStyle
    wt = WEIGHTS[0]
    mods, only = MUTANTS[mutant]
    seps = []
    for tag in CONFIGS:
        c = cases(tag)
        raw = lr.raw_of(c.raw, [m for m in c.modules if m.endswith(mods)])
        try:
            true = LoraStyle(c.net, raw)
            true.apply(wt)
            ok = lr.worst(c.measure(true, wt, only))[1]
            c.restore()
            with pytest.MonkeyPatch.context() as mp:
                _mutate(mutant, mp, c.net)
                style = LoraStyle(c.net, raw)
                style.apply(wt)
            name, sep = lr.worst(c.measure(style, wt, only))
            seps.append(sep)
            print(f"[lora-mutant] {mutant:<44} {tag:<5} worst error/bound {sep:.3g} on {name} (the true merge of these entries: {ok:.3g})")
            assert ok <= 1.0
        finally:
            c.restore()
    assert all(s >= SEPARATION for s in seps), f"{mutant}: separations {seps}, the comparison needs {SEPARATION}"


# ---- text encoders ----------------------------------------------------------------------------------------------------------------
def _clip_cfgs():
    from sdlcm_amd.clip import CLIP_BIGG, CLIP_H, CLIP_L
    small = dict(vocab_size=512, hidden_size=128, intermediate_size=512, num_attention_heads=4)
    return {"clip-l": (dict(CLIP_L, num_hidden_layers=3, **small), 0),
            "clip-h": (dict(CLIP_H, num_hidden_layers=3, **small), 0),
            "projected": (dict(CLIP_BIGG, num_hidden_layers=2, projection_dim=64, **small), 1)}


@pytest.mark.parametrize("tag", ["clip-l", "clip-h", "projected"])
def test_text_encoder_merges_like_the_merged_checkpoint(tag):
    from sdlcm_amd.clip import ClipTextHip, synthetic_clip
    from sdlcm_amd.lora import ClipLora
    cfg, index = _clip_cfgs()[tag]
    sd = synthetic_clip(cfg, seed=5)
    enc = ClipTextHip(_copy(sd), cfg, device="cpu")
    assert enc.has_proj == (index == 1) and enc.act == (2 if tag == "clip-l" else 3)
    targets = [(i, sub) for i in range(cfg["num_hidden_layers"]) for sub in lr.TE_SUBS]
    mine, deltas = lr.make_te_lora(sd, targets, index=index, r=R, alpha=ALPHA, seed=41)
    other, _ = lr.make_te_lora(sd, targets, index=1 - index, r=R, alpha=ALPHA, seed=43)       # the other encoder's entries
    unet = {"lora_unet_mid_block_attentions_0_proj_in.lora_down.weight": torch.zeros(R, 8),
            "lora_unet_mid_block_attentions_0_proj_in.lora_up.weight": torch.zeros(8, R)}
    assert not set(mine) & set(other)
    pre = ("lora_te2_", "text_encoder_2.") if index else ("lora_te_", "lora_te1_", "text_encoder.")
    assert all(k.startswith(pre) for k in mine) and not any(k.startswith(pre) for k in other)
    if not index:
        assert {k[:9] for k in mine if k.startswith("lora_te")} == {"lora_te_t", "lora_te1_"}
    before = lr.snapshot(enc.w)
    style = ClipLora(enc, {**other, **mine, **unet}, index)
    assert sorted(style.used) == sorted(k for k in mine if not k.endswith(".alpha")) and len(style.modules) == len(targets)
    expected = lr.expected_touched_te(targets)
    for wt in WEIGHTS:
        ref = ClipTextHip(lr.merged_checkpoint(sd, deltas, wt), cfg, device="cpu").w
        style.apply(wt)
        lr.check(lr.measure(enc.w, ref, before, expected, style.delta, wt), expected, f"{tag} wt={wt:g}")
    style.apply(0.75)
    style.apply(0.3)
    direct = lr.snapshot(enc.w)
    style.apply(0.0)
    assert all(la.same_bits(enc.w[n], before[n]) for n in enc.w), "weight 0 does not restore every tensor"
    style.apply(0.3)
    assert all(la.same_bits(enc.w[n], direct[n]) for n in enc.w) and any(not la.same_bits(direct[n], before[n]) for n in direct)
