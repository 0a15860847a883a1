"""Designed attention operands: logits that are stated, not drawn, so that every branch of the three attention kernels
(csrc/attention.hip) carries weight in the output.  A plain module (like tests/pool_scenario.py): tests/test_launch_audit.py
replays the kernels' recurrences over ``table()`` on the CPU and shows that each planted fault is rejected by
``launch_audit.attention_check``; tests/test_attention_stress_gpu.py runs the same table through the kernels.

How a logit is designed.  The first c channels of a head are profile channels: query row i is (+-) one-hot over them (row i
follows kind i mod len(kinds), so the 32 rows of a wave follow different profiles: one row can trigger the wave-wide rescale of
the streaming kernel while its neighbours are far below their running max) and k_j[ch] = profile_ch[j].  The logit of (i, j)
is the profile value -- exactly representable in fp16, offset included (asserted) -- plus the product of the remaining channels,
small noise (sigma NOISE on both sides).  With scale <= 0 the profile IS the base-2 logit the kernels work in; with scale > 0
the one-hot amplitude is fl16(1 / (scale log2 e)), so the base-2 logit is the profile to within the fp16 rounding of the scaled Q.

Profiles are stated in key tiles of the kernel under test (64 keys; 32 for d = 512; the key-split boundary is tile ceil(n / 2)):
flat; staircases per tile with steps THR -+ 1/8 (rising: the running max moves at every tile or at every other one; falling: P
runs down into the fp16 subnormals; a cliff of -40 per tile over the tiles in which the rising neighbours move their max: a
lane that followed the wave's rescale downwards would scale its O out of fp32); a single key above a flat row by THR -+ 1/2 at
the first key, the last key of a full tile, both ends of the ragged tail, either side of the key-split boundary, and with all
the mass in one key group (the keys before the spike hold >= 25 % of the row's mass -- asserted -- so O, l and the folded max
all matter after the rescale; where a short sequence cannot hold that at THR + 1/2 the spike is lowered); one key per tile at 0
above a floor of -15.5; stairs and spikes under common offsets +-256 and +-1000.5 (softmax does not see them, the (hi, lo) fold
and the fp32 subtraction do); causal: a ramp whose largest visible key is the diagonal, and row 0 with its single key.

Values: v = 1 + 0.1 randn (|o| is of the size of sum p |v|), 3.0 on the keys a profile singles out; ``valt``: signs alternate
by key; ``vbig``: 60000 on one dominant key (the output comes close to the fp16 maximum and must stay finite).
"""
from __future__ import annotations

import math
import zlib
from dataclasses import dataclass, field

import numpy as np
import torch

from launch_audit import attention_kernel as kernel_of, attention_key_split, attention_tile     # the dispatch, stated once

THR = 8.0               # attn2_kernel: the running max moves when a score exceeds it by more than 2^THR
NOISE = 0.2
FLOOR = -30.0           # "no mass here": 2^-30 of a key at 0
LOG2E = 1.4426950408889634


@dataclass
class Case:
    name: str
    d: int
    heads: int
    Sq: int
    Sk: int
    causal: bool
    scale: float                     # 0.0: prescaled (base-2 logits); else d ** -0.5
    vmode: str                       # "pos" | "alt" | "big"
    profiles: list                   # [Sk] float64 arrays, the channels of every head
    kinds: list                      # (channel, sign): row i follows kinds[i % len(kinds)]
    marked: list = field(default_factory=list)      # keys whose value is 3.0
    big_key: int = -1

    @property
    def kernel(self):
        return kernel_of(self.d, self.Sk, self.causal)

    @property
    def tile(self):
        return attention_tile(self.d, self.Sk, self.causal)

    @property
    def ksplit(self):
        """the key-split form serves this shape under the default switches"""
        return attention_key_split(self.d, self.Sk, self.causal)

    @property
    def form(self):
        if self.kernel == "attn2":
            return f"attn2<{self.d}> KS {2 if self.ksplit else 1}"
        if self.kernel == "wide":
            return "attn_wide<512,32>"
        return f"attn<{self.d}>" + (" causal" if self.causal else "")

    @property
    def family(self):
        return self.kernel + ("_causal" if self.causal else "")

    def amplitude(self):
        return 1.0 if self.scale <= 0 else float(torch.tensor(1.0 / (self.scale * LOG2E)).half())

    def operands(self):
        """-> q [Sq, heads * d], k, v [Sk, heads * d] fp16 on the CPU (deterministic: seeded by the case's name)."""
        g = torch.Generator().manual_seed(zlib.crc32(self.name.encode()))
        C, c = self.heads * self.d, len(self.profiles)
        assert c + 8 <= self.d
        q = NOISE * torch.randn(self.Sq, C, generator=g)
        k = NOISE * torch.randn(self.Sk, C, generator=g)
        v = 1.0 + 0.1 * torch.randn(self.Sk, C, generator=g)
        v[self.marked] = 3.0
        if self.vmode == "alt":
            v[1::2] *= -1.0
        if self.vmode == "big":
            v[self.big_key] = 60000.0
        prof = torch.tensor(np.stack(self.profiles), dtype=torch.float64)         # [c, Sk]
        assert torch.equal(prof.half().double(), prof), f"{self.name}: a profile value is not an fp16 number"
        amp = self.amplitude()
        for h in range(self.heads):
            q[:, h * self.d:h * self.d + c] = 0.0
            for i in range(self.Sq):
                ch, sign = self.kinds[(i + h) % len(self.kinds)]           # the heads follow the kinds one row apart
                q[i, h * self.d + ch] = sign * amp
            k[:, h * self.d:h * self.d + c] = prof.T.float()
        return q.half(), k.half(), v.half()


# ---- profiles ----------------------------------------------------------------------------------------------------------
def _tiles(Sk, tile):
    return (Sk + tile - 1) // tile


def flat(Sk, off=0.0):
    return np.full(Sk, off)


def stair(Sk, tile, step, *, rising=True, top=None, bottom=None, steps=5):
    """levels per tile: rising over the LAST min(n, steps) tiles (flat before them), or falling over the first ones (flat after).
    top / bottom pin the highest / lowest level (an offset that keeps every value inside the fp16 grid of its step)."""
    n = _tiles(Sk, tile)
    s = min(n, steps)
    t = np.arange(Sk) // tile
    lvl = np.clip(t - (n - s), 0, s - 1) if rising else np.clip(s - 1 - t, 0, s - 1)
    p = step * lvl.astype(np.float64)
    if top is not None:
        p += top - step * (s - 1)
    elif bottom is not None:
        p += bottom
    return p


def spike(Sk, pos, h, *, off=0.0, after=-8.0, lo=0, hi=None):
    """keys [lo, pos) at off, key pos at off + h, keys (pos, hi) at off + after, everything else at off + FLOOR."""
    hi = Sk if hi is None else hi
    p = np.full(Sk, off + FLOOR)
    p[lo:pos] = off
    p[pos] = off + h
    p[pos + 1:hi] = off + after
    return p


def two_level(Sk, tile):
    p = np.full(Sk, -15.5)
    for t in range(_tiles(Sk, tile)):
        p[min(Sk - 1, t * tile + (7 * t + 3) % tile)] = 0.0
    return p


def earlier_share(p, pos):
    w = np.exp2(p - p.max())
    return float(w[:pos].sum() / w.sum())


def spike_height(want, earlier, lowered):
    """want, or (lowered) the largest multiple of 1/2 at which `earlier` keys at 0 still hold 25 % of 1 * earlier + 2^h."""
    if not lowered or earlier == 0:
        return want
    return min(want, math.floor(2 * math.log2(3 * earlier)) / 2 - (8.5 - want))


def spike_positions(Sk, tile, ksplit):
    """name -> (key, first key carrying mass, end of the keys carrying mass)"""
    n, full = _tiles(Sk, tile), Sk // tile
    pos = {"first": (0, 0, Sk)}
    tf = min(full, 192 // tile)                                   # a full tile with 191 keys in front of its last, if there is one
    pos["full_last"] = (tf * tile - 1, 0, Sk)
    if Sk % tile:
        pos["tail_first"] = (full * tile, 0, Sk)
    pos["tail_last" if Sk % tile else "last"] = (Sk - 1, 0, Sk)
    if n > 6:
        pos["middle"] = ((n // 2) * tile + tile // 2 + 1, 0, Sk)
    if ksplit:
        bk = ((n + 1) // 2) * tile
        pos["split_left"] = (bk - 1, 0, Sk)
        pos["split_right"] = (bk, 0, Sk)
        pos["group1_only"] = (bk + 3 * tile + 17, bk, Sk)
        pos["group0_only"] = (3 * tile + 17, 0, bk)
    return pos


# ---- the table ---------------------------------------------------------------------------------------------------------
def _shape_cases(tag, d, heads, Sq, Sk, causal, *, kinds_of=("steps", "spikes", "offsets", "scaled"), vmodes=()):
    kern = kernel_of(d, Sk, causal)
    tile, ksplit = attention_tile(d, Sk, causal), attention_key_split(d, Sk, causal)
    lowered = kern != "attn2"                   # no threshold to straddle there: keep the 25 % instead
    positions = spike_positions(Sk, tile, ksplit)
    out = []

    def add(kind, scale, vmode, profiles, kinds, marked, big_key=-1):
        out.append(Case(f"{tag}-{kind}" + ("" if vmode == "pos" else f"-v{vmode}"), d, heads, Sq, Sk, causal, scale, vmode,
                        profiles, kinds, sorted(set(int(m) for m in marked)), big_key))

    def spikes(want, names=None, off=0.0):
        profs, marks = [], []
        for nm, (key, lo, hi) in positions.items():
            if names is not None and nm not in names:
                continue
            h = spike_height(want, key - lo, lowered)
            p = spike(Sk, key, h, off=off, lo=lo, hi=hi)
            assert key == lo or earlier_share(p, key) >= 0.25, (tag, nm, earlier_share(p, key))
            profs.append(p)
            marks.append(key)
        return profs, marks

    if causal:
        ramp = np.arange(Sk) / 2.0                                  # the diagonal is the largest key a row sees
        profs = [ramp, flat(Sk), spike(Sk, 0, 8.5, after=0.0), two_level(Sk, tile), spike(Sk, min(Sk - 1, 70), 8.5)]
        kinds = [(0, 1), (1, 1), (2, 1), (0, -1), (3, 1), (4, 1)]
        marked = [0, min(Sk - 1, 70)]
        add("causal", 0.0, "pos", profs, kinds, marked)
        add("causal_scaled", d ** -0.5, "pos", profs, kinds, marked)
        for vm in vmodes:
            add("causal", 0.0, vm, profs, kinds, marked, big_key=min(Sk - 1, 70))
        return out

    n = _tiles(Sk, tile)
    last_tile = [(n - 1) * tile + 5 % (Sk - (n - 1) * tile)]
    if "steps" in kinds_of:
        profs = [flat(Sk), stair(Sk, tile, THR - 0.125), stair(Sk, tile, THR + 0.125), stair(Sk, tile, THR - 0.125, rising=False),
                 stair(Sk, tile, THR + 0.125, rising=False), two_level(Sk, tile), stair(Sk, tile, -40.0)]
        add("steps", 0.0, "pos", profs, [(c, 1) for c in range(7)] + [(2, -1)], [5] + last_tile)
    if "spikes" in kinds_of:
        hi_p, marks = spikes(THR + 0.5)
        lo_p, _ = spikes(THR - 0.5)
        add("spikes", 0.0, "pos", hi_p + lo_p, [(c, 1) for c in range(len(hi_p) + len(lo_p))], marks)
        for vm in vmodes:
            big = positions["full_last"][0]
            add("spikes", 0.0, vm, hi_p, [(c, 1) for c in range(len(hi_p))], marks, big_key=big)
    if "offsets" in kinds_of:
        where = ("split_right",) if ksplit else ("middle",) if "middle" in positions else ("full_last",)
        profs, marks = [], []
        for off, step in ((256.0, THR + 0.125), (-256.0, THR + 0.125), (1000.5, THR + 0.5), (-1000.5, THR + 0.5)):
            profs.append(stair(Sk, tile, step, top=off) if off > 0 else stair(Sk, tile, step, bottom=off))
            sp, mk = spikes(THR + 0.5, where, off)
            profs += sp
            marks += mk
        add("offsets", 0.0, "pos", profs, [(c, 1) for c in range(len(profs))], marks + last_tile)
    if "scaled" in kinds_of:
        sp, mk = spikes(THR + 0.5, ("first", "full_last", "tail_last", "last", "split_right", "group1_only"))
        profs = [flat(Sk), stair(Sk, tile, THR + 0.125), stair(Sk, tile, THR + 0.125, rising=False), two_level(Sk, tile)] + sp
        add("scaled", d ** -0.5, "pos", profs, [(c, 1) for c in range(len(profs))], mk + last_tile)
    return out


def table():
    """every case: (form, shape) x (steps | spikes | offsets | scaled), the sign-alternating and the large-value variants once
    per kernel.  Two heads (one for d = 512), Sq != Sk wherever the ABI allows it."""
    T = []
    both = ("alt", "big")
    # attn_kernel<40/64/80>: Sk < 128 (one full tile and a ragged one)
    T += _shape_cases("a40-70x77", 40, 2, 70, 77, False, vmodes=both)
    T += _shape_cases("a40-40x127", 40, 2, 40, 127, False)
    T += _shape_cases("a64-40x127", 64, 2, 40, 127, False)
    T += _shape_cases("a80-70x77", 80, 2, 70, 77, False)
    # attn_kernel<160>
    T += _shape_cases("a160-70x200", 160, 2, 70, 200, False)
    T += _shape_cases("a160-33x64", 160, 2, 33, 64, False)
    # attn_kernel, causal (150: a workgroup whose first two tiles take the unmasked path)
    T += _shape_cases("c64-77", 64, 2, 77, 77, True)
    T += _shape_cases("c64-150", 64, 2, 150, 150, True, vmodes=both)
    # attn2, one key group: 330 keys, and 4160 (just past the key-split range)
    for d in (40, 64, 80):
        T += _shape_cases(f"s{d}-96x330", d, 2, 96, 330, False, vmodes=both if d == 40 else ())
        T += _shape_cases(f"s{d}-96x4160", d, 2, 96, 4160, False)
    # attn2, two key groups: 1030 (17 tiles: group 1 idles once, ragged tail in group 1) and 1088 (17 full tiles)
    for d in (40, 64, 80):
        T += _shape_cases(f"s{d}-96x1030", d, 2, 96, 1030, False, vmodes=both if d == 64 else ())
        T += _shape_cases(f"s{d}-96x1088", d, 2, 96, 1088, False)
    # attn2<40>, 256 query rows x 2 key groups (reached with 8 waves forced): two workgroups
    T += _shape_cases("s40-300x1088", 40, 2, 300, 1088, False, kinds_of=("steps", "spikes"))
    # attn_wide<512, 32>
    T += _shape_cases("w512-70x100", 512, 1, 70, 100, False, vmodes=both)
    T += _shape_cases("w512-33x33", 512, 1, 33, 33, False)
    names = [c.name for c in T]
    assert len(set(names)) == len(names)
    return T
