"""Operand isolation: the result of a launch depends on its logical operands and on nothing else in memory.

A plain module (like tests/launch_audit.py and tests/pool_scenario.py).  tests/test_isolation_gpu.py runs the device entry
points of ``sdlcm_amd.ops`` under it; tests/test_isolation_cpu.py checks on the CPU that it rejects emulated launches that are
wrong in exactly one way (a row past M multiplied by zero, a stale workspace slab added with weight 0, ...) and accepts the
correct ones.  Without those controls a helper that compares nothing would pass every kernel.

What it tests.  The model allocates activations and workspaces with ``torch.empty`` and reuses them across requests, so a
kernel that reads one row past M, one key past Sk or one slab of stale workspace reads the leftovers of another request.  If it
discards them with ``0 * x`` or a masked add instead of a select, a leftover NaN or infinity changes the result -- and with
finite leftovers nothing shows.  So every operand is embedded in a larger allocation of the test's own (``guarded``): a guard
zone in front, one behind and, for pitched operands, guard columns after every row; every workspace is one the test filled
(``scratch``).  The same launch then runs with three fill patterns (``check_isolated``):

    ZERO    all bits clear
    NAN     fp16 0x7E00 / fp32 0x7FC00000 (integers: all bits set)
    PINF    fp16 0x7C00 / fp32 0x7F800000 (integers: all bits set).  fmaxf(m, NaN) == m: a stray read that only feeds a
            running maximum is invisible to NaN and visible to +inf, hence both.

and must give bit-identical, finite logical outputs while every guard still holds its pattern.  ``check_batch_isolated`` does
the same between the images of one batch: one image's operands are overwritten with the pattern and every OTHER image's
outputs must be those of the clean run, bit for bit.

The guards are wide (``guard_elems``) so that a stray read of less than a tile lands inside the allocation the test owns: no
operand ever sits at the end of an allocation and nothing here is meant to fault.
"""
from __future__ import annotations

import torch

from launch_audit import same_bits

ZERO, NAN, PINF = "zero", "nan", "pinf"
PATTERNS = (ZERO, NAN, PINF)
GUARD_ROWS = 256            # guard rows (of the operand's pitch) in front of and behind an operand
GUARD_COLS = 64             # guard columns after every row of a pitched operand: pitches stay multiples of 8 halves / 16 bytes
GUARD_BYTES = 64 << 10      # never less than this in front and behind
ALIGN = 128                 # guards are whole multiples of this many elements: the operand keeps the allocation's alignment

_INT_OF = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
_BITS = {(2, NAN): 0x7E00, (2, PINF): 0x7C00, (4, NAN): 0x7FC00000, (4, PINF): 0x7F800000,
         (8, NAN): 0x7FF8000000000000, (8, PINF): 0x7FF0000000000000}


def pattern_bits(dtype, fill):
    """The integer every element of a guard of this dtype holds (as the same-width signed integer)."""
    if fill == ZERO:
        return 0
    if fill not in (NAN, PINF):
        raise ValueError(f"unknown fill pattern {fill!r}")
    if dtype.is_floating_point:
        return _BITS[(torch.empty(0, dtype=dtype).element_size(), fill)]
    return -1           # 0xFF..: all bits set (u8 255)


def _as_int(t):
    return t.view(_INT_OF[t.element_size()]) if t.dtype != torch.bool else t.view(torch.int8)


def fill_(t, fill):
    """Overwrite a CONTIGUOUS tensor, or any view row by row, with the pattern's bits."""
    bits = pattern_bits(t.dtype, fill)
    if t.is_contiguous():
        _as_int(t).fill_(bits)
    else:
        t.copy_(_as_int(torch.empty(t.shape, dtype=t.dtype, device=t.device)).fill_(bits).view(t.dtype))
    return t


def holds(t, fill):
    """Every element of t is exactly the pattern."""
    if t.numel() == 0:
        return True
    return bool((_as_int(t.contiguous()) == pattern_bits(t.dtype, fill)).all())


def guard_elems(pitch, elsize, rows=GUARD_ROWS, image_w=None):
    """Elements of one front / back guard: >= ``rows`` rows of the pitch, >= 2 (W + 2) pixels of a pixel-major image operand,
    >= 64 KiB, rounded up to ALIGN elements."""
    n = max(rows * pitch, GUARD_BYTES // elsize)
    if image_w is not None:
        n = max(n, 2 * (image_w + 2) * pitch)
    return -(-n // ALIGN) * ALIGN


class Arena:
    """One allocation holding a logical operand and its guards.  ``view`` is what the entry point receives."""

    def __init__(self, buf, start, shape, pitch, fill):
        self.buf, self.start, self.shape, self.pitch, self.fill = buf, start, tuple(shape), pitch, fill
        if pitch is None:
            n = 1
            for s in shape:
                n *= s
            self.span = n
            self.view = buf[start:start + n].view(shape)
        else:
            R, Cc = shape
            self.span = R * pitch                   # the last row's guard columns are inside the span, the back guard after it
            self.view = buf[start:start + R * pitch].view(R, pitch)[:, :Cc]

    def guards(self):
        """The guard zones as a list of (name, tensor)."""
        g = [("front", self.buf[:self.start]), ("back", self.buf[self.start + self.span:])]
        if self.pitch is not None:
            R, Cc = self.shape
            g.append(("columns", self.buf[self.start:self.start + self.span].view(R, self.pitch)[:, Cc:]))
        return g

    def damaged(self):
        """Names of the guard zones that no longer hold the fill pattern."""
        return [n for n, t in self.guards() if not holds(t, self.fill)]


def guarded(t, fill, rows=GUARD_ROWS, cols=None, image_w=None):
    """Embed the logical operand ``t`` in a larger allocation filled with ``fill`` -> (view, arena).
    cols None: ``t`` (any shape) is tightly packed, guards in front and behind.  cols = c (GUARD_COLS): ``t`` is 2-D and every
    row is followed by c guard columns (pitch = width + c).  image_w: W of a pixel-major image operand (guard >= 2 (W + 2)
    pixels).  The view has the values of ``t``."""
    elsize = t.element_size()
    if cols is None:
        pitch_for_guard = t.shape[-1] if t.dim() >= 2 else 1
        g = guard_elems(pitch_for_guard, elsize, rows, image_w)
        total, pitch = 2 * g + t.numel(), None
        shape = t.shape
    else:
        if t.dim() != 2:
            raise ValueError("a pitched operand is 2-D")
        if cols % 8:
            raise ValueError("guard columns keep pitches multiples of 8 elements")
        pitch = t.shape[1] + cols
        g = guard_elems(pitch, elsize, rows, image_w)
        total = 2 * g + t.shape[0] * pitch
        shape = t.shape
    buf = fill_(torch.empty(total, dtype=t.dtype, device=t.device), fill)
    ar = Arena(buf, g, shape, pitch, fill)
    ar.view.copy_(t)
    return ar.view, ar


def scratch(n, dtype, fill, device="cpu"):
    """A workspace of n elements whose every element is the pattern (stale contents of a reused buffer), inside guards of its
    own -> (view, arena).  Serves the split-K workspace, statistics buffers, GroupNorm / canny / resize workspaces."""
    v, ar = guarded(torch.empty(n, dtype=dtype, device=device), fill)
    fill_(v, fill)
    return v, ar


class Op:
    """How ``check_isolated`` places one operand.  t: the logical contents.  cols: guard columns (pitched 2-D operand).
    image_w: W of a pixel-major image operand.  stale: the logical extent starts as the fill pattern, not as ``t`` (an output
    the launch must write completely).  images: the operand's leading dimension stacks this many images (``poison_image``).
    copies: the leading dimension stacks that many groups of ``images`` images and image j lives in every group (the [2B, 4, h, w]
    state of a guided pass: rows j and B + j)."""

    def __init__(self, t, cols=None, image_w=None, stale=False, images=0, copies=1):
        self.t, self.cols, self.image_w, self.stale, self.images, self.copies = t, cols, image_w, stale, images, copies
        if images and t.shape[0] % (images * copies):
            raise ValueError("the leading dimension of a per-image operand is a multiple of the image count")


def _op(o):
    return o if isinstance(o, Op) else Op(o)


def _place(operands, scratch_spec, fill, scratch_fill=None):
    views, arenas = {}, {}
    for name, o in operands.items():
        if o is None:
            views[name] = None
            continue
        o = _op(o)
        v, ar = guarded(o.t, fill, cols=o.cols, image_w=o.image_w)
        if o.stale:
            fill_(v, fill)
        views[name], arenas[name] = v, ar
    for name, (n, dtype) in (scratch_spec or {}).items():
        dev = next(iter(arenas.values())).buf.device if arenas else "cpu"
        views[name], arenas[name] = scratch(n, dtype, fill if scratch_fill is None else scratch_fill, dev)
    return views, arenas


place = _place          # for a test that needs one placed set of operands of its own (a profiled launch, a custom check)


def _sync(views):
    for v in views.values():
        if v is not None and v.is_cuda:
            torch.cuda.synchronize(v.device)
            return


def _collect(views, outputs, extra):
    got = {n: views[n].clone() for n in outputs}
    for n, t in (extra if isinstance(extra, dict) else {}).items():       # ops entry points return ``out``: not a dict
        if n in got:
            raise ValueError(f"launch returned an output named like the operand {n!r}")
        got[n] = t.clone()
    return got


def _finite(t):
    return bool(torch.isfinite(t).all()) if t.is_floating_point() else True


def check_isolated(launch, operands, outputs, scratch=None, patterns=PATTERNS, what=""):
    """Run ``launch`` once per fill pattern and assert that its result depends on none of them.

    operands: {name: tensor | Op | None}, each embedded by ``guarded`` (None is passed through).  scratch: {name: (n, dtype)},
    workspaces whose every element is the pattern.  launch(v) gets {name: view} of both and may return {name: tensor} of further
    logical outputs (statistics partials up to P, tables, side outputs; views of scratch are fine: they are copied at once).
    outputs: names of operands the launch writes.

    Asserts: every logical output finite; bit-identical across the patterns; every guard zone of every operand and workspace
    still its pattern.  -> {pattern: {name: tensor}} (copies), so a caller can also hold one run against a reference."""
    runs = {}
    for fill in patterns:
        views, arenas = _place(operands, scratch, fill)
        extra = launch(views)
        _sync(views)
        got = _collect(views, outputs, extra)
        for name, ar in arenas.items():
            bad = ar.damaged()
            assert not bad, f"{what}: {fill} guard of {name!r} overwritten ({', '.join(bad)})"
        for name, t in got.items():
            assert _finite(t), f"{what}: output {name!r} is not finite under {fill} guards / scratch"
        runs[fill] = got
    first = patterns[0]
    for fill in patterns[1:]:
        assert runs[fill].keys() == runs[first].keys(), f"{what}: outputs differ in kind between {first} and {fill}"
        for name, t in runs[fill].items():
            assert same_bits(t, runs[first][name]), f"{what}: output {name!r} differs between {first} and {fill} guards / scratch"
    return runs


def poison_image(views, operands, j, fill):
    """Overwrite image j of every per-image operand (``Op.images``) with the pattern, in place in the views."""
    for name, o in operands.items():
        if o is None:
            continue
        o = _op(o)
        if not o.images:
            continue
        v = views[name]
        n = v.shape[0] // (o.images * o.copies)
        for c in range(o.copies):
            r0 = (c * o.images + j) * n
            fill_(v[r0:r0 + n], fill)


def _image(t, j, B, copies=1):
    """image j of a tensor that stacks ``copies`` groups of B images along its leading dimension"""
    n = t.shape[0] // (B * copies)
    return torch.cat([t[(c * B + j) * n:(c * B + j + 1) * n] for c in range(copies)])


def check_batch_isolated(launch, B, operands, outputs, scratch=None, fills=(NAN, PINF), images=None, what=""):
    """One clean run, then one run per poisoned image j (default 0 and B // 2: masked lanes read row 0) and fill: the outputs of
    every OTHER image must be bit-identical to the clean run and finite.

    operands / scratch / launch as in ``check_isolated``; per-image operands carry ``Op(..., images=B)``.  Outputs named in
    ``outputs`` must be per-image operands; further outputs returned by ``launch`` must stack B images along their leading
    dimension (statistics partials [B * P, ...], tables [B, C]).  Guards and workspaces are zero in every run: what they may
    leak is ``check_isolated``'s subject.  -> the clean run's outputs."""
    if B < 2:
        raise ValueError("batch isolation needs two images")
    for n in outputs:
        if not _op(operands[n]).images:
            raise ValueError(f"output {n!r} is not a per-image operand")
    images = sorted(set(images if images is not None else (0, B // 2)))

    def run(j, fill):
        views, arenas = _place(operands, scratch, ZERO)
        if j is not None:
            poison_image(views, operands, j, fill)
        extra = launch(views)
        _sync(views)
        got = _collect(views, outputs, extra)
        for name, ar in arenas.items():
            bad = ar.damaged()
            assert not bad, f"{what}: guard of {name!r} overwritten ({', '.join(bad)})"
        return got

    copies = {n: _op(operands[n]).copies for n in outputs}
    clean = run(None, None)
    for name, t in clean.items():
        assert t.shape[0] % (B * copies.get(name, 1)) == 0, f"{what}: output {name!r} does not stack {B} images"
        assert _finite(t), f"{what}: output {name!r} of the clean run is not finite"
    for j in images:
        for fill in fills:
            got = run(j, fill)
            for name, t in got.items():
                for i in range(B):
                    if i == j:
                        continue
                    a, b = _image(t, i, B, copies.get(name, 1)), _image(clean[name], i, B, copies.get(name, 1))
                    assert _finite(a), f"{what}: image {i} of {name!r} is not finite with image {j} filled with {fill}"
                    assert same_bits(a.contiguous(), b.contiguous()), \
                        f"{what}: image {i} of {name!r} changed with image {j} filled with {fill}"
    return clean
