"""Negative controls of tests/isolation.py on the CPU: torch emulations of a launch that are wrong in exactly one way -- each
reads memory outside its logical operands (or another image of its batch) and discards it in a way that finite leftovers hide
-- must be rejected, and the correct emulation accepted.  Without this the helper could compare nothing and pass every kernel.
The emulations reach past their operands with ``as_strided`` on the operand's own storage, as a kernel's address arithmetic
does; the guards of ``isolation.guarded`` are what they then read."""
import pytest
import torch

import isolation as iso
from isolation import NAN, PINF, ZERO, Op


def _rnd(*shape, seed=0, dtype=torch.float16):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dtype)


def _past(v, rows=0, cols=0):
    """The 2-D view ``v`` extended by rows past its end and columns past its width, on the same storage."""
    return v.as_strided((v.shape[0] + rows, v.shape[1] + cols), v.stride(), v.storage_offset())


# ---- the arenas themselves ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32, torch.uint8, torch.int32])
@pytest.mark.parametrize("fill", iso.PATTERNS)
def test_guard_geometry_and_patterns(dtype, fill):
    t = (torch.arange(5 * 24) % 7).to(dtype).view(5, 24)
    for cols, image_w in ((None, None), (iso.GUARD_COLS, None), (None, 33)):
        v, ar = iso.guarded(t, fill, cols=cols, image_w=image_w)
        assert torch.equal(v, t) and v.shape == t.shape
        pitch = 24 + (cols or 0)
        assert v.stride(0) == pitch and pitch % 8 == 0
        assert (v.data_ptr() - ar.buf.data_ptr()) % 16 == 0 and ar.buf.data_ptr() % 16 == 0
        front, back = ar.guards()[0][1], ar.guards()[1][1]
        for g in (front, back):
            assert g.numel() >= iso.GUARD_ROWS * pitch and g.numel() * g.element_size() >= 64 << 10
            if image_w:
                assert g.numel() >= 2 * (image_w + 2) * pitch
        assert front.numel() + back.numel() + 5 * pitch == ar.buf.numel()          # nothing of the allocation is unaccounted for
        assert ar.damaged() == []
        assert len(ar.guards()) == (3 if cols else 2)
    bits = {ZERO: 0, NAN: {2: 0x7E00, 4: 0x7FC00000}, PINF: {2: 0x7C00, 4: 0x7F800000}}[fill]
    if dtype.is_floating_point:
        want = bits if fill == ZERO else bits[t.element_size()]
        assert int(front.view(torch.int16 if dtype == torch.float16 else torch.int32)[0]) == want
        if fill == NAN:
            assert bool(torch.isnan(front).all())
        if fill == PINF:
            assert bool((front == float("inf")).all())
    elif dtype == torch.uint8:
        assert int(front[0]) == (0 if fill == ZERO else 0xFF)
    else:
        assert int(front[0]) == (0 if fill == ZERO else -1)


def test_every_guard_zone_is_watched():
    t = _rnd(4, 16)
    for zone, (r, c) in (("front", (-1, 0)), ("back", (4 + iso.GUARD_ROWS - 1, 3)), ("columns", (2, 16 + 63)), ("columns", (3, 16))):
        v, ar = iso.guarded(t, NAN, cols=iso.GUARD_COLS)
        ar.buf[ar.start + r * ar.pitch + c] = 1.0
        assert ar.damaged() == [zone]
    s, ar = iso.scratch(100, torch.float32, PINF)
    assert s.shape == (100,) and iso.holds(s, PINF) and ar.damaged() == []
    ar.buf[ar.start + 100] = 0.0
    assert ar.damaged() == ["back"]


def test_a_pitched_operand_must_be_two_dimensional_and_keep_its_alignment():
    with pytest.raises(ValueError):
        iso.guarded(_rnd(2, 3, 8), ZERO, cols=64)
    with pytest.raises(ValueError):
        iso.guarded(_rnd(3, 8), ZERO, cols=4)


# ---- 1. a GEMM that multiplies one row past M by zero ---------------------------------------------------------------------
def _gemm_stats(v, masked_by_product):
    """out = a w^T with the column sums of out as fused statistics; the tile has one row more than M."""
    a, w = v["a"], v["w"]
    M = a.shape[0]
    tile = _past(a, rows=1).float() @ w.float().T                  # [M + 1, N]: the last row is whatever follows the operand
    v["out"].copy_(tile[:M].half())
    if masked_by_product:
        keep = torch.ones(M + 1, 1)
        keep[M] = 0.0
        v["stats"].copy_((tile * keep).sum(0))                     # 0 * leftover
    else:
        v["stats"].copy_(tile[:M].sum(0))                          # select


def _gemm_case(launch, **kw):
    M, N, K = 5, 16, 32
    ops_ = dict(a=_rnd(M, K), w=_rnd(N, K, seed=1), out=Op(torch.zeros(M, N, dtype=torch.float16), cols=64, stale=True))
    return iso.check_isolated(launch, ops_, ("out",), scratch=dict(stats=(N, torch.float32)), what="gemm", **kw)


def test_gemm_row_past_m_times_zero_is_rejected():
    runs = _gemm_case(lambda v: (_gemm_stats(v, False), dict(stats=v["stats"]))[1])
    assert set(runs) == set(iso.PATTERNS) and runs[NAN]["out"].shape == (5, 16)
    with pytest.raises(AssertionError, match="stats"):
        _gemm_case(lambda v: (_gemm_stats(v, True), dict(stats=v["stats"]))[1])


# ---- 2. a GEMM that reads a gap column with a zero weight -----------------------------------------------------------------
def _gemm_padded_k(v, pad):
    a, w = v["a"], v["w"]
    if pad:
        a = _past(a, cols=8)                                         # K rounded up to the k-tile: 8 gap columns of the pitch
        w = torch.cat([w, torch.zeros(w.shape[0], 8, dtype=w.dtype)], 1)
    v["out"].copy_((a.float() @ w.float().T).half())


def test_gemm_gap_column_with_zero_weight_is_rejected():
    M, N, K = 7, 16, 24
    ops_ = dict(a=Op(_rnd(M, K), cols=64), w=_rnd(N, K, seed=1), out=Op(torch.zeros(M, N, dtype=torch.float16), stale=True))
    iso.check_isolated(lambda v: _gemm_padded_k(v, False), ops_, ("out",))
    with pytest.raises(AssertionError, match="'out'"):
        iso.check_isolated(lambda v: _gemm_padded_k(v, True), ops_, ("out",))
    # packed, the same faulty read lands in the next row (finite, weight 0) -- except for the last row, which reads the back guard
    ops_["a"] = Op(_rnd(M, K), cols=None)
    with pytest.raises(AssertionError, match="'out'"):
        iso.check_isolated(lambda v: _gemm_padded_k(v, True), ops_, ("out",))


# ---- 3. a softmax whose running maximum includes one element past n -------------------------------------------------------
def _softmax(v, n, past):
    x = v["x"]
    xe = _past(x, cols=past).float()
    m = xe[:, 0]
    for c in range(1, n + past):
        m = torch.fmax(m, xe[:, c])                                  # fmaxf: a NaN operand is ignored
    e = torch.exp(xe[:, :n] - m[:, None])
    x.copy_((e / e.sum(1, keepdim=True)).half())


def test_softmax_max_past_n_needs_the_infinity_pattern():
    n = 40
    ops_ = dict(x=Op(_rnd(9, n), cols=64))
    good = lambda v: _softmax(v, n, 0)
    bad = lambda v: _softmax(v, n, 1)
    iso.check_isolated(good, ops_, ("x",))
    iso.check_isolated(bad, ops_, ("x",), patterns=(ZERO, NAN))      # NaN alone does NOT see it: fmaxf(m, NaN) == m
    with pytest.raises(AssertionError, match="pinf"):
        iso.check_isolated(bad, ops_, ("x",), patterns=(ZERO, PINF))
    with pytest.raises(AssertionError, match="pinf"):
        iso.check_isolated(bad, ops_, ("x",))


# ---- 4. a reduce that sums a stale workspace slab with weight 0 -----------------------------------------------------------
def _splitk(v, parts, slabs_summed):
    a, w, ws = v["a"].float(), v["w"].float(), v["ws"]
    M, K = a.shape
    N = w.shape[0]
    slab = ws[:(parts + 1) * M * N].view(parts + 1, M, N)
    for p in range(parts):
        ks = slice(p * K // parts, (p + 1) * K // parts)
        slab[p] = a[:, ks] @ w[:, ks].T
    wt = torch.tensor([1.0] * parts + [0.0] * (slabs_summed - parts))
    v["out"].copy_((slab[:slabs_summed] * wt[:, None, None]).sum(0).half())


def test_reduce_of_a_stale_slab_with_weight_zero_is_rejected():
    M, N, K, parts = 6, 8, 64, 3
    ops_ = dict(a=_rnd(M, K), w=_rnd(N, K, seed=1), out=Op(torch.zeros(M, N, dtype=torch.float16), stale=True))
    sc = dict(ws=((parts + 1) * M * N, torch.float32))
    iso.check_isolated(lambda v: _splitk(v, parts, parts), ops_, ("out",), scratch=sc)
    with pytest.raises(AssertionError, match="'out'"):
        iso.check_isolated(lambda v: _splitk(v, parts, parts + 1), ops_, ("out",), scratch=sc)


# ---- 5. a statistics finalize that relies on a zeroed buffer --------------------------------------------------------------
def _stats_then_finalize(v, accumulate):
    x, st = v["x"].float(), v["stats"]
    C = x.shape[1]
    part = st[:2 * C].view(2, C)
    if accumulate:
        part[0] += x.sum(0)                                          # correct only in a buffer that was zero
        part[1] += (x * x).sum(0)
    else:
        part[0] = x.sum(0)
        part[1] = (x * x).sum(0)
    mean = part[0] / x.shape[0]
    v["tables"].copy_(torch.stack([mean, part[1] / x.shape[0] - mean * mean]))


def test_finalize_that_needs_a_zeroed_statistics_buffer_is_rejected():
    ops_ = dict(x=_rnd(35, 16), tables=Op(torch.zeros(2, 16), stale=True))
    sc = dict(stats=(64, torch.float32))
    launch = lambda acc: (lambda v: (_stats_then_finalize(v, acc), dict(partials=v["stats"][:32]))[1])
    iso.check_isolated(launch(False), ops_, ("tables",), scratch=sc)
    with pytest.raises(AssertionError, match="'(tables|partials)' is not finite under nan"):
        iso.check_isolated(launch(True), ops_, ("tables",), scratch=sc)


# ---- 6. a GroupNorm whose image-1 statistics include one pixel of image 0 -------------------------------------------------
def _groupnorm(v, B, HW, early):
    x = v["x"]
    for b in range(B):
        rows = x[b * HW:(b + 1) * HW].float()
        lo = b * HW - (early if b else 0)                            # image b > 0 starts its statistics ``early`` pixels early
        s = x[lo:(b + 1) * HW].float()
        mean, var = s.mean(), s.var(unbiased=False)
        v["out"][b * HW:(b + 1) * HW] = ((rows - mean) * torch.rsqrt(var + 1e-5)).half()


def test_groupnorm_statistics_that_include_a_pixel_of_the_previous_image_are_rejected():
    B, HW, C = 3, 35, 8
    ops_ = dict(x=Op(_rnd(B * HW, C), images=B, image_w=7), out=Op(torch.zeros(B * HW, C, dtype=torch.float16), images=B, stale=True))
    iso.check_batch_isolated(lambda v: _groupnorm(v, B, HW, 0), B, ops_, ("out",))
    with pytest.raises(AssertionError, match="image 1 of 'out' .* image 0"):
        iso.check_batch_isolated(lambda v: _groupnorm(v, B, HW, 1), B, ops_, ("out",))
    # the leak is invisible to an unpoisoned batch, whatever surrounds it
    iso.check_isolated(lambda v: _groupnorm(v, B, HW, 1), ops_, ("out",))


# ---- 7. an attention that admits the next image's first key with P = 0 but multiplies it into PV --------------------------
def _attention(v, B, Sq, Sk, d, extra):
    q, k, vv, out = v["q"], v["k"], v["v"], v["out"]
    for b in range(B):
        qb = q[b * Sq:(b + 1) * Sq].float()
        n = Sk + extra                                               # the key tile is one key longer than Sk
        kb = k.as_strided((n, d), k.stride(), k.storage_offset() + b * Sk * k.stride(0)).float()
        vb = vv.as_strided((n, d), vv.stride(), vv.storage_offset() + b * Sk * vv.stride(0)).float()
        s = qb @ kb[:Sk].T * d ** -0.5
        s = torch.cat([s, torch.full((Sq, extra), float("-inf"))], 1)        # masked BEFORE the softmax: its P is exactly 0
        p = torch.softmax(s, 1)
        out[b * Sq:(b + 1) * Sq] = (p @ vb).half()                   # ... and 0 * v[Sk] goes into the product


def test_attention_that_multiplies_a_masked_key_of_the_next_image_is_rejected():
    B, Sq, Sk, d = 3, 5, 7, 8
    ops_ = dict(q=Op(_rnd(B * Sq, d), cols=64, images=B), k=Op(_rnd(B * Sk, d, seed=1), cols=64, images=B),
                v=Op(_rnd(B * Sk, d, seed=2), cols=64, images=B), out=Op(torch.zeros(B * Sq, d, dtype=torch.float16), cols=64, images=B, stale=True))
    iso.check_batch_isolated(lambda v: _attention(v, B, Sq, Sk, d, 0), B, ops_, ("out",))
    bad = lambda v: _attention(v, B, Sq, Sk, d, 1)
    with pytest.raises(AssertionError, match="image 0 of 'out' .* image 1"):
        iso.check_batch_isolated(bad, B, ops_, ("out",))
    iso.check_batch_isolated(bad, B, ops_, ("out",), images=(0,))    # image 0 is nobody's successor: why B // 2 is poisoned too
    with pytest.raises(AssertionError):                              # the last image's extra key is the back guard
        iso.check_isolated(bad, ops_, ("out",))


# ---- 8. a launch that writes one element into a guard ---------------------------------------------------------------------
def _copy(v, stray):
    v["out"].copy_(v["x"])
    if stray == "row":
        _past(v["out"], rows=1)[-1, 0] = 1.0
    if stray == "column":
        _past(v["out"], cols=1)[2, -1] = 1.0
    if stray == "scratch":
        ws = v["ws"]
        ws.as_strided((ws.numel() + 1,), (1,), ws.storage_offset())[-1] = 1.0
    if stray == "input":
        x = v["x"]
        x.as_strided((1,), (1,), x.storage_offset() - 1)[0] = 1.0


@pytest.mark.parametrize("stray", ["row", "column", "scratch", "input"])
def test_a_write_into_a_guard_is_rejected(stray):
    ops_ = dict(x=_rnd(4, 16), out=Op(torch.zeros(4, 16, dtype=torch.float16), cols=64, stale=True))
    sc = dict(ws=(32, torch.float32))
    iso.check_isolated(lambda v: _copy(v, None), ops_, ("out",), scratch=sc)
    with pytest.raises(AssertionError, match="guard of .* overwritten"):
        iso.check_isolated(lambda v: _copy(v, stray), ops_, ("out",), scratch=sc)
    bops = dict(x=Op(_rnd(4, 16), images=2), out=Op(torch.zeros(4, 16, dtype=torch.float16), cols=64, stale=True, images=2))
    with pytest.raises(AssertionError, match="guard of .* overwritten"):
        iso.check_batch_isolated(lambda v: _copy(v, stray), 2, bops, ("out",), scratch=sc)


def test_an_output_that_is_not_written_completely_is_rejected():
    """A stale output keeps the pattern where the launch skipped it: not finite under NAN, different between patterns."""
    ops_ = dict(x=_rnd(4, 16), out=Op(torch.zeros(4, 16, dtype=torch.float16), stale=True))
    with pytest.raises(AssertionError, match="'out'"):
        iso.check_isolated(lambda v: v["out"][:3].copy_(v["x"][:3]), ops_, ("out",))


def test_poison_image_touches_per_image_operands_only():
    ops_ = dict(x=Op(_rnd(6, 8), images=3, cols=64), w=_rnd(8, 8), ids=Op(torch.arange(6, dtype=torch.int32), images=3), none=None)
    views, arenas = iso._place(ops_, None, ZERO)
    iso.poison_image(views, ops_, 1, NAN)
    assert iso.holds(views["x"][2:4], NAN) and torch.equal(views["x"][:2], ops_["x"].t[:2]) and torch.equal(views["x"][4:], ops_["x"].t[4:])
    assert torch.equal(views["w"], ops_["w"]) and views["ids"].tolist() == [0, 1, -1, -1, 4, 5]
    assert all(ar.damaged() == [] for ar in arenas.values())


def test_an_image_that_lives_in_both_halves_of_a_doubled_state():
    """Op(copies=2): image j is rows j and B + j; a launch that copies the front half from its NEIGHBOUR's back half is rejected."""
    B = 3
    x = _rnd(2 * B, 8)

    def launch(v, shift):
        s = v["state"]
        s[B:] = s[B:] * 2
        s[:B] = torch.roll(s[B:], shift, 0)

    ops_ = dict(state=Op(x, images=B, copies=2))
    iso.check_batch_isolated(lambda v: launch(v, 0), B, ops_, ("state",))
    with pytest.raises(AssertionError, match="image 1 of 'state' .* image 0 filled"):
        iso.check_batch_isolated(lambda v: launch(v, 1), B, ops_, ("state",))
