"""Operand isolation of the device entry points of ``sdlcm_amd.ops`` (tests/isolation.py): every launch runs with its operands
inside ZERO / NaN / +inf guards and its workspaces filled with the same pattern, and must give the same finite bits; the
per-image entry points run with one image of the batch overwritten by NaN / +inf, and every other image must keep the bits of
the clean run.  One case per (entry point, kernel form) also holds the NaN-guard run against the fp64 reference of
tests/launch_audit.py (ratio <= 1): a kernel that computes nothing is isolated too.

Shapes are the smallest at which a kernel still has an edge: one row, a ragged last tile, more than one workgroup, images whose
rows are no multiple of the tile, odd image sides.  All poison lives in allocations of the test's own; the guards are wider
than any tile, so a stray read stays inside them."""
import numpy as np
import pytest
import torch

import isolation as iso
import launch_audit as la
from isolation import NAN, PINF, ZERO, Op
from sdlcm_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
GC = iso.GUARD_COLS
F16, F32, U8 = torch.float16, torch.float32, torch.uint8


def rnd(*shape, seed=0, scale=1.0, dtype=F16):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(DEV)


def ru8(*shape, seed=0):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)).to(DEV)


def out16(*shape, **kw):
    """an fp16 output the launch must write completely: it starts as the fill pattern"""
    return Op(torch.zeros(*shape, dtype=F16, device=DEV), stale=True, **kw)


def outof(dtype, *shape, **kw):
    return Op(torch.zeros(*shape, dtype=dtype, device=DEV), stale=True, **kw)


def to_nhwc(x):
    B, C, H, W = x.shape
    return x.permute(0, 2, 3, 1).reshape(B * H * W, C).contiguous()


def pack3x3(w):
    return w.permute(0, 2, 3, 1).contiguous().reshape(w.shape[0], -1)


def _reset():
    ops.plan_reset()
    ops.set_kernel_variant(-1)
    ops.set_staged_epilogue(1)
    ops.set_seg_mode(0)
    ops.set_split_policy()
    ops.set_persist_n(0)
    ops.set_halo_pipe_threshold(768)
    ops.set_conv_impl(1)
    ops.set_gn_fused_bytes(8 << 20)
    ops.set_attention_ksplit(1)
    ops.set_attention_impl(1)
    ops.set_workspace(None)


@pytest.fixture(autouse=True)
def _library_defaults():
    """every switch a case forces goes back to the library's default, whatever the case did"""
    try:
        yield
    finally:
        torch.cuda.synchronize()
        _reset()


def launch_names(launch, operands, sc):
    """the kernels one launch on placed operands runs, by the library's own launch profile (as tests/test_narrow_tiles_gpu.py)"""
    views, _ = iso.place(operands, sc, ZERO)
    ops.profile_begin()
    launch(views)
    names = [n for n, _ in ops.profile_end()]
    torch.cuda.synchronize()
    return names


def _same_everywhere(runs_by_form, what):
    """the forms the dispatcher may choose give one result (the ZERO run of each)"""
    tags = list(runs_by_form)
    first = runs_by_form[tags[0]][ZERO]
    for tag in tags[1:]:
        for name, t in runs_by_form[tag][ZERO].items():
            assert la.same_bits(t, first[name]), f"{what}: output {name!r} differs between forms {tags[0]} and {tag}"


# ==== dense contractions ===================================================================================================
def _gemm_forms(M, N, K, m_img):
    """(tag, setup) of the forms the dispatcher may be made to choose for this shape: plan-table tiles (160 wide included), ring
    variants, the 32-column tile, the staged epilogue on / off."""
    sp = ops.canonical_splits(0, m_img, N, K)
    forms = [("default", lambda: None)]

    def plan(bm, bn, var, staged=1, narrow=False):
        def setup():
            ops.plan_set(0, M, N, K, 1, bm, bn, sp, var)
            if narrow:
                ops.narrow_set(0, M, N, K, 1)
            ops.set_staged_epilogue(staged)
        return setup

    for bm, bn, var in ((64, 64, 0), (64, 64, 4), (128, 64, 2), (64, 128, 1), (128, 128, 3), (64, 160, 1), (128, 160, 2)):
        if N % bn or (bm == 128 and M < 128):
            continue
        forms.append((f"{bm}x{bn} v{var}", plan(bm, bn, var)))
    forms.append(("64x64 v1 staged epilogue off", plan(64, 64, 1, staged=0)))
    forms.append(("64x64 v2 staged gemm epilogue", plan(64, 64, 2, staged=3)))
    forms.append(("32-column tile", plan(64, 64, -1, narrow=True)))
    return forms


def _with_form(setup, fn):
    ops.plan_clear()
    ops.narrow_clear()
    try:
        setup()
        return fn()
    finally:
        torch.cuda.synchronize()
        _reset()


@pytest.mark.parametrize("M,N,K,img,stats", [(1, 64, 64, 0, False), (77, 320, 64, 0, False), (77, 64, 320, 0, False),
                                             (459, 320, 320, 153, False), (480, 64, 320, 160, True), (480, 320, 64, 160, True)])
def test_gemm_shapes_and_forms(M, N, K, img, stats):
    """bias + residual, lda / ldo / ldr = width + 64, one row, a ragged m-tile, images of 153 rows (no multiple of a tile) and of
    160 rows with fused statistics, under every form."""
    a, w, b, r = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=K ** -0.5), rnd(N, seed=3), rnd(M, N, seed=4)
    operands = dict(a=Op(a, cols=GC), w=w, bias=b, res=Op(r, cols=GC), out=out16(M, N, cols=GC))
    sc = dict(stats=(ops.stats_floats(M, N, img), F32)) if stats else None

    def launch(v):
        st = ops.Stats(v["stats"]) if stats else None
        ops.gemm(v["a"], v["w"], v["out"], bias=v["bias"], res=v["res"], stats=st, img_rows=img)
        if stats:
            assert st.P == img // 32
            return dict(partials=v["stats"][:(M // img) * st.P * N * 2])

    runs, names = {}, {}
    for tag, setup in _gemm_forms(M, N, K, img or M):
        def one():
            names[tag] = launch_names(launch, operands, sc)
            return iso.check_isolated(launch, operands, ("out",), scratch=sc, what=f"gemm {M}x{N}x{K} {tag}")
        runs[tag] = _with_form(setup, one)
    _same_everywhere(runs, f"gemm {M}x{N}x{K}")
    for tag, ns in names.items():                                     # a plan the dispatcher did not take would re-test the default form
        if tag[0].isdigit() and "x" in tag.split()[0] and "column" not in tag:
            bm, bn = tag.split()[0].split("x")
            assert any(f"_kernel<{bm}, {bn}, " in n for n in ns), (tag, ns)
    assert any("igemm" in n and "_kernel<64, 32, " in n for n in names["32-column tile"]), names["32-column tile"]
    ref, bnd = la.gemm_reference(a, w, bias=b, res=r)
    assert la.worst_ratio(runs["default"][NAN]["out"], ref, bnd) <= 1.0


@pytest.mark.parametrize("epilogue", [0, 1, 2, 3])
def test_gemm_epilogues_concat_rowadd_alias(epilogue):
    """the a2 concat, a per-image row add, out_scale and the activation epilogues; epilogue 0 also with ``res`` sharing storage
    with ``out``."""
    from sdlcm_amd.packing import pack_geglu
    M, N, K1, K2, rpb = 154, 320, 64, 64, 77
    a1, a2 = rnd(M, K1, seed=1), rnd(M, K2, seed=2)
    w, b = rnd(N, K1 + K2, seed=3, scale=(K1 + K2) ** -0.5), rnd(N, seed=4)
    if epilogue == 1:
        w, b = (t.to(DEV) for t in pack_geglu(w.cpu(), b.cpu()))
    radd, r = rnd(M // rpb, N, seed=5), rnd(M, N, seed=6)
    No = N // 2 if epilogue == 1 else N
    geglu = epilogue == 1
    if geglu:                                                         # the library refuses GEGLU with a concat, a row add or a residual
        a1, a2 = torch.cat([a1, a2], 1), None
    operands = dict(a=Op(a1, cols=GC), a2=None if geglu else Op(a2, cols=GC), w=w, bias=b, rowadd=None if geglu else Op(radd, cols=GC),
                    res=None if geglu else Op(r, cols=GC), out=out16(M, No, cols=GC))

    def launch(v):
        ops.gemm(v["a"], v["w"], v["out"], a2=v["a2"], bias=v["bias"], rowadd=v["rowadd"], rows_per_batch=0 if geglu else rpb,
                 res=v["res"], epilogue=epilogue, out_scale=1.0 if geglu else 0.5, img_rows=rpb)

    runs = iso.check_isolated(launch, operands, ("out",), what=f"gemm epilogue {epilogue}")
    ref, bnd = la.gemm_reference(a1, w, a2=a2, bias=b, rowadd=None if geglu else radd, rows_per_batch=rpb,
                                 res=None if geglu else r, out_scale=1.0 if geglu else 0.5, epilogue=epilogue)
    assert la.worst_ratio(runs[NAN]["out"], ref, bnd) <= 1.0
    if epilogue == 0:
        alias = dict(operands, res=None, out=Op(r, cols=GC))          # out starts as the residual and is read as ``res``

        def launch_alias(v):
            ops.gemm(v["a"], v["w"], v["out"], a2=v["a2"], bias=v["bias"], rowadd=v["rowadd"], rows_per_batch=rpb, res=v["out"],
                     out_scale=0.5, img_rows=rpb)

        got = iso.check_isolated(launch_alias, alias, ("out",), what="gemm res aliases out")
        assert la.same_bits(got[NAN]["out"], runs[NAN]["out"])


def test_gemm_batched_with_strided_gaps():
    """batch = 2: 8 rows between the two problems of A and of out hold NaN (A) or stay stale (out)."""
    Z, M, N, K, gap = 2, 70, 64, 128, 8
    a = rnd(Z * (M + gap), K, seed=1)
    for z in range(Z):
        a[z * (M + gap) + M:(z + 1) * (M + gap)] = float("nan")
    w = rnd(Z * N, K, seed=2, scale=K ** -0.5)
    operands = dict(a=Op(a, cols=GC), w=w, out=out16(Z * (M + gap), N, cols=GC))

    def launch(v):
        A, O = v["a"], v["out"]
        ops.gemm(A, v["w"], O, M=M, N=N, K=K, lda=A.stride(0), ldo=O.stride(0), batch=Z, strideA=(M + gap) * A.stride(0),
                 strideW=N * K, strideO=(M + gap) * O.stride(0), out_scale=0.25)
        return {f"out{z}": O[z * (M + gap):z * (M + gap) + M] for z in range(Z)}

    def gaps_untouched(v, fill):
        return all(iso.holds(v["out"][z * (M + gap) + M:(z + 1) * (M + gap)].contiguous(), fill) for z in range(Z))

    runs = iso.check_isolated(launch, operands, (), what="gemm batch 2")
    for z in range(Z):
        ref, bnd = la.gemm_reference(a[z * (M + gap):z * (M + gap) + M], w[z * N:(z + 1) * N], out_scale=0.25)
        assert la.worst_ratio(runs[NAN][f"out{z}"], ref, bnd) <= 1.0
    for fill in iso.PATTERNS:                                         # the gap rows of out are nobody's to write
        views, _ = iso.place(operands, None, fill)
        launch(views)
        torch.cuda.synchronize()
        assert gaps_untouched(views, fill)


@pytest.mark.parametrize("seg", [2, 1])
def test_gemm_split_k_with_a_stale_workspace(seg):
    """a shape whose canonical K partition has parts: the split launch + reduce (seg 2) and the segmented form (seg 1) with
    every slab of the workspace, and the statistics buffer, holding the pattern."""
    M, N, K = 64, 1280, 2560
    parts = ops.canonical_splits(0, M, N, K)
    assert parts > 1, "pick a shape whose canonical partition has parts"
    a, w, b, r = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=K ** -0.5), rnd(N, seed=3), rnd(M, N, seed=4)
    operands = dict(a=Op(a, cols=GC), w=w, bias=b, res=Op(r, cols=GC), out=out16(M, N, cols=GC))
    sc = dict(ws=(parts * M * N + 4096, F32), stats=(ops.stats_floats(M, N, M), F32))

    def launch(v):
        ops.set_workspace(v["ws"])
        ops.set_seg_mode(seg)
        st = ops.Stats(v["stats"])
        ops.gemm(v["a"], v["w"], v["out"], bias=v["bias"], res=v["res"], stats=st)
        assert st.P > 0
        return dict(partials=v["stats"][:st.P * N * 2])

    runs = iso.check_isolated(launch, operands, ("out",), scratch=sc, what=f"gemm split-K seg {seg}")
    ref, bnd = la.gemm_reference(a, w, bias=b, res=r)
    assert la.worst_ratio(runs[NAN]["out"], ref, bnd) <= 1.0


def test_gemm_images_of_a_batch():
    """B = 3 images of 160 rows: row add per image, residual, fused statistics; one image poisoned at a time."""
    B, img, N, K = 3, 160, 320, 320
    M = B * img
    operands = dict(a=Op(rnd(M, K, seed=1), cols=GC, images=B), w=rnd(N, K, seed=2, scale=K ** -0.5), bias=rnd(N, seed=3),
                    rowadd=Op(rnd(B, N, seed=5), images=B), res=Op(rnd(M, N, seed=4), cols=GC, images=B), out=out16(M, N, cols=GC, images=B))
    sc = dict(stats=(ops.stats_floats(M, N, img), F32))

    def launch(v):
        st = ops.Stats(v["stats"])
        ops.gemm(v["a"], v["w"], v["out"], bias=v["bias"], rowadd=v["rowadd"], rows_per_batch=img, res=v["res"], stats=st, img_rows=img)
        assert st.P == img // 32
        return dict(partials=v["stats"][:B * st.P * N * 2].view(B * st.P, N * 2))

    for tag, setup in _gemm_forms(M, N, K, img)[:4]:
        _with_form(setup, lambda: iso.check_batch_isolated(launch, B, operands, ("out",), scratch=sc, what=f"gemm batch {tag}"))


@pytest.mark.parametrize("M,img", [(1, 0), (77, 0), (459, 153)])
@pytest.mark.parametrize("geglu", [False, True])
def test_gemm_ln(M, img, geglu):
    from sdlcm_amd.packing import pack_geglu
    K, N = 320, 640
    x = (rnd(M, K, seed=1).float() * 0.7 + 1.0).half()
    W, c = rnd(N, K, seed=4, scale=K ** -0.5).cpu().float(), rnd(N, seed=5, scale=0.3).cpu().float()
    if geglu:
        W, c = pack_geglu(W, c)
    Wh = W.half().to(DEV)
    g, c = Wh.float().sum(1), c.to(DEV)
    operands = dict(a=Op(x, cols=GC), w=Wh, g=g, c=c, out=out16(M, N // 2 if geglu else N, cols=GC))
    launch = lambda v: ops.gemm_ln(v["a"], v["w"], v["g"], v["c"], v["out"], epilogue=1 if geglu else 0, img_rows=img)
    runs = {}
    for tag, setup in _gemm_forms(M, N, K, img or M):
        if "160" in tag and geglu:
            continue
        runs[tag] = _with_form(setup, lambda: iso.check_isolated(launch, operands, ("out",), what=f"gemm_ln M={M} {tag}"))
    _same_everywhere(runs, f"gemm_ln M={M}")
    ref, bnd = la.gemm_ln_reference(x, Wh, g, c, epilogue=1 if geglu else 0)
    assert la.worst_ratio(runs["default"][NAN]["out"], ref, bnd) <= 1.0
    if img:
        bops = dict(operands, a=Op(x, cols=GC, images=3), out=out16(M, N // 2 if geglu else N, cols=GC, images=3))
        iso.check_batch_isolated(launch, 3, bops, ("out",), what="gemm_ln batch")


@pytest.mark.parametrize("extra", [0, 77])
def test_mlp_geglu_at_its_smallest_row_count(extra):
    """the smallest M the fused FeedForward serves, and that M + 77: a ragged last workgroup"""
    from sdlcm_amd.packing import pack_ff2_cols, pack_geglu
    C, Fh = 320, 1280
    M = next(m for m in range(1, 1 << 16) if ops.mlp_fused_applies(m, C, 0))
    assert not ops.mlp_fused_applies(M - 1, C, 0)
    M += extra
    assert ops.mlp_fused_applies(M, C, 0)
    x = (rnd(M, C, seed=1).float() * 0.7 + 0.5).half()
    gamma, beta = 1 + 0.2 * rnd(C, seed=2).cpu().float(), rnd(C, seed=3, scale=0.2).cpu().float()
    W1, b1 = rnd(2 * Fh, C, seed=4, scale=C ** -0.5).cpu().float(), rnd(2 * Fh, seed=5, scale=0.3).cpu().float()
    Wg, c = pack_geglu(W1 * gamma[None, :], W1 @ beta + b1)
    W1h = Wg.half().to(DEV)
    g = W1h.float().sum(1)
    W2p, b2 = pack_ff2_cols(rnd(C, Fh, seed=6, scale=Fh ** -0.5).cpu()).to(DEV), rnd(C, seed=7, scale=0.3)
    operands = dict(x=Op(x, cols=GC), w1=W1h, g=g, c=c.to(DEV), w2=W2p, b2=b2, out=out16(M, C, cols=GC))
    launch = lambda v: ops.mlp_geglu(v["x"], v["w1"], v["g"], v["c"], v["w2"], v["b2"], v["out"])
    runs = iso.check_isolated(launch, operands, ("out",), what="mlp_geglu")
    for rows in (slice(0, 128), slice(M - 128, M)):
        ref, bnd = la.mlp_geglu_reference(x, W1h, g, c.to(DEV), W2p, b2, rows=rows)
        assert la.worst_ratio(runs[NAN]["out"][rows], ref, bnd) <= 1.0


@pytest.mark.parametrize("M,N,K,xr,rr,si,so", [(1, 64, 64, None, None, False, True), (5, 320, 320, None, None, True, False),
                                               (77, 320, 64, None, None, False, False), (6, 64, 320, 2, 3, True, True)])
def test_linear_rows(M, N, K, xr, rr, si, so):
    x, w, b, r = rnd(xr or M, K, seed=1), rnd(N, K, seed=2, scale=K ** -0.5), rnd(N, seed=3), rnd(rr or M, N, seed=4)
    operands = dict(x=Op(x, cols=GC), w=w, bias=b, res=Op(r, cols=GC), out=out16(M, N, cols=GC))
    launch = lambda v: ops.linear_rows(v["x"], v["w"], v["out"], M, N, K, x_rows=xr, bias=v["bias"], res=v["res"], res_rows=rr,
                                       silu_in=si, silu_out=so)
    runs = iso.check_isolated(launch, operands, ("out",), what="linear_rows")
    ref, bnd = la.linear_reference(x, w, M, x_rows=xr, bias=b, res=r, res_rows=rr, silu_in=si, silu_out=so)
    assert la.worst_ratio(runs[NAN]["out"], ref, bnd) <= 1.0


@pytest.mark.parametrize("M,N,K,si,so", [(1, 320, 64, False, True), (3, 64, 320, True, False), (8, 320, 320, False, False)])
def test_linear_smallm(M, N, K, si, so):
    x, w, b, r = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=K ** -0.5), rnd(N, seed=3), rnd(M, N, seed=4)
    operands = dict(x=Op(x, cols=GC), w=w, bias=b, res=Op(r, cols=GC), out=out16(M, N, cols=GC))
    launch = lambda v: ops.linear_smallm(v["x"], v["w"], v["out"], M, N, K, bias=v["bias"], res=v["res"], silu_in=si, silu_out=so)
    runs = iso.check_isolated(launch, operands, ("out",), what="linear_smallm")
    ref, bnd = la.linear_reference(x, w, M, bias=b, res=r, silu_in=si, silu_out=so)
    assert la.worst_ratio(runs[NAN]["out"], ref, bnd) <= 1.0


# ==== 3x3 convolutions =====================================================================================================
SIDES = [(1, 1), (5, 7), (9, 13), (16, 16), (17, 33)]


def _conv_forms(kind, M, Cout, K, aux, sp, Wo, narrow=False):
    """halo (single buffer / pipelined by threshold and by variant), row gather, tiles, staged epilogue off"""
    def plan(bm, bn, var, thr=768, staged=1):
        def setup():
            ops.plan_set(kind, M, Cout, K, aux, bm, bn, sp, var)
            ops.set_halo_pipe_threshold(thr)
            ops.set_staged_epilogue(staged)
        return setup

    forms = [("default", lambda: None), ("row gather", lambda: ops.set_conv_impl(0)),
             ("pipelined", lambda: ops.set_halo_pipe_threshold(1 << 30)), ("single buffer", lambda: ops.set_halo_pipe_threshold(0))]
    for var in (1, 2, 3):
        forms.append((f"64x64 v{var}", plan(64, 64, var)))
    forms.append(("64x64 v3 staged epilogue off", plan(64, 64, 3, staged=0)))
    if Cout % 128 == 0 and M >= 128 and (Wo % 16 == 0 or Wo > 16):
        forms.append(("128x128 v3", plan(128, 128, 3)))
    if narrow:                                                        # the narrow table serves plain stride-1 launches that run pipelined

        def narrow_form():
            ops.narrow_set(2, M, Cout, K, aux)
            ops.set_halo_pipe_threshold(1 << 30)
        forms.append(("32-column tile", narrow_form))
    return forms


def _conv_geometry(H, W, stride, ups, odd):
    out_hw = None
    if ups == 1 and odd:
        out_hw = (2 * H - 1, 2 * W - 1)
    Ho, Wo = out_hw if out_hw else (2 * H, 2 * W) if ups else ((H + 1) // 2, (W + 1) // 2) if stride == 2 else (H, W)
    return out_hw, Ho, Wo


@pytest.mark.parametrize("H,W", SIDES)
@pytest.mark.parametrize("mode", ["s1", "s2", "ups1 odd", "ups2"])
def test_conv3x3(H, W, mode):
    """B = 3, bias + row add + residual, 64 -> 128 (128 -> 64 for the upsamples); every form with a statistics buffer (the halo
    kernels then always write statistics, the row-gather ones where Ho Wo is a multiple of 32) and without one: same output bits."""
    from sdlcm_amd.packing import pack_conv3x3_up2
    B = 3
    stride, ups, odd = dict(s1=(1, 0, False), s2=(2, 0, False), ups2=(1, 2, False))[mode] if mode != "ups1 odd" else (1, 1, True)
    Cin, Cout = (128, 64) if ups else (64, 128)
    out_hw, Ho, Wo = _conv_geometry(H, W, stride, ups, odd)
    HW, M, K = Ho * Wo, B * Ho * Wo, (4 if ups == 2 else 9) * Cin
    kind, aux, ph = (1, 1, 0) if stride == 2 else (2, Wo << 1, 1 if ups == 2 else 0)
    x = to_nhwc(rnd(B, Cin, H, W, seed=1))
    w4 = rnd(Cout, Cin, 3, 3, seed=2, scale=(9 * Cin) ** -0.5)
    w = pack_conv3x3_up2(w4.cpu()).to(DEV) if ups == 2 else pack3x3(w4)
    b, ra, rs = rnd(Cout, seed=3), rnd(B, Cout, seed=4), rnd(M, Cout, seed=5)
    operands = dict(x=Op(x, image_w=W, images=B), w=w, bias=b, rowadd=Op(ra, images=B), res=Op(rs, image_w=Wo, images=B),
                    out=out16(M, Cout, image_w=Wo, images=B))
    sc = dict(stats=(ops.stats_floats(M, Cout, HW), F32))

    def launch(v, stats=True):
        st = ops.Stats(v["stats"]) if stats else None
        ops.conv3x3(v["x"], v["w"], v["out"], B, H, W, Cin, Cout, bias=v["bias"], rowadd=v["rowadd"], res=v["res"], stride=stride,
                    ups=ups, stats=st, out_hw=out_hw)
        if stats and st.P > 0:
            return dict(partials=v["stats"][:B * st.P * Cout * 2].view(B * st.P, Cout * 2))

    sp = ops.canonical_splits(kind, HW, Cout, K, aux, ph)
    runs, names = {}, {}
    for tag, setup in _conv_forms(kind, M, Cout, K, aux, sp, Wo, narrow=(mode == "s1")):
        if stride == 2 and tag not in ("default", "64x64 v1", "64x64 v2"):
            continue                                                  # the stride-2 conv has the row-gather kernel only
        what = f"conv3x3 {mode} {H}x{W} {tag}"

        def one():
            names[tag] = launch_names(launch, operands, sc)
            on = iso.check_isolated(launch, operands, ("out",), scratch=sc, what=what)
            off = iso.check_isolated(lambda v: launch(v, False), operands, ("out",), scratch=sc, what=what + ", statistics off")
            assert la.same_bits(off[ZERO]["out"], on[ZERO]["out"]), f"{what}: the output depends on whether statistics are asked for"
            return on
        runs[tag] = _with_form(setup, one)
    halo = {t: r for t, r in runs.items() if t != "row gather"}       # the two implementations differ in summation order
    _same_everywhere(halo, f"conv3x3 {mode} {H}x{W}")
    if mode == "s1" and any(n.startswith("conv_halo") for n in names["default"]):     # the forced forms ran the kernels they name
        assert any(n.startswith("igemm") for n in names["row gather"]) and not any("conv_halo" in n for n in names["row gather"])
        assert any(n.startswith("conv_halo_pipe_kernel<") for n in names["pipelined"]), names["pipelined"]
        assert any(n.startswith("conv_halo_kernel<") for n in names["single buffer"]) and not any("_pipe_" in n for n in names["single buffer"])
        assert any(n.startswith("conv_halo_pipe_kernel<") and ", 32, " in n for n in names["32-column tile"]), names["32-column tile"]
    for tag in ("default", "row gather"):
        if tag in runs:
            assert la.conv_check(runs[tag][NAN]["out"], x, w, B, H, W, bias=b, rowadd=ra, res=rs, stride=stride, ups=ups, out_hw=out_hw) <= 1.0
    iso.check_batch_isolated(launch, B, operands, ("out",), scratch=sc, what=f"conv3x3 {mode} {H}x{W} batch")


@pytest.mark.parametrize("seg", [2, 1])
def test_conv3x3_split_k_with_a_stale_workspace(seg):
    B, H, W, Cin, Cout = 2, 8, 8, 1280, 1280
    HW, M, K = H * W, B * H * W, 9 * Cin
    parts = ops.canonical_splits(2, HW, Cout, K, W << 1, 0)
    assert parts > 1
    x, w = to_nhwc(rnd(B, Cin, H, W, seed=1)), pack3x3(rnd(Cout, Cin, 3, 3, seed=2, scale=K ** -0.5))
    b, ra, rs = rnd(Cout, seed=3), rnd(B, Cout, seed=4), rnd(M, Cout, seed=5)
    operands = dict(x=Op(x, image_w=W, images=B), w=w, bias=b, rowadd=Op(ra, images=B), res=Op(rs, image_w=W, images=B),
                    out=out16(M, Cout, image_w=W, images=B))
    sc = dict(ws=(parts * M * Cout + 4096, F32), stats=(ops.stats_floats(M, Cout, HW), F32))

    def launch(v):
        ops.set_workspace(v["ws"])
        ops.set_seg_mode(seg)
        st = ops.Stats(v["stats"])
        ops.conv3x3(v["x"], v["w"], v["out"], B, H, W, Cin, Cout, bias=v["bias"], rowadd=v["rowadd"], res=v["res"], stats=st)
        assert st.P > 0
        return dict(partials=v["stats"][:B * st.P * Cout * 2].view(B * st.P, Cout * 2))

    runs = iso.check_isolated(launch, operands, ("out",), scratch=sc, what=f"conv3x3 split-K seg {seg}")
    assert la.conv_check(runs[NAN]["out"], x, w, B, H, W, bias=b, rowadd=ra, res=rs) <= 1.0
    iso.check_batch_isolated(launch, B, operands, ("out",), scratch=sc, what=f"conv3x3 split-K seg {seg} batch")


@pytest.mark.parametrize("H,W", SIDES)
@pytest.mark.parametrize("concat,tables", [(True, True), (False, True), (True, False)])
def test_conv3x3_gn(H, W, concat, tables):
    """the channel concat [x | x2] and the GroupNorm-apply (+SiLU) prologue from per-image tables"""
    B, C1, C2, Cout = 3, 64, (64 if concat else 0), 64
    C, HW, M = C1 + C2, H * W, B * H * W
    x, x2 = to_nhwc(rnd(B, C1, H, W, seed=1)), to_nhwc(rnd(B, C2, H, W, seed=3)) if concat else None
    w = pack3x3(rnd(Cout, C, 3, 3, seed=2, scale=(9 * C) ** -0.5))
    sc_t = (1 + 0.1 * rnd(B, C, seed=8, dtype=F32)) if tables else None
    sh_t = 0.1 * rnd(B, C, seed=9, dtype=F32) if tables else None
    b, ra, rs = rnd(Cout, seed=11), rnd(B, Cout, seed=12), rnd(M, Cout, seed=13)
    img = lambda t, **kw: None if t is None else Op(t, images=B, **kw)
    operands = dict(x=img(x, image_w=W), x2=img(x2, image_w=W), w=w, sc=img(sc_t), sh=img(sh_t), bias=b, rowadd=img(ra),
                    res=img(rs, image_w=W), out=out16(M, Cout, image_w=W, images=B))
    scr = dict(stats=(ops.stats_floats(M, Cout, HW), F32))

    def launch(v, stats=True):
        st = ops.Stats(v["stats"]) if stats else None
        ops.conv3x3_gn(v["x"], v["w"], v["out"], B, H, W, C1, Cout, x2=v["x2"], C2=C2, gn_scale=v["sc"], gn_shift=v["sh"], silu=True,
                       bias=v["bias"], rowadd=v["rowadd"], res=v["res"], stats=st)
        if stats and st.P > 0:
            return dict(partials=v["stats"][:B * st.P * Cout * 2].view(B * st.P, Cout * 2))

    aux = (W << 1) | (1 if tables else 0)
    sp = ops.canonical_splits(2, HW, Cout, 9 * C, aux, 0)
    runs = {}
    for tag, setup in _conv_forms(2, M, Cout, 9 * C, aux, sp, W):
        if tag == "row gather":
            continue
        what = f"conv3x3_gn {H}x{W} {tag}"

        def one():
            on = iso.check_isolated(launch, operands, ("out",), scratch=scr, what=what)
            off = iso.check_isolated(lambda v: launch(v, False), operands, ("out",), scratch=scr, what=what + ", statistics off")
            assert la.same_bits(off[ZERO]["out"], on[ZERO]["out"]), f"{what}: the output depends on whether statistics are asked for"
            return on
        runs[tag] = _with_form(setup, one)
    _same_everywhere(runs, f"conv3x3_gn {H}x{W}")
    assert la.conv_check(runs["default"][NAN]["out"], x, w, B, H, W, C1=C1, x2=x2, gn_scale=sc_t, gn_shift=sh_t, silu=True, bias=b,
                         rowadd=ra, res=rs) <= 1.0
    iso.check_batch_isolated(launch, B, operands, ("out",), scratch=scr, what=f"conv3x3_gn {H}x{W} batch")


@pytest.mark.parametrize("H,W", [(2, 2), (5, 7), (9, 13), (16, 16), (17, 33)])
def test_conv3x3_down(H, W):
    B, Cin, Cout = 3, 64, 128
    Ho, Wo = (H - 2) // 2 + 1, (W - 2) // 2 + 1
    M = B * Ho * Wo
    x, w, b = to_nhwc(rnd(B, Cin, H, W, seed=1)), pack3x3(rnd(Cout, Cin, 3, 3, seed=2, scale=(9 * Cin) ** -0.5)), rnd(Cout, seed=3)
    operands = dict(x=Op(x, image_w=W, images=B), w=w, bias=b, out=out16(M, Cout, image_w=Wo, images=B))
    sc = dict(stats=(ops.stats_floats(M, Cout, Ho * Wo), F32))

    def launch(v):
        st = ops.Stats(v["stats"])
        ops.conv3x3_down(v["x"], v["w"], v["out"], B, H, W, Cin, Cout, bias=v["bias"], stats=st)
        if st.P > 0:
            return dict(partials=v["stats"][:B * st.P * Cout * 2].view(B * st.P, Cout * 2))

    runs = iso.check_isolated(launch, operands, ("out",), scratch=sc, what=f"conv3x3_down {H}x{W}")
    import vae_encoder_reference as ver
    ref, bnd = ver.down_reference(x, w, b, B, H, W)
    assert la.worst_ratio(runs[NAN]["out"], ref.to(DEV), bnd.to(DEV)) <= 1.0
    iso.check_batch_isolated(launch, B, operands, ("out",), scratch=sc, what=f"conv3x3_down {H}x{W} batch")


@pytest.mark.parametrize("H,W", SIDES)
@pytest.mark.parametrize("Cin,Cout,mode,gn", [(64, 4, 0, False), (128, 3, 1, False), (128, 4, 0, True), (64, 3, 1, True)])
def test_conv3x3_smalln(H, W, Cin, Cout, mode, gn):
    B = 3
    M = B * H * W
    x, w, b = to_nhwc(rnd(B, Cin, H, W, seed=1)), pack3x3(rnd(Cout, Cin, 3, 3, seed=2, scale=(9 * Cin) ** -0.5)), rnd(Cout, seed=3, scale=0.1)
    sc_t = (1 + 0.1 * rnd(B, Cin, seed=8, dtype=F32)) if gn else None
    sh_t = 0.1 * rnd(B, Cin, seed=9, dtype=F32) if gn else None
    operands = dict(x=Op(x, image_w=W, images=B), w=w, bias=b, sc=Op(sc_t, images=B) if gn else None, sh=Op(sh_t, images=B) if gn else None,
                    of=outof(F32, M, Cout, image_w=W, images=B))
    outs = ("of",)
    if mode == 1:
        operands["o8"] = outof(U8, M, Cout, image_w=W, images=B)
        outs = ("of", "o8")

    def launch(v):
        if mode == 0:
            ops.conv3x3_smalln(v["x"], v["w"], v["of"], B, H, W, Cin, Cout, bias=v["bias"], mode=0, gn_scale=v["sc"], gn_shift=v["sh"])
        else:
            ops.conv3x3_smalln(v["x"], v["w"], v["o8"], B, H, W, Cin, Cout, bias=v["bias"], mode=1, out_f32=v["of"], gn_scale=v["sc"],
                               gn_shift=v["sh"])

    runs = iso.check_isolated(launch, operands, outs, what=f"conv3x3_smalln {H}x{W} mode {mode}")
    assert la.conv_check(runs[NAN]["of"], x, w, B, H, W, gn_scale=sc_t, gn_shift=sh_t, silu=True, bias=b, out_fp16=False) <= 1.0
    if mode == 1:                                                     # the u8 picture is the rounding of the launch's own fp32 output
        assert la.rgb8_check(runs[NAN]["o8"], runs[NAN]["of"])[0] == 0
    iso.check_batch_isolated(launch, B, operands, outs, what=f"conv3x3_smalln {H}x{W} batch")


@pytest.mark.parametrize("H,W", SIDES)
@pytest.mark.parametrize("form", ["plain", "pre", "res"])
def test_conv3x3_c4(H, W, form):
    B, Cout = 3, 64
    M = B * H * W
    lat = rnd(B, 4, H, W, seed=1, dtype=F32)
    w, b = pack3x3(rnd(Cout, 4, 3, 3, seed=2, scale=1 / 6)), rnd(Cout, seed=3)
    pw, pb = rnd(4, 4, seed=4, scale=0.5, dtype=F32), rnd(4, seed=5, scale=0.1, dtype=F32)
    rs = rnd(M, Cout, seed=6)
    operands = dict(lat=Op(lat, images=B), w=w, bias=b, pw=pw, pb=pb, res=Op(rs, image_w=W, images=B) if form == "res" else None,
                    out=out16(M, Cout, image_w=W, images=B))

    def launch(v):
        if form == "res":
            ops.conv3x3_c4_res(v["lat"], v["w"], v["out"], B, H, W, Cout, bias=v["bias"], res=v["res"])
        else:
            pre = form == "pre"
            ops.conv3x3_c4(v["lat"], v["w"], v["out"], B, H, W, Cout, bias=v["bias"], pre_w=v["pw"] if pre else None,
                           pre_b=v["pb"] if pre else None, in_scale=1 / 0.18215 if pre else 1.0)

    runs = iso.check_isolated(launch, operands, ("out",), what=f"conv3x3_c4 {form} {H}x{W}")
    got = runs[NAN]["out"]
    if form == "res":
        assert la.conv_c4_res_check(got, lat, w, b, rs, B, H, W) <= 1.0
    else:
        z, ez = la.c4_input(lat, pw if form == "pre" else None, pb if form == "pre" else None, 1 / 0.18215 if form == "pre" else 1.0)
        assert la.hint_layer_check(got, z, ez, w, b, B, H, W, 1, False, la.C4_RES_K) <= 1.0
    iso.check_batch_isolated(launch, B, operands, ("out",), what=f"conv3x3_c4 {form} {H}x{W} batch")


@pytest.mark.parametrize("H,W", SIDES)
@pytest.mark.parametrize("entry", ["hint_conv_u8", "vae_enc_conv_in_u8"])
def test_u8_picture_convs(H, W, entry):
    B, Cout = 3, 16 if entry == "hint_conv_u8" else 128
    img = ru8(B, H, W, 3, seed=H + W)
    w, b = pack3x3(rnd(Cout, 3, 3, 3, seed=2, scale=0.2)), rnd(Cout, seed=3)
    operands = dict(img=Op(img, images=B), w=w, bias=b, out=out16(B * H * W, Cout, image_w=W, images=B))

    def launch(v):
        if entry == "hint_conv_u8":
            ops.hint_conv_u8(v["img"], v["w"], v["out"], B, H, W, Cout, bias=v["bias"], silu=True)
        else:
            ops.vae_enc_conv_in_u8(v["img"], v["w"], v["out"], B, H, W, Cout, bias=v["bias"])

    runs = iso.check_isolated(launch, operands, ("out",), what=f"{entry} {H}x{W}")
    if entry == "hint_conv_u8":
        xin, xerr = la.hint_u8_input(img)
        assert la.hint_layer_check(runs[NAN]["out"], xin, xerr, w, b, B, H, W, 1, True, la.HINT_U8_K) <= 1.0
    else:
        import vae_encoder_reference as ver
        assert ver.conv_in_check(runs[NAN]["out"], img, w, b, B, H, W) <= 1.0
    iso.check_batch_isolated(launch, B, operands, ("out",), what=f"{entry} {H}x{W} batch")


@pytest.mark.parametrize("H,W", SIDES)
@pytest.mark.parametrize("Cin,Cout,stride", [(16, 32, 1), (32, 96, 2), (96, 256, 2), (96, 96, 1)])
def test_hint_conv(H, W, Cin, Cout, stride):
    B = 3
    Ho, Wo = ((H + 1) // 2, (W + 1) // 2) if stride == 2 else (H, W)
    x, w, b = to_nhwc(rnd(B, Cin, H, W, seed=1)), pack3x3(rnd(Cout, Cin, 3, 3, seed=2, scale=(9 * Cin) ** -0.5)), rnd(Cout, seed=3)
    operands = dict(x=Op(x, image_w=W, images=B), w=w, bias=b, out=out16(B * Ho * Wo, Cout, image_w=Wo, images=B))
    launch = lambda v: ops.hint_conv(v["x"], v["w"], v["out"], B, H, W, Cin, Cout, bias=v["bias"], stride=stride, silu=True)
    runs = iso.check_isolated(launch, operands, ("out",), what=f"hint_conv {H}x{W}")
    assert la.hint_layer_check(runs[NAN]["out"], x.double().view(B, H, W, Cin), None, w, b, B, H, W, stride, True, 9 * Cin) <= 1.0
    iso.check_batch_isolated(launch, B, operands, ("out",), what=f"hint_conv {H}x{W} batch")


# ==== attention ============================================================================================================
ATTENTION = [  # (kernel form, d, Sq, Sk, causal)
    ("attn<40>", 40, 33, 63, False), ("attn<64>", 64, 150, 77, False), ("attn<80>", 80, 33, 1, False), ("attn<40> 1 key", 40, 150, 1, False),
    ("attn<160>", 160, 33, 77, False), ("attn<160> long", 160, 150, 330, False), ("attn<160> 63", 160, 330, 63, False),
    ("causal<64>", 64, 150, 150, True), ("causal<40> 77", 40, 77, 77, True),
    ("attn2<40> one group", 40, 150, 330, False), ("attn2<64> one group", 64, 330, 330, False), ("attn2<80> one group", 80, 33, 330, False),
    ("attn2<40> two groups", 40, 33, 1030, False), ("attn2<80> two groups", 80, 1030, 1030, False), ("attn2<64> two groups", 64, 150, 1030, False),
    ("attn_wide<512,32>", 512, 33, 77, False), ("attn_wide<512,32> 63", 512, 150, 63, False), ("attn_wide<512,32> long", 512, 33, 330, False),
]


@pytest.mark.parametrize("prescaled", [False, True])
@pytest.mark.parametrize("form,d,Sq,Sk,causal", ATTENTION, ids=[a[0] for a in ATTENTION])
def test_attention(form, d, Sq, Sk, causal, prescaled):
    """B = 2, two heads, ld = heads * d + 64: guard columns follow the last head, guard rows the last key.  The forms are those
    of tests/attention_cases.py (asserted against the dispatch as launch_audit states it)."""
    B, heads = 2, 2
    kernel = la.attention_kernel(d, Sk, causal)
    assert kernel == ("attn2" if form.startswith("attn2") else "wide" if "wide" in form else "attn")
    if "groups" in form:
        assert la.attention_key_split(d, Sk, causal) == ("two" in form)
    C = heads * d
    q, k, v_ = rnd(B * Sq, C, seed=1), rnd(B * Sk, C, seed=2), rnd(B * Sk, C, seed=3)
    scale = d ** -0.5
    if prescaled:
        q = (q.float() * (scale * 1.4426950408889634)).half()
    operands = dict(q=Op(q, cols=GC, images=B), k=Op(k, cols=GC, images=B), v=Op(v_, cols=GC, images=B), out=out16(B * Sq, C, cols=GC, images=B))

    def launch(v):
        ld = C + GC
        assert v["k"].stride(0) == ld
        ops.attention(v["q"], v["k"], v["v"], v["out"], B, heads, Sq, Sk, d, ldq=ld, ldk=ld, ldv=ld, ldo=ld,
                      scale=0.0 if prescaled else None, causal=causal)

    runs = iso.check_isolated(launch, operands, ("out",), what=f"attention {form}")
    assert la.attention_check(runs[NAN]["out"], q, k, v_, B, heads, Sq, Sk, d, scale=0.0 if prescaled else scale, causal=causal) <= 1.0
    iso.check_batch_isolated(launch, B, operands, ("out",), what=f"attention {form} batch")


# ==== norms and rows =======================================================================================================
def _gn_operands(B, HW, C1, C2, seed=1):
    x = (rnd(B * HW, C1, seed=seed).float() * 1.5 + 0.3).half()
    x2 = (rnd(B * HW, C2, seed=seed + 1).float() * 0.7 - 0.5).half() if C2 else None
    C = C1 + C2
    return x, x2, (1 + 0.1 * rnd(C, seed=3).float()).half(), rnd(C, seed=4, scale=0.1)


@pytest.mark.parametrize("HW", [1, 35, 221])
@pytest.mark.parametrize("C2", [0, 64])
def test_groupnorm(HW, C2):
    B, C1 = 3, 64
    C = C1 + C2
    x, x2, gamma, beta = _gn_operands(B, HW, C1, C2)
    operands = dict(x=Op(x, images=B), x2=Op(x2, images=B) if C2 else None, gamma=gamma, beta=beta, out=out16(B * HW, C, images=B))
    sc = dict(ws=(ops.groupnorm_ws_bytes(B, HW, C) // 4 + 16, F32))
    launch = lambda v: ops.groupnorm(v["x"], v["gamma"], v["beta"], v["out"], B, HW, C1, v["ws"], x2=v["x2"], C2=C2, silu=True)
    runs = iso.check_isolated(launch, operands, ("out",), scratch=sc, what=f"groupnorm HW={HW} C2={C2}")
    worst, _ = la.gn_check(None, None, [x] + ([x2] if C2 else []), B, HW, 32, gamma, beta, 1e-5, out=runs[NAN]["out"], silu=True)
    assert worst <= 1.0
    iso.check_batch_isolated(launch, B, operands, ("out",), scratch=sc, what=f"groupnorm HW={HW} batch")


@pytest.mark.parametrize("HW", [1, 35, 221])
@pytest.mark.parametrize("C2", [0, 64])
def test_groupnorm_affine(HW, C2):
    B, C1 = 3, 64
    C = C1 + C2
    x, x2, gamma, beta = _gn_operands(B, HW, C1, C2)
    operands = dict(x=Op(x, images=B), x2=Op(x2, images=B) if C2 else None, gamma=gamma, beta=beta,
                    scale=outof(F32, B, C, images=B), shift=outof(F32, B, C, images=B))
    sc = dict(ws=(ops.groupnorm_ws_bytes(B, HW, C) // 4 + 16, F32))
    launch = lambda v: ops.groupnorm_affine(v["x"], v["gamma"], v["beta"], v["scale"], v["shift"], B, HW, C1, v["ws"], x2=v["x2"], C2=C2)
    runs = iso.check_isolated(launch, operands, ("scale", "shift"), scratch=sc, what=f"groupnorm_affine HW={HW} C2={C2}")
    worst, _ = la.gn_check(runs[NAN]["scale"], runs[NAN]["shift"], [x] + ([x2] if C2 else []), B, HW, 32, gamma, beta, 1e-5)
    assert worst <= 1.0
    iso.check_batch_isolated(launch, B, operands, ("scale", "shift"), scratch=sc, what=f"groupnorm_affine HW={HW} batch")


@pytest.mark.parametrize("H,W", [(1, 1), (5, 7), (13, 17), (16, 16)])
@pytest.mark.parametrize("C2", [0, 64])
@pytest.mark.parametrize("entry", ["groupnorm_from_stats one launch", "groupnorm_from_stats two launches", "groupnorm_tables_from_stats"])
def test_groupnorm_from_producer_statistics(H, W, C2, entry):
    """The statistics come from guarded convolutions into stale statistics buffers (the model creates its own once and never
    clears them); GroupNorm reads exactly the P slabs the producer reported."""
    B, C1, Cin = 3, 64, 64
    HW, M, C = H * W, B * H * W, C1 + C2
    x0 = to_nhwc(rnd(B, Cin, H, W, seed=1))
    w1, w2 = (pack3x3(rnd(c, Cin, 3, 3, seed=s, scale=(9 * Cin) ** -0.5)) for c, s in ((C1, 2), (64, 3)))
    _, _, gamma, beta = _gn_operands(B, HW, C1, C2)
    tables = entry == "groupnorm_tables_from_stats"
    operands = dict(x0=Op(x0, image_w=W, images=B), w1=w1, w2=w2, gamma=gamma, beta=beta, x=out16(M, C1, image_w=W, images=B),
                    x2=out16(M, 64, image_w=W, images=B) if C2 else None, out=None if tables else out16(M, C, images=B))
    sc = dict(st1=(ops.stats_floats(M, C1, HW), F32), st2=(ops.stats_floats(M, 64, HW), F32),
              ws=(max(ops.groupnorm_ws_bytes(B, HW, C) // 4, 2 * B * C) + 16, F32))

    def launch(v):
        ops.set_gn_fused_bytes(0 if "two" in entry else 1 << 40)
        st1, st2 = ops.Stats(v["st1"]), ops.Stats(v["st2"])
        ops.conv3x3(v["x0"], v["w1"], v["x"], B, H, W, Cin, C1, stats=st1)
        if C2:
            ops.conv3x3(v["x0"], v["w2"], v["x2"], B, H, W, Cin, 64, stats=st2)
        assert st1.P > 0 and (not C2 or st2.P > 0)
        kw = dict(C2=C2, st2=st2 if C2 else None)
        if tables:
            s, t = ops.groupnorm_tables_from_stats(v["gamma"], v["beta"], B, HW, C1, st1, v["ws"], **kw)
            return dict(scale=s, shift=t)
        ops.groupnorm_from_stats(v["x"], v["gamma"], v["beta"], v["out"], B, HW, C1, st1, v["ws"], x2=v["x2"], **kw)

    outs = ("x",) + (("x2",) if C2 else ()) + (() if tables else ("out",))
    runs = iso.check_isolated(launch, operands, outs, scratch=sc, what=f"{entry} {H}x{W} C2={C2}")
    got = runs[NAN]
    xs = [got["x"]] + ([got["x2"]] if C2 else [])
    worst, _ = la.gn_check(got.get("scale"), got.get("shift"), xs, B, HW, 32, gamma, beta, 1e-5, out=got.get("out"), silu=True)
    assert worst <= 1.0
    iso.check_batch_isolated(launch, B, operands, outs, scratch=sc, what=f"{entry} {H}x{W} batch")


@pytest.mark.parametrize("M", [1, 5, 77])
@pytest.mark.parametrize("C", [320, 1280])
def test_layernorm(M, C):
    x = (rnd(M, C, seed=1).float() * 3 + 1).half()
    g, b = (1 + 0.1 * rnd(C, seed=2).float()).half(), rnd(C, seed=3, scale=0.1)
    operands = dict(x=x, g=g, b=b, out=out16(M, C))
    runs = iso.check_isolated(lambda v: ops.layernorm(v["x"], v["g"], v["b"], v["out"], M, C), operands, ("out",), what="layernorm")
    ref, bnd = la.layernorm_reference(x, g, b, 1e-5)
    assert la.worst_ratio(runs[NAN]["out"], ref, bnd) <= 1.0


@pytest.mark.parametrize("rows,n,ld", [(37, 100, 128), (9, 7, 64)])
def test_softmax_rows(rows, n, ld):
    """in place on rows of ld columns of which n count: the padding columns arrive as +inf (a maximum or a sum that included one
    would not be finite) and leave as zeros -- the whole pitch belongs to the operand, so the guards are in front and behind."""
    x = rnd(rows, ld, seed=1, scale=3.0)
    x[:, n:] = float("inf")
    operands = dict(x=Op(x))

    def launch(v):
        ops.softmax_rows(v["x"], rows, n, ld)

    runs = iso.check_isolated(launch, operands, ("x",), what="softmax_rows")
    got = runs[NAN]["x"]
    assert not got[:, n:].any()
    ref, bnd = la.softmax_reference(x, n)
    assert la.worst_ratio(got[:, :n], ref, bnd) <= 1.0


def test_transpose():
    Z, R, Cc = 2, 100, 72
    x = rnd(Z * R, Cc, seed=2)
    operands = dict(x=Op(x, cols=GC), out=out16(Z * Cc, R, cols=GC))

    def launch(v):
        X, O = v["x"], v["out"]
        ops.transpose(X, O, R, Cc, ldi=X.stride(0), ldo=O.stride(0), batch=Z, stride_in=R * X.stride(0), stride_out=Cc * O.stride(0))

    runs = iso.check_isolated(launch, operands, ("out",), what="transpose")
    assert torch.equal(runs[NAN]["out"].view(Z, Cc, R), x.view(Z, R, Cc).transpose(1, 2))


def test_embed_tokens_and_prompt_emphasis():
    B, S, D, vocab = 3, 77, 64, 50
    ids = torch.from_numpy(np.random.default_rng(1).integers(-3, vocab + 3, (B, S))).to(torch.int32).to(DEV)    # out-of-range ids are clamped
    tok, pos = rnd(vocab, D, seed=1), rnd(S, D, seed=2)
    operands = dict(ids=Op(ids.view(-1), images=B), tok=tok, pos=pos, out=out16(B * S, D, images=B))
    launch = lambda v: ops.embed_tokens(v["ids"], v["tok"], v["pos"], v["out"], B, S, D)
    runs = iso.check_isolated(launch, operands, ("out",), what="embed_tokens")
    assert la.same_bits(runs[NAN]["out"], la.embed_reference(ids, tok, pos, B, S))
    iso.check_batch_isolated(launch, B, operands, ("out",), what="embed_tokens batch")
    import prompt_reference as pr
    D = 768
    z, w = (rnd(B * S, D, seed=3).float() + 0.5).half(), (1 + 0.3 * rnd(B * S, seed=4, dtype=F32)).abs()
    operands = dict(z=Op(z, images=B), w=Op(w, images=B), out=out16(B * S, D, cols=GC, images=B))
    launch = lambda v: ops.prompt_emphasis(v["z"], v["w"], v["out"], B, S, D)
    runs = iso.check_isolated(launch, operands, ("out",), what="prompt_emphasis")
    zn, wn = z.cpu().numpy().reshape(B, S, D), w.cpu().numpy().reshape(B, S)
    assert pr.conditioning(zn, wn) >= 0.1                             # what emphasis_bound assumes of the chunk means
    err = np.abs(runs[NAN]["out"].cpu().numpy().reshape(B, S, D).astype(np.float64) - pr.emphasis_fp64(zn, wn))
    assert (err <= pr.emphasis_bound(zn, wn)).all()
    iso.check_batch_isolated(launch, B, operands, ("out",), what="prompt_emphasis chunks")


def test_timestep_embeddings():
    B, dim = 3, 320
    operands = dict(out=out16(B, dim))
    runs = iso.check_isolated(lambda v: ops.timestep_embedding(759.0, v["out"], B, dim), operands, ("out",), what="timestep_embedding")
    ref, bnd = la.timestep_reference([759.0], B, dim)
    assert la.worst_ratio(runs[NAN]["out"], ref.to(DEV), bnd.to(DEV)) <= 1.0
    ts = [999.0, 759.0, 19.0]
    operands = dict(out=out16(len(ts) * B, dim))
    runs = iso.check_isolated(lambda v: ops.timestep_embedding_steps(ts, v["out"], B, dim), operands, ("out",), what="timestep_embedding_steps")
    ref, bnd = la.timestep_reference(ts, B, dim)
    assert la.worst_ratio(runs[NAN]["out"], ref.to(DEV), bnd.to(DEV)) <= 1.0


# ==== latent and image glue ================================================================================================
LATENTS = [(13, 9), (1, 1)]


def r32(*shape, seed=0, scale=1.0):
    return rnd(*shape, seed=seed, scale=scale, dtype=F32)


def _lcm_coefficients(last):
    from sdlcm_amd.scheduler import LCMSchedule
    s = LCMSchedule()
    ts = s.timesteps(2, 0.5)
    coef, is_last = s.step_coefficients(ts, 1 if last else 0)
    assert bool(is_last) == bool(last)
    return coef, s.renoise_coefficients(ts[1])


def _state(B, h, w, dup, seed=3):
    """the latents a step works on: with dup the second half of [2B, 4, h, w]; the front half is written too, so it counts as output"""
    x = r32(B, 4, h, w, seed=seed, scale=2.0)
    return x, (torch.cat([torch.full_like(x, 7.0), x]) if dup else x)


@pytest.mark.parametrize("h,w", LATENTS)
@pytest.mark.parametrize("pred", ["epsilon", "v_prediction", "sample"])
@pytest.mark.parametrize("guided", [False, True])
def test_scheduler_step(h, w, pred, guided):
    B = 3
    coef, _ = _lcm_coefficients(False)
    m, mu, x, n = r32(B, h, w, 4, seed=1, scale=1.3), r32(B, h, w, 4, seed=2, scale=1.1), r32(B, 4, h, w, seed=3, scale=2.0), r32(B, 4, h, w, seed=4)
    operands = dict(m=Op(m, images=B), mu=Op(mu, images=B) if guided else None, lat=Op(x, images=B), noise=Op(n, images=B))
    kw = dict(guidance=7.5) if guided else {}
    launch = lambda v: ops.scheduler_step(v["m"], v["lat"], v["noise"], coef, 0, B, h, w, eps_uncond=v["mu"], pred=pred, **kw)
    runs = iso.check_isolated(launch, operands, ("lat",), what="scheduler_step")
    ref, bnd = la.sampler_step_reference(m, x, n, coef, False, m_u=mu if guided else None, guidance=7.5 if guided else 1.0, pred=pred)
    assert la.worst_ratio(runs[NAN]["lat"], ref, bnd) <= 1.0
    iso.check_batch_isolated(launch, B, operands, ("lat",), what="scheduler_step batch")


@pytest.mark.parametrize("h,w", LATENTS)
@pytest.mark.parametrize("dup,guided", [(False, False), (True, True), (False, True)])
def test_scheduler_step_handover(h, w, dup, guided):
    """dup: the state is [2B, 4, h, w], image j at rows j and B + j (Op(copies=2)); guided: the unconditional model output is a
    per-image operand of its own"""
    B = 3
    coef, (nsa, nsb) = _lcm_coefficients(True)
    m, mu, n = r32(B, h, w, 4, seed=1, scale=1.3), r32(B, h, w, 4, seed=2, scale=1.1), r32(B, 4, h, w, seed=4)
    x, state = _state(B, h, w, dup)
    kw = dict(guidance=7.5) if guided else {}
    operands = dict(m=Op(m, images=B), mu=Op(mu, images=B) if guided else None, state=Op(state, images=B, copies=2 if dup else 1),
                    noise=Op(n, images=B), xk=outof(F32, B, 4, h, w, images=B))
    launch = lambda v: ops.scheduler_step_handover(v["m"], v["state"][B:] if dup else v["state"], v["noise"], v["xk"], coef, nsa, nsb,
                                                   B, h, w, eps_uncond=v["mu"], dup=dup, **kw)
    runs = iso.check_isolated(launch, operands, ("state", "xk"), what="scheduler_step_handover")
    got = runs[NAN]
    assert la.handover_check(got["xk"], got["state"][B:] if dup else got["state"], got["state"][:B] if dup else None, m, x, n, coef, nsa, nsb, B,
                             m_u=mu if guided else None, guidance=7.5 if guided else 1.0) <= 1.0
    iso.check_batch_isolated(launch, B, operands, ("state", "xk"), what="scheduler_step_handover batch")


SAMPLER_ROWS = {  # (sa, sb, cx, c0, c1, cn): a first DPM++ 2M / Euler / DDIM step, one with history, an ancestral one, a last one
    "first": (0.068264848, 0.99766723, 0.78848246, 0.56358234, 0.0, 0.0),
    "history": (0.61740797, 0.78664312, 0.03706272, 1.73268458, -0.75599250, 0.0),
    "ancestral": (0.068264848, 0.99766723, 0.06873991, 0.61271545, 0.0, 0.78364803),
    "last": (0.99957490, 0.029155134, 0.0, 1.0, 0.0, 0.0),
}


@pytest.mark.parametrize("h,w", LATENTS)
@pytest.mark.parametrize("row", list(SAMPLER_ROWS))
@pytest.mark.parametrize("pred,dup", [("epsilon", False), ("v_prediction", True), ("sample", False)])
def test_sampler_step(h, w, row, pred, dup):
    import sampler_reference as sref
    B = 3
    c = tuple(float(np.float32(v)) for v in SAMPLER_ROWS[row])
    guided, g = dup, float(np.float32(2.5))                           # the guided form goes with the doubled state, as in a pass
    m, mu = r32(B, h, w, 4, seed=1, scale=1.3), r32(B, h, w, 4, seed=2, scale=1.1)
    x0p, n = r32(B, 4, h, w, seed=5, scale=0.9), r32(B, 4, h, w, seed=4)
    x, state = _state(B, h, w, dup)
    kw = dict(guidance=g) if guided else {}
    operands = dict(m=Op(m, images=B), mu=Op(mu, images=B) if guided else None, state=Op(state, images=B, copies=2 if dup else 1),
                    x0p=Op(x0p, images=B), noise=Op(n, images=B) if c[5] else None)
    launch = lambda v: ops.sampler_step(v["m"], v["state"][B:] if dup else v["state"], v["x0p"], v["noise"], *c, B, h, w,
                                        eps_uncond=v["mu"], pred=pred, dup=dup, **kw)
    runs = iso.check_isolated(launch, operands, ("state", "x0p"), what=f"sampler_step {row}")
    got = runs[NAN]
    # fp64 from the fp32 operands.  Unguided: at most six fp32 roundings, each of a value no larger than the sum of the terms'
    # magnitudes (8 U).  Guidance adds d = m - mu and fma(g, d, mu): two more, on magnitudes within |mu| + |g| |d| (12 U).
    sa, sb, cx, c0, c1, cn = c
    X, M, P, N = x.double(), m.double().permute(0, 3, 1, 2), x0p.double(), n.double()
    Mmag = M.abs()
    if guided:
        Mu = mu.double().permute(0, 3, 1, 2)
        Mmag = Mu.abs() + g * (M - Mu).abs()
        M = Mu + g * (M - Mu)
    ref, x0 = sref.step(X, M, P, N, c, pred)
    mag0 = {"epsilon": (X.abs() + sb * Mmag) / sa, "v_prediction": sa * X.abs() + sb * Mmag, "sample": Mmag}[pred]
    mag = abs(cx) * X.abs() + abs(c0) * mag0 + abs(c1) * P.abs() + abs(cn) * N.abs()
    k = 12 if guided else 8
    assert la.worst_ratio(got["state"][B:] if dup else got["state"], ref, k * la.U * mag + 1e-38) <= 1.0
    assert la.worst_ratio(got["x0p"], x0, (k - 4) * la.U * mag0 + 1e-38) <= 1.0
    if dup:
        assert la.same_bits(got["state"][:B], got["state"][B:])
    iso.check_batch_isolated(launch, B, operands, ("state", "x0p"), what=f"sampler_step {row} batch")


@pytest.mark.parametrize("h,w", LATENTS)
@pytest.mark.parametrize("last,dup", [(0, False), (1, False), (0, True)])
def test_scheduler_step_inpaint(h, w, last, dup):
    B = 3
    coef, (ksa, ksb) = _lcm_coefficients(last)
    guided = dup
    m, n, z, e1 = r32(B, h, w, 4, seed=1, scale=1.3), r32(B, 4, h, w, seed=4), r32(B, 4, h, w, seed=6), r32(B, 4, h, w, seed=7)
    mu = r32(B, h, w, 4, seed=2, scale=1.1)
    kw = dict(guidance=7.5) if guided else {}
    mask = (torch.rand(B, h, w, generator=torch.Generator().manual_seed(8)) < 0.5).to(U8).to(DEV)
    x, state = _state(B, h, w, dup)
    operands = dict(m=Op(m, images=B), mu=Op(mu, images=B) if guided else None, state=Op(state, images=B, copies=2 if dup else 1),
                    noise=None if last else Op(n, images=B), z=Op(z, images=B), e1=None if last else Op(e1, images=B), mask=Op(mask, images=B))
    launch = lambda v: ops.scheduler_step_inpaint(v["m"], v["state"][B:] if dup else v["state"], v["noise"], v["z"], v["e1"], v["mask"], coef,
                                                  last, ksa, ksb, B, h, w, eps_uncond=v["mu"], dup=dup, **kw)
    runs = iso.check_isolated(launch, operands, ("state",), what="scheduler_step_inpaint")
    got = runs[NAN]["state"]
    stepped, bs = la.sampler_step_reference(m, x, n, coef, bool(last), m_u=mu if guided else None, guidance=7.5 if guided else 1.0)
    kept, bk = (z.double(), torch.full_like(z.double(), 1e-38)) if last else la.renoise_reference(z, e1, ksa, ksb)
    sel = mask.bool()[:, None].expand(B, 4, h, w)
    assert la.worst_ratio(got[B:] if dup else got, torch.where(sel, stepped, kept), torch.where(sel, bs, bk)) <= 1.0
    if dup:
        assert la.same_bits(got[:B], got[B:])
    iso.check_batch_isolated(launch, B, operands, ("state",), what="scheduler_step_inpaint batch")


@pytest.mark.parametrize("h,w", LATENTS)
@pytest.mark.parametrize("dup", [False, True])
def test_latents_renoise_and_upscale_renoise(h, w, dup):
    import hires_reference as hr
    B, sa, sb = 3, 0.5477, 0.8367
    x0, n = r32(B, 4, h, w, seed=1), r32(B, 4, h, w, seed=2)
    rows = 2 * B if dup else B
    operands = dict(x0=Op(x0, images=B), noise=Op(n, images=B), lat=outof(F32, rows, 4, h, w, images=B, copies=2 if dup else 1))
    launch = lambda v: ops.latents_renoise(v["x0"], v["noise"], sa, sb, v["lat"], B, h, w, dup=dup)
    runs = iso.check_isolated(launch, operands, ("lat",), what="latents_renoise")
    assert la.renoise_check(runs[NAN]["lat"], x0, n, sa, sb, B, dup) <= 1.0
    iso.check_batch_isolated(launch, B, operands, ("lat",), what="latents_renoise batch")
    H, W = 2 * h + 1, 2 * w - 1 if w > 1 else 3
    n2 = r32(B, 4, H, W, seed=3)
    for mode in (0, 1, 2):
        operands = dict(x0=Op(x0, images=B), noise=Op(n2, images=B), lat=outof(F32, rows, 4, H, W, images=B, copies=2 if dup else 1),
                        up=outof(F32, B, 4, H, W, images=B))
        launch = lambda v: ops.latents_upscale_renoise(v["x0"], h, w, v["noise"], sa, sb, mode, v["lat"], B, H, W, x_up=v["up"], dup=dup)
        runs = iso.check_isolated(launch, operands, ("lat", "up"), what=f"latents_upscale_renoise mode {mode}")
        up, ref = hr.upscale_renoise_fp64(x0.cpu().numpy(), n2.cpu().numpy(), sa, sb, H, W, mode)
        tol = hr.operator_tolerance(x0.cpu().numpy(), n2.cpu().numpy())
        got = runs[NAN]
        assert np.abs(got["lat"][:B].cpu().numpy() - ref).max() <= tol and np.abs(got["up"].cpu().numpy() - up).max() <= tol
        if dup:
            assert la.same_bits(got["lat"][:B], got["lat"][B:])
        iso.check_batch_isolated(launch, B, operands, ("lat", "up"), what=f"latents_upscale_renoise mode {mode} batch")


@pytest.mark.parametrize("h,w", [(9, 11), (1, 1)])
@pytest.mark.parametrize("dup", [False, True])
def test_vae_posterior_renoise(h, w, dup):
    import vae_encoder_reference as ver
    B, sa, sb = 3, 0.5477, 0.8367
    g = torch.Generator().manual_seed(31)
    pre_m, pre_l = torch.randn(B, h, w, 4, generator=g).to(DEV), (3.0 * torch.randn(B, h, w, 4, generator=g)).to(DEV)
    qw, qb = (torch.eye(8) + 0.1 * torch.randn(8, 8, generator=g)).contiguous().to(DEV), (0.02 * torch.randn(8, generator=g)).to(DEV)
    e0, e1 = r32(B, 4, h, w, seed=5), r32(B, 4, h, w, seed=6)
    rows = 2 * B if dup else B
    img = lambda t: Op(t, images=B)
    operands = dict(pm=img(pre_m), pl=img(pre_l), qw=qw, qb=qb, e0=img(e0), e1=img(e1), z=outof(F32, B, 4, h, w, images=B),
                    lat=outof(F32, rows, 4, h, w, images=B, copies=2 if dup else 1), mom=outof(F32, B, 8, h, w, images=B))
    launch = lambda v: ops.vae_posterior_renoise(v["pm"], v["pl"], v["qw"], v["qb"], v["e0"], v["e1"], 0.18215, sa, sb, v["z"], v["lat"],
                                                 B, h, w, moments=v["mom"], dup=dup)
    runs = iso.check_isolated(launch, operands, ("z", "lat", "mom"), what="vae_posterior_renoise")
    got = runs[NAN]
    ref = ver.posterior_reference(pre_m.cpu(), pre_l.cpu(), qw.cpu(), qb.cpu(), e0.cpu(), e1.cpu(), 0.18215, sa, sb)
    assert ver.posterior_check(got["z"], got["lat"], ref, B, dup, got_moments=got["mom"]) <= 1.0
    iso.check_batch_isolated(launch, B, operands, ("z", "lat", "mom"), what="vae_posterior_renoise batch")


@pytest.mark.parametrize("h,w", LATENTS)
def test_noise_variation(h, w):
    """every slot blended in place with a source of its own; 8e-5 max|low| is the ceiling tests/test_variation_gpu.py puts on its
    measured fp32-restatement bound"""
    import variation_reference as vr
    B, t = 3, 0.3
    lo, hi = r32(B, 4, h, w, seed=1), r32(B, 4, h, w, seed=2)
    operands = dict(lat=Op(lo, images=B), hi=Op(hi, images=B))
    launch = lambda v: ops.noise_variation(v["lat"], B, h, w, [(None, v["hi"][b], h, w, t) for b in range(B)])
    runs = iso.check_isolated(launch, operands, ("lat",), what="noise_variation")
    for b in range(B):
        ref = vr.blend_fp64(lo[b].cpu().numpy(), hi[b].cpu().numpy(), t)
        assert np.abs(runs[NAN]["lat"][b].cpu().numpy() - ref).max() <= 8e-5 * float(lo[b].abs().max())
    iso.check_batch_isolated(launch, B, operands, ("lat",), what="noise_variation batch")


@pytest.mark.parametrize("h,w", [(13, 9), (1, 1), (7, 23)])
def test_latents_pool8(h, w):
    B = 3
    lat = r32(B, 4, h, w, seed=1)
    operands = dict(lat=Op(lat, images=B), out=out16(B, 4, 8, 8, images=B))
    launch = lambda v: ops.latents_pool8(v["lat"], v["out"], B, h, w)
    runs = iso.check_isolated(launch, operands, ("out",), what="latents_pool8")
    ref, bnd = la.pool8_reference(lat)
    assert la.worst_ratio(runs[NAN]["out"], ref, bnd) <= 1.0
    iso.check_batch_isolated(launch, B, operands, ("out",), what="latents_pool8 batch")


@pytest.mark.parametrize("vertical", [True, False])
def test_vae_blend_and_place_tile(vertical):
    B, ah, aw, extent = 3, 13, 9, 5
    bh, bw = (11, aw) if vertical else (ah, 7)
    a, b = r32(B, ah, aw, 3, seed=1), r32(B, bh, bw, 3, seed=2)
    operands = dict(a=Op(a, images=B), b=Op(b, images=B))
    launch = lambda v: ops.vae_blend(v["a"], ah, aw, v["b"], bh, bw, B, extent, vertical)
    runs = iso.check_isolated(launch, operands, ("b",), what="vae_blend")
    ref, bnd, _ = la.blend_reference(a, b, extent, vertical)
    assert la.worst_ratio(runs[NAN]["b"], ref, bnd) <= 1.0
    iso.check_batch_isolated(launch, B, operands, ("b",), what="vae_blend batch")
    # the crop [0:ch, 0:cw] of the tile goes to (oy, ox) of a picture that already holds its other tiles
    H, W, oy, ox, ch, cw = 17, 13, 4, 3, 10, 8
    pic8, pic32 = ru8(B, H, W, 3, seed=3), r32(B, H, W, 3, seed=4)
    operands = dict(tile=Op(a, images=B), o8=Op(pic8, images=B), o32=Op(pic32, images=B))
    launch = lambda v: ops.vae_place_tile(v["tile"], ah, aw, v["o8"], v["o32"], H, W, B, oy, ox, ch, cw)
    runs = iso.check_isolated(launch, operands, ("o8", "o32"), what="vae_place_tile")
    got = runs[NAN]
    want32 = pic32.clone()
    want32[:, oy:oy + ch, ox:ox + cw] = a[:, :ch, :cw]
    assert la.same_bits(got["o32"], want32)
    assert la.rgb8_check(got["o8"][:, oy:oy + ch, ox:ox + cw], a[:, :ch, :cw])[0] == 0
    keep = torch.ones(B, H, W, 3, dtype=torch.bool, device=DEV)
    keep[:, oy:oy + ch, ox:ox + cw] = False
    assert torch.equal(got["o8"][keep], pic8[keep])
    iso.check_batch_isolated(launch, B, operands, ("o8", "o32"), what="vae_place_tile batch")


def test_grid_combine_rgb8():
    import sdupscale_reference as sr
    W, H, tw, th, ov = 77, 45, 32, 24, 7
    xs, ys = sr.geometry(W, H, tw, th, ov)
    tiles = sr.random_tiles(W, H, tw, th, ov, seed=1)
    operands = dict(tiles=Op(torch.from_numpy(tiles).to(DEV)), out=outof(U8, H, W, 3))
    launch = lambda v: ops.grid_combine_rgb8(v["tiles"], v["out"], (W, H, tw, th, ov, xs, ys))
    runs = iso.check_isolated(launch, operands, ("out",), what="grid_combine_rgb8")
    assert np.array_equal(runs[NAN]["out"].cpu().numpy(), sr.combine_int(tiles, W, H, ov, xs, ys).astype(np.uint8))


@pytest.mark.parametrize("H,W,sigma", [(16, 24, 0), (16, 24, 4), (8, 8, 12)])
def test_inpaint_mask_prepare_and_composite(H, W, sigma):
    import inpaint_reference as ir
    from sdlcm_amd.pipeline import mask_blur_weights
    B = 3
    m = np.random.default_rng(H + sigma).integers(0, 256, (B, H, W), dtype=np.uint8)
    r, wts = mask_blur_weights(sigma)
    wd = torch.from_numpy(wts.astype(np.int64)).to(torch.int32).to(DEV) if r > 0 else None
    operands = dict(mask=Op(torch.from_numpy(m).to(DEV), images=B), w=wd, alpha=outof(U8, B, H, W, images=B),
                    lm=outof(U8, B, H // 8, W // 8, images=B))
    sc = dict(tmp=(B * H * W, U8))
    launch = lambda v: ops.inpaint_mask_prepare(v["mask"], v["w"], r, v["alpha"], v["tmp"], v["lm"], B, H, W) and None
    runs = iso.check_isolated(launch, operands, ("alpha", "lm"), scratch=sc, what="inpaint_mask_prepare")
    want = ir.blur(m, sigma)
    assert np.array_equal(runs[NAN]["alpha"].cpu().numpy(), want) and np.array_equal(runs[NAN]["lm"].cpu().numpy(), ir.latent_mask(want))
    iso.check_batch_isolated(launch, B, operands, ("alpha", "lm"), scratch=sc, what="inpaint_mask_prepare batch")
    gen, init = ru8(B, H, W, 3, seed=1), ru8(B, H, W, 3, seed=2)
    operands = dict(rgb=Op(gen, images=B), init=Op(init, images=B), alpha=Op(torch.from_numpy(want).to(DEV), images=B))
    launch = lambda v: ops.inpaint_composite_rgb8(v["rgb"], v["init"], v["alpha"], B, H, W)
    runs = iso.check_isolated(launch, operands, ("rgb",), what="inpaint_composite_rgb8")
    assert np.array_equal(runs[NAN]["rgb"].cpu().numpy(), ir.composite(gen.cpu().numpy(), init.cpu().numpy(), want))
    iso.check_batch_isolated(launch, B, operands, ("rgb",), what="inpaint_composite_rgb8 batch")


@pytest.mark.parametrize("H,W", [(1, 1), (9, 13), (37, 70)])
def test_canny_and_invert(H, W):
    import canny_reference as cr
    B = 3
    imgs = np.stack([np.random.default_rng(s).integers(0, 256, (H, W, 3), dtype=np.uint8) for s in range(B)])
    imgs[:, :, W // 2:] //= 4                                         # an edge down the middle besides the noise
    d = torch.from_numpy(imgs).to(DEV)
    nws = ops.canny_ws_bytes(B, H, W)
    operands = dict(rgb=Op(d, images=B), out=outof(U8, B, H, W, 3, images=B))
    sc = dict(ws=(nws, U8))
    launch = lambda v: ops.canny_rgb8(v["rgb"], v["out"], v["ws"], B, H, W, 100.0, 200.0)
    runs = iso.check_isolated(launch, operands, ("out",), scratch=sc, what="canny_rgb8")
    assert np.array_equal(runs[NAN]["out"].cpu().numpy(), cr.canny(imgs, 100, 200))
    iso.check_batch_isolated(launch, B, operands, ("out",), scratch=sc, what="canny_rgb8 batch")
    lo, hi = cr.thresholds(100, 200)
    operands = dict(rgb=Op(d, images=B), cls=outof(U8, B, H, W, images=B))
    launch = lambda v: ops.canny_classes(v["rgb"], v["cls"], B, H, W, lo, hi)
    runs = iso.check_isolated(launch, operands, ("cls",), what="canny_classes")
    cls = np.stack([cr.classes(i, lo, hi) for i in imgs])
    assert np.array_equal(runs[NAN]["cls"].cpu().numpy(), cls)
    iso.check_batch_isolated(launch, B, operands, ("cls",), what="canny_classes batch")
    operands = dict(cls=Op(torch.from_numpy(cls).to(DEV), images=B), out=outof(U8, B, H, W, 3, images=B))
    launch = lambda v: ops.canny_link(v["cls"], v["out"], v["ws"], B, H, W)
    runs = iso.check_isolated(launch, operands, ("out",), scratch=sc, what="canny_link")
    assert np.array_equal(runs[NAN]["out"].cpu().numpy(), cr.link_rgb(cls))
    iso.check_batch_isolated(launch, B, operands, ("out",), scratch=sc, what="canny_link batch")
    operands = dict(x=Op(d, images=B), out=outof(U8, B, H, W, 3, images=B))
    runs = iso.check_isolated(lambda v: ops.invert_u8(v["x"], v["out"]), operands, ("out",), what="invert_u8")
    assert np.array_equal(runs[NAN]["out"].cpu().numpy(), 255 - imgs)
    iso.check_batch_isolated(lambda v: ops.invert_u8(v["x"], v["out"]), B, operands, ("out",), what="invert_u8 batch")


@pytest.mark.parametrize("sh,sw,oh,ow,window", [(37, 53, 64, 96, None), (37, 53, 16, 24, None), (40, 30, 64, 96, (16, 0, 64, 64)), (1, 1, 8, 8, None)])
def test_resize_lanczos_u8(sh, sw, oh, ow, window):
    """source rows 64 bytes apart from the next (guard columns), destination likewise; the workspace's tables are uploaded by the
    entry point itself, its intermediate starts as the pattern"""
    import resize_reference as rr
    src = np.random.default_rng(sh).integers(0, 256, (sh, sw, 3), dtype=np.uint8)
    x0, y0, w, h = window or (0, 0, ow, oh)
    operands = dict(src=Op(torch.from_numpy(src).to(DEV).view(sh, sw * 3), cols=GC), dst=outof(U8, h, w * 3, cols=GC))
    sc = dict(ws=(ops.resize_ws_bytes(sw, sh, 3, ow, oh, window), U8))

    def launch(v):
        s, d = v["src"], v["dst"]
        s3 = s.as_strided((sh, sw, 3), (s.stride(0), 3, 1), s.storage_offset())
        d3 = d.as_strided((h, w, 3), (d.stride(0), 3, 1), d.storage_offset())
        ops.resize_lanczos_u8(s3, d3, v["ws"], ow, oh, window)

    runs = iso.check_isolated(launch, operands, ("dst",), scratch=sc, what="resize_lanczos_u8")
    assert np.array_equal(runs[NAN]["dst"].cpu().numpy().reshape(h, w, 3), rr.resize(src, ow, oh, window))


@pytest.mark.parametrize("in_place", [False, True])
def test_axpy(in_place):
    n = 70008                                                         # a multiple of 8 (the entry point's precondition), of no larger power of two
    base, delta = rnd(n, seed=1), rnd(n, seed=2)
    operands = dict(base=Op(base), delta=delta, out=None if in_place else out16(n))
    launch = lambda v: ops.axpy(v["base"], v["delta"], 0.37, v["base"] if in_place else v["out"])
    name = "base" if in_place else "out"
    runs = iso.check_isolated(launch, operands, (name,), what="axpy")
    ref = base.double() + float(np.float32(0.37)) * delta.double()
    assert la.worst_ratio(runs[NAN][name], ref, la.store_bound(ref, 2 * la.U * (base.double().abs() + delta.double().abs()))) <= 1.0


def test_ln_fold_refresh():
    """g[n] = sum_k w[n][k] of the live fp16 weight, c = c_base + alpha c_delta: tolerances of test_gemm_with_folded_layernorm"""
    N, K = 320, 320
    w, cb, cd = rnd(N, K, seed=1, scale=K ** -0.5), r32(N, seed=2), r32(N, seed=3)
    operands = dict(w=w, cb=cb, cd=cd, g=outof(F32, N), c=outof(F32, N))
    launch = lambda v: ops.ln_fold_refresh(v["w"], v["g"], v["cb"], v["cd"], 0.5, v["c"])
    runs = iso.check_isolated(launch, operands, ("g", "c"), what="ln_fold_refresh")
    g = w.double().sum(1)
    assert float((runs[NAN]["g"].double() - g).abs().max()) < 1e-4 * max(1.0, float(g.abs().max()))
    assert torch.allclose(runs[NAN]["c"], cb + 0.5 * cd, atol=1e-6)


# ==== super-resolution launches (sdlcm_amd.superres drives them through the C ABI, not through ops) ===========================
@pytest.mark.parametrize("W,H,tile,chunk", [(37, 29, 16, 4), (16, 16, 16, 1), (23, 9, 16, 3)])
def test_super_resolution_pass(W, H, tile, chunk):
    """One pass as SuperResNet._pass enqueues it -- chroma_h, then per chunk of tiles conv1, conv3x3 (64), conv3x3 (32),
    conv4_shuffle, then merge -- with the two activation buffers and the luma / chroma planes, which the pass allocates with
    torch.empty and reuses from chunk to chunk, as poisoned workspaces.  37 x 29 at tile 16: 3 x 2 overlapping tiles in chunks
    of 4 and 2 (the second chunk leaves two tiles of stale activations behind its own); 23 x 9: a tile shorter than the tile
    size.  Every byte of the planes and of the picture must be written; the picture is held against tests/sr_reference.py under
    the bound tests/test_superres_gpu.py derives for a pass (5: Y truncation, PIL's chroma tables and bicubic)."""
    import ctypes as C

    import sr_reference as sref
    from sdlcm_amd import lib, superres as S
    L, R = lib.load(), 3
    sd = S.load_weights("synthetic")
    wt = {k: v.to(DEV) for k, v in S.pack_weights(sd).items()}
    rgb = sref.test_images()(W, H, W + H)
    tw, th = min(tile, W), min(tile, H)
    nt = len(S.tile_plan(W, tw)) * len(S.tile_plan(H, th))
    assert nt == 1 or nt % chunk, "the last chunk is ragged"
    operands = dict(src=Op(torch.from_numpy(rgb).to(DEV)), out=outof(U8, R * H, R * W, 3), **{k: v for k, v in wt.items()})
    sc = dict(a=(chunk * th * tw * 64, F16), b=(chunk * th * tw * 64, F16), yp=(R * H * R * W, U8), cc=(H * R * W * 2, U8))
    p = lambda t: C.c_void_p(t.data_ptr())

    def launch(v):
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        src, a, b, yp, cc = v["src"], v["a"], v["b"], v["yp"], v["cc"]
        lib.check(L.lcm_sr_chroma_h(p(src), W, H, R, p(cc), s), "lcm_sr_chroma_h")
        for t0 in range(0, nt, chunk):
            n = min(chunk, nt - t0)
            lib.check(L.lcm_sr_conv1(p(src), W, H, tw, th, t0, n, p(v["w1"]), p(v["b1"]), p(a), s), "lcm_sr_conv1")
            lib.check(L.lcm_sr_conv3x3(p(a), n, th, tw, 64, p(v["w2"]), p(v["b2"]), p(b), s), "lcm_sr_conv3x3 conv2")
            lib.check(L.lcm_sr_conv3x3(p(b), n, th, tw, 32, p(v["w3"]), p(v["b3"]), p(a), s), "lcm_sr_conv3x3 conv3")
            lib.check(L.lcm_sr_conv4_shuffle(p(a), W, H, tw, th, t0, n, p(v["w4"]), p(v["b4"]), R, p(yp), s), "lcm_sr_conv4_shuffle")
        lib.check(L.lcm_sr_merge(p(yp), p(cc), W, H, R, p(v["out"]), s), "lcm_sr_merge")
        return dict(y_plane=yp, cbcr_h=cc)

    runs = iso.check_isolated(launch, operands, ("out",), scratch=sc, what=f"super-resolution {W}x{H}")
    want = sref.upscale_once(sd, rgb, tile)
    d = np.abs(runs[NAN]["out"].cpu().numpy().astype(np.int16) - want)
    assert d.max() <= 5, int(d.max())


# ==== whole passes on the module pipeline ==================================================================================
@pytest.fixture(scope="module")
def nets():
    from sdlcm_amd import weights
    from sdlcm_amd.model import UNetHip, VAEDecoderHip
    return UNetHip(weights.synthetic_unet(), None, DEV), VAEDecoderHip(weights.synthetic_vae(), None, DEV)


def _pass_isolated(run, B, poison):
    """run(j, fill) -> outputs [B, ...] of the pass with image j's inputs filled (j None: clean).  The pass reuses the nets'
    activation buffers from run to run, as the server does between requests: what a poisoned run leaves in them is the next
    run's stale memory."""
    ws = torch.empty(16 << 20, dtype=F32, device=DEV)
    ops.set_workspace(ws)
    try:
        clean = run(None, None)
        assert bool(torch.isfinite(clean.float()).all())
        for j in poison:
            for fill in (NAN, PINF):
                iso.fill_(ws, fill)
                got = run(j, fill)
                for i in range(B):
                    if i != j:
                        assert la.same_bits(got[i].contiguous(), clean[i].contiguous()), f"image {i} changed with image {j} filled with {fill}"
        again = run(None, None)                                      # and the leftovers of the poisoned passes change nothing
        assert la.same_bits(again, clean)
    finally:
        torch.cuda.synchronize()
        ops.set_workspace(None)
    return clean


def test_unet_forward_keeps_the_images_of_a_batch_apart(nets):
    from sdlcm_amd.pipeline import guidance_scale_embedding
    unet, _ = nets
    B, h, w, t = 3, 9, 17, 759
    lat0 = r32(B, 4, h, w, seed=11)
    pe0 = rnd(B * 77, 768, seed=12)
    wemb = torch.from_numpy(guidance_scale_embedding(np.zeros(B, np.float32), 256)).to(DEV, F16)

    def run(j, fill):
        lat, pe = lat0.clone(), pe0.clone()
        if j is not None:
            iso.fill_(lat[j], fill)
            iso.fill_(pe[j * 77:(j + 1) * 77], fill)
        eps = iso.fill_(torch.empty(B, h, w, 4, dtype=F32, device=DEV), fill or NAN)
        kv = unet.encode_context(pe, B)
        unet.forward(lat, t, kv, wemb, B, h, w, eps)
        torch.cuda.synchronize()
        return eps

    _pass_isolated(run, B, (0, 1))


def test_vae_decode_keeps_the_images_of_a_batch_apart(nets):
    _, vae = nets
    B, h, w = 3, 9, 17
    lat0 = r32(B, 4, h, w, seed=13, scale=0.9)

    def run(j, fill):
        lat = lat0.clone()
        if j is not None:
            iso.fill_(lat[j], fill)
        rgb = torch.zeros(B, 8 * h, 8 * w, 3, dtype=U8, device=DEV)
        img = iso.fill_(torch.empty(B, 8 * h, 8 * w, 3, dtype=F32, device=DEV), fill or NAN)
        vae.decode(lat, B, h, w, rgb, img_f32=img)
        torch.cuda.synchronize()
        return torch.cat([img.reshape(B, -1), rgb.reshape(B, -1).float()], 1)

    _pass_isolated(run, B, (0, 1))
