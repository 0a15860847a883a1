"""The launches of tests/test_entry_path_gpu.py, shared with the generator of its golden hashes
(tests/golden/make_parent_bits_entry_path.py): the smallest inputs at which an index computed in front of a kernel's first
load -- tile split, k-tile bounds, ring issue order, patch / phase / slab coordinates -- can go wrong.  `run_cases()` runs every
case on the GPU and returns {case name: sha256 over the output bytes, the statistics slab count and the statistics bytes}."""
import hashlib

import numpy as np
import torch

from sdlcm_amd import ops

DEV = "cuda"


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(torch.float16)


def to_nhwc(x):
    B, C, H, W = x.shape
    return x.permute(0, 2, 3, 1).reshape(B * H * W, C).contiguous()


def pack3x3(w):
    return w.permute(0, 2, 3, 1).contiguous().reshape(w.shape[0], -1)


def digest(out, st=None):
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(out.detach().cpu().numpy()).tobytes())
    if st is not None:
        h.update(str(int(st.P)).encode())
        h.update(np.ascontiguousarray(st.buf.detach().cpu().numpy()).tobytes())
    return h.hexdigest()


def _stats(M, N, hw):
    return ops.Stats(torch.zeros(ops.stats_floats(M, N, hw), dtype=torch.float32, device=DEV))


def _gemm(res, name, M, N, K, *, img_rows=0, parts=0, seg=2, bias=True, rowadd=False, residual=False, K1=0, plan=None, persist=0,
          narrow=False):
    """parts > 0: the canonical partition of the per-image shape has `parts` parts (seg 2: split launch + reduce, 1: segmented)."""
    m_img = img_rows or M
    ops.plan_clear()
    ops.narrow_clear()
    if parts:
        ops.plan_set(0, m_img, N, K, 1, 64, 64, parts)
        ops.plan_set(0, M, N, K, 1, 64, 64, parts)
        assert ops.canonical_splits(0, m_img, N, K) == parts
    if plan:
        ops.plan_set(0, M, N, K, 1, *plan)
    if narrow:
        ops.narrow_set(0, M, N, K, 1)
    ops.set_seg_mode(seg)
    ops.set_persist_n(persist)
    a = rnd(M, K1 or K, seed=1).to(DEV)
    a2 = rnd(M, K - K1, seed=5).to(DEV) if K1 else None
    w = rnd(N, K, seed=2, scale=K ** -0.5).to(DEV)
    images = M // m_img
    b = rnd(N, seed=11).to(DEV) if bias else None
    ra = rnd(images, N, seed=12).to(DEV) if rowadd else None
    rs = rnd(M, N, seed=13).to(DEV) if residual else None
    o = torch.full((M, N), 7.0, dtype=torch.float16, device=DEV)
    st = _stats(M, N, m_img)
    ops.gemm(a, w, o, a2=a2, bias=b, rowadd=ra, rows_per_batch=m_img if rowadd else 0, res=rs, stats=st, img_rows=img_rows)
    res[name] = digest(o, st)


def _conv(res, name, B, H, W, Cin, Cout, *, stride=1, ups=0, out_hw=None, parts=0, seg=2, plan=None, residual=True, rowadd=True,
          unsplit=False):
    from sdlcm_amd.packing import pack_conv3x3_up2
    Ho, Wo = out_hw if out_hw else (2 * H, 2 * W) if ups else ((H + 1) // 2, (W + 1) // 2) if stride == 2 else (H, W)
    HW, K = Ho * Wo, (4 if ups == 2 else 9) * Cin
    M = B * HW
    kind, aux, ph = (1, 1, 0) if stride == 2 else (2, Wo << 1, 1 if ups == 2 else 0)
    ops.plan_clear()
    ops.narrow_clear()
    ops.set_split_policy(max_rows_per_image=0) if unsplit else ops.set_split_policy()
    if parts:
        ops.plan_set(kind, HW, Cout, K, aux, 64, 64, parts)
        ops.plan_set(kind, M, Cout, K, aux, 64, 64, parts)
        assert ops.canonical_splits(kind, HW, Cout, K, aux, ph) == parts, name
    if plan:
        ops.plan_set(kind, M, Cout, K, aux, *plan)
    ops.set_seg_mode(seg)
    x = to_nhwc(rnd(B, Cin, H, W, seed=1)).to(DEV)
    w4 = rnd(Cout, Cin, 3, 3, seed=2, scale=(9 * Cin) ** -0.5)
    w = (pack_conv3x3_up2(w4) if ups == 2 else pack3x3(w4)).to(DEV)
    b = rnd(Cout, seed=11).to(DEV)
    ra = rnd(B, Cout, seed=12).to(DEV) if rowadd else None
    rs = rnd(M, Cout, seed=13).to(DEV) if residual else None
    o = torch.full((M, Cout), 7.0, dtype=torch.float16, device=DEV)
    st = _stats(M, Cout, HW)
    ops.conv3x3(x, w, o, B, H, W, Cin, Cout, bias=b, rowadd=ra, res=rs, stride=stride, ups=ups, stats=st, out_hw=out_hw)
    res[name] = digest(o, st)


def _conv_gn(res, name, B, H, W, C1, C2, Cout, *, xform, parts=0):
    Cin, HW = C1 + C2, H * W
    M, K = B * HW, 9 * (C1 + C2)
    ops.plan_clear()
    ops.narrow_clear()
    ops.set_split_policy()
    if parts:
        ops.plan_set(2, HW, Cout, K, W << 1, 64, 64, parts)
        ops.plan_set(2, M, Cout, K, W << 1, 64, 64, parts)
    ops.set_seg_mode(2)
    x = to_nhwc(rnd(B, C1, H, W, seed=1)).to(DEV)
    x2 = to_nhwc(rnd(B, C2, H, W, seed=3)).to(DEV) if C2 else None
    w = pack3x3(rnd(Cout, Cin, 3, 3, seed=2, scale=K ** -0.5)).to(DEV)
    sc = (1 + 0.1 * torch.randn(B, Cin, generator=torch.Generator().manual_seed(8))).float().to(DEV) if xform else None
    sh = (0.1 * torch.randn(B, Cin, generator=torch.Generator().manual_seed(9))).float().to(DEV) if xform else None
    o = torch.full((M, Cout), 7.0, dtype=torch.float16, device=DEV)
    st = _stats(M, Cout, HW)
    ops.conv3x3_gn(x, w, o, B, H, W, C1, Cout, x2=x2, C2=C2, gn_scale=sc, gn_shift=sh, silu=True, bias=rnd(Cout, seed=11).to(DEV),
                   rowadd=rnd(B, Cout, seed=12).to(DEV), stats=st)
    res[name] = digest(o, st)


def _groupnorm(res, name, B, HW, C1, C2):
    C = C1 + C2
    xs = [(rnd(B * HW, c, seed=20 + i) + 0.25).to(DEV) for i, c in enumerate((C1, C2)) if c]
    P = (HW + 31) // 32
    sts = []
    for x in xs:                      # the statistics as a producer writes them: per 32-pixel slab (the last one ragged) and channel
        c = x.shape[1]
        xf = torch.zeros(B, P * 32, c, dtype=torch.float32, device=DEV)
        xf[:, :HW] = x.float().view(B, HW, c)
        xf = xf.view(B, P, 32, c)
        st = ops.Stats(torch.stack([xf.sum(2), (xf * xf).sum(2)], dim=-1).contiguous().view(-1))
        st.P = P
        sts.append(st)
    gamma, beta = (1 + 0.1 * rnd(C, seed=6).float()).half().to(DEV), rnd(C, seed=7, scale=0.1).to(DEV)
    ws = torch.zeros(ops.groupnorm_ws_bytes(B, HW, C) // 4 + 16, dtype=torch.float32, device=DEV)
    y = torch.full((B * HW, C), 3.0, dtype=torch.float16, device=DEV)
    ops.groupnorm_from_stats(xs[0], gamma, beta, y, B, HW, C1, sts[0], ws, x2=xs[1] if C2 else None, C2=C2, st2=sts[1] if C2 else None)
    res[name] = digest(y)


def _attention(res, name, d, heads, Sq, Sk):
    ld = heads * d
    q, k, v = rnd(Sq, ld, seed=31).to(DEV), rnd(Sk, ld, seed=32).to(DEV), rnd(Sk, ld, seed=33).to(DEV)
    o = torch.full((Sq, ld), 5.0, dtype=torch.float16, device=DEV)
    ops.attention(q, k, v, o, 1, heads, Sq, Sk, d, ldq=ld, ldk=ld, ldv=ld, ldo=ld)
    res[name] = digest(o)


def run_cases():
    res = {}
    ws = torch.zeros(8 << 20, dtype=torch.float32, device=DEV)
    ops.set_workspace(ws)
    try:
        # ---- GEMM ----
        _gemm(res, "gemm M=77 img_rows=77", 77, 320, 320, img_rows=77)
        _gemm(res, "gemm M=154 img_rows=77 rowadd", 154, 320, 320, img_rows=77, rowadd=True, residual=True)
        _gemm(res, "gemm M=64*3+1", 193, 320, 320, residual=True)
        _gemm(res, "gemm N=320 n_iters=5", 24576, 320, 320, plan=(64, 64, 1, 4), persist=1, residual=True)
        for parts in (5, 8):
            _gemm(res, f"gemm K=1344 split {parts}", 256, 320, 1344, img_rows=256, parts=parts, rowadd=True, residual=True)
            _gemm(res, f"gemm K=1344 segmented {parts}", 256, 320, 1344, img_rows=256, parts=parts, seg=1, residual=True)
        _gemm(res, "gemm K=1344 split 5, last slab of 8 rows", 72, 64, 1344, parts=5, residual=True)
        _gemm(res, "gemm two-input K1=320", 100, 320, 640, K1=320)
        _gemm(res, "gemm 32-column tile", 256, 1280, 1280, img_rows=256, narrow=True, residual=True)
        for variant in (1, 2, 3):      # single buffer, double buffer, three stages: each ring depth's prologue
            _gemm(res, f"gemm M=193 ring variant {variant}", 193, 320, 320, plan=(64, 64, 1, variant), residual=True)
        _gemm(res, "gemm 128x160 tile", 300, 320, 320, plan=(128, 160, 1, 3), residual=True)
        ops.plan_clear()
        ops.set_persist_n(0)
        # blockIdx.z = 3 with strides
        Mz, Nz, Kz = 70, 64, 128
        a, w = rnd(4, Mz, Kz, seed=1).to(DEV), rnd(4, Nz, Kz, seed=2, scale=Kz ** -0.5).to(DEV)
        o = torch.full((4, Mz, Nz), 7.0, dtype=torch.float16, device=DEV)
        ops.gemm(a, w, o, M=Mz, N=Nz, K=Kz, lda=Kz, ldo=Nz, batch=4, strideA=Mz * Kz, strideW=Nz * Kz, strideO=Mz * Nz)
        res["gemm batch 4 strided"] = digest(o)
        # the LayerNorm fold
        a, w = rnd(100, 320, seed=1).to(DEV), rnd(320, 320, seed=2, scale=320 ** -0.5).to(DEV)
        g, c = torch.randn(320, generator=torch.Generator().manual_seed(4)).to(DEV), torch.randn(320, generator=torch.Generator().manual_seed(5)).to(DEV)
        o = torch.full((100, 320), 7.0, dtype=torch.float16, device=DEV)
        ops.gemm_ln(a, w, g, c, o)
        res["gemm LayerNorm fold"] = digest(o)

        # ---- stride-2 conv (row-gather kernel, MODE 1) ----
        _conv(res, "conv stride 2 9x13", 1, 9, 13, 128, 64, stride=2)
        _conv(res, "conv stride 2 16x16 split 4", 2, 16, 16, 128, 64, stride=2, parts=4)
        _conv(res, "conv stride 2 16x16 segmented 4", 2, 16, 16, 128, 64, stride=2, parts=4, seg=1)

        # ---- halo conv: 1 and 5 parts (the reduce walks 4x8 patches at 8x8 and 9x13 -- ragged there -- and 2x16 ones at 24x40) ----
        for H, W in ((8, 8), (9, 13), (24, 40)):
            _conv(res, f"conv {H}x{W} 1 part", 1, H, W, 320, 64, unsplit=True)
            _conv(res, f"conv {H}x{W} 5 parts", 1, H, W, 320, 64, parts=5)
            _conv(res, f"conv {H}x{W} 5 parts segmented", 2, H, W, 320, 64, parts=5, seg=1)
        for variant in (1, 2, 3):      # single-buffer kernel | pipelined, one tap per step | a row of taps per step
            _conv(res, f"conv 24x40 unsplit variant {variant} (staged epilogue)", 1, 24, 40, 128, 64, plan=(64, 64, 1, variant), unsplit=True)
            _conv(res, f"conv 9x13 5 parts variant {variant}", 1, 9, 13, 320, 64, parts=5, plan=(64, 64, 5, variant))
        _conv(res, "conv 24x40 128-row tile", 1, 24, 40, 128, 128, plan=(128, 128, 1, 3), unsplit=True)
        _conv(res, "conv phase upsample 8x8 4 parts", 1, 8, 8, 256, 64, ups=2, parts=4, residual=False)
        _conv(res, "conv phase upsample 8x8 unsplit", 1, 8, 8, 256, 64, ups=2, unsplit=True)
        _conv(res, "conv cropped upsample 5x7 -> 9x13 4 parts", 1, 5, 7, 256, 64, ups=1, out_hw=(9, 13), parts=4)
        _conv_gn(res, "conv skip concat 9x13", 1, 9, 13, 64, 128, 64, xform=False)
        _conv_gn(res, "conv skip concat 9x13 3 parts", 1, 9, 13, 64, 128, 64, xform=False, parts=3)
        _conv_gn(res, "conv GroupNorm-staged 9x13", 1, 9, 13, 128, 0, 64, xform=True)
        _conv_gn(res, "conv GroupNorm-staged concat 24x40", 2, 24, 40, 64, 64, 64, xform=True)

        # ---- GroupNorm from statistics, single launch ----
        _groupnorm(res, "groupnorm 81 x 320", 1, 81, 320, 0)
        _groupnorm(res, "groupnorm 81 x 320+640", 1, 81, 320, 640)
        _groupnorm(res, "groupnorm B=2 256 x 64+64", 2, 256, 64, 64)

        # ---- attention (sources untouched: the launches are here so that a later change of this kind has them) ----
        _attention(res, "attn_kernel<160> 33 x 64 keys", 160, 2, 33, 64)
        _attention(res, "attn2_kernel<40> 96 x 1088 keys", 40, 2, 96, 1088)
        torch.cuda.synchronize()
    finally:
        ops.set_seg_mode(0)
        ops.set_split_policy()
        ops.set_persist_n(0)
        ops.plan_reset()
        ops.set_workspace(None)
    return res
