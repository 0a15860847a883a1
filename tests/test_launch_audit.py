"""The launch audit's error bound (tests/launch_audit.py) on the CPU: a product computed the way the kernels compute it (fp16
operands, fp32 accumulation over the k-tiles of each part of the K partition, parts added in order, fp16 store) passes it;
the same product wrong by one K term, one 64-wide K chunk, one output row or a skipped prologue SiLU does not.  Without this a
bound could grow loose enough to accept anything."""
import torch

import launch_audit as la


def _kernel_like(a16, w16, splits=1, bias=None, drop_k=None, drop_chunk=None, store=True):
    """out = fl16(sum over parts (fp32 sum over 16-wide k steps of the part) + bias), parts of the K partition in order
    (store=False: the fp32 value before the store)."""
    M, K = a16.shape
    a, w = a16.float().clone(), w16.float()
    if drop_k is not None:
        a[:, drop_k] = 0
    if drop_chunk is not None:
        a[:, drop_chunk * 64:(drop_chunk + 1) * 64] = 0
    nk = K // 64
    tot = torch.zeros(M, w.shape[0], dtype=torch.float32)
    for s in range(splits):
        acc = torch.zeros_like(tot)
        for t in range(s * nk // splits, (s + 1) * nk // splits):
            for k0 in range(t * 64, t * 64 + 64, 16):
                acc = acc + a[:, k0:k0 + 16] @ w[:, k0:k0 + 16].T
        tot = tot + acc
    if bias is not None:
        tot = tot + bias.float()
    return tot.half() if store else tot


def _operands(M, N, K, seed=0):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(M, K, generator=g).half()
    w = (torch.randn(N, K, generator=g) * K ** -0.5).half()
    b = torch.randn(N, generator=g).half()
    return a, w, b


def test_gemm_bound_accepts_kernel_order_and_rejects_a_dropped_term():
    M, N, K = 96, 64, 2880
    a, w, b = _operands(M, N, K)
    ref, bnd = la.gemm_reference(a, w, bias=b)
    for splits in (1, 3, 5):
        assert la.worst_ratio(_kernel_like(a, w, splits, bias=b), ref, bnd) <= 1.0
    good = _kernel_like(a, w, 5, bias=b)
    assert la.worst_ratio(_kernel_like(a, w, 5, bias=b, drop_k=1234), ref, bnd) > 1.0, "one K term dropped"
    assert la.worst_ratio(_kernel_like(a, w, 5, bias=b, drop_chunk=17), ref, bnd) > 1.0, "one 64-wide K chunk dropped"
    shifted = good.clone()
    shifted[40] = good[41]
    assert la.worst_ratio(shifted, ref, bnd) > 1.0, "an output row taken from its neighbour"


def test_gemm_bound_with_epilogue_residual_and_scale():
    M, N, K = 64, 128, 640
    a, w, b = _operands(M, N, K, seed=1)
    res = torch.randn(M, N, generator=torch.Generator().manual_seed(3)).half()
    ref, bnd = la.gemm_reference(a, w, bias=b, res=res, out_scale=0.5)
    acc = _kernel_like(a, w, 2, bias=b, store=False)
    assert la.worst_ratio((acc * 0.5 + res.float()).half(), ref, bnd) <= 1.0
    out_noscale = (acc + res.float()).half()
    assert la.worst_ratio(out_noscale, ref, bnd) > 1.0


def test_conv_gn_bound_rejects_a_skipped_silu():
    """3x3 conv behind a GroupNorm-apply + SiLU prologue: the kernel rounds the normalised operand to fp16."""
    B, Hh, Ww, C, Cout = 1, 6, 5, 64, 64
    g = torch.Generator().manual_seed(4)
    x = (torch.randn(B * Hh * Ww, C, generator=g) * 3 + 1).half()
    w = (torch.randn(Cout, 9 * C, generator=g) * (9 * C) ** -0.5).half()
    scale = (torch.rand(B, C, generator=g) + 0.2).float()
    shift = torch.randn(B, C, generator=g).float()

    def run(silu):
        v = x.float() * scale[0] + shift[0]
        xn = (v * torch.sigmoid(v) if silu else v).half().reshape(Hh, Ww, C)
        cols = torch.stack([torch.nn.functional.pad(xn.float(), (0, 0, 1, 1, 1, 1))[ky:ky + Hh, kx:kx + Ww]
                            for ky in range(3) for kx in range(3)], 2).reshape(Hh * Ww, 9 * C).half()
        return _kernel_like(cols, w)

    kw = dict(gn_scale=scale, gn_shift=shift, silu=True)
    assert la.conv_check(run(True), x, w, B, Hh, Ww, **kw) <= 1.0
    assert la.conv_check(run(False), x, w, B, Hh, Ww, **kw) > 1.0, "prologue SiLU skipped"


def test_stats_bound():
    """fused statistics: fp32 partial sums over 32-row slabs of the stored fp16 output pass, a slab counted twice does not."""
    class St:
        pass
    out = torch.randn(2 * 128, 64, generator=torch.Generator().manual_seed(5)).half()
    x = out.float().reshape(2, 4, 32, 64)
    st = St()
    st.P = 4
    st.buf = torch.stack([x.sum(2), (x * x).sum(2)], -1).reshape(-1).contiguous()
    assert la.stats_check(st, out, 2) <= 1.0
    st.buf = st.buf.reshape(2, 4, 64, 2).clone()
    st.buf[1, 2] = st.buf[1, 3]
    st.buf = st.buf.reshape(-1)
    assert la.stats_check(st, out, 2) > 1.0
