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


# ---- the other entry points of a pass ------------------------------------------------------------------------------------
def _gn_kernel_like(xs, B, HW, groups, gamma, beta, eps, *, no_eps=False, nm1=False, seam_shift=0, drop_slab=None):
    """GroupNorm tables the way the kernels compute them: fp32 (sum, sum of squares) per channel over 32-row slabs, the
    partials of each group combined in fp32, the one-pass variance, rsqrt -> (scale, shift) fp32 [B, C]."""
    x = torch.cat([t.float() for t in xs], 1).reshape(B, HW, -1)
    C = x.shape[2]
    P = -(-HW // 32)
    xp = torch.nn.functional.pad(x, (0, 0, 0, P * 32 - HW)).reshape(B, P, 32, C)
    part = torch.stack([xp.sum(2), (xp * xp).sum(2)], -1)               # [B, P, C, 2] fp32
    if drop_slab is not None:
        part[:, drop_slab] = 0
    cpg = C // groups
    bounds = [g * cpg for g in range(groups + 1)]
    if seam_shift:
        seam = xs[0].shape[1]
        bounds = [b + seam_shift if b < seam < b + cpg else b for b in bounds]
    n = HW * cpg
    scale = torch.empty(B, C, dtype=torch.float32)
    shift = torch.empty(B, C, dtype=torch.float32)
    inv = torch.tensor(1.0 / ((n - 1) if nm1 else n), dtype=torch.float32)
    for g in range(groups):
        s = part[:, :, bounds[g]:bounds[g + 1]].sum((1, 2))
        mean = s[:, 0] * inv
        var = torch.clamp(s[:, 1] * inv - mean * mean, min=0)
        rstd = torch.rsqrt(var + (0.0 if no_eps else eps))
        cs = slice(g * cpg, (g + 1) * cpg)
        scale[:, cs] = rstd[:, None] * gamma[cs].float()
        shift[:, cs] = beta[cs].float() - mean[:, None] * scale[:, cs]
    return scale, shift


def _gn_case(B, HW, C1, C2=0, mean=0.5, std=1.0, mean2=-1.0, std2=0.5, seed=20):
    g = torch.Generator().manual_seed(seed)
    xs = [(torch.randn(B * HW, C1, generator=g) * std + mean).half()]
    if C2:
        xs.append((torch.randn(B * HW, C2, generator=g) * std2 + mean2).half())
    C = C1 + C2
    gamma = (1 + 0.1 * torch.randn(C, generator=g)).half()
    beta = (0.1 * torch.randn(C, generator=g)).half()
    return xs, gamma, beta


def _gn_ratio(xs, B, HW, gamma, beta, eps=1e-5, **wrong):
    sc, sh = _gn_kernel_like(xs, B, HW, 32, gamma, beta, eps, **wrong)
    return la.gn_check(sc, sh, xs, B, HW, 32, gamma, beta, eps)


def test_gn_tables_bound_accepts_the_kernel_and_rejects_wrong_statistics():
    # the fused concat of an up block: C = 1280 + 640, 60 channels per group, group 21 straddles the seam
    xs, gamma, beta = _gn_case(2, 64, 1280, 640)
    r, kap = _gn_ratio(xs, 2, 64, gamma, beta)
    assert r <= 1.0 and kap < la.KAPPA_TRIP
    assert _gn_ratio(xs, 2, 64, gamma, beta, seam_shift=1)[0] > 1.0, "group boundary shifted by one channel at the seam"
    xs, gamma, beta = _gn_case(1, 256, 320)
    assert _gn_ratio(xs, 1, 256, gamma, beta)[0] <= 1.0
    assert _gn_ratio(xs, 1, 256, gamma, beta, drop_slab=5)[0] > 1.0, "one 32-row slab missing"
    # 1x1 spatial: n = channels per group = 40
    xs, gamma, beta = _gn_case(2, 1, 1280)
    assert _gn_ratio(xs, 2, 1, gamma, beta)[0] <= 1.0
    assert _gn_ratio(xs, 2, 1, gamma, beta, nm1=True)[0] > 1.0, "divided by n - 1"
    # a variance comparable to eps
    xs, gamma, beta = _gn_case(1, 64, 320, mean=0.0, std=1e-5 ** 0.5)
    assert _gn_ratio(xs, 1, 64, gamma, beta)[0] <= 1.0
    assert _gn_ratio(xs, 1, 64, gamma, beta, no_eps=True)[0] > 1.0, "eps omitted"


def test_gn_one_pass_variance_of_an_offset_group_is_rejected_or_tripped():
    """|mean| / std = 300: the one-pass fp32 variance cancels; the bound or the kappa tripwire must catch it."""
    xs, gamma, beta = _gn_case(1, 1024, 320, mean=300.0, std=1.0)
    r, kap = _gn_ratio(xs, 1, 1024, gamma, beta)
    assert r > 1.0 or kap > la.KAPPA_TRIP
    assert 100 < la.KAPPA_TRIP < 130


def test_gn_apply_bound_rejects_a_skipped_silu():
    xs, gamma, beta = _gn_case(1, 64, 320)
    sc, sh = _gn_kernel_like(xs, 1, 64, 32, gamma, beta, 1e-5)
    v = xs[0].float() * sc[0] + sh[0]
    good = (v * torch.sigmoid(v)).half()
    assert la.gn_check(None, None, xs, 1, 64, 32, gamma, beta, 1e-5, out=good, silu=True)[0] <= 1.0
    assert la.gn_check(None, None, xs, 1, 64, 32, gamma, beta, 1e-5, out=v.half(), silu=True)[0] > 1.0


def _ln_kernel_like(x, g, b, eps, eps_outside=False):
    X = x.float()
    mean = X.mean(1, keepdim=True)
    d = X - mean
    var = (d * d).mean(1, keepdim=True)
    rstd = 1.0 / (torch.sqrt(var) + eps) if eps_outside else torch.rsqrt(var + eps)
    return (d * rstd * g.float() + b.float()).half()


def test_layernorm_bound_rejects_eps_outside_the_sqrt():
    gen = torch.Generator().manual_seed(21)
    C = 768
    x = torch.randn(16, C, generator=gen)
    x[8:] *= 1e-5 ** 0.5                                  # rows whose variance is comparable to eps
    x = (x + 0.25).half()
    g, b = (1 + 0.1 * torch.randn(C, generator=gen)).half(), (0.1 * torch.randn(C, generator=gen)).half()
    ref, bnd = la.layernorm_reference(x, g, b, 1e-5)
    assert la.worst_ratio(_ln_kernel_like(x, g, b, 1e-5), ref, bnd) <= 1.0
    assert la.worst_ratio(_ln_kernel_like(x, g, b, 1e-5, eps_outside=True), ref, bnd) > 1.0


def _softmax_kernel_like(x, n, drop=None, pad=False):
    X = x.float()
    m = X[:, :n].max(1, keepdim=True).values
    p = torch.exp(X[:, :n] - m)
    keep = torch.ones(n, dtype=torch.bool)
    if drop is not None:
        keep[drop] = False
    s = p[:, keep].sum(1, keepdim=True)
    if pad:
        s = s + torch.exp(X[:, n:n + 1] - m)
    return (p / s).half()


def test_softmax_bound_rejects_a_dropped_or_a_padding_column():
    gen = torch.Generator().manual_seed(22)
    n, ld = 100, 128
    x = (torch.randn(12, ld, generator=gen) * 2).half()
    x[:, n:] = 0                                          # the zero key rows of the padded VAE attention give score 0
    ref, bnd = la.softmax_reference(x, n)
    assert la.worst_ratio(_softmax_kernel_like(x, n), ref, bnd) <= 1.0
    assert la.worst_ratio(_softmax_kernel_like(x, n, drop=37), ref, bnd) > 1.0, "one column dropped from the sum"
    assert la.worst_ratio(_softmax_kernel_like(x, n, pad=True), ref, bnd) > 1.0, "a padding column counted"


def _step_kernel_like(m, lat, noise, coef, last, m_u=None, g=1.0, pred="epsilon", swap=False, cfg_wrong=False):
    sa, sb, c_skip, c_out, sap, sbp = (torch.tensor(c, dtype=torch.float32) for c in coef)
    if swap:
        c_skip, c_out = c_out, c_skip
    M = m.permute(0, 3, 1, 2)
    if m_u is not None:
        Mu = m_u.permute(0, 3, 1, 2)
        M = (M + g * (M - Mu)) if cfg_wrong else (Mu + g * (M - Mu))
    x = lat
    x0 = (x - sb * M) / sa if pred == "epsilon" else (sa * x - sb * M if pred == "v_prediction" else M)
    den = c_out * x0 + c_skip * x
    return den if last else sap * den + sbp * noise


def test_sampler_step_bound_rejects_wrong_forms():
    from sdlcm_amd.scheduler import LCMSchedule
    s = LCMSchedule()
    ts = s.timesteps(4)
    gen = torch.Generator().manual_seed(23)
    B, h, w = 2, 8, 12
    m, mu = torch.randn(B, h, w, 4, generator=gen), torch.randn(B, h, w, 4, generator=gen)
    lat, noise = torch.randn(B, 4, h, w, generator=gen) * 14, torch.randn(B, 4, h, w, generator=gen)
    for i in range(4):
        coef, last = s.step_coefficients(ts, i)
        for pred in ("epsilon", "v_prediction", "sample"):
            for cfg in (None, 7.5):
                kw = dict(m_u=mu, g=cfg) if cfg else {}
                ref, bnd = la.sampler_step_reference(m, lat, noise, coef, last, pred=pred,
                                                     **(dict(m_u=mu, guidance=cfg) if cfg else {}))
                assert la.worst_ratio(_step_kernel_like(m, lat, noise, coef, last, pred=pred, **kw), ref, bnd) <= 1.0, (i, pred, cfg)
                if pred == "v_prediction":
                    assert la.worst_ratio(_step_kernel_like(m, lat, noise, coef, last, pred="epsilon", **kw), ref, bnd) > 1.0
                assert la.worst_ratio(_step_kernel_like(m, lat, noise, coef, last, pred=pred, swap=True, **kw), ref, bnd) > 1.0
                if cfg:
                    assert la.worst_ratio(_step_kernel_like(m, lat, noise, coef, last, pred=pred, cfg_wrong=True, **kw),
                                          ref, bnd) > 1.0


def _temb_kernel_like(t, B, dim, swap=False, half_exp=None):
    half = dim // 2
    k = torch.arange(half, dtype=torch.float32)
    f = torch.exp(torch.tensor(-9.210340371976184, dtype=torch.float32) * k / float(half if half_exp is None else half_exp))
    a = torch.tensor(float(t), dtype=torch.float32) * f
    c, s = torch.cos(a), torch.sin(a)
    row = torch.cat([s, c] if swap else [c, s])
    return row.half().repeat(B, 1)


def test_timestep_embedding_bound_rejects_swapped_halves_and_a_wrong_exponent():
    for t in (999, 759, 19, 0):
        ref, bnd = la.timestep_reference([t], 2, 320)
        assert la.worst_ratio(_temb_kernel_like(t, 2, 320), ref, bnd) <= 1.0, t
        if t:
            assert la.worst_ratio(_temb_kernel_like(t, 2, 320, swap=True), ref, bnd) > 1.0
            assert la.worst_ratio(_temb_kernel_like(t, 2, 320, half_exp=159), ref, bnd) > 1.0
    # several steps, rows step-major
    ts = [999, 759, 499, 259]
    ref, bnd = la.timestep_reference(ts, 3, 320)
    got = torch.cat([_temb_kernel_like(t, 3, 320) for t in ts])
    assert la.worst_ratio(got, ref, bnd) <= 1.0
    assert la.worst_ratio(torch.cat([_temb_kernel_like(t, 3, 320) for t in ts[::-1]]), ref, bnd) > 1.0


def test_place_tile_u8_rejects_truncation():
    gen = torch.Generator().manual_seed(24)
    v = torch.randn(1, 40, 56, 3, generator=gen) * 0.7
    u = torch.clamp(v * 0.5 + 0.5, 0, 1) * 255.0
    assert la.rgb8_check(torch.round(u).to(torch.uint8), v)[0] == 0
    assert la.rgb8_check(torch.trunc(u).to(torch.uint8), v)[0] > 0, "truncated instead of rounded"
    # exact ties round half to even
    tie = torch.tensor([(2 * k + 1) / 255.0 - 1.0 for k in (10, 11)], dtype=torch.float64)   # u * 255 = k + 0.5
    assert la.rgb8_reference(tie)[1].all()


def test_blend_bound_rejects_a_shifted_ramp():
    gen = torch.Generator().manual_seed(25)
    a, b = torch.randn(1, 64, 48, 3, generator=gen), torch.randn(1, 64, 48, 3, generator=gen)
    for vertical in (True, False):
        e = 32
        ref, bnd, band = la.blend_reference(a, b, e, vertical)
        for shift in (0, 1):
            t = (torch.arange(e, dtype=torch.float32) + shift) / e
            got = b.clone()
            if vertical:
                got[:, :e] = a[:, 64 - e:] * (1 - t[None, :, None, None]) + b[:, :e] * t[None, :, None, None]
            else:
                got[:, :, :e] = a[:, :, 48 - e:] * (1 - t[None, None, :, None]) + b[:, :, :e] * t[None, None, :, None]
            r = la.worst_ratio(got, ref, bnd)
            assert (r <= 1.0) if shift == 0 else (r > 1.0), (vertical, shift)


def test_pool8_bound_rejects_rounded_bins():
    gen = torch.Generator().manual_seed(26)
    for h, w in ((12, 20), (100, 96), (13, 9)):
        lat = torch.randn(2, 4, h, w, generator=gen)
        ref, bnd = la.pool8_reference(lat)
        good = torch.nn.functional.adaptive_avg_pool2d(lat, 8).half()
        assert la.worst_ratio(good, ref, bnd) <= 1.0
        rb = lambda n: [(round(o * n / 8), round((o + 1) * n / 8)) for o in range(8)]
        wrong = la.pool8_reference(lat, rb(h), rb(w))[0].half()
        assert la.worst_ratio(wrong, ref, bnd) > 1.0, (h, w)


def _glue_direct(tiles, ni, nj, extent, limit, left_first=False):
    """tiled_decode's glue written out pixel row by pixel row (the blend order selectable, for the wrong-order check)."""
    res = {k: v.clone() for k, v in tiles.items()}
    rows = []
    for i in range(ni):
        row = []
        for j in range(nj):
            t = res[(i, j)]
            for vertical in ((False, True) if left_first else (True, False)):
                if vertical and i > 0:
                    a = res[(i - 1, j)]
                    e = min(a.shape[1], t.shape[1], extent)
                    for y in range(e):
                        t[:, y] = a[:, a.shape[1] - e + y] * (1 - y / e) + t[:, y] * (y / e)
                if not vertical and j > 0:
                    a = res[(i, j - 1)]
                    e = min(a.shape[2], t.shape[2], extent)
                    for x in range(e):
                        t[:, :, x] = a[:, :, a.shape[2] - e + x] * (1 - x / e) + t[:, :, x] * (x / e)
            row.append(t[:, :limit, :limit])
        rows.append(torch.cat(row, 2))
    return torch.cat(rows, 1)


def test_tiled_glue_reference_matches_a_direct_restatement():
    """The glue reference (blend above, then left, extents clipped to the neighbours; crop to ``limit``) on ragged tile
    sizes; the wrong tile order (left before above) differs from it."""
    gen = torch.Generator().manual_seed(27)
    sample, H, W = 64, 100, 76                           # tiles 64 px, stride 48 px, extent 16, limit 48
    ys, xs = list(range(0, H, 48)), list(range(0, W, 48))
    tiles = {(i, j): torch.randn(1, min(64, H - y), min(64, W - x), 3, generator=gen, dtype=torch.float64)
             for i, y in enumerate(ys) for j, x in enumerate(xs)}
    img, E = la.tiled_glue_reference(tiles, sample, H, W)
    assert img.shape == (1, H, W, 3)
    assert (img - _glue_direct(tiles, len(ys), len(xs), 16, 48)).abs().max() <= 1e-12
    assert (E < 1e-5).all()
    wrong = _glue_direct(tiles, len(ys), len(xs), 16, 48, left_first=True)
    assert la.worst_ratio(wrong, img, E) > 1.0, "left before above must not pass as the glue"
