"""The launch audit's error bound (tests/launch_audit.py) on the CPU: a product computed the way the kernels compute it (fp16
operands, fp32 accumulation over the k-tiles of each part of the K partition, parts added in order, fp16 store) passes it;
the same product wrong by one K term, one 64-wide K chunk, one output row or a skipped prologue SiLU does not.  Without this a
bound could grow loose enough to accept anything.  The same for attention: the online softmax of each attention kernel replayed
over the designed logits of tests/attention_cases.py stays inside attention_check, and each of nine planted faults leaves it."""
import numpy as np
import pytest
import torch

import attention_cases as ac
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


# ---- odd geometry: cropped upsample targets, stride 2 on odd inputs, ragged key tiles ---------------------------------------
def _im2col(img, stride=1, pad_mode="constant"):
    """img [H, W, C] fp32 -> [Ho * Wo, 9 * C] (tap major, channel minor), padding 1."""
    Hh, Ww, C = img.shape
    xp = torch.nn.functional.pad(img.permute(2, 0, 1)[None], (1, 1, 1, 1), mode=pad_mode)[0].permute(1, 2, 0)
    Ho, Wo = ((Hh + 1) // 2, (Ww + 1) // 2) if stride == 2 else (Hh, Ww)
    parts = [xp[ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride] for ky in range(3) for kx in range(3)]
    return torch.stack(parts, 2).reshape(Ho * Wo, 9 * C)


def _conv_case(Hh, Ww, C=64, Cout=64, seed=30):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(Hh * Ww, C, generator=g).half()
    w4 = torch.randn(Cout, C, 3, 3, generator=g) * (9 * C) ** -0.5
    return x, w4


def _up2(img):
    return img.repeat_interleave(2, 0).repeat_interleave(2, 1)


def test_odd_upsample_target_bound_rejects_an_ignored_crop_and_phase_weights_at_the_border():
    """Upsample2D to an odd skip size: nearest 2x cropped to (2H-1, 2W-1), zero padding AFTER the crop, plain 3x3 weights.  A
    conv of the full 2x image cropped afterwards, and the phase-packed form (which is that conv), differ in the last row and
    column only -- and are rejected; crops in one direction only likewise."""
    from sdlcm_amd.packing import pack_conv3x3, pack_conv3x3_up2
    Hh, Ww, C = 5, 4, 64
    x, w4 = _conv_case(Hh, Ww)
    w = pack_conv3x3(w4).half()
    img = x.float().reshape(Hh, Ww, C)
    full = _kernel_like(_im2col(_up2(img)).half(), w).reshape(2 * Hh, 2 * Ww, -1)          # conv of the uncropped 2x image
    wp = pack_conv3x3_up2(w4).half()
    ph = torch.cat([t[1] for t in la.conv_bands(img.double(), None, wp, phases=True)]).half().reshape(2 * Hh, 2 * Ww, -1)
    assert la.conv_check(ph.reshape(-1, 64), x, wp, 1, Hh, Ww, ups=2) <= 1.0              # the phase form is right for 2H x 2W
    for Ho, Wo in ((2 * Hh - 1, 2 * Ww - 1), (2 * Hh - 1, 2 * Ww), (2 * Hh, 2 * Ww - 1)):
        kw = dict(ups=1, out_hw=(Ho, Wo))
        good = _kernel_like(_im2col(_up2(img)[:Ho, :Wo]).half(), w)
        assert la.conv_check(good, x, w, 1, Hh, Ww, **kw) <= 1.0, (Ho, Wo)
        late = full[:Ho, :Wo].reshape(Ho * Wo, -1)
        assert la.conv_check(late, x, w, 1, Hh, Ww, **kw) > 1.0, ("crop ignored: full 2x conv cropped afterwards", Ho, Wo)
        inner = (late.reshape(Ho, Wo, -1)[:2 * Hh - 2, :2 * Ww - 2] == good.reshape(Ho, Wo, -1)[:2 * Hh - 2, :2 * Ww - 2]).all()
        assert inner, "the wrong form must differ in the last row / column only"
        assert la.conv_check(ph[:Ho, :Wo].reshape(Ho * Wo, -1), x, w, 1, Hh, Ww, **kw) > 1.0, ("phase-packed weights at the border", Ho, Wo)


def test_stride2_bound_on_an_odd_input_rejects_a_replicated_last_row():
    from sdlcm_amd.packing import pack_conv3x3
    for Hh, Ww in ((9, 7), (9, 8), (8, 7)):
        x, w4 = _conv_case(Hh, Ww, seed=31)
        w = pack_conv3x3(w4).half()
        img = x.float().reshape(Hh, Ww, 64)
        good = _kernel_like(_im2col(img, 2).half(), w)
        assert good.shape[0] == ((Hh + 1) // 2) * ((Ww + 1) // 2)
        assert la.conv_check(good, x, w, 1, Hh, Ww, stride=2) <= 1.0, (Hh, Ww)
        if Hh % 2 or Ww % 2:        # the tap past an odd edge reads the zero row / column, not a copy of the last one
            wrong = _kernel_like(_im2col(img, 2, "replicate").half(), w)
            # only the far border may differ: keep the near border of the correct result
            Ho, Wo = (Hh + 1) // 2, (Ww + 1) // 2
            g3, w3 = good.reshape(Ho, Wo, -1), wrong.reshape(Ho, Wo, -1).clone()
            w3[0], w3[:, 0] = g3[0], g3[:, 0]
            if not Hh % 2:
                w3[-1] = g3[-1]
            if not Ww % 2:
                w3[:, -1] = g3[:, -1]
            assert la.conv_check(w3.reshape(Ho * Wo, -1), x, w, 1, Hh, Ww, stride=2) > 1.0, (Hh, Ww)


def _attn_kernel_like(q, k, v, scale, extra_zero_key=False, drop_last=False):
    """one head: fp32 logits of the fp16 operands, fp32 softmax sum, P rounded to fp16 for the PV product, fp16 store."""
    K, V = k.float(), v.float()
    if drop_last:
        K, V = K[:-1], V[:-1]
    if extra_zero_key:           # a padding row of a ragged last key tile that is not masked: logit 0, value 0
        K, V = torch.cat([K, torch.zeros(1, K.shape[1])]), torch.cat([V, torch.zeros(1, V.shape[1])])
    S = (q.float() @ K.T) * scale
    p = torch.exp(S - S.max(1, keepdim=True).values)
    return ((p.half().float() @ V) / p.sum(1, keepdim=True)).half()


def test_attention_bound_rejects_a_padding_key_and_a_dropped_last_key():
    """Sk = 63 (one ragged register-staged tile) and Sk = 825 (ragged last tile of the streaming kernel).  The logits of the
    real keys sit near -5 (a zero padding key would carry weight), the last key near -1 with a value of its own (it carries
    weight too); values are positive so that |o| is of the size of sum p |v|."""
    d, Sq = 40, 16
    scale = d ** -0.5
    for Sk in (63, 825):
        g = torch.Generator().manual_seed(32 + Sk)
        q = (1.0 + 0.1 * torch.randn(Sq, d, generator=g)).half()
        k = (-0.79 + 0.05 * torch.randn(Sk, d, generator=g))
        k[-1] = -0.16
        k = k.half()
        v = (1.0 + 0.1 * torch.randn(Sk, d, generator=g))
        v[-1] = 3.0
        v = v.half()
        chk = lambda got: la.attention_check(got, q, k, v, 1, 1, Sq, Sk, d, scale=scale)
        assert chk(_attn_kernel_like(q, k, v, scale)) <= 1.0, Sk
        assert chk(_attn_kernel_like(q, k, v, scale, extra_zero_key=True)) > 1.0, ("a zero padding key admitted", Sk)
        assert chk(_attn_kernel_like(q, k, v, scale, drop_last=True)) > 1.0, ("the last real key dropped", Sk)


# ---- the online softmax of csrc/attention.hip, replayed ----------------------------------------------------------------
# fault -> the kernel families (attention_cases.Case.family) whose code has the step the fault breaks
ATTN_FAULTS = {
    "o_not_rescaled": ("attn", "attn_causal", "attn2", "wide"),       # O keeps its old unit when the running max moves
    "l_not_rescaled": ("attn", "attn_causal", "attn2", "wide"),       # forms whose row sum is a register (no ONES row in O^T)
    "fold_lo_dropped": ("attn2",),                                    # d = 40: only the fp16 hi part of -m enters the MFMA
    "delta_not_clamped": ("attn2",),                                  # a lane below its max follows the wave's rescale downwards
    "p_clamped_at_1": ("attn2",),                                     # P of the deferred rescale reaches 2^THR
    "last_key_masked": ("attn", "attn_causal", "attn2", "wide"),
    "padding_key_admitted": ("attn", "attn2", "wide"),
    "diagonal_masked": ("attn_causal",),
    "merge_without_a2": ("attn2",),                                   # key split: group 1's state added without 2^(m2 - m)
}


def _attn_replay(q, k, v, *, tile=64, thr=None, fold=False, ones=False, ksplit=False, causal=False, sc=1.0, wave=32,
                 pad="zero", fault=None):
    """One head the way the kernels compute it: fp32 logits of the fp16 operands per key tile, the running max / row sum / O
    recurrence in fp32, P rounded to fp16 for the PV product, fp32 PV, fp16 store.
      thr None: the max moves on every increase, P = exp2(s * sc - m) (attn_kernel, attn_wide_kernel);
      thr: Q is scaled and rounded to fp16 first, the max moves (for the lanes of a `wave`-row wave together) only when one of
        them grows by more than thr, each lane by its own max(grow, 0) (attn2_kernel); fold: -m enters the logit as fp16 hi + lo;
      ones: the row sum accumulates the fp16 P (a row of O^T), else the fp32 P;
      ksplit: tiles [0, ceil(n/2)) and [ceil(n/2), n) as two independent states, merged at the end;
      pad: the rows of a ragged tile past Sk are zeros ("zero") or repeat the last key ("dup") before they are masked."""
    Sq, Sk = q.shape[0], k.shape[0]
    f32 = torch.float32
    sc32 = torch.tensor(sc, dtype=f32)
    Q = (q.float() * sc32).half().float() if thr is not None else q.float()
    K, V = k.float(), v.float()
    n = (Sk + tile - 1) // tile
    rows = torch.arange(Sq)

    def any_wave(t):
        w = torch.nn.functional.pad(t.float(), (0, -Sq % wave)).view(-1, wave).sum(1) > 0
        return w.repeat_interleave(wave)[:Sq]

    def stream(t0, t1):
        m = torch.zeros(Sq) if thr is not None else torch.full((Sq,), -1.0e30)
        l, O = torch.zeros(Sq), torch.zeros(Sq, V.shape[1])
        hi = lo = torch.zeros(Sq)
        for it, t in enumerate(range(t0, t1)):
            keys = torch.arange(t * tile, (t + 1) * tile)
            src = keys.clamp(max=Sk - 1)
            Kt, Vt = K[src], V[src]
            if pad == "zero":
                Kt, Vt = Kt * (keys < Sk)[:, None], Vt * (keys < Sk)[:, None]
            S = Q @ Kt.T
            if fold:
                S = (S.double() + hi.double()[:, None] + lo.double()[:, None]).float()
            limit = Sk + 1 if fault == "padding_key_admitted" and Sk % tile else Sk - 1 if fault == "last_key_masked" else Sk
            masked = (keys >= limit)[None, :].expand(Sq, -1)
            if causal:
                masked = masked | ((keys[None, :] >= rows[:, None]) if fault == "diagonal_masked" else (keys[None, :] > rows[:, None]))
            S = torch.where(masked, torch.tensor(-1.0e30), S)
            mt = S.max(1).values
            if thr is None:
                m_new = torch.maximum(m, mt * sc32)
                alpha = torch.exp2(m - m_new)
                m = m_new
                P = torch.exp2(S * sc32 - m[:, None])
            else:
                grow = mt if fold else mt - m
                if it == 0:
                    trig, delta, alpha = torch.ones(Sq, dtype=torch.bool), grow, torch.ones(Sq)
                else:
                    trig = any_wave(grow > thr)
                    delta = torch.where(trig, grow if fault == "delta_not_clamped" else grow.clamp(min=0.0), torch.zeros(Sq))
                    alpha = torch.exp2(-delta)
                m = m + delta
                if fold:
                    S = S - delta[:, None]
                    nhi = (-m).half().float()
                    nlo = torch.zeros(Sq) if fault == "fold_lo_dropped" else (-m - nhi).half().float()
                    hi, lo = torch.where(trig, nhi, hi), torch.where(trig, nlo, lo)
                P = torch.exp2(S if fold else S - m[:, None])
                if fault == "p_clamped_at_1":
                    P = P.clamp(max=1.0)
            if fault != "l_not_rescaled":
                l = l * alpha
            if fault != "o_not_rescaled":
                O = O * alpha[:, None]
            P16 = P.half().float()
            l = l + (P16 if ones else P).sum(1)
            O = O + P16 @ Vt
        return m, l, O

    if ksplit:
        nh = (n + 1) // 2
        (m1, l1, O1), (m2, l2, O2) = stream(0, nh), stream(nh, n)
        m = torch.maximum(m1, m2)
        a1 = torch.exp2(m1 - m)
        a2 = torch.ones(Sq) if fault == "merge_without_a2" else torch.exp2(m2 - m)
        l, O = l1 * a1 + l2 * a2, O1 * a1[:, None] + O2 * a2[:, None]
    else:
        _, l, O = stream(0, n)
    return (O * (1.0 / l)[:, None]).half()


def _replay_case(case, ops, fault=None):
    """the whole case through the replay of the kernel that serves it -> [Sq, heads * d] fp16"""
    q, k, v = ops
    d, kern = case.d, case.kernel
    sc = float(np.float32(case.scale) * np.float32(1.4426950408889634)) if case.scale > 0 else 1.0
    kw = dict(tile=case.tile, causal=case.causal, sc=sc, fault=fault)
    if kern == "attn2":
        kw.update(thr=ac.THR, fold=d == 40, ones=d in (40, 80), ksplit=case.ksplit, pad="dup")
    elif kern == "wide":
        kw.update(wave=16, pad="dup")
    else:
        kw.update(ones=d in (40, 80))
    return torch.cat([_attn_replay(*(t[:, h * d:(h + 1) * d] for t in (q, k, v)), **kw) for h in range(case.heads)], 1)


def _case_ratio(case, ops, got):
    q, k, v = ops
    return la.attention_check(got, q, k, v, 1, case.heads, case.Sq, case.Sk, case.d, scale=case.scale, causal=case.causal)


def _fault_applies(fault, case):
    if case.family not in ATTN_FAULTS[fault]:
        return False
    if fault == "l_not_rescaled":
        return case.d not in (40, 80) or case.kernel == "wide"
    if fault == "fold_lo_dropped":
        return case.d == 40
    if fault == "merge_without_a2":
        return case.ksplit
    if fault == "padding_key_admitted":
        return case.Sk % case.tile != 0
    return True


@pytest.fixture(scope="module")
def attention_table():
    return [(c, c.operands()) for c in ac.table()]


def test_attention_replay_is_within_the_bound_on_every_designed_case(attention_table):
    """The faithful replay of each kernel's recurrence stays inside attention_check on every case of tests/attention_cases.py:
    the condition under which the GPU test may demand the same of the kernels.  Prints the worst ratio per kernel form."""
    worst = {}
    for case, ops in attention_table:
        got = _replay_case(case, ops)
        assert torch.isfinite(got.float()).all(), case.name
        r = _case_ratio(case, ops, got)
        worst[case.form] = max(worst.get(case.form, 0.0), r)
        assert r <= 1.0, (case.name, r)
    print("\n".join(f"replay worst ratio  {f:24s} {r:.3f}" for f, r in sorted(worst.items())))


@pytest.mark.parametrize("fault", sorted(ATTN_FAULTS))
def test_attention_cases_reject_a_planted_fault(attention_table, fault):
    """every planted fault leaves the bound on at least one designed case of each kernel family whose code has that step"""
    caught = {fam: None for fam in ATTN_FAULTS[fault]}
    for case, ops in attention_table:
        if caught.get(case.family, True) is not None or not _fault_applies(fault, case):
            continue
        r = _case_ratio(case, ops, _replay_case(case, ops, fault))
        if r > 1.0:
            caught[case.family] = (case.name, r)
    assert all(caught.values()), (fault, caught)
    print("\n".join(f"{fault:22s} {fam:12s} rejected by {c[0]} at {c[1]:.3g}" for fam, c in sorted(caught.items())))


def test_dropped_fold_lo_is_rejected_on_every_large_offset_case(attention_table):
    """The fp16 lo half of the folded max is what the +-1000.5 offsets are for: dropping it must leave the bound on each d = 40
    streaming case that carries them below 4160 keys, not on one alone.  (At 330 keys the margin is 1.6x: the one to watch when a
    derived term is added to attention_check; the key-split shapes stand at 5x.)"""
    names = ("s40-96x330-offsets", "s40-96x1030-offsets", "s40-96x1088-offsets")
    seen = 0
    for case, ops in attention_table:
        if case.name in names:
            seen += 1
            r = _case_ratio(case, ops, _replay_case(case, ops, "fold_lo_dropped"))
            assert r > 1.0, (case.name, r)
    assert seen == len(names)


def test_frame_writes_counts_a_row_past_the_output():
    """the layout of tests/test_attention_stress_gpu.py: out at column 8 of a wider pitch between two sentinel rows.  A row
    stored past the last one (a lost `qrow < Sq` guard) or in front of the first lands outside launch_audit.out_window; the
    whole-buffer comparison counts every element of it."""
    rows, C, pad = 70, 80, 16
    ldo = C + pad
    buf = torch.full(((rows + 2) * ldo,), -7.0, dtype=torch.float16)
    out = buf.as_strided((rows, C), (ldo, 1), ldo + pad // 2)
    before = buf.clone()
    out.fill_(1.0)
    assert la.frame_writes(before, buf, out) == 0
    buf.as_strided((1, C), (ldo, 1), (rows + 1) * ldo + pad // 2).fill_(2.0)          # row `rows`
    assert la.frame_writes(before, buf, out) == C
    buf.as_strided((1, C), (ldo, 1), pad // 2).fill_(2.0)                             # row -1
    assert la.frame_writes(before, buf, out) == 2 * C
    buf[ldo + pad // 2 + C] = 3.0                                                     # a gap column of row 0
    assert la.frame_writes(before, buf, out) == 2 * C + 1


def test_attention_bound_charges_the_q_rounding_only_where_it_happens():
    """The fp16 rounding of a scaled Q (H max sum |q k|) is charged to the streaming kernel called with scale > 0 and to nothing
    else: the same wrong result (two cancelling channels of Q moved one fp16 step apart) passes only where it is charged."""
    assert la.attention_kernel(40, 128, False) == "attn2" and la.attention_kernel(40, 127, False) == "attn"
    assert la.attention_kernel(64, 4096, True) == "attn" and la.attention_kernel(160, 4096, False) == "attn"
    assert la.attention_kernel(512, 4096, False) == "wide"
    assert la.attention_tile(512, 100, False) == 32 and la.attention_tile(40, 100, False) == 64
    assert [la.attention_key_split(40, Sk, False) for Sk in (1023, 1024, 4096, 4097)] == [False, True, True, False]
    assert not la.attention_key_split(160, 2048, False) and not la.attention_key_split(64, 2048, True)
    assert la.attention_rounds_q(40, 330, False, 40 ** -0.5) and not la.attention_rounds_q(40, 330, False, 0.0)
    assert not la.attention_rounds_q(40, 77, False, 40 ** -0.5) and not la.attention_rounds_q(512, 330, False, 512 ** -0.5)
    d, Sq, Sk = 40, 8, 330
    g = torch.Generator().manual_seed(7)
    q = torch.zeros(Sq, d)
    q[:, 0], q[:, 1] = 1.0, -1.0                          # two large products that cancel: the logit is the noise ...
    k = 0.2 * torch.randn(Sk, d, generator=g)
    k[:, :2] = 0.0
    k[:Sk // 2, :2] = 400.0                               # ... unless the two channels of q are rounded apart
    v = 1.0 + 0.1 * torch.randn(Sk, d, generator=g)
    v[Sk // 2:] = 3.0
    q, k, v = q.half(), k.half(), v.half()
    kw = dict(tile=64, thr=ac.THR, fold=True, ones=True, pad="dup")
    good = _attn_replay(q, k, v, **kw)
    q_off = q.clone()
    q_off[:, 0] = 1.0 + 2.0 ** -10                        # one fp16 step: what rounding a scaled Q channel by channel may do
    off = _attn_replay(q_off, k, v, **kw)
    chk = lambda got, **o: la.attention_check(got, q, k, v, 1, 1, Sq, Sk, d, scale=0.0, **o)
    assert chk(good) <= 1.0
    assert chk(off) > 1.0 and chk(off, q_rounded=True) <= 1.0


# ---- ControlNet: hint stack, conv_in + hint embedding ----------------------------------------------------------------------
def _hilo_chain(cols32, w16, bias, lo=True):
    """fp32 chain bias + hi . w (+ lo . w): the operand enters the MFMA as fp16 hi + fp16 lo against the same weights."""
    hi = cols32.half()
    acc = (bias.float() if bias is not None else 0.0) + hi.float() @ w16.float().T
    if lo:
        acc = acc + (cols32 - hi.float()).half().float() @ w16.float().T
    return acc


def test_hint_u8_bound_rejects_an_input_carried_as_one_fp16():
    from sdlcm_amd.packing import pack_conv3x3
    g = torch.Generator().manual_seed(33)
    B, Hh, Ww, Cout = 2, 24, 20, 16
    img = torch.randint(0, 256, (B, Hh, Ww, 3), generator=g, dtype=torch.uint8)
    img[0, :4, :4], img[0, -4:, -4:] = 0, 255
    w = pack_conv3x3(torch.randn(Cout, 3, 3, 3, generator=g) * 27 ** -0.5).half()
    bias = (0.01 * torch.randn(Cout, generator=g)).half()
    x, xerr = la.hint_u8_input(img)

    def run(lo):
        x32 = img.float() / 255.0
        acc = torch.cat([_hilo_chain(_im2col(x32[b]), w, bias, lo) for b in range(B)])
        return (acc * torch.sigmoid(acc)).half()
    chk = lambda got: la.hint_layer_check(got, x, xerr, w, bias, B, Hh, Ww, 1, True, la.HINT_U8_K)
    assert chk(run(True)) <= 1.0
    assert chk(run(False)) > 1.0, "u8 / 255 carried as a single fp16"
    # hint_conv: a narrow fp16 layer at stride 2 on an odd input
    xin = (torch.randn(B * 9 * 7, 16, generator=g)).half()
    w2 = pack_conv3x3(torch.randn(32, 16, 3, 3, generator=g) * 144 ** -0.5).half()
    b2 = (0.1 * torch.randn(32, generator=g)).half()
    x3 = xin.float().reshape(B, 9, 7, 16)

    def run2(mode, silu=True):
        acc = torch.cat([b2.float() + _im2col(x3[b], 2, mode) @ w2.float().T for b in range(B)])
        return (acc * torch.sigmoid(acc) if silu else acc).half()
    chk2 = lambda got: la.hint_layer_check(got, x3.double(), None, w2, b2, B, 9, 7, 2, True, 144)
    assert chk2(run2("constant")) <= 1.0
    assert chk2(run2("replicate")) > 1.0 and chk2(run2("constant", silu=False)) > 1.0


def test_conv_c4_res_bound_rejects_a_conv_rounded_before_the_residual():
    """res ~ -conv: the sum is small, so the fp16 rounding of the conv alone (H |conv|) is far outside H |sum| + E."""
    from sdlcm_amd.packing import pack_conv3x3
    g = torch.Generator().manual_seed(34)
    B, Hh, Ww, Cout = 2, 9, 7, 64
    lat = torch.randn(2 * B, 4, Hh, Ww, generator=g) * 4.0               # [2B]: the launch reads the first B images
    w = pack_conv3x3(torch.randn(Cout, 4, 3, 3, generator=g) * 0.3).half()
    bias = (0.1 * torch.randn(Cout, generator=g)).half()
    acc = torch.cat([_hilo_chain(_im2col(lat[b].permute(1, 2, 0)), w, bias) for b in range(B)])
    res = (-acc + 0.01 * torch.randn(acc.shape, generator=g)).half()
    chk = lambda got: la.conv_c4_res_check(got, lat, w, bias, res, B, Hh, Ww)
    assert chk((acc + res.float()).half()) <= 1.0
    assert chk((acc.half().float() + res.float()).half()) > 1.0, "conv rounded to fp16 before the residual"
    assert chk(acc.half()) > 1.0, "residual dropped"


# ---- refinement: re-noise and the hand-over step ----------------------------------------------------------------------------
def test_renoise_and_handover_bounds_reject_an_unwritten_first_half():
    from sdlcm_amd.scheduler import LCMSchedule
    gen = torch.Generator().manual_seed(35)
    B, h, w = 2, 9, 5
    for pred in ("epsilon", "v_prediction"):
        s = LCMSchedule(prediction_type=pred)
        ts = s.timesteps(4, 0.5)
        coef, last = s.step_coefficients(ts, 3)
        assert last
        nsa, nsb = s.renoise_coefficients(ts[0])
        fsa, fsb = torch.tensor(nsa, dtype=torch.float32), torch.tensor(nsb, dtype=torch.float32)
        m, mu = torch.randn(B, h, w, 4, generator=gen), torch.randn(B, h, w, 4, generator=gen)
        x, n = torch.randn(B, 4, h, w, generator=gen) * 12, torch.randn(B, 4, h, w, generator=gen)
        for cfg in (None, 5.0):
            kw = dict(m_u=mu, g=cfg) if cfg else {}
            rkw = dict(m_u=mu, guidance=cfg) if cfg else {}
            xk = _step_kernel_like(m, x, None, coef, True, pred=pred, **kw)
            state = fsa * xk + fsb * n
            chk = lambda xk_, st_, front: la.handover_check(xk_, st_, front, m, x, n, coef, nsa, nsb, B, pred=pred, **rkw)
            assert chk(xk, state, state.clone() if cfg else None) <= 1.0, (pred, cfg)
            assert chk(xk, fsa * xk + fsb * n.flip(0), None) > 1.0, "re-noised with another image's noise"
            assert chk(xk, fsb * xk + fsa * n, None) > 1.0, "re-noise coefficients swapped"
            assert chk(state, state, None) > 1.0, "x^k holds the re-noised state"
            if cfg:
                assert chk(xk, state, x.clone()) > 1.0, "dup: the first half left unwritten"
                front = state.clone()
                front[1, 2, 3, 4] = torch.nextafter(front[1, 2, 3, 4], torch.tensor(1e9))
                assert chk(xk, state, front) > 1.0, "dup: halves differ in one bit"
        # latents_renoise: lat [2B] with dup
        lat = torch.cat([fsa * x + fsb * n] * 2)
        assert la.renoise_check(lat, x, n, nsa, nsb, B, True) <= 1.0 and la.renoise_check(lat[:B], x, n, nsa, nsb, B, False) <= 1.0
        half = lat.clone()
        half[B:] = -7.0
        assert la.renoise_check(half, x, n, nsa, nsb, B, True) > 1.0, "dup: second copy unwritten"
        assert la.renoise_check(torch.cat([fsa * x + fsa * n] * 2), x, n, nsa, nsb, B, True) > 1.0


# ---- what a contraction launch must not write -------------------------------------------------------------------------------
def _audited_fake_gemm(stray=None, touch_a=False):
    """Audit's hook around an emulated lcm_gemm_f16 writing a column slice of a fused [M + 2, 3 N] buffer (the layout of the QKV
    buffer / a skip concat with spare rows) -> the check it recorded.  stray: (row, column) of the buffer written on top."""
    import inspect
    from sdlcm_amd import ops
    M, N, K = 70, 64, 128                       # a ragged last row tile
    a, w, b = _operands(M, N, K, seed=36)
    buf = torch.full((M + 2, 3 * N), 0.5, dtype=torch.float16)
    out = buf[:, N:2 * N]
    sig = inspect.signature(ops.gemm)

    def fake(*args, **kw):
        A = sig.bind(*args, **kw).arguments
        o = A["out"]
        o.as_strided((A["M"], A["N"]), (A["ldo"], 1), o.storage_offset()).copy_(_kernel_like(A["a"], A["w"], bias=A["bias"]))
        if stray is not None:
            buf[stray] = 1.0
        if touch_a:
            A["a"][3, 5] += 1
        return o
    fake.__signature__ = sig
    au = la.Audit()
    au.recs = []
    au._wrap("gemm", fake)(a, w, out, bias=b, M=M, N=N, ldo=3 * N)
    (c,) = au.checks
    return c


def test_hooked_launch_must_not_write_outside_its_logical_output():
    M, N = 70, 64
    c = _audited_fake_gemm()
    assert c["ratio"] <= 1.0 and not c["stray"] and not la.failures([c])
    for where, stray in (("one element past row M", (M, N + 3)), ("a gap column behind the slice", (2, 2 * N + 1)),
                         ("a gap column in front of the slice", (5, N - 1)), ("the last spare row", (M + 1, 2 * N - 1))):
        c = _audited_fake_gemm(stray)
        assert c["ratio"] > 1.0 and len(c["stray"]) == 1 and "operand out" in c["stray"][0] and la.failures([c]), where
    c = _audited_fake_gemm(touch_a=True)
    assert c["ratio"] > 1.0 and "operand a" in c["stray"][0]
    # the window arithmetic on its own: batched output with a batch stride, gap between the batch entries
    buf = torch.zeros(2 * 40 + 8)
    out = buf[4:]
    start, n, keep = la.out_window(out, 3, 5, 8, batch=2, stride_o=40)
    assert start == 1 and not keep[3:8].any() and keep[8:11].all() and not keep[3 + 40:8 + 40].any()
    assert int((~keep).sum()) == 2 * 3 * 5
    before = la.window_of(out, start, n).clone()
    buf[4 + 40 + 2 * 8 + 5] = 1.0                # column 5 of the last row of batch entry 1: a gap column
    assert la.stray_writes(before, la.window_of(out, start, n), keep) == 1
