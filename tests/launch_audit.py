"""Launch audit: every contraction / attention launch of a real sampler pass against a float64 reference computed from the
launch's own fp16 operands, under a per-element error bound derived from the operation (not fitted to a run).

A plain module (like tests/pool_scenario.py): tests/test_configs_gpu.py runs the passes under ``Audit``, tests/test_launch_audit.py
checks on the CPU that the bound rejects a result that is wrong by one K term.

The bound.  For an output element y = sum_k a_k w_k (fp16 operands, exact fp32 products) the kernels accumulate in fp32: a
workgroup walks its k-tiles in order and the parts of the canonical K partition are added in part order (csrc/igemm.hip, "What
decides the numbers").  Whatever the partition, that is at most K fp32 additions, each with a rounding error of at most
U = 2^-24 times a partial sum bounded by S = sum_k |a_k w_k|.  Rounding errors of that kind behave as independent zero-mean
terms, so their sum stays within

    E_acc = C_ACC * U * sqrt(K) * S          C_ACC = 8   (the worst case K * U * S is not reached by a sum of mixed signs)

The fp32 epilogue (bias, row add, scale, activation, residual) adds one rounding per operation, bounded by a few U times the
magnitude of what it adds; the fp16 store adds at most half an fp16 ulp, i.e. H * |v| (H = 2^-11) for normal values and
SUB = 2^-25 in the subnormal range.  With E the error of the fp32 value v before the store:

    |got - ref| <= H * |ref| + SUB + (1 + H) * E

Where the kernel rounds a COMPUTED operand to fp16 (the GroupNorm / SiLU prologue of a conv, the GEGLU intermediate of the fused
FeedForward) that operand carries H * |a| + SUB more, which enters E as sum_k (H |a_k| + SUB) |w_k|: one more fp64 GEMM on
absolute values.  Every sum of absolute values is a second fp64 GEMM on |a| and |w|.

The references use torch float64 matmuls (rocBLAS on the GPU, or the CPU) -- never the project's kernels.
"""
from __future__ import annotations

import inspect
import math

import torch

U = 2.0 ** -24          # fp32 unit roundoff
H = 2.0 ** -11          # fp16 unit roundoff: half an ulp relative to the value
SUB = 2.0 ** -25        # half the fp16 subnormal step
C_ACC = 8.0             # multiple of sqrt(K) * U * S allowed for fp32 accumulation (see above)
GELU_APPROX = 1e-7      # |gelu_erf_f(x) - gelu(x)| / |x|: Abramowitz-Stegun 7.1.26 erf (|err| <= 1.5e-7) times x / 2
BAND_BYTES = 1 << 30    # working set of one im2col band (three fp64 copies of it live at once)
LN2 = math.log(2.0)


def acc_err(K, S):
    return (C_ACC * U * math.sqrt(K)) * S


def store_bound(ref, E, fp16=True):
    """bound of |got - ref| for a value computed in fp32 with error E and stored as fp16 (fp32 when fp16 is False)."""
    if fp16:
        return H * ref.abs() + SUB + (1.0 + H) * E
    return U * ref.abs() + (1.0 + U) * E + 1e-38


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound over the elements (inf where got is not finite)."""
    g = got.to(ref.device, torch.float64)
    r = (g - ref).abs() / bound
    r = torch.where(torch.isfinite(g), r, torch.full_like(r, math.inf))
    return float(r.max()) if r.numel() else 0.0


def _f64(t, dev):
    return None if t is None else t.to(dev, torch.float64)


def _mm(A, W, Aerr=None):
    """A [R, K] @ W[N, K]^T in fp64 -> (value, sum |a||w| [, sum err_a |w|])."""
    Wa = W.abs()
    out = (A @ W.T, A.abs() @ Wa.T)
    return out + ((Aerr @ Wa.T),) if Aerr is not None else out


def _gelu(x):
    return 0.5 * x * (1.0 + torch.special.erf(x * (0.5 ** 0.5)))


def _act(v, E, epilogue):
    """activation epilogues of lcm_gemm_f16 on an fp32 value v with error E -> (value, error); |slope| <= 1.13 for both."""
    if epilogue == 2:           # quick_gelu x * sigmoid(1.702 x): exp2 / rcp approximations, a few fp32 ulps
        y = v * torch.sigmoid(1.702 * v)
        return y, 1.13 * E + 8 * U * v.abs()
    if epilogue == 3:
        y = _gelu(v)
        return y, 1.13 * E + (GELU_APPROX + 8 * U) * v.abs()
    return v, E


def geglu_split(Y, E):
    """[R, 2F] product in the packed row order of pack_geglu (value / gate in blocks of 16) -> x * gelu(g) [R, F] in the stored
    column order (packing.geglu_col_order), with its error."""
    from sdlcm_amd.packing import geglu_col_order
    F = Y.shape[1] // 2
    c = geglu_col_order(F).to(Y.device)
    vcol = 32 * (c // 16) + c % 16
    x, g, ex, eg = Y[:, vcol], Y[:, vcol + 16], E[:, vcol], E[:, vcol + 16]
    gg = _gelu(g)
    y = x * gg
    Ey = gg.abs() * ex + x.abs() * (1.13 * eg + GELU_APPROX * g.abs() + 8 * U * gg.abs()) + ex * 1.13 * eg + 2 * U * y.abs()
    return y, Ey


def _epilogue(Y, S, E, *, bias=None, rowadd=None, res=None, out_scale=1.0, epilogue=0):
    """v = act(out_scale * (Y + bias + rowadd)) + res (igemm_epilogue order) -> (ref, E before the fp16 store)."""
    v, mag = Y, S
    if bias is not None:
        v = v + bias
        mag = mag + bias.abs()
    if rowadd is not None:
        v = v + rowadd
        mag = mag + rowadd.abs()
    E = E + 2 * U * mag
    if out_scale != 1.0:
        v, E = v * out_scale, (E + U * v.abs()) * abs(out_scale)
    if epilogue == 1:
        v, E = geglu_split(v, E)
    else:
        v, E = _act(v, E, epilogue)
    if res is not None:
        v = v + res
        E = E + U * v.abs()
    return v, E


# ---- dense contractions ------------------------------------------------------------------------------------------------
def gemm_reference(a, w, *, a2=None, bias=None, rowadd=None, rows_per_batch=0, res=None, out_scale=1.0, epilogue=0, rows=None):
    """lcm_gemm_f16 of one batch entry: a [M, K1] (+ a2 [M, K2]), w [N, K] fp16 -> (ref, bound) fp64 for output rows ``rows``
    (a slice; None = all)."""
    dev = a.device
    rows = rows if rows is not None else slice(0, a.shape[0])
    A = a[rows].to(torch.float64)
    if a2 is not None:
        A = torch.cat([A, a2[rows].to(torch.float64)], 1)
    W = w.to(torch.float64)
    Y, S = _mm(A, W)
    ra = None
    if rowadd is not None:
        idx = torch.arange(rows.start, rows.stop, device=dev) // rows_per_batch
        ra = rowadd.to(torch.float64)[idx]
    v, E = _epilogue(Y, S, acc_err(A.shape[1], S), bias=_f64(bias, dev), rowadd=ra,
                     res=_f64(res[rows], dev) if res is not None else None, out_scale=out_scale, epilogue=epilogue)
    return v, store_bound(v, E)


def _ln_product(a, w, ln_g, ln_c, eps, rows):
    """LayerNorm folded into the product (lcm_gemm_ln_f16): y = rstd * (a W'^T - mean * g) + c, fp64, with its error.
    The kernel's row statistics are fp32 sums of a and a^2 over K and var = sumsq / K - mean^2 (igemm_common.h)."""
    A = a[rows].to(torch.float64)
    K = A.shape[1]
    W = w.to(torch.float64)
    g, c = ln_g.to(torch.float64), ln_c.to(torch.float64)
    Y, S = _mm(A, W)
    mean = A.mean(1, keepdim=True)
    sq = (A * A).mean(1, keepdim=True)
    var = ((A - mean) ** 2).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    E_mean = C_ACC * U * math.sqrt(K) * A.abs().mean(1, keepdim=True) + U * mean.abs()
    E_var = C_ACC * U * math.sqrt(K) * sq + 2 * mean.abs() * E_mean + 2 * U * (sq + mean * mean)
    v = var + eps
    rel_r = torch.sqrt(v / torch.clamp(v - E_var, min=eps)) - 1.0 + 4 * U       # rsqrtf of a perturbed variance
    core = Y - mean * g
    E_core = acc_err(K, S) + E_mean * g.abs() + U * core.abs()
    y = rstd * core + c
    E = rstd * E_core * (1.0 + rel_r) + rel_r * rstd * core.abs() + 2 * U * (y.abs() + c.abs())
    return y, E


def gemm_ln_reference(a, w, ln_g, ln_c, *, eps=1e-5, epilogue=0, rows=None):
    rows = rows if rows is not None else slice(0, a.shape[0])
    y, E = _ln_product(a, w, ln_g, ln_c, eps, rows)
    if epilogue == 1:
        y, E = geglu_split(y, E)
    return y, store_bound(y, E)


def mlp_geglu_reference(x, w1, ln_g, ln_c, w2, b2, *, eps=1e-5, rows=None):
    """out = x + GEGLU(LN-fold(x) W1^T) W2^T + b2 with the [M, 4C] intermediate rounded to fp16 by the kernel."""
    rows = rows if rows is not None else slice(0, x.shape[0])
    h, Eh = _ln_product(x, w1, ln_g, ln_c, eps, rows)
    h, Eh = geglu_split(h, Eh)
    Ein = (1.0 + H) * Eh + H * h.abs() + SUB                      # fp16 intermediate
    W2 = w2.to(torch.float64)
    Y, S, Eprop = _mm(h, W2, Ein)
    v, E = _epilogue(Y, S + Eprop, acc_err(h.shape[1], S + Eprop) + Eprop, bias=b2.to(torch.float64),
                     res=x[rows].to(torch.float64))
    return v, store_bound(v, E)


def linear_reference(x, w, M, *, x_rows=None, bias=None, res=None, res_rows=None, silu_in=False, silu_out=False):
    """lcm_linear_rows_f16 / lcm_linear_smallm_f16: out[m] = act_out(act_in(x[m % x_rows]) W^T + bias + res[m % res_rows])."""
    dev = x.device
    xr = x_rows or M
    A = x[torch.arange(M, device=dev) % xr].to(torch.float64)
    Aerr = None
    if silu_in:                                                   # silu in fp32 (not rounded to fp16): a few ulps
        A = A * torch.sigmoid(A)
        Aerr = 8 * U * A.abs()
    W = w.to(torch.float64)
    r = _mm(A, W, Aerr)
    Y, S = r[0], r[1]
    E = acc_err(A.shape[1], S) + (r[2] if Aerr is not None else 0.0)
    rr = None
    if res is not None:
        rr = res[torch.arange(M, device=dev) % (res_rows or M)].to(torch.float64)
    v, E = _epilogue(Y, S, E, bias=_f64(bias, dev), res=rr)
    if silu_out:
        v, E = v * torch.sigmoid(v), 1.1 * E + 8 * U * v.abs()
    return v, store_bound(v, E)


# ---- 3x3 convolutions (im2col in row bands) ----------------------------------------------------------------------------
def _upsample(x, oh, ow):
    return x.repeat_interleave(2, 0).repeat_interleave(2, 1)[:oh, :ow]


def conv_bands(xin, xerr, w, *, stride=1, phases=False, band_rows=None):
    """One image: xin fp64 [Hi, Wi, Cin] (already normalised / upsampled), xerr its operand error or None; w fp16 [Cout, 9*Cin]
    (phases: [4*Cout, 4*Cin], ups=2 packing) -> yields (out rows slice, Y, S, Eop) over pixel-major output rows."""
    Hi, Wi, Cin = xin.shape
    W = w.to(torch.float64)
    pad = torch.nn.functional.pad
    xp = pad(xin, (0, 0, 1, 1, 1, 1))
    ep = pad(xerr, (0, 0, 1, 1, 1, 1)) if xerr is not None else None
    taps = 4 if phases else 9
    if phases:
        Ho, Wo, Wc = 2 * Hi, 2 * Wi, Wi
    else:
        Ho, Wo = ((Hi + 1) // 2, (Wi + 1) // 2) if stride == 2 else (Hi, Wi)
        Wc = Wo
    per_row = Wc * taps * Cin * 8 * 3
    band = band_rows or max(1, min(Ho if not phases else Hi, BAND_BYTES // per_row))

    def cols(src, y0, y1, py=0, px=0):
        if phases:
            parts = [src[y0 + py + dy:y1 + py + dy, px + dx:px + dx + Wi] for dy in range(2) for dx in range(2)]
        elif stride == 2:
            parts = [src[ky + 2 * y0:ky + 2 * (y1 - 1) + 1:2, kx:kx + 2 * (Wo - 1) + 1:2] for ky in range(3) for kx in range(3)]
        else:
            parts = [src[y0 + ky:y1 + ky, kx:kx + Wo] for ky in range(3) for kx in range(3)]
        return torch.stack(parts, 2).reshape(-1, taps * Cin)

    if not phases:
        for y0 in range(0, Ho, band):
            y1 = min(Ho, y0 + band)
            r = _mm(cols(xp, y0, y1), W, cols(ep, y0, y1) if ep is not None else None)
            yield (slice(y0 * Wo, y1 * Wo),) + tuple(r) + ((None,) if ep is None else ())
        return
    Cout = W.shape[0] // 4
    Wph = W.reshape(4, Cout, 4 * Cin)
    for y0 in range(0, Hi, band):
        y1 = min(Hi, y0 + band)
        Y = torch.empty(y1 - y0, 2, Wi, 2, Cout, dtype=torch.float64, device=xin.device)
        S = torch.empty_like(Y)
        for py in range(2):
            for px in range(2):
                y, s = _mm(cols(xp, y0, y1, py, px), Wph[py * 2 + px])
                Y[:, py, :, px] = y.reshape(y1 - y0, Wi, Cout)
                S[:, py, :, px] = s.reshape(y1 - y0, Wi, Cout)
        yield slice(2 * y0 * Wo, 2 * y1 * Wo), Y.reshape(-1, Cout), S.reshape(-1, Cout), None


def conv_check(got, x, w, B, Hin, Win, *, C1=None, x2=None, gn_scale=None, gn_shift=None, silu=True, bias=None, rowadd=None,
               res=None, stride=1, ups=0, out_hw=None, images=None, out_fp16=True, band_rows=None):
    """Worst error / bound ratio of a 3x3 convolution (lcm_conv3x3_f16 / _gn_f16 / _smalln) over images ``images`` (None: all):
    x [B*Hin*Win, >= C1] fp16 pixel-major (x2 the second source of a fused concat), got [B*Ho*Wo, Cout] as stored;
    gn_scale / gn_shift [B, C] fp32: the GroupNorm-apply (+SiLU) prologue, rounded to fp16 by the kernel."""
    dev = got.device
    C1 = x.shape[1] if C1 is None else C1
    if ups == 2:
        Ho, Wo = 2 * Hin, 2 * Win
    elif ups:
        Ho, Wo = tuple(out_hw) if out_hw is not None else (2 * Hin, 2 * Win)
    else:
        Ho, Wo = ((Hin + 1) // 2, (Win + 1) // 2) if stride == 2 else (Hin, Win)
    worst = 0.0
    for b in (range(B) if images is None else images):
        xin = x[b * Hin * Win:(b + 1) * Hin * Win, :C1].to(dev, torch.float64).reshape(Hin, Win, C1)
        if x2 is not None:
            xin = torch.cat([xin, x2[b * Hin * Win:(b + 1) * Hin * Win].to(dev, torch.float64).reshape(Hin, Win, -1)], 2)
        xerr = None
        if gn_scale is not None:      # GroupNorm-apply (+SiLU) in fp32, rounded to fp16 for the MFMA
            v = xin * gn_scale[b].to(dev, torch.float64) + gn_shift[b].to(dev, torch.float64)
            xin = v * torch.sigmoid(v) if silu else v
            xerr = (H + 16 * U) * xin.abs() + SUB + 4 * U * v.abs()
        if ups == 1:
            xin = _upsample(xin, Ho, Wo)
            xerr = _upsample(xerr, Ho, Wo) if xerr is not None else None
        for rows, Y, S, Eop in conv_bands(xin, xerr, w, stride=stride, phases=(ups == 2), band_rows=band_rows):
            E = acc_err(w.shape[1], S)
            if Eop is not None:
                E = E + Eop + acc_err(w.shape[1], Eop)
            base = b * Ho * Wo
            gr = slice(base + rows.start, base + rows.stop)
            v, E = _epilogue(Y, S, E, bias=_f64(bias, dev), rowadd=_f64(rowadd[b:b + 1], dev) if rowadd is not None else None,
                             res=_f64(res[gr], dev) if res is not None else None)
            worst = max(worst, worst_ratio(got[gr], v, store_bound(v, E, out_fp16)))
    return worst


def c4_input(lat, pre_w, pre_b, in_scale):
    """lcm_conv3x3_c4_f32in's operand: z = pre_w (lat * in_scale) + pre_b per pixel (fp32 math), entering the MFMA as fp16
    hi + lo parts (~22 bits) -> (z [B, H, W, 4] fp64, its error)."""
    r = lat.to(torch.float64).permute(0, 2, 3, 1) * float(in_scale)
    if pre_w is None:
        return r, 2.0 ** -21 * r.abs() + U * r.abs()
    pw, pb = pre_w.to(torch.float64).reshape(4, 4), pre_b.to(torch.float64)
    z = r @ pw.T + pb
    return z, 2.0 ** -21 * z.abs() + 6 * U * (r.abs() @ pw.abs().T + pb.abs())


# ---- attention ---------------------------------------------------------------------------------------------------------
def attention_check(got, q, k, v, B, heads, Sq, Sk, d, *, scale, causal=False, images=None, chunk_bytes=1 << 29):
    """softmax(Q K^T * scale) V in fp64 (scale <= 0: Q carries scale * log2 e, the logits are base-2).  Bound: the logits are
    off by at most D = scale * (H + C_ACC U sqrt(d)) * max_j sum_i |q_i k_ji| (Q pre-scaled in fp16, fp32 accumulation), which
    moves each unnormalised probability by a factor within exp(+-D); P is rounded to fp16 for the PV product; the online
    rescales are Sk / 32 fp32 multiplications at most.  Hence
        |o - o_ref| <= (2 (e^(2D) - 1) + 2 H + (2 C_ACC sqrt(Sk) + Sk / 32 + 8) U) * sum_j p_j |v_j|  (+ the fp16 store)."""
    dev = got.device
    s = LN2 if scale <= 0 else scale
    worst = 0.0
    for b in (range(B) if images is None else images):
        for hh in range(heads):
            cs = slice(hh * d, (hh + 1) * d)
            Q = q[b * Sq:(b + 1) * Sq, cs].to(dev, torch.float64)
            Kh = k[b * Sk:(b + 1) * Sk, cs].to(dev, torch.float64)
            V = v[b * Sk:(b + 1) * Sk, cs].to(dev, torch.float64)
            step = max(1, chunk_bytes // (Sk * 8 * 3))
            for r0 in range(0, Sq, step):
                r1 = min(Sq, r0 + step)
                L = (Q[r0:r1] @ Kh.T) * s
                La = (Q[r0:r1].abs() @ Kh.abs().T) * s
                if causal:
                    mask = torch.arange(Sk, device=dev)[None, :] > torch.arange(r0, r1, device=dev)[:, None]
                    L = L.masked_fill(mask, -math.inf)
                    La = La.masked_fill(mask, 0.0)
                P = torch.softmax(L, 1)
                o = P @ V
                pv = P @ V.abs()
                D = (H + C_ACC * U * math.sqrt(d)) * La.max(1, keepdim=True).values + 4 * U * L.abs().nan_to_num(0, 0, 0).max(1, keepdim=True).values
                rel = 2 * torch.expm1(2 * D) + 2 * H + (2 * C_ACC * math.sqrt(Sk) + Sk / 32 + 8) * U
                E = rel * pv
                worst = max(worst, worst_ratio(got[b * Sq + r0:b * Sq + r1, cs], o, store_bound(o, E)))
    return worst


# ---- fused GroupNorm statistics ----------------------------------------------------------------------------------------
def stats_check(stats, out, n_images):
    """stats: ops.Stats of a launch (P > 0), out [n_images * rows, N] its fp16 output.  The partials are fp32 (sum, sum of
    squares) of the STORED fp16 values over canonical 32-pixel slabs: <= 31 fp32 additions each (and one rounded square), so
    summed in fp64 per (image, channel) they lie within 33 U * sum|x| (resp. 33 U * sum x^2) of the exact fp64 sums."""
    N = out.shape[1]
    P = stats.P
    part = stats.buf[:n_images * P * N * 2].view(n_images, P, N, 2).to(torch.float64).sum(1)
    x = out.to(torch.float64).reshape(n_images, -1, N)
    s1, s2, a1 = x.sum(1), (x * x).sum(1), x.abs().sum(1)
    r1 = (part[..., 0] - s1).abs() / (33 * U * a1 + 1e-30)
    r2 = (part[..., 1] - s2).abs() / (33 * U * s2 + 1e-30)
    r = torch.maximum(r1, r2)
    r = torch.where(torch.isfinite(part).all(-1), r, torch.full_like(r, math.inf))
    return float(r.max())


# ---- the hook ----------------------------------------------------------------------------------------------------------
HOOKED = ("gemm", "gemm_ln", "mlp_geglu", "conv3x3", "conv3x3_gn", "conv3x3_smalln", "conv3x3_c4", "linear_rows",
          "linear_smallm", "attention")


def _pick_images(n, limit):
    """images checked of an n-image launch: all up to ``limit``, else the first and the last (the batch borders)."""
    return list(range(n)) if limit is None or n <= limit else [0, n - 1]


def _row_slices(n_img, rows_img, images):
    return [slice(b * rows_img, (b + 1) * rows_img) for b in _pick_images(n_img, images)]


def _ident(k, v):
    """what identifies a launch's shape: tensor shapes / strides, flags, scalars (not the data, not the statistics buffer)"""
    if torch.is_tensor(v):
        return k, tuple(v.shape), tuple(v.stride())
    if k == "stats":
        return k, v is not None
    return k, v if isinstance(v, (int, float, bool, str, type(None))) else repr(v)


class Audit:
    """``with Audit() as au:`` wraps the contraction / attention entry points of ``sdlcm_amd.ops``; the first launch of each
    distinct (entry point, argument shapes) is synchronised and checked against its fp64 reference right away.
    au.checks: one dict per checked launch (plan key, table entry, config, worst ratio, statistics ratio)."""

    def __init__(self, images=None):
        from sdlcm_amd import lib
        self.images = images                 # per launch: all images (None), or up to this many, else the first and the last
        self.table = lib.known_plans()
        self.checks = []
        self.seen = set()
        self.recs = None

    def __enter__(self):
        from sdlcm_amd import ops
        self._ops = ops
        self._saved = {n: getattr(ops, n) for n in HOOKED}
        for n, f in self._saved.items():
            setattr(ops, n, self._wrap(n, f))
        self._rec_cm = ops.recording()
        self.recs = self._rec_cm.__enter__()
        return self

    def __exit__(self, *exc):
        self._rec_cm.__exit__(*exc)
        for n, f in self._saved.items():
            setattr(self._ops, n, f)
        return False

    def record_keys(self):
        return {r[0] for r in self.recs if r[0] is not None}

    def checked_keys(self):
        return {c["key"] for c in self.checks if c["key"] is not None}

    def _wrap(self, name, real):
        sig = inspect.signature(real)

        def hooked(*args, **kw):
            ba = sig.bind(*args, **kw)
            ba.apply_defaults()
            A = dict(ba.arguments)
            ident = (name,) + tuple(_ident(k, v) for k, v in A.items())
            if ident in self.seen:
                return real(*args, **kw)
            self.seen.add(ident)
            out = A["out"]
            keep = {}
            for k, v in A.items():        # whatever the launch may overwrite: inputs sharing the output's storage
                if torch.is_tensor(v) and k != "out" and v.untyped_storage().data_ptr() == out.untyped_storage().data_ptr():
                    keep[k] = v.clone()
            n0 = len(self.recs)
            r = real(*args, **kw)
            if out.is_cuda:
                torch.cuda.current_stream().synchronize()
            A.update(keep)
            rec = self.recs[n0] if len(self.recs) > n0 else (None, None, None)
            self._check(name, A, rec[0], rec[1] or {})
            del keep, A
            return r
        return hooked

    def _config(self, key, meta):
        if key is None:
            return None, None
        from sdlcm_amd import autotune, ops
        entry = self.table.get(key)
        splits = autotune._canonical_splits(key, meta, meta.get("m_img", key[1]))
        if entry is not None:
            bm, bn, v = int(entry[0]), int(entry[1]), int(entry[3])
        else:                                                  # no entry: the occupancy heuristic picks the tile
            bm, bn, v = 0, 0, -1
        return entry, (key[0], bm, bn, splits, v)

    def _check(self, name, A, key, meta):
        entry, cfg = self._config(key, meta)
        ratio, sratio = getattr(self, "_ref_" + name)(A)
        st = A.get("stats")
        if st is not None and st.P > 0:
            out = A["out"]
            rows_img = self._stats_rows(name, A)
            sratio = stats_check(st, out, out.shape[0] // rows_img)
        self.checks.append(dict(op=name, key=key, entry=(tuple(entry[:4]) if entry is not None else None), config=cfg,
                                ratio=ratio, stats_ratio=sratio))

    @staticmethod
    def _stats_rows(name, A):
        if name == "gemm":
            M = A["M"] if A["M"] is not None else A["a"].shape[0]
            return A["img_rows"] if A["img_rows"] and M % A["img_rows"] == 0 else M
        B, H, W = A["B"], A["H"], A["W"]
        if A.get("ups"):
            Ho, Wo = tuple(A["out_hw"]) if A.get("out_hw") is not None else (2 * H, 2 * W)
        elif A.get("stride", 1) == 2:
            Ho, Wo = (H + 1) // 2, (W + 1) // 2
        else:
            Ho, Wo = H, W
        return Ho * Wo

    # -- per entry point: (worst output ratio, statistics ratio or None)
    def _ref_gemm(self, A):
        a, w, out = A["a"], A["w"], A["out"]
        M = a.shape[0] if A["M"] is None else A["M"]
        K = (a.shape[-1] + (A["a2"].shape[-1] if A["a2"] is not None else 0)) if A["K"] is None else A["K"]
        N = w.shape[0] if A["N"] is None else A["N"]
        lda = a.stride(-2) if A["lda"] is None else A["lda"]
        ldo = out.stride(-2) if A["ldo"] is None else A["ldo"]
        batch = A["batch"]
        worst = 0.0
        if batch > 1:
            Nout = N // 2 if A["epilogue"] == 1 else N
            av = a.as_strided((batch, M, K), (A["strideA"], lda, 1), a.storage_offset())
            wv = w.as_strided((batch, N, K), (A["strideW"], K, 1), w.storage_offset())
            ov = out.as_strided((batch, M, Nout), (A["strideO"], ldo, 1), out.storage_offset())
            for z in _pick_images(batch, self.images):
                ref, bnd = gemm_reference(av[z], wv[z], bias=A["bias"], out_scale=A["out_scale"], epilogue=A["epilogue"])
                worst = max(worst, worst_ratio(ov[z], ref, bnd))
            return worst, None
        K1 = a.shape[-1] if A["a2"] is not None else K
        av = a.as_strided((M, K1), (lda, 1), a.storage_offset())
        Nout = N // 2 if A["epilogue"] == 1 else N
        ov = out.as_strided((M, Nout), (ldo, 1), out.storage_offset())
        m_img = A["img_rows"] if A["img_rows"] and M % A["img_rows"] == 0 else M
        for rows in _row_slices(M // m_img, m_img, self.images):
            ref, bnd = gemm_reference(av, w, a2=A["a2"], bias=A["bias"], rowadd=A["rowadd"], rows_per_batch=A["rows_per_batch"],
                                      res=A["res"], out_scale=A["out_scale"], epilogue=A["epilogue"], rows=rows)
            worst = max(worst, worst_ratio(ov[rows], ref, bnd))
        return worst, None

    def _ref_gemm_ln(self, A):
        a, out = A["a"], A["out"]
        M = a.shape[0]
        m_img = A["img_rows"] if A["img_rows"] and M % A["img_rows"] == 0 else M
        worst = 0.0
        for rows in _row_slices(M // m_img, m_img, self.images):
            ref, bnd = gemm_ln_reference(a, A["w"], A["ln_g"], A["ln_c"], eps=A["eps"], epilogue=A["epilogue"], rows=rows)
            worst = max(worst, worst_ratio(out[rows], ref, bnd))
        return worst, None

    def _ref_mlp_geglu(self, A):
        x, out = A["x"], A["out"]
        M = x.shape[0]
        m_img = A["img_rows"] if A["img_rows"] and M % A["img_rows"] == 0 else M
        worst = 0.0
        for rows in _row_slices(M // m_img, m_img, self.images):
            ref, bnd = mlp_geglu_reference(x, A["w1"], A["ln_g"], A["ln_c"], A["w2"], A["b2"], eps=A["eps"], rows=rows)
            worst = max(worst, worst_ratio(out[rows], ref, bnd))
        return worst, None

    def _ref_conv3x3(self, A):
        imgs = _pick_images(A["B"], self.images)
        w = A["w"]
        return conv_check(A["out"], A["x"], w, A["B"], A["H"], A["W"], C1=A["Cin"], bias=A["bias"], rowadd=A["rowadd"],
                          res=A["res"], stride=A["stride"], ups=A["ups"], out_hw=A["out_hw"], images=imgs), None

    def _ref_conv3x3_gn(self, A):
        imgs = _pick_images(A["B"], self.images)
        return conv_check(A["out"], A["x"], A["w"], A["B"], A["H"], A["W"], C1=A["C1"], x2=A["x2"], gn_scale=A["gn_scale"],
                          gn_shift=A["gn_shift"], silu=A["silu"], bias=A["bias"], rowadd=A["rowadd"], res=A["res"],
                          ups=A["ups"], images=imgs), None

    def _ref_conv3x3_smalln(self, A):
        imgs = _pick_images(A["B"], self.images)
        B, Hh, Ww, Cout = A["B"], A["H"], A["W"], A["Cout"]
        if A["mode"] == 0:
            got, fp16 = A["out"], False
        elif A["out_f32"] is not None:
            got, fp16 = A["out_f32"], False
        else:
            raise AssertionError("conv3x3_smalln mode 1 without a float copy: nothing exact to compare")
        got = got.reshape(B * Hh * Ww, Cout)
        return conv_check(got, A["x"], A["w"], B, Hh, Ww, C1=A["Cin"], gn_scale=A["gn_scale"], gn_shift=A["gn_shift"],
                          silu=A["silu"], bias=A["bias"], images=imgs, out_fp16=fp16), None

    def _ref_conv3x3_c4(self, A):
        B, Hh, Ww = A["B"], A["H"], A["W"]
        z, ez = c4_input(A["lat_f32"], A["pre_w"], A["pre_b"], A["in_scale"])
        worst = 0.0
        w = A["w"]
        dev = A["out"].device
        for b in _pick_images(B, self.images):
            for rows, Y, S, Eop in conv_bands(z[b].to(dev), ez[b].to(dev), w):
                E = acc_err(w.shape[1], S + Eop) + Eop
                v, E = _epilogue(Y, S + Eop, E, bias=_f64(A["bias"], dev))
                gr = slice(b * Hh * Ww + rows.start, b * Hh * Ww + rows.stop)
                worst = max(worst, worst_ratio(A["out"][gr], v, store_bound(v, E)))
        return worst, None

    def _ref_linear_rows(self, A):
        ref, bnd = linear_reference(A["x"], A["w"], A["M"], x_rows=A["x_rows"], bias=A["bias"], res=A["res"],
                                    res_rows=A["res_rows"], silu_in=A["silu_in"], silu_out=A["silu_out"])
        return worst_ratio(A["out"][:A["M"]], ref, bnd), None

    def _ref_linear_smallm(self, A):
        M = A["M"]
        x = A["x"] if A["ldx"] is None else A["x"].as_strided((M, A["K"]), (A["ldx"], 1), A["x"].storage_offset())
        out = A["out"] if A["ldo"] is None else A["out"].as_strided((M, A["N"]), (A["ldo"], 1), A["out"].storage_offset())
        ref, bnd = linear_reference(x[:M], A["w"], M, bias=A["bias"], res=A["res"], silu_in=A["silu_in"], silu_out=A["silu_out"])
        return worst_ratio(out[:M], ref, bnd), None

    def _ref_attention(self, A):
        d = A["d"]
        scale = d ** -0.5 if A["scale"] is None else A["scale"]
        return attention_check(A["out"], A["q"], A["k"], A["v"], A["B"], A["heads"], A["Sq"], A["Sk"], d, scale=scale,
                               causal=A["causal"], images=_pick_images(A["B"], self.images)), None


def config_table(checks):
    """rows (kind, bm, bn, splits, variant) -> [launches checked, worst ratio, worst statistics ratio]."""
    rows = {}
    for c in checks:
        if c["config"] is None:
            continue
        r = rows.setdefault(c["config"], [0, 0.0, 0.0])
        r[0] += 1
        r[1] = max(r[1], c["ratio"])
        if c["stats_ratio"] is not None:
            r[2] = max(r[2], c["stats_ratio"])
    return rows
