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

The other entry points of a pass (``CHECKED``: norms, softmax, gathers, time embedding, sampler step, pooling, tiled-decode
glue) are checked the same way, each from its operands as they were BEFORE the launch (every tensor argument is copied first:
several of them write in place), and each also checks that what the launch must not write is unchanged.

GroupNorm statistics.  Of one (image, group) of n = HW * cpg fp16 values, from the STORED tensors (both sources of a fused
concat).  The kernels sum x and x^2 in fp32 (32-row slabs of the producer epilogue, or the row chunks of the standalone
statistics pass: at most 33 roundings each, stats_check), combine the partials in a fixed order (<= n terms) and take the
one-pass variance var = q / n - mean^2 in fp32.  With Q = q / n = var + mean^2:

    E_mean = A(n) U mean|x| + 2 U |mean|                      A(n) = 33 + C_ACC sqrt(n)
    E_var  = (A(n) + 1 + ONE_PASS_C) U Q + 2 |mean| E_mean + E_mean^2      ONE_PASS_C = 3 (q / n, mean^2, the subtraction)

Q = kappa (var + eps): the error of the variance relative to what rstd = rsqrt(var + eps) sees grows with
kappa = (var + mean^2) / (var + eps).  rstd is off by rel_r (the perturbed-variance form of _ln_product, + 4 U for rsqrtf);
scale = gamma rstd is off by |scale| (rel_r + U), shift = beta - mean scale by |mean| E_scale + |scale| E_mean + 2 U (|mean
scale| + |shift|).  The apply pass adds one fma rounding and the SiLU (exp2 / rcp approximations: 8 U |v|, slope <= 1.1).

Tripwire.  The one-pass term alone, (ONE_PASS_STAT + ONE_PASS_C) U kappa relative to var + eps (the slab sum of squares and
the three roundings at the magnitude Q), moves rstd by half that and so the normalised output by half that relative to
itself.  A quarter of an fp16 ulp is at least 2^-13 relative, hence every GroupNorm launch must keep

    kappa <= KAPPA_TRIP = 2^-12 / ((ONE_PASS_STAT + ONE_PASS_C) U) = 2^12 / 36 ~= 114

beyond which the variance must be computed without cancellation (slab (count, mean, M2) combined in Chan's form).

LayerNorm (two-pass, one wave per row): E_mean = C_ACC sqrt(C) U mean|x| + U |mean|; centred on the kernel's mean the sum of
squares gains exactly C E_mean^2 (the cross term vanishes about the exact mean), so E_var = (C_ACC sqrt(C) + 4) U var +
E_mean^2; rstd as above; (x - mean) rstd gamma + beta adds E_mean rstd |gamma| and four roundings per element.
Row softmax: exp of a fp32 difference (relative error U |v - m| + 2 U, __expf), an fp32 sum of n positive terms
(C_ACC sqrt(n) U), a reciprocal and a product: relative error (2 max|v - m| + C_ACC sqrt(n) + 8) U, then the fp16 store;
padding columns written as exact zeros.  Gathers (transpose, token + position embedding) are exact: the embedding adds two
fp16 values in fp32 and rounds once, which IS the reference fl16(fl32(a + b)).  Time embedding: the argument t 10000^(-k/half)
is formed in fp32 from exp of a rounded exponent: relative error (3 |ln(10^4) k / half| + 4) U, i.e. an absolute error of
that times |t f| in the argument; cos / sin add 4 U; then the fp16 store.  Sampler step: one rounding per operation, each
bounded by U times the magnitude it produces (sampler_step_reference), never relative to the result (x0 divides by
sqrt(alpha_t) ~ 0.07 at t = 999).  latents_pool8: L-term fp32 bin sums, (L + 1) U mean|x| before the fp16 store.
vae_blend: 4 U (|a| + |b|).  vae_place_tile: the fp32 copy is exact, the u8 value is round-half-even(clamp(v/2 + 1/2) 255)
except within 4 U 255 of a .5 tie, where either neighbour is accepted (and counted).

ControlNet hint stack (hint_conv_u8 / hint_conv: one fp32 chain per output, no K split).  E_acc = acc_err(K, S) with K the
number of non-zero K slots (54 for the u8 layer: 27 hi + 27 lo); the u8 layer's operand x = u8 / 255 is one fp32 division
(U |x|) carried as fp16 hi + lo (2^-21 |x|), entering E through sum err |w|; the bias is the accumulator's first term (one
rounding at the magnitude of the sum and of the bias); SiLU 1.1 E + 8 U |v|; then the fp16 store.  conv3x3_c4_res is
conv3x3_c4 without the pre-transform (K = 72 slots: 36 hi + 36 lo) and with the fp16 residual added in fp32 BEFORE the one
fp16 rounding: a conv rounded to fp16 first carries H |conv| more, which the bound does not hold.
Re-noise: fl(fma(sb, n, fl(sa x))): two roundings, each at most U times a magnitude below |sa x| + |sb n| + their own
error: 4 U (|sa x| + |sb n|) (tests/refine_reference.py).  Hand-over step: x^k is the `last` form of the sampler step
(sampler_step_reference, bound E_k), lat its re-noise: 4 U (|nsa x^k| + |nsb n|) + |nsa| E_k.  With dup the copy written in
front of ``lat`` (the other classifier-free-guidance half) must equal it bit for bit.

What a contraction launch must not write (``HOOKED``).  Every tensor argument is copied before the launch; afterwards every
argument that does not share storage with ``out`` is bit-identical, and so is every element of ``out``'s storage window
outside the logical [batch, rows, columns] extent of the launch: the window runs from (ldo - columns) elements before the
first output element (the gap columns in front of a column slice) to the end of the last row's pitch or of the tensor passed,
whichever is further (rows past M, gap columns of the written rows).
"""
from __future__ import annotations

import inspect
import math

import numpy as np
import torch

U = 2.0 ** -24          # fp32 unit roundoff
H = 2.0 ** -11          # fp16 unit roundoff: half an ulp relative to the value
SUB = 2.0 ** -25        # half the fp16 subnormal step
C_ACC = 8.0             # multiple of sqrt(K) * U * S allowed for fp32 accumulation (see above)
GELU_APPROX = 1e-7      # |gelu_erf_f(x) - gelu(x)| / |x|: Abramowitz-Stegun 7.1.26 erf (|err| <= 1.5e-7) times x / 2
BAND_BYTES = 1 << 30    # working set of one im2col band (three fp64 copies of it live at once)
LN2 = math.log(2.0)
ONE_PASS_STAT = 33      # roundings of one fp32 slab sum of squares (stats_check)
ONE_PASS_C = 3          # q / n, mean^2 and their difference, all at the magnitude Q = var + mean^2
KAPPA_TRIP = 2.0 ** -12 / ((ONE_PASS_STAT + ONE_PASS_C) * U)     # ~= 113.8 (module docstring)


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


def same_bits(a, b):
    """bit-identical (NaN payloads of never-written scratch compare equal to themselves)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.is_floating_point():
        it = {2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
        a, b = a.view(it), b.view(it)
    return torch.equal(a, b)


def tail_same(after, before, n):
    """the elements of ``after`` past the first n (flattened) are those of ``before``: a launch that writes a logical prefix
    of a larger buffer must leave the rest of it alone."""
    return same_bits(after.reshape(-1)[n:], before.reshape(-1)[n:])


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
P_SUBNORMAL = 14.0      # a probability more than 2^-14 below its row's largest may be stored as an fp16 subnormal


def attention_kernel(d, Sk, causal):
    """which kernel of csrc/attention.hip serves a call (lcm_attention_f16, default switches): "attn2" the streaming kernel of
    the long non-causal sequences, "wide" the d = 512 kernel, "attn" the register-staged kernel of everything else."""
    if not causal and Sk >= 128 and d in (40, 64, 80):
        return "attn2"
    return "wide" if d == 512 else "attn"


def attention_tile(d, Sk, causal):
    """keys per K/V tile of the kernel that serves the call"""
    return 32 if attention_kernel(d, Sk, causal) == "wide" else 64


def attention_key_split(d, Sk, causal):
    """True where the streaming kernel splits the keys of a query block over two wave groups (launch_attn2, default switches):
    tiles [0, ceil(n / 2)) and [ceil(n / 2), n)."""
    return attention_kernel(d, Sk, causal) == "attn2" and 1024 <= Sk <= 4096


def attention_rounds_q(d, Sk, causal, scale):
    """True where the launch rounds a SCALED Q to fp16: the streaming kernel called with scale > 0 (x = (half)(x * sc)).  With
    scale <= 0 it multiplies by 1.0 (exact); the other two kernels multiply the fp32 accumulator by the scale."""
    return scale > 0 and attention_kernel(d, Sk, causal) == "attn2"


def attention_check(got, q, k, v, B, heads, Sq, Sk, d, *, scale, causal=False, images=None, chunk_bytes=1 << 29, q_rounded=None):
    """softmax(Q K^T * scale) V in fp64 (scale <= 0: Q carries scale * log2 e, the logits are base-2).  Bound, per query row.

    Logits.  With A = max_j sum_i |q_i k_ji| * scale and |L| = max_j |logit_j| (natural units) a logit is off by at most
        D = (h_q + C_ACC U sqrt(d)) A + 4 U |L|
    h_q = H where the launch rounds the scaled Q to fp16 (attention_rounds_q: the streaming kernel with scale > 0), else 0:
    nothing is rounded before the fp32 accumulation.  The predicate assumes the default switches; under set_attention_impl(0) or
    2 forced waves the register-staged kernel serves those shapes and rounds nothing, so the predicate errs towards the looser
    bound, never the tighter.  q_rounded overrides it (tests/test_launch_audit.py: what the term hides where it does not belong).
    C_ACC U sqrt(d) A is that accumulation.  4 U |L| covers the fp32 roundings of s * sc and s - m (at most 3 U |L|, |s - m| <=
    2 |L|) and, in the d = 40 streaming form, the running max carried in the QK^T MFMA as an fp16 (hi, lo) split of -m: hi + lo
    is -m to 2^-22 |m| = 4 U |m|; the tile that moves the max subtracts the exact fp32 delta while every later tile sees the
    split, so the two disagree by up to 2^-22 |m| with |m| <= |L| (base-2 units need |m| < 65504, the fp16 range of hi).
    D moves each unnormalised probability by a factor within exp(+-D).

    P is rounded to fp16 for the PV product (the streaming kernel defers its rescale, so P <= 2^8: still H relative); the
    online rescales are Sk / 32 fp32 multiplications at most; O and l accumulate in fp32:
        E = (2 (e^(2D) - 1) + 2 H + (2 C_ACC sqrt(Sk) + Sk / 32 + 8) U) * sum_j p_j |v_j| + E_sub
    E_sub, the fp16-subnormal range of P.  In the units of the running max at its tile the largest P so far is >= 1 (the max
    never exceeds the largest score seen), so l >= 1 from there on and later rescales multiply P's error and l alike by a
    factor <= 1.  A key whose score is within 2^-14 of the row's largest has P >= 2^-14, a normal fp16.  Every other unmasked key
    (set J) is off by at most SUB absolute -- also when it flushes to 0 -- which moves the numerator by SUB sum_J |v_j| and l by
    SUB |J|:
        E_sub = SUB (sum_J |v_j| + |J| |o|)
    then the fp16 store (store_bound)."""
    dev = got.device
    s = LN2 if scale <= 0 else scale
    h_q = H if (attention_rounds_q(d, Sk, causal, scale) if q_rounded is None else q_rounded) else 0.0
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
                D = (h_q + C_ACC * U * math.sqrt(d)) * La.max(1, keepdim=True).values + 4 * U * L.abs().nan_to_num(0, 0, 0).max(1, keepdim=True).values
                rel = 2 * torch.expm1(2 * D) + 2 * H + (2 * C_ACC * math.sqrt(Sk) + Sk / 32 + 8) * U
                J = (torch.isfinite(L) & (L < L.max(1, keepdim=True).values - P_SUBNORMAL * LN2)).to(torch.float64)
                E = rel * pv + SUB * (J @ V.abs() + J.sum(1, keepdim=True) * o.abs())
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


# ---- GroupNorm / LayerNorm ---------------------------------------------------------------------------------------------
def _rel_rstd(v, E_var, eps):
    """relative error of rsqrtf(var' + eps) with |var' - var| <= E_var, v = var + eps (fp64)."""
    return torch.sqrt(v / torch.clamp(v - E_var, min=eps)) - 1.0 + 4 * U


def gn_group_stats(xs, b, HW, groups):
    """fp64 statistics of image b of the concat of the fp16 sources ``xs`` ([B*HW, Ci] each) -> (x [HW, C] fp64, mean, var,
    Q = E[x^2], mean|x|) per group, n = HW * C / groups."""
    x = torch.cat([s[b * HW:(b + 1) * HW].to(torch.float64) for s in xs], 1)
    g = x.reshape(HW, groups, -1)
    mean = g.mean((0, 2))
    var = ((g - mean[None, :, None]) ** 2).mean((0, 2))
    return x, mean, var, (g * g).mean((0, 2)), g.abs().mean((0, 2))


def gn_tables_reference(mean, var, Q, amean, n, gamma, beta, eps):
    """(scale, shift) [C] fp64 of one image with their error bounds and kappa per group (module docstring)."""
    A = 33 + C_ACC * math.sqrt(n)
    E_mean = A * U * amean + 2 * U * mean.abs()
    E_var = (A + 1 + ONE_PASS_C) * U * Q + 2 * mean.abs() * E_mean + E_mean * E_mean
    v = var + eps
    rel_r = _rel_rstd(v, E_var, eps)
    cpg = gamma.numel() // mean.numel()
    r = lambda t: t.repeat_interleave(cpg)
    g, bt = gamma.to(torch.float64), beta.to(torch.float64)
    scale = g / torch.sqrt(r(v))
    shift = bt - r(mean) * scale
    E_scale = scale.abs() * (r(rel_r) + U)
    E_shift = r(mean).abs() * E_scale + scale.abs() * r(E_mean) + 2 * U * ((r(mean) * scale).abs() + shift.abs())
    return scale, shift, E_scale + 1e-38, E_shift + 1e-38, Q / v


def gn_apply_reference(x, scale, shift, E_scale, E_shift, silu):
    """y = act(x scale + shift) of one image (x [HW, C] fp64) -> (ref, bound) for the fp16 output."""
    v = x * scale + shift
    E = x.abs() * E_scale + E_shift + U * v.abs()
    if silu:
        y = v * torch.sigmoid(v)
        E = 1.1 * E + 8 * U * v.abs()
    else:
        y = v
    return y, store_bound(y, E)


def gn_check(got_scale, got_shift, xs, B, HW, groups, gamma, beta, eps, *, out=None, silu=True, images=None):
    """Worst ratio of the tables (and of the applied output ``out`` [B*HW, C] if given) of a GroupNorm launch, worst kappa."""
    C = sum(s.shape[1] for s in xs)
    n = HW * (C // groups)
    worst, kap = 0.0, 0.0
    for b in (range(B) if images is None else images):
        x, mean, var, Q, amean = gn_group_stats(xs, b, HW, groups)
        sc, sh, Es, Eh, k = gn_tables_reference(mean, var, Q, amean, n, gamma.to(x.device), beta.to(x.device), eps)
        kap = max(kap, float(k.max()))
        if got_scale is not None:
            worst = max(worst, worst_ratio(got_scale[b], sc, Es), worst_ratio(got_shift[b], sh, Eh))
        if out is not None:
            ref, bnd = gn_apply_reference(x, sc, sh, Es, Eh, silu)
            worst = max(worst, worst_ratio(out[b * HW:(b + 1) * HW], ref, bnd))
    return worst, kap


def layernorm_reference(x, gamma, beta, eps):
    """two-pass LayerNorm of fp16 rows x [M, C] -> (ref, bound) fp64."""
    X = x.to(torch.float64)
    C = X.shape[1]
    mean = X.mean(1, keepdim=True)
    d = X - mean
    var = (d * d).mean(1, keepdim=True)
    E_mean = C_ACC * math.sqrt(C) * U * X.abs().mean(1, keepdim=True) + U * mean.abs()
    E_var = (C_ACC * math.sqrt(C) + 4) * U * var + E_mean * E_mean
    v = var + eps
    rel_r = _rel_rstd(v, E_var, eps)
    g, bt = gamma.to(x.device, torch.float64), beta.to(x.device, torch.float64)
    rstd = 1.0 / torch.sqrt(v)
    core = d * rstd * g
    y = core + bt
    E = (E_mean + U * d.abs()) * rstd * g.abs() + core.abs() * (rel_r + 2 * U) + U * (y.abs() + bt.abs())
    return y, store_bound(y, E)


# ---- row softmax, gathers, time embedding --------------------------------------------------------------------------------
def softmax_reference(x, n):
    """softmax over the first n columns of fp16 rows x [R, ld] -> (ref [R, n], bound)."""
    X = x[:, :n].to(torch.float64)
    m = X.max(1, keepdim=True).values
    P = torch.softmax(X, 1)
    spread = (X - m).abs()
    rel = (spread + 2 * spread.max(1, keepdim=True).values + C_ACC * math.sqrt(n) + 8) * U
    return P, store_bound(P, rel * P)


def embed_reference(ids, tok, pos, B, S):
    """CLIP token + position embedding, ids clamped to the vocabulary: fl16(fl32(tok + pos)) (exact: one rounding)."""
    idx = ids.reshape(-1).long().clamp(0, tok.shape[0] - 1)
    p = pos[:S].repeat(B, 1)
    return (tok[idx].to(torch.float64) + p.to(torch.float64)).to(torch.float32).to(torch.float16)


def timestep_reference(ts, B, dim, half_exp=None):
    """rows step-major [len(ts) * B, dim]: cos | sin of t 10000^(-k / half) -> (ref, bound).  half_exp: the exponent's
    denominator (default half; the CPU self-test passes a wrong one)."""
    half = dim // 2
    k = torch.arange(half, dtype=torch.float64)
    expo = math.log(10000.0) * k / (half if half_exp is None else half_exp)
    f = torch.exp(-expo)
    t = torch.tensor([float(np.float32(v)) for v in ts], dtype=torch.float64).repeat_interleave(B)[:, None]
    a = t * f[None, :]
    Ea = a.abs() * (3 * expo + 4)[None, :] * U
    ref = torch.cat([torch.cos(a), torch.sin(a)], 1)
    E = torch.cat([Ea, Ea], 1) + 4 * U
    return ref, store_bound(ref, E)


# ---- sampler step --------------------------------------------------------------------------------------------------------
def sampler_step_reference(m, lat, noise, coef6, last, *, m_u=None, guidance=1.0, pred="epsilon"):
    """LCMScheduler.step in fp64 from the fp32 operands: m / m_u NHWC [B, h, w, 4] model output(s), lat / noise NCHW, coef6 as
    the kernel receives them (fp32) -> (new lat NCHW, bound).  Every rounding is bounded by U times the magnitude of what that
    operation produces (the terms, not the result: the epsilon form divides by sqrt(alpha_t))."""
    c = [float(np.float32(v)) for v in coef6]
    sa, sb, c_skip, c_out, sap, sbp = c
    M = m.to(torch.float64).permute(0, 3, 1, 2)
    X = lat.to(torch.float64)
    if m_u is not None:
        Mu = m_u.to(torch.float64).permute(0, 3, 1, 2)
        g = float(np.float32(guidance))
        d = M - Mu
        M = Mu + g * d
        E_m = U * (d.abs() + 2 * abs(g) * d.abs() + M.abs())
    else:
        E_m = torch.zeros_like(M)
    if pred == "epsilon":
        num = X - sb * M
        E_num = sb * E_m + U * (sb * M.abs() + num.abs())
        x0 = num / sa
        E_x0 = E_num / sa + 2 * U * x0.abs()
    elif pred == "v_prediction":
        x0 = sa * X - sb * M
        E_x0 = sb * E_m + 2 * U * (sa * X.abs() + sb * M.abs()) + U * x0.abs()
    else:
        x0, E_x0 = M, E_m
    den = c_out * x0 + c_skip * X
    E = abs(c_out) * E_x0 + 2 * U * (abs(c_out * 1.0) * x0.abs() + abs(c_skip) * X.abs()) + U * den.abs()
    if last:
        return den, 2 * E + 1e-38
    N = noise.to(torch.float64)
    out = sap * den + sbp * N
    E = abs(sap) * E + 2 * U * (abs(sap) * den.abs() + abs(sbp) * N.abs()) + U * out.abs()
    return out, 2 * E + 1e-38


# ---- latents preview pooling, tiled-decode glue --------------------------------------------------------------------------
def pool8_bins(n):
    """adaptive_avg_pool2d bins of an n-long side into 8: [floor(o n / 8), ceil((o + 1) n / 8))."""
    return [(o * n // 8, -(-(o + 1) * n // 8)) for o in range(8)]


def pool8_reference(lat, bins_h=None, bins_w=None):
    """lat fp32 [B, 4, h, w] -> (ref [B, 4, 8, 8], bound) for the fp16 output."""
    L = lat.to(torch.float64)
    bh, bw = bins_h or pool8_bins(L.shape[2]), bins_w or pool8_bins(L.shape[3])
    ref = torch.empty(L.shape[0], 4, 8, 8, dtype=torch.float64, device=L.device)
    E = torch.empty_like(ref)
    for oy, (y0, y1) in enumerate(bh):
        for ox, (x0, x1) in enumerate(bw):
            blk = L[:, :, y0:y1, x0:x1]
            cnt = (y1 - y0) * (x1 - x0)
            ref[:, :, oy, ox] = blk.mean((2, 3))
            E[:, :, oy, ox] = (cnt + 1) * U * blk.abs().mean((2, 3))
    return ref, store_bound(ref, E)


def blend_reference(a, b, extent, vertical):
    """diffusers blend_v / blend_h of tile a into the first ``extent`` rows / columns of tile b (fp32 [B, h, w, 3])
    -> (b after, bound on the band, band mask)."""
    A, Bt = a.to(torch.float64), b.to(torch.float64)
    out = Bt.clone()
    dev = Bt.device
    t = torch.arange(extent, dtype=torch.float64, device=dev) / extent
    if vertical:
        av, bv = A[:, A.shape[1] - extent:], Bt[:, :extent]
        out[:, :extent] = av * (1 - t[None, :, None, None]) + bv * t[None, :, None, None]
    else:
        av, bv = A[:, :, A.shape[2] - extent:], Bt[:, :, :extent]
        out[:, :, :extent] = av * (1 - t[None, None, :, None]) + bv * t[None, None, :, None]
    bnd = torch.full_like(out, 1e-38)
    band = torch.zeros_like(out, dtype=torch.bool)
    if vertical:
        bnd[:, :extent] = 4 * U * (av.abs() + bv.abs()) + 1e-38
        band[:, :extent] = True
    else:
        bnd[:, :, :extent] = 4 * U * (av.abs() + bv.abs()) + 1e-38
        band[:, :, :extent] = True
    return out, bnd, band


def rgb8_reference(v):
    """fp32 image values -> (u8 round-half-even(clamp(v/2 + 1/2, 0, 1) 255) as int64, mask of near-ties)."""
    r = torch.clamp(v.to(torch.float64) * 0.5 + 0.5, 0.0, 1.0) * 255.0
    u8 = torch.round(r)
    tie = ((r - torch.floor(r)) - 0.5).abs() <= 4 * U * 255.0
    return u8.to(torch.int64), tie


def rgb8_check(got_u8, v):
    """-> (number of pixels off by more than the tie allowance, number of near-tie pixels off by one)."""
    ref, tie = rgb8_reference(v)
    d = (got_u8.to(ref.device, torch.int64) - ref).abs()
    return int(((d > 0) & ~tie).sum() + (d > 1).sum()), int(((d == 1) & tie).sum())


def tiled_glue_reference(tiles, sample, H, W, overlap=0.25):
    """diffusers AutoencoderKL.tiled_decode glue from the decoded tiles {(i, j): fp32 [B, th, tw, 3]} (tile order: rows of
    tiles top to bottom): blend above, then left, with the already-blended neighbours; extent = min(a, b, extent); each tile
    cropped to ``limit`` and the rows concatenated -> (image fp64 [B, H, W, 3], bound)."""
    extent = int(sample * overlap)
    limit = sample - extent
    ni = 1 + max(i for i, _ in tiles)
    nj = 1 + max(j for _, j in tiles)
    res = {k: t.to(torch.float64) for k, t in tiles.items()}
    err = {k: torch.zeros_like(t) for k, t in res.items()}
    rows = []
    for i in range(ni):
        cols = []
        for j in range(nj):
            t, e = res[(i, j)], err[(i, j)]
            for vertical, nb in ((True, (i - 1, j)), (False, (i, j - 1))):
                if min(nb) < 0:
                    continue
                a, ea = res[nb], err[nb]
                ext = min(a.shape[1 if vertical else 2], t.shape[1 if vertical else 2], extent)
                new, bnd, band = blend_reference(a, t, ext, vertical)
                w = torch.arange(ext, dtype=torch.float64, device=t.device) / ext
                if vertical:
                    ws = (1 - w)[None, :, None, None]
                    e = e.clone()
                    e[:, :ext] = ea[:, a.shape[1] - ext:] * ws + e[:, :ext] * (1 - ws)
                else:
                    ws = (1 - w)[None, None, :, None]
                    e = e.clone()
                    e[:, :, :ext] = ea[:, :, a.shape[2] - ext:] * ws + e[:, :, :ext] * (1 - ws)
                t, e = new, e + torch.where(band, bnd, torch.zeros_like(bnd))
            res[(i, j)], err[(i, j)] = t, e
            cols.append((t[:, :limit, :limit], e[:, :limit, :limit]))
        rows.append((torch.cat([c[0] for c in cols], 2), torch.cat([c[1] for c in cols], 2)))
    img = torch.cat([r[0] for r in rows], 1)[:, :H, :W]
    E = torch.cat([r[1] for r in rows], 1)[:, :H, :W]
    return img, E + 1e-38



# ---- ControlNet hint stack -------------------------------------------------------------------------------------------------
HINT_U8_K = 54          # non-zero K slots of hint_conv_u8: 27 hi + 27 lo


def hint_u8_input(img_u8, dev=None, lo=True):
    """hint_conv_u8's operand: x = u8 / 255 (one fp32 division) carried as fp16 hi + lo -> (x [B, H, W, 3] fp64, its error).
    lo=False: the error of a single fp16 (what the bound must NOT be: the CPU self-test)."""
    x = img_u8.to(dev if dev is not None else img_u8.device, torch.float64) / 255.0
    return x, ((2.0 ** -21 if lo else H) + U) * x.abs()


def hint_layer_check(got, xin64, xerr, w, bias, B, Hh, Ww, stride, silu, K_eff, images=None):
    """Worst |got - ref| / bound of one hint layer (hint_conv_u8 / hint_conv / the stack's last conv): xin64 [B, H, W, Cin] fp64
    the layer's own stored input, xerr its operand error or None, got [B * Ho * Wo, Cout] (module docstring)."""
    Ho, Wo = ((Hh + 1) // 2, (Ww + 1) // 2) if stride == 2 else (Hh, Ww)
    worst = 0.0
    b64 = bias.to(got.device, torch.float64) if bias is not None else None
    for b in (range(B) if images is None else images):
        xe = None if xerr is None else xerr[b]
        for rows, Y, S, Eop in conv_bands(xin64[b], xe, w, stride=stride):
            E = acc_err(K_eff, S)
            if Eop is not None:
                E = E + Eop + acc_err(K_eff, Eop)
            v = Y
            if b64 is not None:
                v = Y + b64
                E = E + U * (v.abs() + b64.abs())
            if silu:
                E = 1.1 * E + 8 * U * v.abs()
                v = v * torch.sigmoid(v)
            gr = slice(b * Ho * Wo + rows.start, b * Ho * Wo + rows.stop)
            worst = max(worst, worst_ratio(got[gr], v, store_bound(v, E)))
    return worst


C4_RES_K = 72           # non-zero K slots of conv3x3_c4_res: 36 hi + 36 lo


def conv_c4_res_check(got, lat, w, bias, res, B, Hh, Ww, images=None):
    """conv3x3_c4_res: conv3x3 of the fp32 NCHW latents (hi + lo operand) + bias + res fp16 [B*H*W, Cout], the residual added
    in fp32 before the single fp16 rounding."""
    dev = got.device
    z, ez = c4_input(lat[:B], None, None, 1.0)
    worst = 0.0
    for b in (range(B) if images is None else images):
        for rows, Y, S, Eop in conv_bands(z[b].to(dev), ez[b].to(dev), w):
            E = acc_err(C4_RES_K, S + Eop) + Eop
            gr = slice(b * Hh * Ww + rows.start, b * Hh * Ww + rows.stop)
            v, E = _epilogue(Y, S + Eop, E, bias=_f64(bias, dev), res=_f64(res[gr], dev))
            worst = max(worst, worst_ratio(got[gr], v, store_bound(v, E)))
    return worst


# ---- multi-pass refinement: re-noise and the hand-over step ----------------------------------------------------------------
def renoise_reference(x, n, sa, sb):
    """lat = sa x + sb n from the fp32 operands (coefficients as the kernel receives them) -> (ref, bound)."""
    sa, sb = float(np.float32(sa)), float(np.float32(sb))
    X, N = x.to(torch.float64), n.to(torch.float64)
    return sa * X + sb * N, 4 * U * ((sa * X).abs() + (sb * N).abs()) + 1e-38


def _halves_ratio(lat, B, ref, bnd, dup):
    """lat [>= B (2B with dup), 4, h, w] after the launch: the first B images against (ref, bnd); with dup images [B, 2B) must
    equal them bit for bit (inf otherwise)."""
    r = worst_ratio(lat[:B], ref, bnd)
    if dup and not same_bits(lat[B:2 * B], lat[:B]):
        return math.inf
    return r


def renoise_check(lat, x0, noise, sa, sb, B, dup):
    ref, bnd = renoise_reference(x0[:B], noise[:B], sa, sb)
    return _halves_ratio(lat, B, ref.to(lat.device), bnd.to(lat.device), dup)


def handover_reference(m, lat, noise, coef6, nsa, nsb, *, m_u=None, guidance=1.0, pred="epsilon"):
    """-> (x^k, its bound, the re-noised state, its bound): the `last` sampler step, then the re-noise of ITS result."""
    xk, Ek = sampler_step_reference(m, lat, None, coef6, True, m_u=m_u, guidance=guidance, pred=pred)
    ref, bnd = renoise_reference(xk, noise, nsa, nsb)
    return xk, Ek, ref, bnd + abs(float(np.float32(nsa))) * Ek


def handover_check(xk, state, front, m, lat0, noise, coef6, nsa, nsb, B, *, m_u=None, guidance=1.0, pred="epsilon"):
    """xk / state [B, 4, h, w] after the launch, front: the copy in front of the state (dup) or None; lat0 the state before."""
    rx, bx, rl, bl = handover_reference(m[:B], lat0[:B], noise[:B], coef6, nsa, nsb, m_u=None if m_u is None else m_u[:B],
                                        guidance=guidance, pred=pred)
    dev = xk.device
    r = max(worst_ratio(xk[:B], rx.to(dev), bx.to(dev)), worst_ratio(state[:B], rl.to(dev), bl.to(dev)))
    if front is not None and not same_bits(front[:B], state[:B]):
        return math.inf
    return r


# ---- what a contraction launch must not write ------------------------------------------------------------------------------
def storage_numel(t):
    return t.untyped_storage().nbytes() // t.element_size()


def out_window(out, rows, cols, ld, batch=1, stride_o=0):
    """The window of ``out``'s storage a launch that writes [batch, rows, cols] at pitch ld (batch stride stride_o) from out's
    first element is answerable for -> (start, length, keep): keep[i] True where storage element start + i is NOT part of the
    logical output (module docstring)."""
    off = out.storage_offset()
    view_end = off + 1 + sum((n - 1) * st for n, st in zip(out.shape, out.stride())) if out.numel() else off
    logical_end = off + (batch - 1) * stride_o + rows * ld
    start = max(0, off - max(0, ld - cols))
    end = min(storage_numel(out), max(view_end, logical_end))
    keep = torch.ones(end - start, dtype=torch.bool, device=out.device)
    keep.as_strided((batch, rows, cols), (stride_o, ld, 1), off - start).fill_(False)
    return start, end - start, keep


def window_of(t, start, length):
    return t.as_strided((length,), (1,), start)


def frame_writes(before, after, view):
    """number of elements of a whole buffer OUTSIDE the strided ``view`` into it whose bits changed (``before``: the buffer
    cloned ahead of the launch): rows in front of and behind the output as well as the gap columns."""
    keep = torch.ones(after.numel(), dtype=torch.bool, device=after.device)
    keep.as_strided(view.shape, view.stride(), view.storage_offset() - after.storage_offset()).fill_(False)
    return stray_writes(before.reshape(-1), after.reshape(-1), keep)


def stray_writes(before, after, keep):
    """number of elements of the window outside the logical output whose bits changed."""
    it = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[before.element_size()]
    return int(((before.view(it) != after.view(it)) & keep).sum())


# ---- the hook ----------------------------------------------------------------------------------------------------------
HOOKED = ("gemm", "gemm_ln", "mlp_geglu", "conv3x3", "conv3x3_gn", "conv3x3_smalln", "conv3x3_c4", "linear_rows",
          "linear_smallm", "attention", "hint_conv_u8", "hint_conv", "conv3x3_c4_res")
WRITES = {"conv3x3_smalln": ("out", "out_f32")}      # HOOKED entry points that write more than ``out``
# the other entry points of a pass -> the arguments each one writes (all others must come out of the launch unchanged);
# "ws" is scratch of the standalone GroupNorm forms (partials + tables: any of it may change)
CHECKED = {"groupnorm_tables_from_stats": ("ws",), "groupnorm": ("out", "ws"), "groupnorm_from_stats": ("out", "ws"),
           "layernorm": ("out",), "softmax_rows": ("x",), "transpose": ("out",), "embed_tokens": ("out",),
           "timestep_embedding": ("out",), "timestep_embedding_steps": ("out",), "scheduler_step": ("lat",),
           "latents_pool8": ("out",), "vae_blend": ("b",), "vae_place_tile": ("out_u8", "out_f32"),
           "latents_renoise": ("lat",), "scheduler_step_handover": ("lat", "xk")}
REFINE_ENTRIES = ("latents_renoise", "scheduler_step_handover")     # reached by refinement chains only (passes > 0)
GN_ENTRIES = ("groupnorm_tables_from_stats", "groupnorm", "groupnorm_from_stats")


def _pick_images(n, limit):
    """images checked of an n-image launch: all up to ``limit``, else the first and the last (the batch borders)."""
    return list(range(n)) if limit is None or n <= limit else [0, n - 1]


def _row_slices(n_img, rows_img, images):
    return [slice(b * rows_img, (b + 1) * rows_img) for b in _pick_images(n_img, images)]


def _ident(k, v):
    """what identifies a launch's shape: tensor shapes / strides, flags, scalars (not the data, not the statistics buffer)"""
    if torch.is_tensor(v):
        return k, tuple(v.shape), tuple(v.stride())
    if k in ("stats", "st1", "st2"):
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
        self.stats_src = {}                  # id(ops.Stats) -> the [rows, C] tensor whose statistics it holds (last producer)

    def __enter__(self):
        from sdlcm_amd import ops
        self._ops = ops
        self._saved = {n: getattr(ops, n) for n in HOOKED + tuple(CHECKED)}
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
            if A.get("stats") is not None:
                self.stats_src[id(A["stats"])] = self._stats_tensor(name, A)
            ident = (name,) + tuple(_ident(k, v) for k, v in A.items())
            if name in GN_ENTRIES:          # every layer once (its statistics differ, not only its shape)
                ident += (A["gamma"].data_ptr(),)
            if ident in self.seen:
                return real(*args, **kw)
            self.seen.add(ident)
            if name in CHECKED:
                return self._launch_checked(name, real, args, kw, A)
            out = A["out"]
            writes = WRITES.get(name, ("out",))
            before = {k: v.clone() for k, v in A.items() if torch.is_tensor(v) and k not in writes}
            shared = {k for k in before if A[k].untyped_storage().data_ptr() == out.untyped_storage().data_ptr()}
            ext = self._out_extent(name, A)
            w_start, w_len, w_keep = out_window(out, *ext)
            w_before = window_of(out, w_start, w_len).clone()
            n0 = len(self.recs)
            r = real(*args, **kw)
            if out.is_cuda:
                torch.cuda.current_stream().synchronize()
            stray = []
            for k, v in before.items():       # what the launch must not write: every operand outside the output's storage
                if k not in shared and not same_bits(A[k], v):
                    stray.append(f"operand {k} changed by the launch")
            n_out = stray_writes(w_before, window_of(out, w_start, w_len), w_keep)
            if n_out:
                stray.append(f"operand out: {n_out} elements outside the logical [{ext[3]} x {ext[0]} x {ext[1]}] output (pitch "
                             f"{ext[2]}) changed by the launch")
            for k in shared:                  # inputs sharing the output's storage: the reference needs them as they were
                A[k] = before[k]
            rec = self.recs[n0] if len(self.recs) > n0 else (None, None, None)
            self._check(name, A, rec[0], rec[1] or {}, stray)
            del before, w_before, w_keep, A
            return r
        return hooked

    @staticmethod
    def _out_extent(name, A):
        """(rows, columns, pitch, batch, batch stride) of the logical output of a HOOKED launch, in elements of ``out``."""
        out = A["out"]
        if name == "gemm":
            M = A["a"].shape[0] if A["M"] is None else A["M"]
            N = A["w"].shape[0] if A["N"] is None else A["N"]
            ldo = out.stride(-2) if A["ldo"] is None else A["ldo"]
            return M, (N // 2 if A["epilogue"] == 1 else N), ldo, A["batch"], (A["strideO"] if A["batch"] > 1 else 0)
        if name == "gemm_ln":
            N = A["w"].shape[0]
            return A["a"].shape[0], (N // 2 if A["epilogue"] == 1 else N), out.stride(0), 1, 0
        if name == "mlp_geglu":
            return A["x"].shape[0], A["x"].shape[1], out.stride(0), 1, 0
        if name == "linear_rows":
            return A["M"], A["N"], out.stride(0), 1, 0
        if name == "linear_smallm":
            return A["M"], A["N"], (out.stride(0) if A["ldo"] is None else A["ldo"]), 1, 0
        if name == "attention":
            return A["B"] * A["Sq"], A["heads"] * A["d"], A["ldo"], 1, 0
        if name == "conv3x3_smalln":          # fp32 [B*H*W, Cout] (mode 0) or the u8 image: Cout values per pixel either way
            return A["B"] * A["H"] * A["W"], A["Cout"], A["Cout"], 1, 0
        if name in ("conv3x3_c4", "conv3x3_c4_res", "hint_conv_u8"):
            return A["B"] * A["H"] * A["W"], A["Cout"], A["Cout"], 1, 0
        if name == "hint_conv":
            Ho, Wo = ((A["H"] + 1) // 2, (A["W"] + 1) // 2) if A["stride"] == 2 else (A["H"], A["W"])
            return A["B"] * Ho * Wo, A["Cout"], A["Cout"], 1, 0
        return A["B"] * Audit._stats_rows(name, A), A["Cout"], A["Cout"], 1, 0          # conv3x3, conv3x3_gn

    @staticmethod
    def _stats_tensor(name, A):
        out = A["out"]
        if name == "gemm" and A["batch"] == 1 and (A["ldo"] is not None or A["N"] is not None):
            M = A["M"] if A["M"] is not None else A["a"].shape[0]
            N = A["N"] if A["N"] is not None else A["w"].shape[0]
            return out.as_strided((M, N), (A["ldo"] if A["ldo"] is not None else out.stride(-2), 1), out.storage_offset())
        return out

    def _launch_checked(self, name, real, args, kw, A):
        before = {k: v.clone() for k, v in A.items() if torch.is_tensor(v)}
        r = real(*args, **kw)
        torch.cuda.current_stream().synchronize()
        after = {k: v for k, v in A.items() if torch.is_tensor(v)}
        for k, v in after.items():                       # what the launch must not write
            if k not in CHECKED[name]:
                assert same_bits(v, before[k]), f"{name}: operand {k} changed by the launch"
        B = dict(A)
        B.update(before)
        self._note = {}
        ratio, kappa = getattr(self, "_ref_" + name)(B, A, r)
        self.checks.append(dict(op=name, key=None, entry=None, config=None, ratio=ratio, stats_ratio=None, kappa=kappa,
                                args=self._scalars(A), **self._note))
        return r

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

    @staticmethod
    def _scalars(A):
        """the non-tensor arguments of a launch (what the reach checks of the tests read)."""
        return {k: (tuple(v) if isinstance(v, (list, tuple)) else v) for k, v in A.items()
                if isinstance(v, (int, float, bool, str, type(None), list, tuple))}

    def _check(self, name, A, key, meta, stray=()):
        entry, cfg = self._config(key, meta)
        ratio, sratio = getattr(self, "_ref_" + name)(A)
        if stray:                            # a write outside the launch's output fails the check, naming the operand
            ratio = math.inf
        st = A.get("stats")
        if st is not None and st.P > 0:
            out = A["out"]
            rows_img = self._stats_rows(name, A)
            sratio = stats_check(st, out, out.shape[0] // rows_img)
        self.checks.append(dict(op=name, key=key, entry=(tuple(entry[:4]) if entry is not None else None), config=cfg,
                                ratio=ratio, stats_ratio=sratio, stray=list(stray), args=self._scalars(A),
                                m_img=meta.get("m_img"), stats_P=(st.P if st is not None else None)))

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

    def _ref_conv3x3_c4_res(self, A):
        return conv_c4_res_check(A["out"], A["lat_f32"], A["w"], A["bias"], A["res"], A["B"], A["H"], A["W"],
                                 images=_pick_images(A["B"], self.images)), None

    def _ref_hint_conv_u8(self, A):
        B, Hh, Ww = A["B"], A["H"], A["W"]
        x, xerr = hint_u8_input(A["img_u8"].reshape(-1)[:B * Hh * Ww * 3].view(B, Hh, Ww, 3), A["out"].device)
        return hint_layer_check(A["out"], x, xerr, A["w"], A["bias"], B, Hh, Ww, 1, A["silu"], HINT_U8_K,
                                images=_pick_images(B, self.images)), None

    def _ref_hint_conv(self, A):
        B, Hh, Ww, Cin = A["B"], A["H"], A["W"], A["Cin"]
        x = A["x"].reshape(-1)[:B * Hh * Ww * Cin].view(B, Hh, Ww, Cin).to(A["out"].device, torch.float64)
        return hint_layer_check(A["out"], x, None, A["w"], A["bias"], B, Hh, Ww, A["stride"], A["silu"], 9 * Cin,
                                images=_pick_images(B, self.images)), None

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

    # -- the other entry points: (B = operands before the launch, A = the live arguments after it, r = what it returned)
    #    -> (worst ratio, worst GroupNorm kappa or None)
    def _gn_sources(self, st, C):
        t = self.stats_src.get(id(st))
        assert t is not None, "GroupNorm statistics whose producing launch the audit did not see"
        assert t.shape[1] == C, f"statistics source has {t.shape[1]} channels, the launch {C}"
        return t

    def _ref_groupnorm_tables_from_stats(self, B, A, r):
        Bn, HW, C1 = A["B"], A["HW"], A["C1"]
        st2 = A["st2"]
        xs = [self._gn_sources(A["st1"], C1)] + ([self._gn_sources(st2, A["C2"])] if st2 is not None else [])
        C = sum(x.shape[1] for x in xs)
        ws, ws0 = A["ws"], B["ws"]
        assert same_bits(ws[2 * Bn * C:], ws0[2 * Bn * C:]), "groupnorm_tables_from_stats wrote past its tables"
        scale, shift = r
        return gn_check(scale, shift, xs, Bn, HW, A["groups"], A["gamma"], A["beta"], A["eps"],
                        images=_pick_images(Bn, self.images))

    def _gn_out(self, B, A, silu):
        xs = [B["x"]] + ([B["x2"]] if B.get("x2") is not None else [])
        C = sum(x.shape[1] for x in xs)
        Bn, HW = A["B"], A["HW"]
        xs = [x[:Bn * HW] for x in xs]
        assert tail_same(A["out"], B["out"], Bn * HW * C), "groupnorm wrote past its B * HW rows"
        return gn_check(None, None, xs, Bn, HW, A["groups"], A["gamma"], A["beta"], A["eps"], out=A["out"].reshape(-1, C),
                        silu=silu, images=_pick_images(Bn, self.images))

    def _ref_groupnorm(self, B, A, r):
        return self._gn_out(B, A, A["silu"])

    def _ref_groupnorm_from_stats(self, B, A, r):
        return self._gn_out(B, A, A["silu"])

    def _ref_layernorm(self, B, A, r):
        M, C = A["M"], A["C"]
        assert tail_same(A["out"], B["out"], M * C), "layernorm wrote past its M rows"
        ref, bnd = layernorm_reference(B["x"].reshape(-1, C)[:M], B["gamma"], B["beta"], A["eps"])
        return worst_ratio(A["out"].reshape(-1, C)[:M], ref, bnd), None

    def _ref_softmax_rows(self, B, A, r):
        rows, n, ld = A["rows"], A["n"], A["ld"]
        x0, x = B["x"].reshape(-1)[:rows * ld].view(rows, ld), A["x"].reshape(-1)[:rows * ld].view(rows, ld)
        assert not x[:, n:].any(), "softmax_rows: padding columns not zeroed"
        assert tail_same(A["x"], B["x"], rows * ld), "softmax_rows wrote past its rows"
        ref, bnd = softmax_reference(x0, n)
        return worst_ratio(x[:, :n], ref, bnd), None

    def _ref_transpose(self, B, A, r):
        R, Cc, nb = A["R"], A["Cc"], A["batch"]
        x, out0, out = B["x"], B["out"], A["out"]
        iv = x.as_strided((nb, R, Cc), (A["stride_in"], A["ldi"], 1), x.storage_offset())
        exp = out0.clone()
        exp.as_strided((nb, Cc, R), (A["stride_out"], A["ldo"], 1), exp.storage_offset()).copy_(iv.transpose(1, 2))
        return (0.0 if same_bits(out, exp) else math.inf), None

    def _ref_embed_tokens(self, B, A, r):
        Bn, S, D = A["B"], A["S"], A["D"]
        ref = embed_reference(B["ids"], B["tok_emb"], B["pos_emb"], Bn, S)
        assert tail_same(A["out"], B["out"], Bn * S * D), "embed_tokens wrote past its B * S rows"
        return (0.0 if torch.equal(A["out"].reshape(-1, D)[:Bn * S], ref) else math.inf), None

    def _temb(self, ts, B, A):
        Bn, dim = A["B"], A["dim"]
        assert tail_same(A["out"], B["out"], len(ts) * Bn * dim), "timestep embedding wrote past its rows"
        ref, bnd = timestep_reference(ts, Bn, dim)
        dev = A["out"].device
        return worst_ratio(A["out"].reshape(-1, dim)[:len(ts) * Bn], ref.to(dev), bnd.to(dev)), None

    def _ref_timestep_embedding(self, B, A, r):
        return self._temb([A["t"]], B, A)

    def _ref_timestep_embedding_steps(self, B, A, r):
        return self._temb(list(A["ts"]), B, A)

    def _ref_scheduler_step(self, B, A, r):
        ref, bnd = sampler_step_reference(B["eps"], B["lat"], B.get("noise"), A["coef6"], A["last"], m_u=B.get("eps_uncond"),
                                          guidance=A["guidance"], pred=A["pred"])
        return worst_ratio(A["lat"], ref, bnd), None

    def _ref_latents_renoise(self, B, A, r):
        Bn, h, w, dup = A["B"], A["h"], A["w"], A["dup"]
        n = (2 if dup else 1) * Bn * 4 * h * w
        assert tail_same(A["lat"], B["lat"], n), "latents_renoise wrote past its images"
        lat = A["lat"].reshape(-1)[:n].view(-1, 4, h, w)
        x0 = B["x0"].reshape(-1)[:Bn * 4 * h * w].view(Bn, 4, h, w)
        nz = B["noise"].reshape(-1)[:Bn * 4 * h * w].view(Bn, 4, h, w)
        return renoise_check(lat, x0, nz, A["sqrt_a"], A["sqrt_b"], Bn, dup), None

    @staticmethod
    def _front_half(lat, n):
        """the n elements in front of ``lat`` in its storage (the other classifier-free-guidance half of a [2B] state)."""
        assert lat.is_contiguous() and lat.storage_offset() >= n, "hand-over with dup: no first half in front of the state"
        return lat.as_strided((n,), (1,), lat.storage_offset() - n)

    def _ref_scheduler_step_handover(self, B, A, r):
        Bn, h, w, dup = A["B"], A["h"], A["w"], A["dup"]
        n = Bn * 4 * h * w
        assert tail_same(A["lat"], B["lat"], n) and tail_same(A["xk"], B["xk"], n), "hand-over step wrote past its images"
        v = lambda t: t.reshape(-1)[:n].view(Bn, 4, h, w)
        e = lambda t: None if t is None else t.reshape(-1)[:n].view(Bn, h, w, 4)
        front = self._front_half(A["lat"], n).view(Bn, 4, h, w) if dup else None
        return handover_check(v(A["xk"]), v(A["lat"]), front, e(B["eps"]), v(B["lat"]), v(B["noise"]), A["coef6"],
                              A["next_sqrt_a"], A["next_sqrt_b"], Bn, m_u=e(B.get("eps_uncond")), guidance=A["guidance"],
                              pred=A["pred"]), None

    def _ref_latents_pool8(self, B, A, r):
        Bn, h, w = A["B"], A["h"], A["w"]
        ref, bnd = pool8_reference(B["lat"].reshape(-1)[:Bn * 4 * h * w].view(Bn, 4, h, w))
        assert tail_same(A["out"], B["out"], Bn * 256), "latents_pool8 wrote past its B x 4 x 8 x 8 values"
        return worst_ratio(A["out"].reshape(-1)[:Bn * 256].view(Bn, 4, 8, 8), ref, bnd), None

    def _ref_vae_blend(self, B, A, r):
        Bn = A["B"]
        a = B["a"].reshape(Bn, A["ah"], A["aw"], 3)
        b0, b = B["b"].reshape(Bn, A["bh"], A["bw"], 3), A["b"].reshape(Bn, A["bh"], A["bw"], 3)
        ref, bnd, band = blend_reference(a, b0, A["extent"], A["vertical"])
        assert same_bits(b[~band], b0[~band]), "vae_blend wrote outside its band"
        return worst_ratio(b, ref, bnd), None

    def _ref_vae_place_tile(self, B, A, r):
        Bn, H, W, oy, ox, ch, cw = A["B"], A["H"], A["W"], A["oy"], A["ox"], A["ch"], A["cw"]
        tile = B["tile"].reshape(Bn, A["th"], A["tw"], 3)[:, :ch, :cw]
        crop = torch.zeros(Bn, H, W, 3, dtype=torch.bool, device=tile.device)
        crop[:, oy:oy + ch, ox:ox + cw] = True
        u8, u80 = A["out_u8"].reshape(Bn, H, W, 3), B["out_u8"].reshape(Bn, H, W, 3)
        assert torch.equal(u8[~crop], u80[~crop]), "vae_place_tile wrote u8 pixels outside its crop"
        bad, ties = rgb8_check(u8[:, oy:oy + ch, ox:ox + cw], tile)
        self._note["ties"] = ties                   # near-tie u8 pixels off by one: allowed, counted
        ok = bad == 0
        if A["out_f32"] is not None:
            f, f0 = A["out_f32"].reshape(Bn, H, W, 3), B["out_f32"].reshape(Bn, H, W, 3)
            ok = ok and same_bits(f[~crop], f0[~crop]) and same_bits(f[:, oy:oy + ch, ox:ox + cw], tile)
        return (0.0 if ok else math.inf), None


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


def entry_table(checks):
    """entry point -> [launches checked, worst ratio, worst GroupNorm kappa (0 if none)]."""
    rows = {}
    for c in checks:
        r = rows.setdefault(c["op"], [0, 0.0, 0.0])
        r[0] += 1
        r[1] = max(r[1], c["ratio"])
        if c.get("kappa") is not None:
            r[2] = max(r[2], c["kappa"])
    return rows


def failures(checks):
    """launches outside their bound, statistics outside theirs, or GroupNorm launches past the kappa tripwire."""
    return [c for c in checks if not (c["ratio"] <= 1.0) or c.get("stray")
            or (c["stats_ratio"] is not None and not (c["stats_ratio"] <= 1.0))
            or (c.get("kappa") is not None and not (c["kappa"] <= KAPPA_TRIP))]


def summary_line(checks):
    worst_k = max((c.get("kappa") or 0.0) for c in checks) if checks else 0.0
    per = ", ".join(f"{op} {n}/{r:.3f}" for op, (n, r, _) in sorted(entry_table(checks).items()))
    ties = [c["ties"] for c in checks if "ties" in c]
    return (f"worst ratio {max((c['ratio'] for c in checks), default=0.0):.3f}, "
            f"worst statistics ratio {max(((c['stats_ratio'] or 0.0) for c in checks), default=0.0):.3f}, "
            f"worst GroupNorm kappa {worst_k:.4g} (tripwire {KAPPA_TRIP:.4g})"
            + (f", u8 near-ties off by one {sum(ties)} over {len(ties)} placed tiles" if ties else "")
            + f"; checked/worst per entry: {per}")

