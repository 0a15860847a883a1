"""The 32-column tiles of the narrow table (include/lcm_hip.h, lcm_narrow_set) compute the bits of the 64-column launches.

A narrow entry replaces the tile width of one exact launch shape and nothing else: every output element accumulates the same
MFMA sequence over the same k-tiles, split launches leave the same fp32 slabs, and the statistics are written per canonical
32-pixel slab.  So every comparison here is torch.equal between one run with the entry set and one with the table cleared.
No test asserts a speed.
"""
import numpy as np
import pytest
import torch

from sdlcm_amd import lib, ops
from test_load_batching_gpu import DEV, epilogue_cases, pack3x3, rnd, to_nhwc, workspace  # noqa: F401  (workspace: fixture)

pytestmark = pytest.mark.gpu


def launch_names(fn):
    ops.profile_begin()
    fn()
    return [n for n, _ in ops.profile_end()]


def is_narrow(names, kernel):
    return any(n.startswith(kernel) and ", 32, " in n for n in names)


# ---- GEMM, plain ---------------------------------------------------------------------------------------------------------
def _gemm_plans(M, N, K, images, parts, variant):
    m_img = M // images
    ops.plan_clear()
    ops.narrow_clear()
    ops.plan_set(0, m_img, N, K, 1, 64, 64, parts, variant)
    ops.plan_set(0, M, N, K, 1, 64, 64, parts, variant)
    assert ops.canonical_splits(0, m_img, N, K) == parts
    return m_img


@pytest.mark.parametrize("variant", [-1, 3])
@pytest.mark.parametrize("parts", [1, 3])
@pytest.mark.parametrize("N", [64, 320])
@pytest.mark.parametrize("M", [64, 72, 256])
def test_gemm_narrow_equals_wide(workspace, M, N, parts, variant):
    """M = 72: the last 32-row slab holds 8 rows.  N = 64: two n-tiles; N = 320: ten.  Ring depth 4 (variant -1) and 3."""
    import launch_audit as la
    K, images = 512, 2
    m_img = _gemm_plans(M, N, K, images, parts, variant)
    a, w = rnd(M, K, seed=1).to(DEV), rnd(N, K, seed=2, scale=K ** -0.5).to(DEV)
    audited = False
    for tag, bias, rowadd, res, alias, scale in epilogue_cases(M, N, images):
        got = []
        for narrow in (True, False):
            ops.narrow_clear()
            if narrow:
                ops.narrow_set(0, M, N, K, 1)
            o = res.clone() if alias else torch.full((M, N), 7.0, dtype=torch.float16, device=DEV)
            st = ops.Stats(torch.zeros(ops.stats_floats(M, N, m_img), dtype=torch.float32, device=DEV))
            workspace.zero_()
            names = launch_names(lambda: ops.gemm(a, w, o, bias=bias, rowadd=rowadd, rows_per_batch=m_img if rowadd is not None else 0,
                                                  res=o if alias else res, out_scale=scale, stats=st, img_rows=m_img))
            assert is_narrow(names, "igemm2_kernel<64, 32, 0, ") == narrow, names
            slabs = workspace[:parts * M * N].clone()
            if parts > 1:
                assert slabs.view(parts, M, N)[parts - 1].abs().sum() > 0, "the launch did not run split"
            got.append((o, st.P, st.buf.clone(), slabs))
        assert torch.equal(got[0][0], got[1][0]), f"M={M} N={N} parts={parts}, {tag}: output differs"
        assert got[0][1] == got[1][1] and torch.equal(got[0][2], got[1][2]), f"M={M} N={N} parts={parts}, {tag}: statistics differ"
        if parts > 1:
            assert torch.equal(got[0][3], got[1][3]), f"M={M} N={N} parts={parts}, {tag}: fp32 slabs differ"
        if not audited and res is not None and not alias and bias is not None:       # one case per shape against the fp64 bound
            ref, bnd = la.gemm_reference(a, w, bias=bias, rowadd=rowadd, rows_per_batch=m_img, res=res, out_scale=scale)
            ratio = la.worst_ratio(got[0][0], ref, bnd)
            print(f"narrow gemm M={M} N={N} parts={parts}: worst ratio to the fp64 bound {ratio:.3f}")
            assert ratio <= 1.0
            audited = True
    assert audited


# ---- GEMM, LayerNorm fold ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [-1, 3])
@pytest.mark.parametrize("N", [64, 320])
@pytest.mark.parametrize("M", [64, 72])
def test_gemm_ln_narrow_equals_wide(M, N, variant):
    K = 320
    x = (rnd(M, K, seed=1).float() * 0.7 + 0.5 + rnd(M, 1, seed=8).float()).half().to(DEV)
    gamma, beta = 1 + 0.2 * rnd(K, seed=2).float(), rnd(K, seed=3, scale=0.2).float()
    W, b = rnd(N, K, seed=4, scale=K ** -0.5).float(), rnd(N, seed=5, scale=0.3).float()
    Wh = (W * gamma[None, :]).half()
    g, c = Wh.float().sum(1).to(DEV), (W @ beta + b).to(DEV)
    Wh = Wh.to(DEV)
    outs = []
    try:
        ops.plan_clear()
        ops.plan_set(0, M, N, K, 1, 64, 64, 1, variant)
        for narrow in (True, False):
            ops.narrow_clear()
            if narrow:
                ops.narrow_set(0, M, N, K, 1)
            o = torch.full((M, N), 7.0, dtype=torch.float16, device=DEV)
            names = launch_names(lambda: ops.gemm_ln(x, Wh, g, c, o))
            assert is_narrow(names, "igemm2_kernel<64, 32, 0, ") == narrow, names
            assert all(", 1, 0>" in n for n in names if n.startswith("igemm2_kernel")), names      # the LayerNorm-fold instantiation
            outs.append(o)
    finally:
        ops.plan_reset()
    assert torch.equal(outs[0], outs[1])
    ref = torch.nn.functional.layer_norm(x.float().cpu(), (K,), gamma, beta, 1e-5) @ W.T + b
    assert (outs[0].float().cpu() - ref).abs().max() <= 6e-3 * (ref.abs().max() + 1)


# ---- convolution ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [-1, 3])
@pytest.mark.parametrize("B,H,W,Cin,Cout", [(2, 8, 8, 256, 64), (1, 9, 9, 256, 128), (1, 16, 16, 128, 64), (1, 5, 7, 256, 64)])
def test_conv_narrow_equals_wide(workspace, B, H, W, Cin, Cout, variant):
    """8 x 8 patches, ragged ones (9 x 9, 5 x 7) and the 4 x 16 patches of a 16-wide image; one tap per K-step (variant -1) and a
    kernel row of taps (variant 3)."""
    HW, K, M = H * W, 9 * Cin, B * H * W
    aux = W << 1
    ops.plan_clear()
    ops.narrow_clear()
    ops.plan_set(2, HW, Cout, K, aux, 64, 64, 4, variant)
    ops.plan_set(2, M, Cout, K, aux, 64, 64, 4, variant)
    parts = ops.canonical_splits(2, HW, Cout, K, aux, 0)
    assert parts > 1, "pick a shape whose canonical partition has parts"
    x = to_nhwc(rnd(B, Cin, H, W, seed=1)).to(DEV)
    w = pack3x3(rnd(Cout, Cin, 3, 3, seed=2, scale=K ** -0.5)).to(DEV)
    for tag, bias, rowadd, res, alias, _ in epilogue_cases(M, Cout, B):
        if alias:
            continue                                # conv3x3 writes a tensor of its own
        got = []
        for narrow in (True, False):
            ops.narrow_clear()
            if narrow:
                ops.narrow_set(2, M, Cout, K, aux)
            o = torch.full((M, Cout), 7.0, dtype=torch.float16, device=DEV)
            st = ops.Stats(torch.zeros(ops.stats_floats(M, Cout, HW), dtype=torch.float32, device=DEV))
            workspace.zero_()
            names = launch_names(lambda: ops.conv3x3(x, w, o, B, H, W, Cin, Cout, bias=bias, rowadd=rowadd, res=res, stats=st))
            assert is_narrow(names, "conv_halo_pipe_kernel<") == narrow, names
            slabs = workspace[:parts * M * Cout].clone()
            assert slabs.view(parts, M, Cout)[parts - 1].abs().sum() > 0, "the launch did not run split"
            got.append((o, st.P, st.buf.clone(), slabs))
        assert torch.equal(got[0][3], got[1][3]), f"{tag}: fp32 slabs differ"
        assert torch.equal(got[0][0], got[1][0]), f"{tag}: output differs"
        assert got[0][1] == got[1][1] and got[0][1] > 0 and torch.equal(got[0][2], got[1][2]), f"{tag}: statistics differ"


# ---- selection -----------------------------------------------------------------------------------------------------------
def test_selection_follows_the_table_and_the_switch(workspace):
    M, N, K, parts = 64, 64, 512, 3
    _gemm_plans(M, N, K, 1, parts, -1)
    ops.plan_set(0, 2 * M, N, K, 1, 64, 64, parts, -1)
    a, w = rnd(M, K, seed=1).to(DEV), rnd(N, K, seed=2, scale=K ** -0.5).to(DEV)
    o = torch.empty(M, N, dtype=torch.float16, device=DEV)
    run = lambda: ops.gemm(a, w, o, img_rows=M)      # noqa: E731
    ops.narrow_set(0, M, N, K, 1)
    try:
        assert is_narrow(launch_names(run), "igemm2_kernel<64, 32, 0, 4, 0, 0>")
        one = o.clone()
        ops.set_narrow_tiles(0)
        assert not is_narrow(launch_names(run), "igemm2_kernel")
        assert torch.equal(o, one)
        ops.set_narrow_tiles(1)
        assert is_narrow(launch_names(run), "igemm2_kernel")
        # two images of the same per-image shape: another total shape, so the wide tile -- and the same per-image bits
        a2, o2 = torch.cat([a, a]), torch.empty(2 * M, N, dtype=torch.float16, device=DEV)
        names = launch_names(lambda: ops.gemm(a2, w, o2, img_rows=M))
        assert not is_narrow(names, "igemm2_kernel") and any(n.startswith("igemm2_kernel<64, 64, ") for n in names), names
        assert torch.equal(o2[:M], one) and torch.equal(o2[M:], one)
        ops.narrow_clear()
        assert not is_narrow(launch_names(run), "igemm2_kernel")
        assert torch.equal(o, one)
    finally:
        ops.set_narrow_tiles(1)


def test_narrow_set_refuses_other_widths():
    L = lib.load()
    try:
        assert L.lcm_narrow_set(0, 64, 64, 512, 1, 64) == -1          # LCM_EINVAL: only bn = 32
        assert L.lcm_narrow_set(0, 64, 64, 512, 1, 16) == -1
        assert L.lcm_narrow_set(0, 64, 80, 512, 1, 32) == -1          # N % 32 != 0
        assert L.lcm_narrow_set(0, 64, 64, 512, 1, 32) == 0
    finally:
        ops.plan_reset()


# ---- whole request -------------------------------------------------------------------------------------------------------
def test_request_bits_do_not_depend_on_the_narrow_table():
    """One 512 x 512 4-step request with the shipped narrow table and one with the switch off: the same bytes.  (That they are
    the parent commit's bytes is test_load_batching_gpu.py::test_requests_give_the_parent_commits_bytes.)"""
    from sdlcm_amd import weights
    from sdlcm_amd.pipeline import LcmHipPipeline
    ops.plan_reset()
    pipe = LcmHipPipeline(weights.synthetic_unet(), weights.synthetic_vae(), device="cuda:0")
    pe = torch.randn(1, 77, 768, generator=torch.Generator().manual_seed(5)).to(torch.float16)
    outs = []
    try:
        for on in (1, 0):
            ops.set_narrow_tiles(on)
            if not on:
                pipe.drop_plans()                   # captured graphs hold the launches of the other setting
            out = pipe.generate(pe, [42], 512, 512, 4, 1.0)
            outs.append({k: np.ascontiguousarray(out[k].detach().cpu().numpy() if isinstance(out[k], torch.Tensor) else out[k])
                         for k in ("rgb", "latents", "pool8")})
    finally:
        ops.set_narrow_tiles(1)
    for k in ("rgb", "latents", "pool8"):
        assert np.array_equal(outs[0][k], outs[1][k]), f"{k} differs between narrow tiles on and off"
