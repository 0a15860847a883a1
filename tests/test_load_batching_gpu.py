"""The kernels that issue their loads in batches (split-K reduce, GroupNorm from statistics, the unsplit tile epilogue)
compute what the one-load-at-a-time forms computed, bit for bit.

* split-K reduce: the fp32 slabs the split launch left in the workspace, combined in torch with the reduce kernel's own
  sequence of fp32 operations (every one of them exact IEEE in torch as on the GPU): torch.equal.
* GroupNorm from statistics: single-launch form == two-launch form, both inside the audit's fp64 bound.
* unsplit epilogue: the ring variants with three and more stages take the batched epilogue, those with one or two stages and
  the segmented / persistent forms the per-fragment one: same bits under every plan.
* whole requests: sha256 of rgb / latents / pool8 equal to those recorded on the parent commit
  (tests/golden/parent_bits_load_batching.json).
"""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from sdlcm_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(torch.float16)


def to_nhwc(x):
    B, C, H, W = x.shape
    return x.permute(0, 2, 3, 1).reshape(B * H * W, C).contiguous()


def pack3x3(w):
    return w.permute(0, 2, 3, 1).contiguous().reshape(w.shape[0], -1)


def combine(slabs, bias, rowadd, rows_per_batch, out_scale, res):
    """The reduce kernel's sequence on fp32 slabs [parts][M][N]: slab 0, += slab s in order, + bias (+0.0 without one),
    + rowadd of the row's image, * out_scale, + res, round to fp16."""
    v = slabs[0].clone()
    for s in range(1, slabs.shape[0]):
        v += slabs[s]
    v += bias.float() if bias is not None else torch.zeros(v.shape[1], device=v.device)
    if rowadd is not None:
        img = torch.arange(v.shape[0], device=v.device) // rows_per_batch
        v += rowadd.float()[img]
    v *= out_scale
    if res is not None:
        v += res.float()
    return v.half()


def epilogue_cases(M, N, images):
    """(tag, bias, rowadd, res, alias, out_scale): every combination the entry points accept, and a scale != 1."""
    b, ra, rs = rnd(N, seed=11).to(DEV), rnd(images, N, seed=12).to(DEV), rnd(M, N, seed=13).to(DEV)
    out = []
    for use_b in (False, True):
        for use_ra in (False, True):
            for use_res in (0, 1, 2):             # 2: the residual IS the output buffer
                out.append((f"bias={use_b} rowadd={use_ra} res={use_res}", b if use_b else None, ra if use_ra else None,
                            rs if use_res else None, use_res == 2, 0.5 if (use_b != use_ra) else 1.0))
    return out


@pytest.fixture
def workspace():
    ws = torch.zeros(8 << 20, dtype=torch.float32, device=DEV)
    ops.set_workspace(ws)
    try:
        yield ws
    finally:
        ops.set_seg_mode(0)
        ops.set_split_policy()
        ops.plan_reset()
        ops.set_workspace(None)


def _gemm_split_vs_reference(ws, M, N, K, parts, images=2):
    m_img = M // images
    ops.plan_clear()
    ops.plan_set(0, m_img, N, K, 1, 64, 64, parts)
    ops.plan_set(0, M, N, K, 1, 64, 64, parts)
    assert ops.canonical_splits(0, m_img, N, K) == parts
    a, w = rnd(M, K, seed=1).to(DEV), rnd(N, K, seed=2, scale=K ** -0.5).to(DEV)
    for tag, bias, rowadd, res, alias, scale in epilogue_cases(M, N, images):
        got = []
        for mode in (2, 1):                       # split + reduce | segmented in one workgroup
            ops.set_seg_mode(mode)
            o = res.clone() if alias else torch.full((M, N), 7.0, dtype=torch.float16, device=DEV)
            st = ops.Stats(torch.zeros(ops.stats_floats(M, N, m_img), dtype=torch.float32, device=DEV))
            if mode == 2:
                ws.zero_()
            ops.gemm(a, w, o, bias=bias, rowadd=rowadd, rows_per_batch=m_img if rowadd is not None else 0,
                     res=o if alias else res, out_scale=scale, stats=st, img_rows=m_img)
            got.append((o, st.P, st.buf.clone()))
            if mode == 2:
                slabs = ws[:parts * M * N].view(parts, M, N).clone()
                assert slabs[parts - 1].abs().sum() > 0, "the launch did not run split"
                want = combine(slabs, bias, rowadd, m_img, scale, res)
                assert torch.equal(o, want), f"reduce of {parts} parts, M={M} N={N}, {tag}: differs from the fp32 recipe"
        assert got[0][1] == got[1][1], tag
        assert torch.equal(got[0][2], got[1][2]), f"statistics differ between split and segmented ({tag})"
        assert torch.equal(got[0][0], got[1][0]), f"segmented output differs ({tag})"


@pytest.mark.parametrize("M", [64, 72, 256])
@pytest.mark.parametrize("N", [64, 320])
def test_reduce_is_the_exact_fp32_recipe(workspace, M, N):
    """M = 72: the last 32-row slab holds 8 rows, its second 16-row fragment none."""
    for parts in (2, 3, 5, 8):
        _gemm_split_vs_reference(workspace, M, N, 512, parts)


def test_reduce_with_more_parts_than_one_batch(workspace):
    """11 parts under a policy of 16: a whole batch of 8 slabs, then 3."""
    ops.set_split_policy(max_parts=16)
    _gemm_split_vs_reference(workspace, 72, 64, 1024, 11)
    _gemm_split_vs_reference(workspace, 64, 320, 1024, 16)


@pytest.mark.parametrize("B,H,W,Cin,Cout,stride,ups,out_hw", [(2, 8, 8, 256, 64, 1, 0, None), (1, 9, 9, 256, 128, 1, 0, None),
                                                             (2, 16, 16, 128, 64, 2, 0, None), (1, 5, 7, 256, 64, 1, 1, (9, 13)),
                                                             (1, 8, 8, 256, 64, 1, 2, None)])
def test_conv_reduce_is_the_exact_fp32_recipe(workspace, B, H, W, Cin, Cout, stride, ups, out_hw):
    """4 x 8 patches with a ragged border (9 x 9), stride 2, an upsampling conv to an odd size, and the phase-decomposed
    upsampling conv (four phase slabs per patch)."""
    from sdlcm_amd.packing import pack_conv3x3_up2
    Ho, Wo = out_hw if out_hw else (2 * H, 2 * W) if ups else ((H + 1) // 2, (W + 1) // 2) if stride == 2 else (H, W)
    HW, K = Ho * Wo, (4 if ups == 2 else 9) * Cin
    M = B * HW
    kind, aux, ph = (1, 1, 0) if stride == 2 else (2, Wo << 1, 1 if ups == 2 else 0)
    ops.plan_clear()
    ops.plan_set(kind, HW, Cout, K, aux, 64, 64, 4)
    ops.plan_set(kind, M, Cout, K, aux, 64, 64, 4)
    parts = ops.canonical_splits(kind, HW, Cout, K, aux, ph)
    assert parts > 1, "pick a shape whose canonical partition has parts"
    x = to_nhwc(rnd(B, Cin, H, W, seed=1)).to(DEV)
    w4 = rnd(Cout, Cin, 3, 3, seed=2, scale=(9 * Cin) ** -0.5)
    w = (pack_conv3x3_up2(w4) if ups == 2 else pack3x3(w4)).to(DEV)
    for tag, bias, rowadd, res, alias, _ in epilogue_cases(M, Cout, B):
        if alias:
            continue                                # conv3x3 writes a tensor of its own
        got = []
        for mode in (2, 1):
            ops.set_seg_mode(mode)
            o = torch.full((M, Cout), 7.0, dtype=torch.float16, device=DEV)
            st = ops.Stats(torch.zeros(ops.stats_floats(M, Cout, HW), dtype=torch.float32, device=DEV))
            if mode == 2:
                workspace.zero_()
            ops.conv3x3(x, w, o, B, H, W, Cin, Cout, bias=bias, rowadd=rowadd, res=res, stride=stride, ups=ups, stats=st,
                        out_hw=out_hw)
            got.append((o, st.P, st.buf.clone()))
            if mode == 2:
                slabs = workspace[:parts * M * Cout].view(parts, M, Cout).clone()
                assert slabs[parts - 1].abs().sum() > 0, "the launch did not run split"
                assert torch.equal(o, combine(slabs, bias, rowadd, HW, 1.0, res)), f"conv reduce, {tag}"
        assert got[0][1] == got[1][1] and got[0][1] > 0, tag
        assert torch.equal(got[0][2], got[1][2]), f"statistics differ between split and segmented ({tag})"
        assert torch.equal(got[0][0], got[1][0]), f"segmented output differs ({tag})"


# ---- GroupNorm from producer statistics ----------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("HW", [64, 81, 256])
@pytest.mark.parametrize("C1,C2", [(320, 0), (64, 64), (1280, 1280), (320, 640), (64, 0)])
def test_groupnorm_single_launch_equals_two_launches(B, HW, C1, C2):
    """(64, 0) at HW = 64: 32 items per 256-thread workgroup, so most prefetch slots are empty.  Statistics slabs are written here
    the way a producer writes them: per 32-pixel slab (the last one ragged at HW = 81) and channel, (sum, sum of squares) of
    the fp16 values."""
    import launch_audit as la
    C = C1 + C2
    xs = [(rnd(B * HW, c, seed=20 + i) + 0.25).to(DEV) for i, c in enumerate((C1, C2)) if c]
    P = (HW + 31) // 32
    sts = []
    for x in xs:
        c = x.shape[1]
        xf = torch.zeros(B, P * 32, c, dtype=torch.float32, device=DEV)
        xf[:, :HW] = x.float().view(B, HW, c)
        xf = xf.view(B, P, 32, c)
        st = ops.Stats(torch.stack([xf.sum(2), (xf * xf).sum(2)], dim=-1).contiguous().view(-1))
        st.P = P
        sts.append(st)
    gamma, beta = (1 + 0.1 * rnd(C, seed=6).float()).half().to(DEV), rnd(C, seed=7, scale=0.1).to(DEV)
    ws = torch.zeros(ops.groupnorm_ws_bytes(B, HW, C) // 4 + 16, dtype=torch.float32, device=DEV)
    ys = []
    try:
        for fused_bytes in (1 << 40, 0):
            ops.set_gn_fused_bytes(fused_bytes)
            y = torch.full((B * HW, C), 3.0, dtype=torch.float16, device=DEV)
            ops.groupnorm_from_stats(xs[0], gamma, beta, y, B, HW, C1, sts[0], ws, x2=xs[1] if C2 else None, C2=C2,
                                     st2=sts[1] if C2 else None)
            ys.append(y)
        torch.cuda.synchronize()
    finally:
        ops.set_gn_fused_bytes(8 << 20)
    assert torch.equal(ys[0], ys[1]), "single-launch GroupNorm differs from finalize + apply"
    for y in ys:
        ratio, _ = la.gn_check(None, None, xs, B, HW, 32, gamma, beta, 1e-5, out=y, silu=True)
        print(f"gn B={B} HW={HW} C={C1}+{C2}: worst ratio to the fp64 bound {ratio:.3f}")
        assert ratio <= 1.0


# ---- unsplit epilogue ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [64, 100, 4096])
def test_unsplit_gemm_epilogue_same_bits_under_every_plan(M):
    """Ring depth 1 and 2 run the per-fragment epilogue, 3 and 4 the batched one, a persistent launch runs it inside the K
    loop: one result."""
    N = K = 320
    a, w = rnd(M, K, seed=1).to(DEV), rnd(N, K, seed=2, scale=K ** -0.5).to(DEV)
    images = 2 if M % 2 == 0 else 1
    try:
        for tag, bias, rowadd, res, alias, scale in epilogue_cases(M, N, images):
            seen = []
            for bm, bn, var, persist in ((64, 64, 1, 0), (64, 64, 2, 0), (64, 64, 3, 0), (64, 64, 4, 0), (64, 64, 4, 1),
                                         (64, 160, 3, 0), (128, 64, 3, 0), (128, 64, 2, 0)):
                if bm > M:
                    continue
                ops.plan_clear()
                ops.plan_set(0, M, N, K, 1, bm, bn, 1, var)
                ops.set_persist_n(persist)
                o = res.clone() if alias else torch.full((M, N), 7.0, dtype=torch.float16, device=DEV)
                st = ops.Stats(torch.zeros(ops.stats_floats(M, N, 0), dtype=torch.float32, device=DEV))
                ops.gemm(a, w, o, bias=bias, rowadd=rowadd, rows_per_batch=M // images if rowadd is not None else 0,
                         res=o if alias else res, out_scale=scale, stats=st)
                seen.append(((bm, bn, var, persist), o, st.P, st.buf.clone()))
            for plan, o, P, sb in seen[1:]:
                assert torch.equal(o, seen[0][1]), f"{tag}: output under plan {plan} differs from plan {seen[0][0]}"
                assert P == seen[0][2] and torch.equal(sb, seen[0][3]), f"{tag}: statistics under plan {plan}"
            ref = a.float() @ w.float().T
            want = combine(ref[None], bias, rowadd, M // images, scale, res)
            err = (seen[0][1].float() - want.float()).abs().max().item()
            assert err <= 2e-2 * (want.float().abs().max().item() + 1), f"{tag}: {err}"
    finally:
        ops.set_persist_n(0)
        ops.plan_reset()


def test_unsplit_conv_epilogue_same_bits_under_every_plan():
    B, H, W, C = 1, 16, 16, 320
    M, K = B * H * W, 9 * C
    x = to_nhwc(rnd(B, C, H, W, seed=1)).to(DEV)
    w = pack3x3(rnd(C, C, 3, 3, seed=2, scale=K ** -0.5)).to(DEV)
    try:
        ops.set_split_policy(max_rows_per_image=0)          # no image may be split: the unsplit kernels run
        for tag, bias, rowadd, res, alias, _ in epilogue_cases(M, C, B):
            if alias:
                continue
            seen = []
            for bm, bn, var in ((64, 64, 1), (64, 64, 2), (64, 64, 3), (128, 64, 3), (128, 160, 2), (128, 64, 1)):
                ops.plan_clear()
                assert ops.canonical_splits(2, M, C, K, W << 1, 0) == 1
                ops.plan_set(2, M, C, K, W << 1, bm, bn, 1, var)
                o = torch.full((M, C), 7.0, dtype=torch.float16, device=DEV)
                st = ops.Stats(torch.zeros(ops.stats_floats(M, C, H * W), dtype=torch.float32, device=DEV))
                ops.conv3x3(x, w, o, B, H, W, C, C, bias=bias, rowadd=rowadd, res=res, stats=st)
                seen.append(((bm, bn, var), o, st.P, st.buf.clone()))
            for plan, o, P, sb in seen[1:]:
                assert torch.equal(o, seen[0][1]), f"{tag}: output under plan {plan} differs from plan {seen[0][0]}"
                assert P == seen[0][2] and P > 0 and torch.equal(sb, seen[0][3]), f"{tag}: statistics under plan {plan}"
    finally:
        ops.set_split_policy()
        ops.plan_reset()


# ---- whole requests: the parent commit's bytes ---------------------------------------------------------------------------
def test_requests_give_the_parent_commits_bytes():
    from sdlcm_amd import weights
    from sdlcm_amd.pipeline import LcmHipPipeline
    with open(os.path.join(os.path.dirname(__file__), "golden", "parent_bits_load_batching.json")) as f:
        doc = json.load(f)
    pipe = LcmHipPipeline(weights.synthetic_unet(), weights.synthetic_vae(), device="cuda:0")
    pe = torch.randn(1, 77, 768, generator=torch.Generator().manual_seed(doc["prompt_seed"])).to(torch.float16)
    for r in doc["requests"]:
        out = pipe.generate(pe, doc["seeds"], r["width"], r["height"], r["steps"], doc["guidance_scale"])
        for k in ("rgb", "latents", "pool8"):
            a = out[k]
            a = np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a)
            assert list(a.shape) == r[k]["shape"] and str(a.dtype) == r[k]["dtype"]
            assert hashlib.sha256(a.tobytes()).hexdigest() == r[k]["sha256"], \
                f"{k} of the {r['width']}x{r['height']} {r['steps']}-step request differs from commit {doc['parent_commit'][:12]}"
