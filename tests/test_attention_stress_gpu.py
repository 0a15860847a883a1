"""Every dispatchable form of the three attention kernels (csrc/attention.hip) on the designed logits of
tests/attention_cases.py, against float64 under the per-element bound of launch_audit.attention_check -- the bound the CPU replay
of tests/test_launch_audit.py stays inside on the same cases and every planted fault leaves.

Per case: the bound and finiteness; nothing written outside the logical output (out sits at column 8 of a wider pitch between
two sentinel rows) and no operand touched; the image run alone equals the same image run last of three, bit for bit; workgroup
forms (the default 4 waves against 8, or the 16-wave d = 40 form, of the streaming kernel; against 2 of the register-staged
one) give the same bits; with the key split switched off the result is inside the bound as well.  Worst ratios per form: DESIGN.md.
"""
import pytest
import torch

import attention_cases as ac
import launch_audit as la
from sdlcm_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -7.0
PAD = 16                # ldo = heads * d + PAD, the output starts at column PAD / 2

CASES = ac.table()


def _launch(case, B, q, k, v):
    """one launch into a sentinel-framed buffer -> the [B * Sq, C] view of its output; asserts that nothing outside the logical
    output changed and that the operands are bit-unchanged."""
    C = case.heads * case.d
    rows, ldo = B * case.Sq, C + PAD
    buf = torch.full(((rows + 2) * ldo,), SENTINEL, dtype=torch.float16, device=DEV)
    out = buf.as_strided((rows, C), (ldo, 1), ldo + PAD // 2)
    start, n, keep = la.out_window(out, rows, C, ldo)
    before = buf.clone()
    kept = [t.clone() for t in (q, k, v)]
    ops.attention(q, k, v, out, B, case.heads, case.Sq, case.Sk, case.d, ldq=C, ldk=C, ldv=C, ldo=ldo, scale=case.scale,
                  causal=case.causal)
    torch.cuda.synchronize()
    # the whole buffer: the sentinel row in front (a row -1), the one behind (rows past Sq of the last image) and the gap columns
    assert la.stray_writes(la.window_of(before, start, n), la.window_of(out, start, n), keep) == 0, "written into the gap columns"
    assert la.frame_writes(before, buf, out) == 0, "written outside the logical output"
    assert all(la.same_bits(a, b) for a, b in zip((q, k, v), kept)), "an operand was written"
    return out


def _ratio(case, got, q, k, v, B=1, images=None):
    return la.attention_check(got, q, k, v, B, case.heads, case.Sq, case.Sk, case.d, scale=case.scale, causal=case.causal,
                              images=images)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_attention_on_designed_logits(case):
    q, k, v = (t.to(DEV) for t in case.operands())
    C = case.heads * case.d
    g = torch.Generator().manual_seed(11)
    q3 = torch.cat([torch.randn(case.Sq, C, generator=g).half().to(DEV), q, q])         # image 0 drawn, image 1 the case with -V
    k3 = torch.cat([torch.randn(case.Sk, C, generator=g).half().to(DEV), k, k])
    v3 = torch.cat([torch.randn(case.Sk, C, generator=g).half().to(DEV), -v, v])
    try:
        out3 = _launch(case, 3, q3, k3, v3)
        assert torch.isfinite(out3).all()
        r = _ratio(case, out3, q3, k3, v3, B=3, images=[2])
        print(f"\nSTRESS | {case.form} | {case.name} | {r:.4f}")
        assert r <= 1.0, (case.name, r)
        solo = _launch(case, 1, q, k, v)
        assert la.same_bits(solo, out3[2 * case.Sq:]), "an image alone differs from the same image last of three"
        if case.kernel != "wide":               # the default at these grid sizes is the 4-wave form: the other one against it
            other = 8 if case.kernel == "attn2" else 2          # (8: the 16-wave form for d = 40 with the key split)
            ops.set_attention_waves(other)
            assert la.same_bits(_launch(case, 1, q, k, v), solo), f"{other}-wave workgroups change the bits"
            ops.set_attention_waves(0)
        if case.ksplit:
            ops.set_attention_ksplit(0)
            unsplit = _launch(case, 1, q, k, v)
            ru = _ratio(case, unsplit, q, k, v)
            print(f"STRESS | attn2<{case.d}> KS 1 (split off) | {case.name} | {ru:.4f}")
            assert ru <= 1.0, (case.name, "key split off", ru)
            ops.set_attention_waves(8)
            assert la.same_bits(_launch(case, 1, q, k, v), unsplit), "8-wave workgroups change the bits (key split off)"
    finally:
        ops.set_attention_waves(0)
        ops.set_attention_ksplit(1)
