"""The overlap that gn_from_stats_fused_kernel documents -- activations fetched before the statistics are reduced -- is a
property of the compiled code, not of the source: the compiler once undid it silently by waiting behind every prefetch.
tools/load_chains.py reads the gfx950 assembly; this test keeps the two round trips overlapped."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_fused_groupnorm_issues_activations_and_statistics_together():
    import load_chains
    hipcc = load_chains.find_hipcc()
    if not hipcc or not (os.path.isfile(hipcc) or shutil.which(hipcc)):
        pytest.skip("hipcc not installed")
    res = load_chains.analyze([os.path.join(load_chains.CSRC, "norm.hip")], hipcc)
    hits = [v for (f, k), v in res.items() if "gn_from_stats_fused_kernel" in k or "gn_from_stats_fused_kernel" in v["mangled"]]
    assert len(hits) == 1
    ev = hits[0]["events"]
    # activation pairs are 4-byte loads (global_load_dword), statistics entries 8-byte ones (global_load_dwordx2)
    first_act = next(i for i, e in enumerate(ev) if e[0] == "load" and e[1] == "global_load_dword")
    first_stat = next(i for i, e in enumerate(ev) if e[0] == "load" and e[1] == "global_load_dwordx2")
    lo, hi = sorted((first_act, first_stat))
    waits = [e for e in ev[lo:hi] if e[0] == "wait"]
    assert not waits, f"s_waitcnt vmcnt between the first activation load and the first statistics load: {waits}"
    assert hits[0]["scratch"] == 0
