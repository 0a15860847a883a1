#!/usr/bin/env python3
"""Per-launch cost of the four most-launched batch-1 kernels at their real shapes, as chains of dependent launches inside a
captured graph (the method of profiles/r01_chain_latency_gemm.txt, tools/chain_latency.py: one event pair around the chain on
a busy stream, wall / launches).  Run once per build; three repeats per case give the run-to-run spread.

  python tools/entry_path_chain.py [label [substring of the cases to run]]

A split case is a pair of launches (the split kernel and splitk_reduce_kernel): its figure is per PAIR."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sdlcm_amd  # noqa: E402,F401
from sdlcm_amd import ops  # noqa: E402

DEV = "cuda"
N, REPLAYS, REPEATS = 240, 5, 3
st = torch.cuda.Stream()


def rnd(*s):
    return torch.randn(*s, device=DEV, dtype=torch.float16)


ONLY = sys.argv[2] if len(sys.argv) > 2 else ""


def chain(name, make_fn):
    if ONLY not in name:
        return
    with torch.cuda.stream(st):
        fns = make_fn()
        for f in fns[:4]:
            f()
        st.synchronize()
        g = ops.Graph()
        with g:
            for i in range(N):
                fns[i % len(fns)]()
        for _ in range(3):
            g.launch()
        st.synchronize()
        us = []
        for _ in range(REPEATS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(REPLAYS):
                g.launch()
            e1.record(st)
            e1.synchronize()
            us.append(e0.elapsed_time(e1) / REPLAYS / N * 1e3)
        print(f"{name:62s} " + " ".join(f"{u:7.2f}" for u in us) + f"  us/launch   min {min(us):7.2f}  spread {max(us) - min(us):5.2f}", flush=True)
        g.close()


def gemm_case(M, Nn, K, sp):
    def mk():
        nset = min(240, max(2, int(400e6 / (Nn * K * 2))))        # more weights than the caches hold: they stream as in a pass
        Ws = [rnd(Nn, K) * K ** -0.5 for _ in range(nset)]
        a, o, b = rnd(M, K), torch.empty(M, Nn, device=DEV, dtype=torch.float16), rnd(Nn)
        ops.plan_clear()
        ops.plan_set(0, M, Nn, K, 1, 64, 64, sp, 4)
        return [(lambda i=i: ops.gemm(a, Ws[i], o, bias=b)) for i in range(nset)]
    return mk


def conv_case(H, W, Cin, Cout, sp):
    def mk():
        K, M = 9 * Cin, H * W
        nset = min(64, max(2, int(400e6 / (Cout * K * 2))))
        Ws = [rnd(Cout, K) * K ** -0.5 for _ in range(nset)]
        x, o, b = rnd(M, Cin), torch.empty(M, Cout, device=DEV, dtype=torch.float16), rnd(Cout)
        ops.plan_reset()               # the shipped plan of this shape: tile, variant and partition as in a pass
        assert ops.canonical_splits(2, M, Cout, K, W << 1, 0) == sp, ops.canonical_splits(2, M, Cout, K, W << 1, 0)
        return [(lambda i=i: ops.conv3x3(x, Ws[i], o, 1, H, W, Cin, Cout, bias=b)) for i in range(nset)]
    return mk


def gn_case(HW, C):
    def mk():
        x = rnd(HW, C)
        P = HW // 32
        xf = x.float().view(P, 32, C)
        s = ops.Stats(torch.stack([xf.sum(1), (xf * xf).sum(1)], dim=-1).contiguous().view(-1))
        s.P = P
        g, b, y = rnd(C), rnd(C), torch.empty(HW, C, device=DEV, dtype=torch.float16)
        ws = torch.zeros(ops.groupnorm_ws_bytes(1, HW, C) // 4 + 16, dtype=torch.float32, device=DEV)
        return [lambda: ops.groupnorm_from_stats(x, g, b, y, 1, HW, C, s, ws)]
    return mk


def main():
    print(f"# {sys.argv[1] if len(sys.argv) > 1 else 'build'}: {torch.cuda.get_device_name(0)}; {N} dependent launches per graph, "
          f"{REPLAYS} replays per timing, {REPEATS} timings")
    ops.set_workspace(torch.empty(64 << 18, dtype=torch.float32, device=DEV))
    chain("spin(0) trivial kernel", lambda: [lambda: ops.debug_spin(0)])
    chain("igemm2<64,64,0,4> proj_in 64^2: M4096 N320 K320", gemm_case(4096, 320, 320, 1))
    chain("igemm2<64,64,0,4> 16^2: M256 N1280 K1280 unsplit", gemm_case(256, 1280, 1280, 1))
    chain("igemm2 + splitk_reduce 16^2: M256 N1280 K1280, 5 parts (pair)", gemm_case(256, 1280, 1280, 5))
    chain("gn_from_stats_fused 16^2 x 1280", gn_case(256, 1280))
    chain("gn_from_stats_fused 64^2 x 320", gn_case(4096, 320))
    chain("conv_halo_pipe + splitk_reduce 16^2 1280->1280, 5 parts (pair)", conv_case(16, 16, 1280, 1280, 5))
    ops.plan_reset()
    ops.set_workspace(None)


if __name__ == "__main__":
    main()
