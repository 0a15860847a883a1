#!/usr/bin/env python3
"""What a wave does before its first vector-memory instruction, read from the compiled gfx950 code (runs on a CPU-only box).

  python tools/entry_path.py [--kernels REGEX] [--launched KERNEL_STATS_CSV] csrc/igemm.hip [csrc/conv_halo.hip ...]

--launched keeps the instantiations named in a rocprofv3 kernel_stats.csv (the kernels a traced run launched).

tools/load_chains.py counts the memory round trips a wave waits for (s_waitcnt vmcnt); it does not see what stands in front
of the first load.  This tool compiles each .hip file with csrc/Makefile's flags (tools/load_chains.py does the compiling) and
prints, per kernel instantiation, over the code as laid out from the kernel's entry:

  entry     instructions from entry to the first vector-memory instruction (global / buffer / flat / scratch load, LDS-DMA
            included, store or atomic)
  rcp       v_rcp_iflag_f32 on that path / in the whole kernel: one per run-time unsigned 32-bit division (a signed or a
            64-bit division expands to more than one, plus its fix-up code)
  swait     s_waitcnt lgkmcnt(N) on that path that retire at least one s_load issued since the previous such wait: every one
            is a scalar-cache (or, right after a kernel boundary, memory) round trip the whole wave stands still for
  sload     s_load instructions on that path / of those, through a base other than the kernel-argument pointer
  got       s_load instructions in the whole kernel whose base comes from s_getpc (the address of a __device__ variable
            fetched from the global offset table) / of those, behind the first LDS-DMA instruction: each stands, with its
            own scalar wait, in front of the DMA that uses the address

The counts are of the code, not of a run: a branch not taken skips what it guards."""
import os
import re
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import load_chains as lc  # noqa: E402

_VMEM = re.compile(r"^(global|buffer|flat|scratch)_(load|store|atomic)")
_SLOAD = re.compile(r"^s_(buffer_)?load_\w+\s+\S+,\s*(s\[\d+:\d+\])")
_LGKM = re.compile(r"lgkmcnt\((\d+)\)")
_GETPC = re.compile(r"^s_getpc_b64\s+(s\[\d+:\d+\])")
_SDST = re.compile(r"^s_\w+\s+(s\[\d+:\d+\]|s\d+)")


def _regs(tok):
    """s[a:b] / sN -> the set of SGPR numbers."""
    m = re.match(r"s\[(\d+):(\d+)\]", tok)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    m = re.match(r"s(\d+)$", tok)
    return {int(m.group(1))} if m else set()


def analyze_asm(path):
    """-> {mangled kernel name: dict(entry, rcp_entry, rcp_all, swait, sload, sload_other, got, got_after_dma)}"""
    lines = open(path).read().splitlines()
    kernels = {m.group(1) for l in lines for m in [re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)] if m}
    start = {}
    for i, l in enumerate(lines):
        m = re.match(r"^([A-Za-z_][\w.$]*):", l)
        if m and m.group(1) in kernels and m.group(1) not in start:
            start[m.group(1)] = i
    res = {}
    for k in sorted(start, key=start.get):
        r = dict(entry=0, rcp_entry=0, rcp_all=0, swait=0, sload=0, sload_other=0, got=0, got_after_dma=0)
        before, seen_dma = True, False
        pending = 0                  # s_loads issued since the previous lgkmcnt wait
        pcregs = set()               # SGPRs that hold an address derived from s_getpc
        kernarg = None               # base of the first s_load that does not come from s_getpc
        i = start[k] + 1
        while i < len(lines):
            l = lines[i].strip()
            i += 1
            if l.startswith(".Lfunc_end"):
                break
            ins = l.split(";")[0].strip()
            if not ins or ins.endswith(":") or ins.startswith("."):
                continue
            if _VMEM.match(ins):
                before = False
                if "_load_lds_" in ins.split()[0]:
                    seen_dma = True
                continue
            if before:
                r["entry"] += 1
            if ins.startswith("v_rcp_iflag"):
                r["rcp_all"] += 1
                r["rcp_entry"] += before
            m = _GETPC.match(ins)
            if m:
                pcregs |= _regs(m.group(1))
                continue
            m = _SLOAD.match(ins)
            if m:
                base = _regs(m.group(2))
                if base <= pcregs:
                    r["got"] += 1
                    r["got_after_dma"] += seen_dma
                elif kernarg is None:
                    kernarg = base
                if before:
                    r["sload"] += 1
                    r["sload_other"] += base != kernarg
                pending += 1
            elif ins.startswith("s_waitcnt"):
                m = _LGKM.search(ins)
                if m and int(m.group(1)) == 0 and pending:        # scalar loads return out of order: only lgkmcnt(0) retires them
                    r["swait"] += before
                    pending = 0
            if not ins.startswith(("s_add_u32", "s_addc_u32", "s_getpc")):      # (the two adds that follow s_getpc keep the pair)
                m = _SDST.match(ins)
                if m and not _SLOAD.match(ins):
                    pcregs -= _regs(m.group(1))
        res[k] = r
    return res


def analyze(sources, hipcc=None):
    """Compile and analyze: -> {(file name, demangled kernel): counts}."""
    hipcc = hipcc or lc.find_hipcc()
    if not hipcc:
        raise RuntimeError("hipcc not found")
    from concurrent.futures import ThreadPoolExecutor
    out = {}
    srcs = [os.path.abspath(s) if os.path.exists(s) else os.path.join(lc.CSRC, os.path.basename(s)) for s in sources]
    with tempfile.TemporaryDirectory() as td, ThreadPoolExecutor(max_workers=min(8, len(srcs))) as pool:
        for src, asm in zip(srcs, pool.map(lambda s: lc.compile_to_asm(hipcc, s, td), srcs)):      # the files compile side by side
            res = analyze_asm(asm)
            names = lc.demangle(list(res))
            for k, v in res.items():
                out[(os.path.basename(src), names[k])] = v
    return out


def read_table(path):
    """A table this tool printed (profiles/entry_path_*.txt) -> {(file, kernel as printed): counts}."""
    out = {}
    for l in open(path):
        m = re.match(r"(\S+)\s+(.{64})\s+(\d+)\s+(\d+)/(\d+)\s+(\d+)\s+(\d+)/(\d+)\s+(\d+)/(\d+)\s*$", l)
        if m:
            v = [int(x) for x in m.groups()[2:]]
            out[(m.group(1), m.group(2).strip())] = dict(zip(("entry", "rcp_entry", "rcp_all", "swait", "sload", "sload_other", "got",
                                                              "got_after_dma"), v))
    return out


def launched(csv_path):
    """Kernel names of a rocprofv3 *_kernel_stats.csv, as this tool prints them."""
    import csv
    names = set()
    for r in csv.DictReader(open(csv_path)):
        n = re.sub(r"^void ", "", r["Name"]).split("(")[0].strip()
        names.add(lc._plain(n)[:64])
    return names


def main(argv):
    only, ran = None, None
    while len(argv) > 1 and argv[0] in ("--kernels", "--launched"):
        if argv[0] == "--kernels":
            only = re.compile(argv[1])
        else:
            ran = launched(argv[1])
            print(f"# kernels named in {os.path.basename(argv[1])}")
        argv = argv[2:]
    if not argv:
        print(__doc__)
        return 2
    res = analyze(argv)
    print(f"{'file':14s} {'kernel':64s} {'entry':>5s} {'rcp':>7s} {'swait':>5s} {'sload':>7s} {'got':>7s}")
    for (f, k), v in sorted(res.items()):
        if (only and not only.search(k)) or (ran is not None and k[:64] not in ran):
            continue
        print(f"{f:14s} {k[:64]:64s} {v['entry']:5d} {v['rcp_entry']:3d}/{v['rcp_all']:<3d} {v['swait']:5d} "
              f"{v['sload']:3d}/{v['sload_other']:<3d} {v['got']:3d}/{v['got_after_dma']:<3d}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main(sys.argv[1:]))
