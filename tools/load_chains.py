#!/usr/bin/env python3
"""Dependent memory round trips of each kernel, read from the compiled gfx950 code (runs on a CPU-only box).

  python tools/load_chains.py [--events KERNEL_SUBSTRING] [--kernels REGEX] csrc/norm.hip [csrc/igemm.hip ...]

Compiles each .hip file to assembly with csrc/Makefile's flags (plus --cuda-device-only -S) into a temporary directory and
prints, per kernel:

  trips    s_waitcnt vmcnt(N) instructions that retire at least one VGPR-destination load (global / buffer / flat / scratch
           load into registers; LDS-DMA loads and stores also count in vmcnt on gfx9 but are not what a wave then sits and
           waits for) issued since the previous vmcnt wait.  Every one of them is a point where the wave stands still for a
           memory round trip of its own; loads issued together share the trip, and the counted-down waits (vmcnt(6), (5), ...)
           by which the compiler consumes one batch count once.  Straight-line count over the code as laid out.
  in_loop  how many of those lie inside a loop (between a label and a later branch back to it): they repeat per iteration
  vgprs / agprs / scratch / occupancy   from the compiler's resource comments of the kernel

A small kernel whose duration is its latency (a few hundred KB moved in 5-9 us) costs about trips x one round trip
(DESIGN.md section 9).  The count is of the code, not of a run: a branch not taken skips its waits."""
import collections
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stable-diffusion-1.5-lcm-onnx-rknn2_amd", "csrc")

_VLOAD = re.compile(r"^(global|buffer|flat|scratch)_load_(?!lds_)")
_VMEM = re.compile(r"^(global|buffer|flat|scratch)_(load|store|atomic)")
_VMCNT = re.compile(r"vmcnt\((\d+)\)")
_BRANCH = re.compile(r"^s_c?branch\w*\s+(\.LBB\w+)")


def find_hipcc():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    m = re.search(r"^HIPCC\s*\?=\s*(\S+)", mk, re.M)
    for c in (os.environ.get("HIPCC"), m.group(1) if m else None, shutil.which("hipcc")):
        if c and (os.path.isfile(c) or shutil.which(c)):
            return c
    return None


def makefile_flags(src_name):
    """The flags csrc/Makefile compiles `src_name` with: CXXFLAGS (ARCH substituted) plus what the file's own rule adds."""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", mk, re.M).group(1)
    flags = re.search(r"^CXXFLAGS\s*=\s*(.*)$", mk, re.M).group(1).replace("$(ARCH)", arch).split()
    obj = os.path.splitext(src_name)[0] + ".o"
    m = re.search(r"^" + re.escape(obj) + r":[^\n]*\n\t\$\(HIPCC\) \$\(CXXFLAGS\)(.*?)-c \$<", mk, re.M)
    if m:
        flags += m.group(1).split()
    return flags


def compile_to_asm(hipcc, src, outdir):
    out = os.path.join(outdir, os.path.basename(src) + ".s")
    cmd = [hipcc] + makefile_flags(os.path.basename(src)) + ["--cuda-device-only", "-S", "-o", out, src]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=os.path.dirname(os.path.abspath(src)))
    if r.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)}\n{r.stderr[-3000:]}")
    return out


def demangle(names):
    tool = None
    for c in ("/opt/rocm/llvm/bin/llvm-cxxfilt", shutil.which("llvm-cxxfilt"), shutil.which("c++filt")):
        if c and os.path.exists(c):
            tool = c
            break
    if not tool or not names:
        return {n: _plain(n) for n in names}
    r = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True)
    out = r.stdout.splitlines()
    if r.returncode != 0 or len(out) != len(names):
        return {n: n for n in names}
    return {n: _plain(re.sub(r"^void ", "", d).split("(")[0]) for n, d in zip(names, out)}


def _plain(name):
    """`_Z<len><identifier>...` the demangler did not know (the _Float16 parameter code): the identifier itself."""
    m = re.match(r"_Z(\d+)", name)
    return name[m.end():m.end() + int(m.group(1))] if m else name


def analyze_asm(path):
    """-> {mangled kernel name: dict(trips, in_loop, vgprs, agprs, scratch, occupancy, events)}; events is the ordered list of
    ("load" | "lds_dma" | "store", opcode) and ("wait", N, retired VGPR loads that were issued since the previous wait) entries of the kernel body."""
    lines = open(path).read().splitlines()
    kernels = {m.group(1) for l in lines for m in [re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)] if m}
    start = {}
    for i, l in enumerate(lines):
        m = re.match(r"^([A-Za-z_][\w.$]*):", l)
        if m and m.group(1) in kernels and m.group(1) not in start:
            start[m.group(1)] = i
    res = {}
    for k in sorted(start, key=start.get):
        i = start[k] + 1
        labels, events, waits, backs = {}, [], [], []
        queue = []                                   # outstanding vmcnt operations, oldest first: (is VGPR-destination load, issued
        fresh_from = 0                               # at event number); fresh_from = event number of the previous vmcnt wait
        info = dict(vgprs=None, agprs=0, scratch=None, occupancy=None)
        while i < len(lines):
            l = lines[i].strip()
            if l.startswith(".Lfunc_end"):
                break
            m = re.match(r"^(\.LBB\w+):", l)
            if m:
                labels[m.group(1)] = i
            ins = l.split(";")[0].strip()
            if _VMEM.match(ins):
                op = ins.split()[0]
                isload = bool(_VLOAD.match(ins))
                queue.append((isload, len(events)))
                events.append(("load" if isload else "lds_dma" if "_load_lds_" in op else "store", op))
            elif ins.startswith("s_waitcnt"):
                m = _VMCNT.search(ins)
                if m:
                    n = int(m.group(1))
                    gone = queue[:max(0, len(queue) - n)]
                    queue = queue[len(gone):]
                    fresh = sum(1 for isl, at in gone if isl and at >= fresh_from)
                    events.append(("wait", n, fresh))
                    if fresh:
                        waits.append(i)
                    fresh_from = len(events)
            else:
                m = _BRANCH.match(ins)
                if m and m.group(1) in labels:
                    backs.append((labels[m.group(1)], i))
            i += 1
        for j in range(i, min(i + 80, len(lines))):       # the compiler's resource comments follow the body
            for key, pat in (("vgprs", r";\s*NumVgprs:\s*(\d+)"), ("agprs", r";\s*NumAgprs:\s*(\d+)"),
                             ("scratch", r";\s*ScratchSize:\s*(\d+)"), ("occupancy", r";\s*Occupancy:\s*(\d+)")):
                m = re.match(pat, lines[j].strip())
                if m:
                    info[key] = int(m.group(1))
            if info["occupancy"] is not None:
                break
        info.update(trips=len(waits), in_loop=sum(any(a <= w <= b for a, b in backs) for w in waits), events=events)
        res[k] = info
    return res


def analyze(sources, hipcc=None):
    """Compile and analyze: -> OrderedDict {(file name, demangled kernel): info}."""
    hipcc = hipcc or find_hipcc()
    if not hipcc:
        raise RuntimeError("hipcc not found")
    out = collections.OrderedDict()
    with tempfile.TemporaryDirectory() as td:
        for src in sources:
            src = os.path.abspath(src) if os.path.exists(src) else os.path.join(CSRC, os.path.basename(src))
            res = analyze_asm(compile_to_asm(hipcc, src, td))
            names = demangle(list(res))
            for k, v in res.items():
                v["mangled"] = k
                out[(os.path.basename(src), names[k])] = v
    return out


def main(argv):
    ev, only = None, None
    while len(argv) > 1 and argv[0] in ("--events", "--kernels"):
        if argv[0] == "--events":
            ev = argv[1]
        else:
            only = re.compile(argv[1])
            print(f"# kernels matching {argv[1]}")
        argv = argv[2:]
    if not argv:
        print(__doc__)
        return 2
    res = analyze(argv)
    print(f"{'file':14s} {'kernel':72s} {'trips':>5s} {'in_loop':>7s} {'vgprs':>5s} {'agprs':>5s} {'scratch':>7s} {'occ':>3s}")
    for (f, k), v in sorted(res.items()):
        if only and not only.search(k):
            continue
        print(f"{f:14s} {k[:72]:72s} {v['trips']:5d} {v['in_loop']:7d} {v['vgprs']!s:>5s} {v['agprs']!s:>5s} {v['scratch']!s:>7s} {v['occupancy']!s:>3s}")
        if ev and ev in k:
            for e in v["events"]:
                print("      ", *e)
    return 0


if __name__ == "__main__":
    raise SystemExit(main(sys.argv[1:]))
