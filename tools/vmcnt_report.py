#!/usr/bin/env python3
"""Where the trace kernels wait for memory, read from the machine code.

Compiles odigos_amd/csrc/trace_kernel.hip device-only to gfx950 assembly with
the product's flags and, for every trace_eval_kernel / trace_multi_kernel
instance, lists the main loop's loads, stores, atomics and s_waitcnt vmcnt
waits in text order with their line numbers in the listing, beside the
kernel's register / scratch / LDS / occupancy figures.

The source marks three places with assembly comments ("; ose.prefetch
issued", "; ose.flush begin", "; ose.flush end").  Where a kernel has them,
check_drain() walks the control-flow graph from the prefetch marker to the
header of the loop it is in (the back edge taken) and reports every
`s_waitcnt vmcnt(0)` met on the way outside a flush block: such a wait
retires the prefetched loads before the next step starts.
tests/test_trace_prefetch.py asserts there is none in the lean instances.

usage: python tools/vmcnt_report.py [--src FILE] [--label NAME] [--out FILE] [--append]
profiles/trace_prefetch_isa.txt is two runs of it appended to one file: --src
on the parent commit's trace_kernel.hip (headers from this tree), then this
tree's.
"""
from __future__ import annotations

import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "odigos_amd" / "csrc"
SRC = CSRC / "trace_kernel.hip"

KERNELS = [
    ("trace_eval_kernel<true, true, false>", "trace_eval_kernelILb1ELb1ELb0EE"),
    ("trace_eval_kernel<true, false, false>", "trace_eval_kernelILb1ELb0ELb0EE"),
    ("trace_eval_kernel<true, true, true>", "trace_eval_kernelILb1ELb1ELb1EE"),
    ("trace_eval_kernel<true, false, true>", "trace_eval_kernelILb1ELb0ELb1EE"),
    ("trace_eval_kernel<false, false, false>", "trace_eval_kernelILb0ELb0ELb0EE"),
    ("trace_multi_kernel<2>", "trace_multi_kernelILi2EE"),
    ("trace_multi_kernel<3>", "trace_multi_kernelILi3EE"),
]
M_PREFETCH, M_FBEGIN, M_FEND = "ose.prefetch issued", "ose.flush begin", "ose.flush end"

_LABEL = re.compile(r"^(\.LBB\d+_\d+):")
_BRANCH = re.compile(r"^\s+(s_cbranch_\w+|s_branch)\s+(\.LBB\d+_\d+)")
_MEM = re.compile(r"^\s+(global_|buffer_|scratch_|flat_)")
_WAIT = re.compile(r"^\s+s_waitcnt\b")
_DRAIN = re.compile(r"^\s+s_waitcnt\b.*vmcnt\(0\)")


def hipcc() -> str | None:
    from_env = os.environ.get("HIPCC")
    if from_env:
        return from_env if Path(from_env).exists() else shutil.which(from_env)
    return "/opt/rocm/bin/hipcc" if Path("/opt/rocm/bin/hipcc").exists() else shutil.which("hipcc")


def hip_flags() -> list[str]:
    sys.path.insert(0, str(ROOT))
    try:
        from odigos_amd.build import HIP_FLAGS
    finally:
        sys.path.pop(0)
    return list(HIP_FLAGS)


def compile_asm(src: Path = SRC) -> tuple[list[str], str]:
    """(assembly lines, the compiler's kernel-resource-usage remarks)"""
    with tempfile.TemporaryDirectory() as td:
        out = Path(td) / "trace_kernel.s"
        cmd = [hipcc(), *hip_flags(), f"-I{CSRC}", "--offload-device-only", "-S",
               "-Rpass-analysis=kernel-resource-usage", str(src), "-o", str(out)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"{' '.join(cmd)}\n{r.stderr}")
        return out.read_text().splitlines(), r.stderr


def function_lines(asm: list[str], mangled: str) -> list[tuple[int, str]]:
    """(1-based line number, text) of one kernel's body"""
    start = next(i for i, l in enumerate(asm) if l.startswith("_Z") and mangled in l and l.split(":")[0].endswith("E"))
    end = next(i for i in range(start, len(asm)) if asm[i].startswith(".Lfunc_end"))
    return [(i + 1, asm[i]) for i in range(start, end)]


def resources(remarks: str, mangled: str) -> str:
    keep = ("VGPRs:", "AGPRs:", "ScratchSize", "Occupancy", "SGPRs Spill", "VGPRs Spill", "LDS Size")
    out, on = [], False
    for l in remarks.splitlines():
        m = re.search(r"remark:\s+(.*?)\s+\[-Rpass", l)
        if not m:
            continue
        t = m.group(1)
        if t.startswith("Function Name:"):
            on = mangled in t
        elif on and t.startswith(keep):
            out.append(t)
    return "; ".join(out)


def main_loop(fn: list[tuple[int, str]]) -> tuple[int, int]:
    """index range [lo, hi) in fn of the depth-1 loop with the most blocks (LLVM's loop comments)"""
    count: dict[str, list[int]] = {}
    for k, (_, l) in enumerate(fn):
        m = re.search(r"(?:Header=|Parent Loop )(BB\d+_\d+) Depth=1", l)
        if m:
            count.setdefault(m.group(1), []).append(k)
    if not count:
        return 0, len(fn)
    head = max(count, key=lambda h: len(count[h]))
    lo = next(k for k, (_, l) in enumerate(fn) if l.startswith(f".L{head}:"))
    hi = max(count[head]) + 1
    while hi < len(fn) and not _LABEL.match(fn[hi][1]) and "; %bb." not in fn[hi][1]:
        hi += 1
    return lo, hi


def listing(fn: list[tuple[int, str]]) -> list[str]:
    lo, hi = main_loop(fn)
    out = [f"  main loop: lines {fn[lo][0]}-{fn[hi - 1][0]}"]
    flush = 0
    n0 = nc = 0
    for no, l in fn[lo:hi]:
        if M_FBEGIN in l:
            flush += 1
        mark = any(m in l for m in (M_PREFETCH, M_FBEGIN, M_FEND))
        if mark or _MEM.match(l) or (_WAIT.match(l) and "vmcnt" in l):
            if _DRAIN.match(l):
                n0 += 1
            elif _WAIT.match(l):
                nc += 1
            out.append(f"  {no:6d}{' F' if flush else '  '} {l.strip()}")
        if M_FEND in l:
            flush = max(0, flush - 1)
    out.append(f"  vmcnt(0) waits: {n0}, counted waits: {nc}  (F: inside a flush block)")
    return out


def check_drain(fn: list[tuple[int, str]]) -> list[tuple[int, str]] | None:
    """`s_waitcnt vmcnt(0)` lines on a path from the prefetch marker to the
    header of its loop, outside the flush blocks; None if the kernel has no marker"""
    text = [l for _, l in fn]
    starts = [k for k, l in enumerate(text) if M_PREFETCH in l]
    if not starts:
        return None
    label_at = {m.group(1): k for k, l in enumerate(text) if (m := _LABEL.match(l))}
    tops = set()
    for k in starts:   # the block comment above the marker names the depth-1 loop's header
        m = next(m for j in range(k, -1, -1) if (m := re.search(r"Header=(BB\d+_\d+) Depth=1", text[j])))
        tops.add(label_at[".L" + m.group(1)])

    def succ(k: int) -> list[int]:
        l = text[k]
        m = _BRANCH.match(l)
        if m:
            t = label_at[m.group(2)]
            return [t] if m.group(1) == "s_branch" else [t, k + 1]
        if re.match(r"^\s+(s_endpgm|s_setpc_b64|s_trap)", l):
            return []
        return [k + 1] if k + 1 < len(text) else []

    # instructions from which the loop header is reachable: the loop's own
    pred: dict[int, list[int]] = {}
    for k in range(len(text)):
        for s in succ(k):
            pred.setdefault(s, []).append(k)
    in_loop, todo = set(tops), list(tops)
    while todo:
        for p in pred.get(todo.pop(), []):
            if p not in in_loop:
                in_loop.add(p)
                todo.append(p)
    seen, todo, found = set(), [(k, False) for k in starts], {}
    while todo:
        k, fl = todo.pop()
        if (k, fl) in seen or k not in in_loop:
            continue
        seen.add((k, fl))
        l = text[k]
        if k in tops:   # the back edge was taken
            continue
        if M_FBEGIN in l:
            fl = True
        elif M_FEND in l:
            fl = False
        if not fl and _DRAIN.match(l):
            found[fn[k][0]] = l.strip()
        todo.extend((s, fl) for s in succ(k))
    return sorted(found.items())


def report(src: Path, label: str) -> tuple[str, dict[str, list | None]]:
    asm, remarks = compile_asm(src)
    out = [f"==== {label}: {src.name}, hipcc {' '.join(hip_flags())} --offload-device-only -S ===="]
    drains = {}
    for name, mangled in KERNELS:
        fn = function_lines(asm, mangled)
        out.append(f"-- {name}")
        out.append(f"  {resources(remarks, mangled)}")
        out.extend(listing(fn))
        d = check_drain(fn)
        drains[name] = d
        if d is None:
            out.append("  prefetch -> back edge: no markers in this source")
        elif d:
            out.append("  prefetch -> back edge, outside flush blocks: vmcnt(0) at " + ", ".join(str(n) for n, _ in d))
        else:
            out.append("  prefetch -> back edge, outside flush blocks: no vmcnt(0)")
    return "\n".join(out) + "\n", drains


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--src", type=Path, default=SRC)
    ap.add_argument("--label", default="this tree")
    ap.add_argument("--out", type=Path, default=None)
    ap.add_argument("--append", action="store_true")
    args = ap.parse_args()
    text, _ = report(args.src, args.label)
    if args.out:
        with open(args.out, "a" if args.append else "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)
