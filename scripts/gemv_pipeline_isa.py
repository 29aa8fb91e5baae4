#!/usr/bin/env python3
"""Main-loop ISA summary of the skinny GEMV instantiations (no GPU needed).

Compiles ops/csrc/gemv.hip to gfx950 assembly with the build's flags and prints, for every
``skinny_kernel`` instantiation whose spelled-out name contains ``--filter``: the VGPR and
spill counts from the code-object metadata and the run-length-compressed sequence of global
loads, ``s_waitcnt vmcnt`` and MFMAs of its hottest loop (the innermost backward-branch
loop holding the most MFMAs).  ``--src`` points at another checkout's csrc directory, to
compare two commits (profiles/r7_gemv_pipeline_isa.txt).

    python scripts/gemv_pipeline_isa.py \\
        --filter "bf16, waves=16, unroll=2, mt=1, SILU, nt=yes, ps=yes, w8=no"
"""
from __future__ import annotations

import argparse
import re
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from agentic_traffic_testing_amd.ops import build as B  # noqa: E402

EPI = {0: "PLAIN", 1: "RESADD", 2: "QKVROPE", 3: "SILU", 4: "SAMPLE"}


def assemble(csrc: Path) -> str:
    with tempfile.TemporaryDirectory() as d:
        out = Path(d) / "gemv.s"
        cmd = [B.HIPCC, f"--offload-arch={B.ARCH}", "-O3", "-std=c++17", "-fPIC",
               "-munsafe-fp-atomics", "-Wno-unused-result", "-I", str(csrc),
               "--cuda-device-only", "-S", str(csrc / "gemv.hip"), "-o", str(out)]
        subprocess.run(cmd, check=True)
        return out.read_text()


def demangle(names):
    """skinny_kernel<T, WAVES, UNROLL, MT, EPI, NTL, PS, W8> spelled from the mangled
    template arguments (binutils' c++filt does not know the 16-bit float manglings)."""
    out = {}
    for n in names:
        m = re.search(r"skinny_kernelI(DF16b|DF16_)((?:L[ib]\d+E)+)E", n)
        if not m:
            out[n] = n
            continue
        a = [int(v) for v in re.findall(r"L[ib](\d+)E", m.group(2))]
        a += [0] * (7 - len(a))
        flags = ", ".join(f"{k}={'yes' if v else 'no'}" for k, v in zip(("nt", "ps", "w8"), a[4:7]))
        out[n] = (f"skinny_kernel<{'bf16' if m.group(1) == 'DF16b' else 'fp16'}, waves={a[0]}, "
                  f"unroll={a[1]}, mt={a[2]}, {EPI.get(a[3], a[3])}, {flags}>")
    return out


def functions(asm: str):
    """{symbol: [instruction lines]} of every skinny_kernel instantiation."""
    out, cur = {}, None
    for line in asm.splitlines():
        m = re.match(r"^(_Z\w*skinny_kernel\w*):", line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is not None:
            if line.startswith("\t.end_amdhsa_kernel") or line.startswith(".Lfunc_end"):
                cur = None
                continue
            cur.append(line.strip())
    return out


def metadata(asm: str):
    meta = {}
    for blk in asm.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk)
        if not name:
            continue
        get = lambda k: int(re.search(rf"\.{k}:\s+(\d+)", blk).group(1))  # noqa: E731
        meta[name.group(1)] = (get("vgpr_count"), get("vgpr_spill_count"), get("sgpr_count"))
    return meta


def hot_loop(lines):
    """(label, body) of the backward-branch loop with the most MFMAs, innermost on ties."""
    pos = {m.group(1): i for i, l in enumerate(lines) if (m := re.match(r"^(\.LBB\w+):", l))}
    best = None
    for i, l in enumerate(lines):
        m = re.match(r"^s_c?branch\w*\s+(\.LBB\w+)", l)
        if not m or m.group(1) not in pos or pos[m.group(1)] > i:
            continue
        body = lines[pos[m.group(1)]:i + 1]
        n = sum("v_mfma" in b for b in body)
        if n and (best is None or n > best[0] or (n == best[0] and len(body) < len(best[2]))):
            best = (n, m.group(1), body)
    return (best[1], best[2]) if best else (None, [])


def compress(body):
    seq = []
    for l in body:
        if l.startswith("global_load") or l.startswith("buffer_load"):
            tok = l.split()[0] + (" nt" if " nt" in l else "")
        elif l.startswith("s_waitcnt") and "vmcnt" in l:
            tok = "s_waitcnt " + re.search(r"vmcnt\(\d+\)", l).group(0)
        elif l.startswith("v_mfma"):
            tok = l.split()[0]
        elif re.match(r"^s_(and_saveexec|cbranch_execz)", l):
            tok = l.split()[0]
        else:
            continue
        if seq and seq[-1][0] == tok:
            seq[-1][1] += 1
        else:
            seq.append([tok, 1])
    return [f"{n} x {t}" if n > 1 else t for t, n in seq]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--src", type=Path, default=B.CSRC, help="csrc directory to compile")
    ap.add_argument("--filter", action="append", default=[],
                    help="substring of the demangled template arguments (repeatable)")
    ap.add_argument("--asm", type=Path, help="read this assembly file instead of compiling")
    a = ap.parse_args(argv)
    asm = a.asm.read_text() if a.asm else assemble(a.src)
    fns, meta = functions(asm), metadata(asm)
    names = demangle(list(fns))
    for sym in sorted(fns, key=lambda s: names[s]):
        nm = names[sym]
        if a.filter and not any(f in nm for f in a.filter):
            continue
        v, sp, sg = meta.get(sym, (-1, -1, -1))
        label, body = hot_loop(fns[sym])
        print(f"{nm}\n  vgpr_count {v}  vgpr_spill_count {sp}  sgpr_count {sg}  loop {label}")
        for t in compress(body):
            print("    " + t)
        print()


if __name__ == "__main__":
    main()
