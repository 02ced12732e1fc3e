#!/usr/bin/env python3
"""Each B G R A kernel instance of a libmm355.so build beside its RGBA twin.

usage: bgra_twins.py LIB.so [--all]

A BGRA instance is its RGBA8 twin with other byte indices and constants
(mm_kernels.hpp PixU8), so its instruction counts, registers and spills are
expected to be the twin's.  For every kernel whose template arguments name a
BGRA code (128: MM_BGRA8, 131: MM_BGRA8_SRGB, the pairs 33040, 33042 and 4480)
the twin is the same kernel with the RGBA code (0, 3, 272, 274, 4352).  Prints
one line per pair with instructions (valu / salu / vmem / lds), VGPRs, SGPRs and
spilled VGPRs of both, and whether the opcode sequences are equal (operands
aside); by default for K1 and the fused compose kernels at N = 2048, 4096 and
8192 and for the kernels without a size (k_compose, k_compose_odd, k_dbg_out,
k_convert), with --all for every pair.  Ends with the number of pairs that differ in
any count.  Disassembly and the fat-binary walk are tools/isa_diff.py's.
"""
import collections
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_diff  # noqa: E402

READELF = "/opt/rocm/llvm/bin/llvm-readelf"
OBJDUMP = "/opt/rocm/llvm/bin/llvm-objdump"
TWIN = {"128": "0", "131": "3", "33040": "272", "33042": "274", "4480": "4352"}
SIZED = ("k_rows_fwd", "k_rows_inv_compose", "k_rows_inv_compose4")   # LOG2N first, then the format
KERNELS = SIZED + ("k_compose", "k_compose_odd", "k_dbg_out", "k_convert")


def metadata(elf):
    """kernel symbol -> {vgpr_count, sgpr_count, vgpr_spill_count} from the code object's notes."""
    with tempfile.NamedTemporaryFile(suffix=".co", delete=False) as f:
        f.write(elf)
        tmp = f.name
    try:
        txt = subprocess.run([READELF, "--notes", tmp], check=True, capture_output=True, text=True).stdout
    finally:
        os.unlink(tmp)
    out, cur = {}, {}
    for line in txt.splitlines():
        m = re.match(r"\s*-?\s*\.(\w+):\s*(\S+)\s*$", line)
        if not m:
            continue
        key, val = m.groups()
        if line.lstrip().startswith("- ") and cur.get("symbol"):
            out[cur["symbol"][:-3] if cur["symbol"].endswith(".kd") else cur["symbol"]] = cur
            cur = {}
        elif line.lstrip().startswith("- "):
            cur = {}
        cur[key] = val.strip("'\"")
    if cur.get("symbol"):
        out[cur["symbol"][:-3] if cur["symbol"].endswith(".kd") else cur["symbol"]] = cur
    return out


def main():
    args = [a for a in sys.argv[1:] if a != "--all"]
    every = "--all" in sys.argv[1:]
    funcs, meta = {}, {}
    for elf in isa_diff.code_objects(args[0], "gfx950"):
        funcs.update(isa_diff.functions(elf, OBJDUMP))
        meta.update(metadata(elf))
    dm = isa_diff.demangle(sorted(funcs))
    by_name = {v: k for k, v in dm.items()}
    rows, differ = [], 0
    for sym in sorted(funcs, key=lambda s: dm[s]):
        name = dm[sym]
        m = re.match(r"void mm::(\w+)<([^>]*)>", name)
        if not m or m.group(1) not in KERNELS:
            continue
        targs = [t.strip() for t in m.group(2).split(",")]
        if not any(t in TWIN for t in targs[:2]):
            continue
        twin_args = [TWIN.get(t, t) if i < 2 else t for i, t in enumerate(targs)]
        if m.group(1) in SIZED:
            twin_args[0] = targs[0]
        twin = by_name.get(name.replace(f"<{m.group(2)}>", "<" + ", ".join(twin_args) + ">", 1))
        if twin is None:
            print(f"NO TWIN {name}")
            differ += 1
            continue

        def counts(s):
            c = collections.Counter(isa_diff.klass(i.split(" ")[0]) for i in funcs[s])
            md = meta.get(s, {})
            return (len(funcs[s]), c["valu"], c["salu"], c["vmem"], c["lds"], md.get("vgpr_count"), md.get("sgpr_count"),
                    md.get("vgpr_spill_count"))
        a, b = counts(sym), counts(twin)
        ops = [i.split(" ")[0] for i in funcs[sym]] == [i.split(" ")[0] for i in funcs[twin]]
        differ += a != b
        if every or m.group(1) not in SIZED or targs[0] in ("11", "12", "13"):
            rows.append((f"{m.group(1)}<{m.group(2)}>", a, b, ops))
    print("kernel<template arguments>: instructions valu salu vmem lds | vgpr sgpr spilled-vgpr   (BGRA instance; RGBA twin)")
    for name, a, b, ops in rows:
        fmt = lambda c: f"{c[0]} {c[1]} {c[2]} {c[3]} {c[4]} | {c[5]} {c[6]} {c[7]}"
        print(f"{name}: {fmt(a)}; twin {fmt(b)}; counts {'equal' if a == b else 'DIFFER'}; "
              f"opcode sequence {'equal' if ops else 'differs'}")
    print(f"pairs that differ in a count, over every BGRA instance of the library: {differ}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
