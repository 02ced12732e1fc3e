#!/usr/bin/env python3
"""Function-by-function diff of the gfx950 code in two libmm355.so builds.

usage: isa_diff.py OLD.so NEW.so [--arch gfx950] [--objdump PATH]

Every translation unit's code object is taken out of the library's fat binary
(the clang offload bundles inside it), disassembled with llvm-objdump, and the
functions the two builds share are compared instruction by instruction.  Three
classes: identical; identical but for the literals of s_add_u32 / s_addc_u32
(the PC-relative offsets of constant data that moved); different.  A function
is the st_size bytes from its symbol, so blocks laid out after its last s_endpgm
are compared and the fill up to the next symbol is not.  Functions
only one build has are listed by name.  Per-kernel instruction counts (valu,
salu, vmem, lds) of the new functions are printed at the end.
"""
import collections
import os
import re
import struct
import subprocess
import sys
import tempfile

MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def code_objects(path, arch):
    """The ELF images of every bundle entry whose triple names `arch`."""
    blob = open(path, "rb").read()
    out = []
    pos = blob.find(MAGIC)
    while pos >= 0:
        (n,) = struct.unpack_from("<Q", blob, pos + len(MAGIC))
        p = pos + len(MAGIC) + 8
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", blob, p)
            triple = blob[p + 24:p + 24 + tl].decode()
            p += 24 + tl
            if arch in triple and size:
                out.append(blob[pos + off:pos + off + size])
        pos = blob.find(MAGIC, pos + len(MAGIC))
    return out


def functions(elf, objdump):
    """name -> list of instruction texts (addresses, encodings and comments dropped)."""
    with tempfile.NamedTemporaryFile(suffix=".co", delete=False) as f:
        f.write(elf)
        tmp = f.name
    try:
        txt = subprocess.run([objdump, "-d", "--no-show-raw-insn", "--no-leading-addr", tmp],
                             check=True, capture_output=True, text=True).stdout
        syms = subprocess.run([objdump, "-t", tmp], check=True, capture_output=True, text=True).stdout
    finally:
        os.unlink(tmp)
    # a function is the st_size bytes from its symbol: basic blocks after its
    # last s_endpgm belong to it, the fill up to the next symbol's alignment
    # (which moves with the neighbours and may decode as instructions) does not
    end = {}
    for line in syms.splitlines():
        m = re.match(r"^([0-9a-f]+) .{7} (\S+)\s+([0-9a-f]+)\s+(?:\.\w+\s+)?(\S+)$", line)
        if m and "F" in line[17:24]:
            end[m.group(4)] = int(m.group(1), 16) + int(m.group(3), 16)
    funcs, cur, stop = {}, None, None
    for line in txt.splitlines():
        m = re.match(r"^(?:[0-9a-f]+ )?<([^>]+)>:$", line)
        if m:
            cur, stop = funcs.setdefault(m.group(1), []), end.get(m.group(1))
            continue
        if cur is None or not line.startswith(("\t", " ")):
            continue
        ins, _, where = line.partition("//")
        ins = ins.strip()
        if not ins or ins == "...":     # (a run of zero bytes)
            continue
        # (the comment holds the instruction's address and its encoding)
        a = re.match(r"\s*([0-9A-Fa-f]+):", where)
        if stop is not None and a and int(a.group(1), 16) >= stop:
            continue
        cur.append(re.sub(r"\s+", " ", ins))
    return funcs


def loose(ins):
    if ins.startswith(("s_add_u32", "s_addc_u32")):
        return re.sub(r"\b(0x[0-9a-f]+|\d+)$", "LIT", ins)
    return ins


def klass(op):
    if op.startswith("v_"):
        return "valu"
    if op.startswith("s_"):
        return "salu"
    if op.startswith(("global_", "flat_", "scratch_", "buffer_")):
        return "vmem"
    if op.startswith("ds_"):
        return "lds"
    return "other"


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
        return dict(zip(names, out.splitlines()))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main():
    args = sys.argv[1:]
    arch, objdump = "gfx950", "/opt/rocm/llvm/bin/llvm-objdump"
    for flag in ("--arch", "--objdump"):
        if flag in args:
            i = args.index(flag)
            val = args[i + 1]
            del args[i:i + 2]
            if flag == "--arch":
                arch = val
            else:
                objdump = val
    old_so, new_so = args
    sides = []
    for so in (old_so, new_so):
        fs = {}
        for elf in code_objects(so, arch):
            for name, ins in functions(elf, objdump).items():
                fs[name] = ins   # (a kernel lives in one translation unit)
        sides.append(fs)
    old, new = sides
    shared = sorted(set(old) & set(new))
    same = [n for n in shared if old[n] == new[n]]
    moved = [n for n in shared if old[n] != new[n] and
             [loose(i) for i in old[n]] == [loose(i) for i in new[n]]]
    diff = [n for n in shared if n not in set(same) and n not in set(moved)]
    added, gone = sorted(set(new) - set(old)), sorted(set(old) - set(new))
    dm = demangle(diff + added + gone)
    print(f"functions: old {len(old)}, new {len(new)}, shared {len(shared)}")
    print(f"identical instructions: {len(same)}")
    print(f"identical but for PC-relative literals (s_add_u32 / s_addc_u32): {len(moved)}")
    print(f"different: {len(diff)}")
    for n in diff:
        print(f"  DIFF {dm[n]}: {len(old[n])} -> {len(new[n])} instructions")
    print(f"only in old: {len(gone)}")
    for n in gone:
        print(f"  GONE {dm[n]}")
    print(f"only in new: {len(added)}")
    for n in added:
        c = collections.Counter(klass(i.split(" ")[0]) for i in new[n])
        print(f"  NEW {dm[n]}: {len(new[n])} instructions, " +
              ", ".join(f"{k} {c[k]}" for k in ("valu", "salu", "vmem", "lds")))
    return 1 if diff or gone else 0


if __name__ == "__main__":
    sys.exit(main())
