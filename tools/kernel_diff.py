#!/usr/bin/env python3
"""Diff the gfx950 code of two builds, symbol by symbol (no GPU needed).

    tools/kernel_diff.py [--rename OLD=NEW]... build_parent build [object ...]

--rename replaces the substring OLD by NEW in the first build's (mangled)
symbol names, so that a renamed kernel compares like the rest.  For each object (default: textpath local lynch synth) the device code object
is unbundled from BUILD/NAME.o and disassembled; every function symbol's
instruction text (addresses, encodings and comments stripped) is compared.
Printed: the symbols only in one build, the symbols whose code differs, and
the count of identical ones.  Calls to out-of-line helpers are pc-relative
(s_getpc_b64 + a literal offset), so a helper that moved shows as a changed
literal in its callers: those lines are masked unless --strict is given.
Exit status 1 when a common symbol differs."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def disasm(obj, strict):
    with tempfile.TemporaryDirectory() as d:
        fb, co = os.path.join(d, "fat.bin"), os.path.join(d, "dev.co")
        subprocess.run([os.path.join(LLVM, "llvm-objcopy"), f"--dump-section=.hip_fatbin={fb}", obj,
                        os.path.join(d, "host.o")], check=True)
        subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", f"--targets={TARGET}",
                        f"--input={fb}", f"--output={co}"], check=True)
        out = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", co],
                             check=True, capture_output=True, text=True).stdout
    syms, cur = {}, None
    for line in out.splitlines():
        m = re.match(r"^[0-9a-f]* ?<(.+)>:$", line.strip())
        if m:
            cur = syms.setdefault(m.group(1), [])
            continue
        if cur is None or not line.strip():
            continue
        t = re.sub(r"\s*//.*$", "", line).strip()
        t = re.sub(r"\s+", " ", t)
        if not strict and re.match(r"^s_(add|addc|sub|subb)_u32 s\d+, s\d+, (0x[0-9a-f]+|-?\d+)$", t):
            t = re.sub(r"(0x[0-9a-f]+|-?\d+)$", "<lit>", t)   # a pc-relative offset (call or constant address)
        cur.append(t)
    for v in syms.values():   # the padding up to the next symbol's alignment is not the function's code
        while v and v[-1] in ("s_nop 0", "...", "s_code_end"):
            v.pop()
    return syms


def main():
    args, renames, it = [], [], iter(sys.argv[1:])
    for x in it:
        if x == "--rename":
            renames.append(next(it).split("=", 1))
        elif x != "--strict":
            args.append(x)
    strict = "--strict" in sys.argv[1:]
    if len(args) < 2:
        sys.exit(__doc__)
    a, b = args[0], args[1]
    names = args[2:] or ["textpath", "local", "lynch", "synth"]
    bad = 0
    for n in names:
        A, B = disasm(os.path.join(a, n + ".o"), strict), disasm(os.path.join(b, n + ".o"), strict)
        for old, new in renames:
            A = {s.replace(old, new): v for s, v in A.items()}
        only_a, only_b = sorted(set(A) - set(B)), sorted(set(B) - set(A))
        diff = sorted(s for s in set(A) & set(B) if A[s] != B[s])
        same = len(set(A) & set(B)) - len(diff)
        print(f"{n}: {same} symbols identical, {len(diff)} differ, {len(only_a)} only in {a}, {len(only_b)} only in {b}")
        for s in diff:
            k = next((i for i, (x, y) in enumerate(zip(A[s], B[s])) if x != y), min(len(A[s]), len(B[s])))
            print(f"  differs: {s} ({len(A[s])} vs {len(B[s])} instructions, first at {k})")
        for s in only_a:
            print(f"  only in {a}: {s}")
        for s in only_b:
            print(f"  only in {b}: {s}")
        bad += len(diff)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
