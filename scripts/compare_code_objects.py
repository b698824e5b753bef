#!/usr/bin/env python3
"""Compare the kernels of two gfx950 code objects byte for byte.

    hipcc <the build's flags for csrc/heligym_amd.hip> --cuda-device-only --no-gpu-bundle-output -c \
          -o before.co csrc/heligym_amd.hip
    (the same at the other commit -> after.co; without --no-gpu-bundle-output, unbundle the outputs with
    clang-offload-bundler --type=o --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --unbundle first)
    python scripts/compare_code_objects.py before.co after.co [--allow NAME ...]

For every function symbol of `before` it compares the symbol's bytes of .text (the machine code) and its
kernel descriptor (NAME.kd in .rodata: register counts, scratch, LDS, argument segment) with `after`'s.
Prints the symbols that differ, are missing or are new, and exits 1 if a symbol of `before` whose
demangled name contains none of the --allow strings changed or is missing.  Needs llvm-readelf (ROCm's
llvm/bin, or $LLVM_READELF)."""
import argparse
import os
import re
import subprocess
import sys

READELF = os.environ.get("LLVM_READELF", "/opt/rocm/lib/llvm/bin/llvm-readelf")


def symbols(path):
    """{name: bytes} of every FUNC symbol and every kernel descriptor object of the code object."""
    blob = open(path, "rb").read()
    secs = {}
    for line in subprocess.check_output([READELF, "-S", "--wide", path], text=True).splitlines():
        m = re.match(r"\s*\[\s*(\d+)\]\s+(\S+)\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", line)
        if m:
            secs[int(m.group(1))] = (int(m.group(3), 16), int(m.group(4), 16))   # address, file offset
    out = {}
    for line in subprocess.check_output([READELF, "-s", "--wide", path], text=True).splitlines():
        f = line.split()
        if len(f) < 8 or f[3] not in ("FUNC", "OBJECT") or not f[6].isdigit():
            continue
        name, addr, size, sec = f[7], int(f[1], 16), int(f[2]), int(f[6])
        if f[3] == "OBJECT" and not name.endswith(".kd"):
            continue
        base, off = secs[sec]
        data = blob[off + addr - base: off + addr - base + size]
        if name.endswith(".kd"):   # bytes 16-23: the code's offset from the descriptor, which moves with the layout
            data = data[:16] + bytes(8) + data[24:]
        out[name] = data
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("before")
    ap.add_argument("after")
    ap.add_argument("--allow", nargs="*", default=[], help="substrings of symbols that may differ")
    a = ap.parse_args()
    old, new = symbols(a.before), symbols(a.after)
    same = [n for n in old if new.get(n) == old[n]]
    changed = [n for n in old if n in new and new[n] != old[n]]
    missing = [n for n in old if n not in new]
    added = [n for n in new if n not in old]
    for tag, names in (("changed", changed), ("missing", missing), ("new", added)):
        for n in sorted(names):
            print(f"{tag}: {n}")
    nk = lambda names: sum(1 for n in names if not n.endswith(".kd"))   # noqa: E731
    print(f"{nk(old)} functions before, {nk(new)} after: {nk(same)} identical (code and descriptor: {len(same)} symbols), "
          f"{nk(changed)} changed, {nk(missing)} missing, {nk(added)} new")
    bad = [n for n in changed + missing if not any(s in n for s in a.allow)]
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
