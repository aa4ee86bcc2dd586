#!/usr/bin/env python3
"""Compare the gfx950 code objects of two builds of libcsa_legacy.so kernel by kernel: VGPRs, AGPRs, SGPRs,
spills, scratch, LDS (from the code object's metadata notes) and code size (the kernel symbol's size).

Usage: python tools/kernel_cmp.py PARENT_LIB TREE_LIB [regex of kernel names]

Prints one line per kernel of PARENT_LIB that differs in TREE_LIB or is missing there, the kernels only
TREE_LIB has, and a summary line; exits 1 when a kernel of PARENT_LIB differs or is missing.
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
FIELDS = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count",
          "private_segment_fixed_size", "group_segment_fixed_size")


def kernels(lib):
    """{demangled kernel name: {field: value, 'code_size': bytes}} of the library's gfx950 code object"""
    with tempfile.TemporaryDirectory() as tmp:
        shutil.copy(lib, os.path.join(tmp, "lib.so"))
        subprocess.check_call([os.path.join(LLVM, "llvm-objdump"), "--offloading", "lib.so"], cwd=tmp,
                              stdout=subprocess.DEVNULL)
        co = [os.path.join(tmp, f) for f in os.listdir(tmp) if f.startswith("lib.so.") and "gfx950" in f][0]
        notes = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", co], text=True)
        syms = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "-sW", co], text=True)
    size = {}
    for line in syms.splitlines():
        f = line.split()
        if len(f) >= 8 and f[3] == "FUNC":
            size[f[7]] = int(f[2], 0)
    out = {}
    for blk in re.split(r"\n  - \.", notes)[1:]:
        f = dict(re.findall(r"\.?([a-z_]+):\s+(\S+)", blk))
        sym = f.get("symbol", "")
        if not sym.endswith(".kd"):
            continue
        row = {k: int(f.get(k, "0"), 0) for k in FIELDS}
        row["code_size"] = size.get(sym[:-3], -1)
        out[sym[:-3]] = row
    names = list(out)
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt", path=LLVM)
    if not filt:
        return out  # mangled names
    dem = subprocess.check_output([filt], input="\n".join(names), text=True).splitlines()
    short = [d.replace("void ", "", 1).replace("(anonymous namespace)::", "") for d in dem]
    return {d: out[m] for d, m in zip(short, names)}


def main():
    parent, tree = kernels(sys.argv[1]), kernels(sys.argv[2])
    pat = re.compile(sys.argv[3] if len(sys.argv) > 3 else ".")
    differ = 0
    for name in sorted(parent):
        if not pat.search(name):
            continue
        if name not in tree:
            differ += 1
            print("MISSING  %s" % name)
        elif tree[name] != parent[name]:
            differ += 1
            d = {k: (parent[name][k], tree[name][k]) for k in parent[name] if parent[name][k] != tree[name][k]}
            print("DIFFERS  %s  %s" % (name, d))
    new = sorted(n for n in tree if n not in parent and pat.search(n))
    for name in new:
        r = tree[name]
        print("NEW      %-62s vgpr %3d agpr %3d sgpr %3d spill %3d scratch %4d lds %6d code %6d" % (
            name[:62], r["vgpr_count"], r["agpr_count"], r["sgpr_count"], r["vgpr_spill_count"],
            r["private_segment_fixed_size"], r["group_segment_fixed_size"], r["code_size"]))
    n = sum(1 for k in parent if pat.search(k))
    print("%d kernels of the parent compared on %s + code_size: %d differ or are missing; %d new kernels" % (
        n, ", ".join(FIELDS), differ, len(new)))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
