#!/bin/bash
# Per-kernel comparison of the gfx950 code objects of two built libraries: reports every kernel symbol
# present in only one of them, and every one whose instruction text or register / LDS / scratch figures
# differ.  Exits non-zero if anything is reported.  Per symbol, not per file: the order in which the
# compiler emits kernels changes the code object's bytes without changing any kernel.
# Usage: bash tools/kernel_isa_cmp.sh A.so B.so
set -eu
[ $# -eq 2 ] || { echo "usage: $0 A.so B.so" >&2; exit 2; }
LLVM=/opt/rocm/lib/llvm/bin
TMP=$(mktemp -d); trap 'rm -rf "$TMP"' EXIT
for side in a b; do
    mkdir "$TMP/$side"
    cp "$1" "$TMP/$side/lib.so"; shift
    (cd "$TMP/$side" && "$LLVM/llvm-objdump" --offloading lib.so > /dev/null)
    CO=$(ls "$TMP/$side"/lib.so.*gfx950*)
    "$LLVM/llvm-objdump" -d --no-show-raw-insn --no-leading-addr "$CO" > "$TMP/$side/isa.txt"
    "$LLVM/llvm-readelf" --notes "$CO" > "$TMP/$side/notes.txt"
done
python3 - "$TMP" <<'EOF'
import re, sys
FIGURES = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "group_segment_fixed_size",
           "private_segment_fixed_size")


def kernels(side):
    meta = {}
    for blk in re.split(r"\n  - \.", open("%s/%s/notes.txt" % (sys.argv[1], side)).read())[1:]:
        f = dict(re.findall(r"\.?([a-z_]+):\s+(\S+)", blk))
        if "symbol" in f:
            meta[f["symbol"].strip("'\"")[:-len(".kd")]] = tuple(f.get(key) for key in FIGURES)
    text, cur = {}, None
    for line in open("%s/%s/isa.txt" % (sys.argv[1], side)):
        m = re.match(r"[0-9a-f]* ?<(.+)>:$", line.strip())
        if m:
            cur = text.setdefault(m.group(1), [])
        elif cur is not None and line.strip():
            cur.append(re.sub(r"\s*//.*$", "", line).strip())
    return {name: (text.get(name), meta[name]) for name in meta}


a, b = kernels("a"), kernels("b")
bad = 0
for name in sorted(set(a) | set(b)):
    if name not in a or name not in b:
        print("only in %s: %s" % ("A" if name in a else "B", name))
    elif not a[name][0] or a[name][0] != b[name][0]:
        print("instructions differ: %s" % name)
    elif a[name][1] != b[name][1]:
        print("metadata differ: %s  %s -> %s" % (name, a[name][1], b[name][1]))
    else:
        continue
    bad += 1
draw = lambda d: sum("draw_" in n for n in d)
print("A: %d kernel symbols (%d draw_*), B: %d (%d draw_*), %d reported" % (len(a), draw(a), len(b), draw(b), bad))
sys.exit(1 if bad else 0)
EOF
