#!/bin/bash
# Is the device code of every translation unit (csrc/*.hip of this tree) the same as at another commit?  usage: tools/device_asm_diff.sh [BASE_REV] (default HEAD)
# Compiles the units at BASE_REV and in the working tree with build.py's flags, device side
# only, and compares the assembly after dropping what a pure host / namespace change may move: comments, .file / .ident, the per-compile
# __hip_cuid symbol, the (anonymous namespace):: / cfear_dev:: qualifiers of demangled names, and the function index in block and function-end
# labels (.LBB3_28, .Lfunc_end3), which moves whenever a function is added to or removed from a unit. The assembly is compared function by
# function (a function's text, its kernel descriptor and its metadata entry; the rest of the unit counts as one more): per unit the lines
# compared and differing in functions both trees have, then the functions only one tree has. The exit status is 1 only when a function both
# trees have differs. A unit the base does not have is compared with nothing (its functions are "only in this tree"), and every unit's line ends
# with the number of kernels it defines (odometry_run and odometry_seq: 0). The normalised files and whole-file diffs stay in $OUT (default /tmp/cfear_asm_diff).
set -u
ROOT=$(cd "$(dirname "$0")/.." && pwd)
BASE=${1:-HEAD}
OUT=${OUT:-/tmp/cfear_asm_diff}
PKG=cfear_radarodometry_code_public_amd
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -Wall -Wno-unused-function -Wno-unused-variable"
mkdir -p "$OUT/base" "$OUT/head" && rm -rf "$OUT/base_src" && mkdir -p "$OUT/base_src" || exit 2
git -C "$ROOT" archive "$BASE" $PKG/csrc include | tar -x -C "$OUT/base_src" || exit 2
norm() { sed -e 's/[ \t]*;.*$//' -e '/^[ \t]*\.file/d' -e '/^[ \t]*\.ident/d' -e 's/__hip_cuid_[0-9a-f]*/__hip_cuid/g' -e 's/\.L\(_Z[A-Za-z0-9_]*\)\./.L \1 ./g' -e 's/\.LBB[0-9]*_/.LBB_/g' -e 's/\.Lfunc_end[0-9]*/.Lfunc_end/g' "$1" | c++filt | sed -e 's/(anonymous namespace):://g' -e 's/cfear_dev:://g' -e '/^[ \t]*$/d'; }
# $1 $2: normalised assembly of the base and of this tree -> the unit's report; exit status 1 when a function both have differs
compare() {
  python3 - "$1" "$2" <<'PY'
import difflib, re, sys

def parts(path):
    """{function name: its lines}, in '' what belongs to no function"""
    L = open(path).read().split("\n")
    starts = []
    for i, l in enumerate(L):
        m = re.match(r"\s*\.type\s+(.*),@function$", l)
        if m:
            while i > 0 and re.match(r"\s*\.(globl|protected|weak|hidden|p2align)\b", L[i - 1]):
                i -= 1
            if i > 0 and re.match(r"\s*\.(section|text)\b", L[i - 1]):  # (the one before that closes the function before)
                i -= 1
            starts.append((i, m.group(1)))
    end = next((i for i, l in enumerate(L) if re.match(r"\s*\.(section\s+\.AMDGPU\.gpr_maximums|amdgpu_metadata)", l)), len(L))
    out = {"": L[:starts[0][0] if starts else end]}
    for (a, name), (b, _) in zip(starts, starts[1:] + [(end, None)]):
        out[name] = L[a:b]
    i = end
    while i < len(L):  # the unit's tail: a kernel's metadata entry (from its "  - ." line to the next) goes to the kernel
        j = i + 1
        if L[i].startswith("  - ."):
            while j < len(L) and L[j].startswith("   "):
                j += 1
            name = next(l.split(":", 1)[1].strip() for l in L[i:j] if l.startswith("    .name:"))
            out[name] = out.get(name, []) + L[i:j]
        else:
            out[""] += L[i:j]
        i = j
    return out

def differing(a, b):
    if a == b:
        return 0
    return sum(max(i2 - i1, 0) + max(j2 - j1, 0) for op, i1, i2, j1, j2 in difflib.SequenceMatcher(None, a, b, autojunk=False).get_opcodes() if op != "equal")

base, head = parts(sys.argv[1]), parts(sys.argv[2])
nosection = lambda ls: [l for l in ls if not re.match(r"\s*\.section", l)]
both = [n for n in head if n in base]
n = sum(differing(base[f], head[f]) for f in both)
nosec = sum(differing(nosection(base[f]), nosection(head[f])) for f in both)
msg = "%d lines compared, %d differing in functions both trees have (%d of them not .section name spellings)" % (sum(len(head[f]) for f in both), n, nosec)
for what, one, other in (("the base", base, head), ("this tree", head, base)):
    only = [f for f in one if f not in other]
    if only:
        msg += "; %d lines only in %s: %s" % (sum(len(one[f]) for f in only), what, ", ".join(f.split("(")[0] for f in only))
print(msg)
sys.exit(1 if nosec else 0)
PY
}
UNITS=$(cd "$ROOT/$PKG/csrc" && ls *.hip | sed 's/\.hip$//')
rc=0
for u in $UNITS; do
  [ -f "$OUT/base_src/$PKG/csrc/$u.hip" ] || echo > "$OUT/base_src/$PKG/csrc/$u.hip"  # (a unit that is new in this tree)
  ( hipcc $FLAGS --cuda-device-only -S "$OUT/base_src/$PKG/csrc/$u.hip" -o "$OUT/base/$u.raw.s" && norm "$OUT/base/$u.raw.s" > "$OUT/base/$u.s" ) &
  ( hipcc $FLAGS --cuda-device-only -S "$ROOT/$PKG/csrc/$u.hip" -o "$OUT/head/$u.raw.s" && norm "$OUT/head/$u.raw.s" > "$OUT/head/$u.s" ) &
done
wait
for u in $UNITS; do
  [ -s "$OUT/base/$u.s" ] && [ -s "$OUT/head/$u.s" ] || { echo "$u: compile failed"; rc=2; continue; }
  diff "$OUT/base/$u.s" "$OUT/head/$u.s" > "$OUT/$u.diff"
  r=$(compare "$OUT/base/$u.s" "$OUT/head/$u.s") || rc=1
  echo "$u: $r; $(grep -c '\.amdhsa_kernel ' "$OUT/head/$u.s") kernels"
done
exit $rc
