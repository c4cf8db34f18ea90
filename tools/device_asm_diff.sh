#!/bin/bash
# Is the device code of the translation units with host code of the launch layer the same as at another commit?  usage: tools/device_asm_diff.sh [BASE_REV] (default HEAD)
# Compiles the units below at BASE_REV and in the working tree with build.py's flags, device side
# only, and diffs the assembly after dropping what a pure host / namespace change may move: comments, .file / .ident, the per-compile
# __hip_cuid symbol, and the (anonymous namespace):: / cfear_dev:: qualifiers of demangled names. Prints lines compared / differing per unit;
# the normalised files and diffs stay in $OUT (default /tmp/cfear_asm_diff).
set -u
ROOT=$(cd "$(dirname "$0")/.." && pwd)
BASE=${1:-HEAD}
OUT=${OUT:-/tmp/cfear_asm_diff}
PKG=cfear_radarodometry_code_public_amd
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -Wall -Wno-unused-function -Wno-unused-variable"
mkdir -p "$OUT/base" "$OUT/head" && rm -rf "$OUT/base_src" && mkdir -p "$OUT/base_src" || exit 2
git -C "$ROOT" archive "$BASE" $PKG/csrc include | tar -x -C "$OUT/base_src" || exit 2
norm() { sed -e 's/[ \t]*;.*$//' -e '/^[ \t]*\.file/d' -e '/^[ \t]*\.ident/d' -e 's/__hip_cuid_[0-9a-f]*/__hip_cuid/g' -e 's/\.L\(_Z[A-Za-z0-9_]*\)\./.L \1 ./g' "$1" | c++filt | sed -e 's/(anonymous namespace):://g' -e 's/cfear_dev:://g' -e '/^[ \t]*$/d'; }
UNITS="pipeline register_step register_step_large replay cabi cfar drift kstrongest"
rc=0
for u in $UNITS; do
  ( hipcc $FLAGS --cuda-device-only -S "$OUT/base_src/$PKG/csrc/$u.hip" -o "$OUT/base/$u.raw.s" && norm "$OUT/base/$u.raw.s" > "$OUT/base/$u.s" ) &
  ( hipcc $FLAGS --cuda-device-only -S "$ROOT/$PKG/csrc/$u.hip" -o "$OUT/head/$u.raw.s" && norm "$OUT/head/$u.raw.s" > "$OUT/head/$u.s" ) &
done
wait
for u in $UNITS; do
  [ -s "$OUT/base/$u.s" ] && [ -s "$OUT/head/$u.s" ] || { echo "$u: compile failed"; rc=2; continue; }
  diff "$OUT/base/$u.s" "$OUT/head/$u.s" > "$OUT/$u.diff"
  n=$(grep -c '^[<>]' "$OUT/$u.diff")
  nosec=$(grep '^[<>]' "$OUT/$u.diff" | grep -vc "^[<>][[:space:]]*\.section")
  echo "$u: $(wc -l < "$OUT/head/$u.s") lines compared, $n differing ($nosec of them not .section name spellings)"
  [ "$nosec" -eq 0 ] || rc=1
done
exit $rc
