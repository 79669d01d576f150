#!/bin/bash
# TEST INFRASTRUCTURE — builds tests/emu/libminppo_emu.so: the csrc/ kernel sources compiled by g++
# against the SIMT emulator shim (no GPU, no hipcc).  Usage: tests/emu/build_emu.sh [extra g++ flags]
# One object per source, MPPO_EMU_JOBS (default 8) at a time: in ONE g++ call the driver compiles the files one after the other, and the
# environment kernel alone takes minutes.  Objects go to tests/emu/_build/<pid>/ and are removed again (every call compiles everything:
# the extra flags are part of the result).
set -e
HERE="$(cd "$(dirname "$0")" && pwd)"
ROOT="$(cd "$HERE/../.." && pwd)"
SRC="$ROOT/minppo_amd/csrc"
OUT="$HERE/libminppo_emu.so"
OBJ="$HERE/_build/$$"
FILES=""
for f in $(cat "$SRC/SOURCES.txt"); do FILES="$FILES $SRC/$f"; done
FILES="$FILES $HERE/emu_runtime.cpp"
[ -f "$HERE/emu_stubs.cpp" ] && FILES="$FILES $HERE/emu_stubs.cpp"
mkdir -p "$OBJ"
trap 'rm -rf "$OBJ"' EXIT
export HERE SRC OBJ
# (k_physics.hip first: the longest one must not start last)
printf '%s\n' $(ls -S $FILES) | xargs -P "${MPPO_EMU_JOBS:-8}" -I{} bash -c \
    'g++ -std=c++17 -O2 -g -fPIC -x c++ -DMPPO_EMU=1 -I"$HERE" -I"$SRC" -Wno-attributes -Wno-unused-value "${@:2}" -c "$1" -o "$OBJ/$(basename "$1").o"' _ {} "$@"
OBJS=""
for f in $FILES; do OBJS="$OBJS $OBJ/$(basename "$f").o"; done   # (linked in the order of SOURCES.txt, as one g++ call over the sources would)
g++ -shared -fPIC -Wl,-Bsymbolic "$@" $OBJS -o "$OUT.tmp.$$"
mv -f "$OUT.tmp.$$" "$OUT"   # (atomic: another process - a rank of a multi-process test - may be loading the library while this one rebuilds it)
echo "built $OUT"
