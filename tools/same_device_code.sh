#!/bin/bash
# same_device_code.sh OTHER_CHECKOUT [SED_EXPR]: does this tree's release device code equal OTHER_CHECKOUT's?
# Compiles every dagl_amd/csrc/*.hip of both trees (release flags, device side only, each in its own tree at the
# same relative path) to assembly and diffs them function by function: blocks sorted by symbol, so a kernel may
# move within its file; basic-block labels lose their function number; comments, the compilation unit's id (a
# hash that covers the source text) and which text section a function sits in (a template instantiation has its
# own) are not compared: every instruction, directive and .amdhsa_ resource line is.  SED_EXPR maps OTHER's names of renamed symbols.
# COMMON=1: a file that gained or lost functions is compared over the functions and kernel metadata both trees have (the others are
# listed by name), for a change that adds kernels next to pinned ones.
set -u
here=$(cd "$(dirname "$0")/.." && pwd); other=$(cd "$1" && pwd); map=${2:-}
out=$(mktemp -d); trap 'rm -rf "$out"' EXIT; tab=$(printf '\t'); bad=0
asm() { mkdir -p "$2"; (cd "$1/dagl_amd/csrc" && ls *.hip | xargs -P "${JOBS:-8}" -I{} sh -c \
    '${HIPCC:-/opt/rocm/bin/hipcc} --offload-arch=gfx950 -O3 -std=c++17 -fPIC --offload-device-only -S -w "$1" -o "$2/${1%.hip}.s"' _ {} "$2"); }
blocks() { sed -E "$map; s/\.LBB[0-9]+_/.LBB_/g; s/\.L(func_begin|func_end|tmp)[0-9]+/.L\1/g; s/__hip_cuid_[0-9a-f]+/__hip_cuid/g; /^\t\.text\$/d; /^\t\.section\t\.text\./d" "$1" | awk '
    function flush(  i) { for (i = 0; i < n; i++) print key "\t" buf[i]; n = 0 }
    BEGIN { key = "0" }
    /-- Begin function /                     { flush(); key = "1 " $NF }     # one block per function ...
    /^\t\.p2alignl / || /^\t\.section\t\.AMDGPU\.gpr_maximums/ { flush(); key = "2" }   # ... the trailer of the file (from the padding behind the last function) ...
    /^amdhsa\.kernels:/                      { flush(); meta = 1 }
    meta && /^  - /                          { flush(); key = "3" }          # ... and one per kernel of the metadata
    meta && /^[a-z]/ && !/^amdhsa\.kernels:/ { flush(); key = "4" }
    meta && /^    \.name:/                   { key = "3 " $2 }
    { sub(/[ \t]*;.*$/, ""); if ($0 != "") buf[n++] = $0 }                 # (comments are notes of the compiler: no code)
    END { flush() }' | LC_ALL=C sort -s -t "$tab" -k1,1; }
keys() { cut -f1 "$1" | grep -E '^[13] ' | LC_ALL=C sort -u; }
asm "$here" "$out/new" && asm "$other" "$out/old" || { echo "compile failed"; exit 2; }
for s in $( (cd "$out/new" && ls; cd "$out/old" && ls) | sort -u); do
    [ -f "$out/new/$s" ] && [ -f "$out/old/$s" ] || { echo "$s: in one tree only"; bad=1; continue; }
    map= blocks "$out/new/$s" > "$out/ka"; blocks "$out/old/$s" > "$out/kb"
    if [ -n "${COMMON:-}" ] && ! diff <(keys "$out/ka") <(keys "$out/kb") > /dev/null; then
        LC_ALL=C comm -3 <(keys "$out/kb") <(keys "$out/ka") | sed "s/^\t/  new only: /; t; s/^/  old only: /" | sed "s/: [13] /: /" | sort -u
        LC_ALL=C comm -12 <(keys "$out/ka") <(keys "$out/kb") > "$out/both"
        for f in ka kb; do awk -F "$tab" 'NR == FNR { keep[$0] = 1; next } $1 in keep' "$out/both" "$out/$f" > "$out/$f.c"; mv "$out/$f.c" "$out/$f"; done
        echo "$s: compared over the $(grep -c '^1 ' "$out/both") functions both trees have"
    fi
    cut -f2- "$out/ka" > "$out/a"; cut -f2- "$out/kb" > "$out/b"
    if diff "$out/b" "$out/a" > "$out/d"; then echo "$s: same ($(grep -c '^[[:space:]]*\.amdhsa_kernel ' "$out/a") kernels, $(wc -l < "$out/a") lines)"
    else echo "$s: DIFFERS"; head -40 "$out/d"; bad=1; fi
done
[ $bad = 0 ] && echo "release device code: same in every file" || { echo "release device code: DIFFERENT"; exit 1; }
