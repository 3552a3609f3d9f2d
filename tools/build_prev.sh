#!/usr/bin/env bash
# Builds the library of git HEAD into csrc/ablate/libsvgp_prev.so for same-box A/B timing against the working tree:
# the translation units and the flags of build.sh.  Needs a git checkout, so run it where the tree is one.
set -euo pipefail
ROOT="$(cd "$(dirname "$0")/.." && pwd)"; TMP=$(mktemp -d); OUT="$ROOT/approximategps.jl_amd/csrc/ablate"; mkdir -p "$OUT"
git -C "$ROOT" archive HEAD approximategps.jl_amd/csrc include | tar -x -C "$TMP"
UNITS=$(cd "$TMP/approximategps.jl_amd/csrc" && for f in *.hip; do echo "${f%.hip}"; done)   # every translation unit HEAD has
pids=()
for f in $UNITS; do
  hipcc -O3 -std=c++17 --offload-arch=gfx950 -fPIC -Wall -Wno-unused-function -c "$TMP/approximategps.jl_amd/csrc/$f.hip" -o "$TMP/$f.o" 2>/dev/null &
  pids+=($!)
done
for p in "${pids[@]}"; do wait "$p"; done
hipcc --offload-arch=gfx950 -shared -fPIC -o "$OUT/libsvgp_prev.so" $(for f in $UNITS; do echo "$TMP/$f.o"; done) -ldl
rm -rf "$TMP"; echo "built $OUT/libsvgp_prev.so from $(git -C "$ROOT" rev-parse --short HEAD)"
