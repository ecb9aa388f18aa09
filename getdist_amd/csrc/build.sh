#!/bin/bash
# Builds libgdhip.so in-tree for gfx950.  Usage: build.sh [outdir]
set -e
HERE="$(cd "$(dirname "$0")" && pwd)"
OUT="${1:-$HERE}"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -Wno-unused-result $GDHIP_EXTRA_FLAGS"
OBJS=""
for f in core stats binning histnd pca mixture density1d kopt2d density2d fft thin draw contours limits1d convolve batch2d comm export ingest colexpr coltab contourpaths devinput select devexport; do
  if [ ! -f "$OUT/$f.o" ] || [ "$HERE/$f.hip" -nt "$OUT/$f.o" ] || [ "$HERE/ctx.hpp" -nt "$OUT/$f.o" ] || [ "$HERE/ldsfft.hpp" -nt "$OUT/$f.o" ] || [ "$HERE/fft288.hpp" -nt "$OUT/$f.o" ] || [ "$HERE/solvers.hpp" -nt "$OUT/$f.o" ] || [ "$f" = binning -a "$HERE/binplan.hpp" -nt "$OUT/$f.o" ] || [ "$f" = stats -a "$HERE/statsplan.hpp" -nt "$OUT/$f.o" ] || [ "$f" = draw -a "$HERE/pcg64.hpp" -nt "$OUT/$f.o" ] || [ \( "$f" = colexpr -o "$f" = coltab \) -a \( "$HERE/colexpr.hpp" -nt "$OUT/$f.o" -o "$HERE/colexpr_kernel.hpp" -nt "$OUT/$f.o" \) ] || [ \( "$f" = thin -o "$f" = draw -o "$f" = export -o "$f" = ingest -o "$f" = contourpaths -o "$f" = select -o "$f" = devexport \) -a "$HERE/tilescan.hpp" -nt "$OUT/$f.o" ] || [ \( "$f" = select -o "$f" = devexport \) -a "$HERE/rowlist.hpp" -nt "$OUT/$f.o" ] || [ "$f" = devexport -a "$HERE/cvtfloat.hpp" -nt "$OUT/$f.o" ] || [ "$f" = ingest -a "$HERE/parsedouble.hpp" -nt "$OUT/$f.o" ] || [ \( "$f" = export -o "$f" = ingest \) -a \( "$HERE/fmtdouble.hpp" -nt "$OUT/$f.o" -o "$HERE/fmtdouble_pow10.inc" -nt "$OUT/$f.o" \) ] || [ "$f" = batch2d -a \( "$HERE/batch2d.hpp" -nt "$OUT/$f.o" -o "$HERE/batch1d.hpp" -nt "$OUT/$f.o" \) ] || [ "$HERE/../../include/gdhip.h" -nt "$OUT/$f.o" ]; then
    rm -f "$OUT/$f.o"  # a failed compile must not leave a stale object for the link
    $HIPCC $FLAGS -c "$HERE/$f.hip" -o "$OUT/$f.o" &
  fi
  OBJS="$OBJS $OUT/$f.o"
done
wait
$HIPCC --offload-arch=gfx950 -shared -fPIC $OBJS -o "$OUT/libgdhip.so" -L/opt/rocm/lib -lrocfft -ldl -Wl,-rpath,/opt/rocm/lib
echo "built $OUT/libgdhip.so"
