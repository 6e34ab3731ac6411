#!/bin/bash
# Build libarx_hip.so for gfx950 in-tree (hipcc cross-compiles without a GPU).
set -e
cd "$(dirname "$0")"
OUT=${ARX_OUT:-../libarx_hip.so}          # ARX_OUT=../libarx_dev.so ARX_HIPCC_EXTRA="-DARX_DEV_VARIANTS": a dev build beside the shipped one
BLD=../_build${ARX_OUT:+_$(basename "$ARX_OUT" .so)}
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-result -ffp-contract=fast"
mkdir -p $BLD
pids=()
# per-kernel register / scratch / spill figures of THIS build go to _build/<file>.resources.txt (tests/test_build_resources.py reads them:
# a hot kernel that spills writes its registers to memory once per wave — 0.4 GB per attention launch when it happened, round 2)
# (fuse.hip computes keyword.fuse bit for bit: two rounded f64 products and one sum, so it is compiled without FMA contraction;
# bm25_build.hip computes keyword.impacts_f64 bit for bit, in numpy's operation order, and is compiled the same way;
# cluster.hip computes topics.finish_host's sum of squares bit for bit, and is compiled the same way too;
# boosted.hip computes boost.boosted_host's rounded product and rounded sum bit for bit, and is compiled the same way;
# pq.hip computes pq.encode_host's and pq.lut_host's sums operation by operation, and is compiled the same way)
for f in runtime encoder search bm25 filter filter_multi prefix grouped range textscan where_eval mmr fuse bm25_build compact facet cluster cluster_assign boosted binary pq graph ivf; do
  PER_FILE=""; { [ $f = fuse ] || [ $f = bm25_build ] || [ $f = cluster ] || [ $f = boosted ] || [ $f = pq ]; } && PER_FILE="-ffp-contract=off"
  ( hipcc $FLAGS $PER_FILE -Rpass-analysis=kernel-resource-usage -c $f.hip -o $BLD/$f.o ${ARX_HIPCC_EXTRA} 2> $BLD/$f.resources.txt \
      || { grep -v "kernel-resource-usage" $BLD/$f.resources.txt >&2; exit 1; } ) &
  pids+=($!)
done
# host-only part of the C ABI (WordPiece feeder): plain C++, no device code
g++ -O3 -std=c++17 -fPIC -pthread -c wordpiece.cpp -o $BLD/wordpiece.o &
pids+=($!)
for p in "${pids[@]}"; do wait $p || exit 1; done
hipcc --offload-arch=gfx950 -shared -fPIC -pthread -o $OUT $BLD/runtime.o $BLD/encoder.o $BLD/search.o $BLD/bm25.o $BLD/filter.o $BLD/filter_multi.o $BLD/prefix.o $BLD/grouped.o $BLD/range.o $BLD/textscan.o $BLD/where_eval.o $BLD/mmr.o $BLD/fuse.o $BLD/bm25_build.o $BLD/compact.o $BLD/facet.o $BLD/cluster.o $BLD/cluster_assign.o $BLD/ivf.o $BLD/binary.o $BLD/pq.o $BLD/boosted.o $BLD/graph.o $BLD/wordpiece.o
echo "built $(realpath $OUT)"
