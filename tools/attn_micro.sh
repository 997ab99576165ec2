#!/bin/bash
# Build kp_attn3 micro-benchmark variants (CPU container, no GPU needed):
#   bash tools/attn_micro.sh build <name> <src_dir> [defines...]   -> variants/attn_micro_<name>
# Run them on the GPU box (same box, same inputs, interleaved twice):
#   bash tools/attn_micro.sh run <tag> <name>...
# The key-range sweep of one variant (ComplEx FB15k-237; S = 0 is the planner's own choice):
#   bash tools/attn_micro.sh streams <tag> <name>
# first one stream, S = 1 .. 16 at 4,204 queries (the slope of ms x n_wg-rounds over S is the
# per-unit overhead), then three streams, S in {0, 2, 3, 4, 5, 6, 8} at four batch sizes
set -eo pipefail
cmd=$1; shift
B=${KP_MICRO_DIR:-variants}  # where the built variants are
if [ "$cmd" = build ]; then
  name=$1; src=$2; shift 2
  mkdir -p $B
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -Iinclude -I"$src" "$@" \
    tools/attn_micro.hip -o $B/attn_micro_$name
  exit 0
fi
tag=$1; shift
O=gpurun_out/$tag; mkdir -p $O
if [ "$cmd" = streams ]; then
  v=$1
  for S in 0 1 2 3 4 5 6 8 11 16; do
    timeout -k 10 60 $B/attn_micro_$v 25 0 14541 4204 60 0.05 0 --ranges $S --streams 1 >> $O/$v.fit.jsonl || exit 1
  done
  for nq in 3000 3730 4204 5000; do
    for S in 0 2 3 4 5 6 8; do
      timeout -k 10 60 $B/attn_micro_$v 25 0 14541 $nq 40 0.05 0 --ranges $S --streams 3 >> $O/$v.streams.jsonl || exit 1
    done
  done
  exit 0
fi
for rep in 1 2; do
  for v in "$@"; do
    # ComplEx FB15k-237 (D = 400, 3,100 queries), ComplEx DB100K, ConvE YAGO3-10 (D = 208)
    for args in "25 0 14541 3100 30" "25 0 99604 1800 10" "13 2 123182 4270 10"; do
      timeout -k 10 120 $B/attn_micro_$v $args 0.05 >> $O/$v.jsonl || exit 1
    done
  done
done
