#!/bin/bash
# final round-4 measurements (GPU box, repo root): default bench line, profiles (kernel stats + PMC traffic), other configs
set -o pipefail
: "${OUT:?set OUT to an output directory}"; mkdir -p "$OUT"
python bench.py --full > $OUT/r4_bench_default.log 2>&1 && grep '^{' $OUT/r4_bench_default.log | tail -1 > $OUT/bench_b256_r4.json && cut -c1-400 $OUT/bench_b256_r4.json
bash tools/profile_bench.sh r4_final r4-final && echo "profiles done"
python bench.py --full --graph --no-cpu-baseline > $OUT/r4_bench_graph.log 2>&1; grep '^{' $OUT/r4_bench_graph.log | tail -1 > $OUT/bench_b256_r4_graph.json; cut -c1-200 $OUT/bench_b256_r4_graph.json
python bench.py --full --workload vit_l16_384_hilbert --no-cpu-baseline --steps 8 --warmup 2 > $OUT/r4_bench_l.log 2>&1; grep '^{' $OUT/r4_bench_l.log | tail -1 > $OUT/bench_vit_l16_384_hilbert_r4.json; cut -c1-200 $OUT/bench_vit_l16_384_hilbert_r4.json
python bench.py --full --workload vit_tiny16_32_hilbert --no-cpu-baseline > $OUT/r4_bench_t.log 2>&1; grep '^{' $OUT/r4_bench_t.log | tail -1 > $OUT/bench_vit_tiny16_32_hilbert_r4.json; cut -c1-200 $OUT/bench_vit_tiny16_32_hilbert_r4.json
