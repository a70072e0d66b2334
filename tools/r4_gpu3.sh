#!/bin/bash
# gather variants: alone (warm / clean-cold / dirty-cold) and inside the step
set -o pipefail
: "${OUT:?set OUT to an output directory}"; mkdir -p "$OUT"
for u in 1 2; do for nt in 1 3; do
  echo "== SFCVIT_GATHER_U=$u SFCVIT_GATHER_NT=$nt"
  SFCVIT_GATHER_U=$u SFCVIT_GATHER_NT=$nt python tools/bench_patch_embed.py > $OUT/r4_pe_u${u}_nt$nt.log 2>&1; grep "gather, tile" $OUT/r4_pe_u${u}_nt$nt.log
  SFCVIT_GATHER_U=$u SFCVIT_GATHER_NT=$nt python bench.py --full --no-cpu-baseline --time-all-kernels > $OUT/r4_bench_u${u}_nt$nt.log 2>&1
  python - <<PY
import json
l=[x for x in open("$OUT/r4_bench_u${u}_nt$nt.log") if x.startswith("{")][-1]
d=json.loads(l)
print("in step:", d["value"], d["ms_per_step"], {k:v for k,v in d.get("roofline_detail",{}).items() if "gather" in k})
PY
done; done
