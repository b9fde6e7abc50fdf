#!/bin/bash
# --kernel-trace --stats of 90 config-5 fused launches, then bench.py's config-5 block on the same box:   tools/trace_config5_fused.sh OUTDIR
set -e
export TMPDIR=/tmp
OUT=${1:?usage: tools/trace_config5_fused.sh OUTDIR}
mkdir -p "$OUT"
rm -rf /tmp/prof/stats_c5 && mkdir -p /tmp/prof
rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof/stats_c5 -o run -- python3 tools/run_stage.py fused --iters 80 --hw 1080x1920 --batch 512 --nbuf 1 --profiling 0 > /dev/null 2>&1
f=$(find /tmp/prof/stats_c5 -name '*kernel_stats.csv' | head -1)
head -1 "$f" > "$OUT/bench_kernel_stats_config5_90launches.csv"
grep -i 'k_fused_mask_lut' "$f" >> "$OUT/bench_kernel_stats_config5_90launches.csv"
cut -c1-60,220-330 "$OUT/bench_kernel_stats_config5_90launches.csv"
python3 bench.py --full --steps 20 --warmup 5 --only config5 > "$OUT/bench_config5_same_box.json" 2>/dev/null
python3 - "$OUT/bench_config5_same_box.json" <<'PY'
import json, sys
d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print(d['config5']['fused_mask']['roofline'])
PY
