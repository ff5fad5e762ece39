#!/bin/bash
# Everything profiles/ needs from one round, in one GPU session:  tools/gpu_round_measure.sh r04 RESULTS_DIR
TAG=${1:-r04}; OUT=${2:?usage: tools/gpu_round_measure.sh TAG RESULTS_DIR}
cd "$(dirname "$0")/.."; mkdir -p "$OUT"
python -m pytest tests -m gpu -x -q 2>&1 | tail -3 > "$OUT/${TAG}_gpu_tests.log"; cat "$OUT/${TAG}_gpu_tests.log"
python bench.py --full > "$OUT/${TAG}_bench_1gpu.json" 2> "$OUT/${TAG}_bench_1gpu.err"; tail -c 600 "$OUT/${TAG}_bench_1gpu.json"; echo
bash tools/gpu_profile.sh 0 $TAG > "$OUT/${TAG}_profile.log" 2>&1; tail -3 "$OUT/${TAG}_profile.log"
for c in strip strip_fused C4 C3_gi C5; do bash tools/gpu_profile_config.sh $TAG $c > "$OUT/${TAG}_profile_$c.log" 2>&1; done
bash tools/gpu_multi_rehearsal.sh $TAG > "$OUT/${TAG}_rehearsal.log" 2>&1; tail -4 "$OUT/${TAG}_rehearsal.log"
python tools/gpu_oneshot.py 2>/dev/null > "$OUT/${TAG}_oneshot.log"; tail -2 "$OUT/${TAG}_oneshot.log"
python tools/setup_probe.py 768 2>/dev/null > "$OUT/${TAG}_setup_probe.log"; cat "$OUT/${TAG}_setup_probe.log"
