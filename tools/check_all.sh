#!/usr/bin/env bash
# GPU box: full parity suite, the headline bench line (a --full run: roofline and kernel times),
# then the mesh configs (tools/bvh_check.sh).  Logs go to $OUT (default out/).
# Every GPU step has its own time limit; a failing step ends the script.
set -u
cd "$(dirname "$0")/.."
OUT=${OUT:-out}
mkdir -p "$OUT"
timeout -k 10 400 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread -p no:cacheprovider \
    > "$OUT/t_all.log" 2>&1 || { tail -30 "$OUT/t_all.log"; exit 1; }
tail -1 "$OUT/t_all.log"
timeout -k 10 300 python bench.py --full --steps 100 --warmup 10 --no-cpu-baseline > "$OUT/b.log" 2>&1 || { tail -20 "$OUT/b.log"; exit 2; }
tail -1 "$OUT/b.log" | python3 -c "import json,sys; d=json.loads(sys.stdin.read()); print('headline', d['ms_per_step'], d['value'], d['roofline']['frac'], d['kernels']['per_launch_bounce_ms'])"
bash tools/bvh_check.sh
