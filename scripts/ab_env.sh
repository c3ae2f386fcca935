#!/bin/bash
# usage (GPU box): scripts/ab_env.sh VAR "v1 v2 ..." [bench args]  -- times bench.py --full under each value of an environment variable;
# one log per value under $F3D_BENCH_LOGS (default bench_out/)
var=$1; vals=$2; shift 2
logs=${F3D_BENCH_LOGS:-bench_out}
mkdir -p "$logs"
for v in $vals; do
  env $var=$v python bench.py --full --steps 20 --warmup 3 --no-cpu-baseline --no-extras "$@" > "$logs/env_${var}_$v.log" 2>&1 || echo FAILED
  python - <<PY
import json
d=json.loads(open('$logs/env_${var}_$v.log').read().strip().split('\n')[-1])
print('$var=$v', 'step', d['ms_per_step'], 'call', d['roofline']['kernel_ms'])
PY
done
