#!/bin/bash
# usage (GPU box): scripts/ab.sh [bench args]  -- times every ab/*.so variant of libf3d_hip.so with bench.py --full (its roofline object
# holds the fused call and the sort timed on their own); one log per variant under $F3D_BENCH_LOGS (default bench_out/).
# The loader is pointed at the variant through F3D_LIBRARY: the product's own library file is never touched.
logs=${F3D_BENCH_LOGS:-bench_out}
mkdir -p "$logs"
for lib in ab/*.so; do
  F3D_LIBRARY=$PWD/$lib python bench.py --full --steps 20 --warmup 3 --no-cpu-baseline --no-extras "$@" > "$logs/ab_$(basename $lib .so).log" 2>&1 || echo "FAILED $lib"
  python - <<PY
import json
d=json.loads(open('$logs/ab_$(basename $lib .so).log').read().strip().split('\n')[-1])
print('$(basename $lib .so)', 'step', d['ms_per_step'], 'call', d['roofline']['kernel_ms'], 'sort', d['roofline']['sort_ms'])
PY
done
