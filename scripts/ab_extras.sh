#!/bin/bash
# usage (GPU box): scripts/ab_extras.sh  -- streaming-kernel timings (bench.py --full) of every ab/*.so variant of libf3d_hip.so (loader
# pointed at the variant through F3D_LIBRARY; the product's library file is never touched); logs under $F3D_BENCH_LOGS (default bench_out/)
logs=${F3D_BENCH_LOGS:-bench_out}
mkdir -p "$logs"
for lib in ab/*.so; do
  F3D_LIBRARY=$PWD/$lib python bench.py --full --steps 5 --warmup 2 --no-cpu-baseline --no-merge > "$logs/abx_$(basename $lib .so).log" 2>&1 || echo "FAILED $lib"
  python - <<PY
import json
d=json.loads(open('$logs/abx_$(basename $lib .so).log').read().strip().split('\n')[-1])
print('$(basename $lib .so)', d['ms_per_step'], {k.split(' ')[0]: v['ms'] for k, v in d['streaming_kernels'].items() if 'ms' in v})
PY
done
