"""Print step / fused-call / sort milliseconds of bench.py --full logs (last line = the JSON line): python scripts/show_ms.py LOG [LOG ...]."""
import json, sys
for f in sys.argv[1:]:
    d = json.loads(open(f).read().strip().split('\n')[-1])
    print(f, 'step', d['ms_per_step'], 'call', d['roofline']['kernel_ms'], 'sort', d['roofline']['sort_ms'])
