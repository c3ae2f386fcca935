#!/usr/bin/env python3
"""Region growing at capture size (f3d_region_grow_dev): one JSON line with, for each of the four refinement floods, the median
of 10 HIP-event timings after a warm-up, the points grown, and the restatement's host time (tests/refinement_ref.py, a deque flood
like the reference's list queue, one core, run in full at this size).  With --color-segment the same single colour seed is also
grown by f3d_color_segment_dev (the same amount of work as color_floodfill_point), repeated --repeats times to show run-to-run noise.

Synthetic cloud: a 10 x 10 wall of n points lifted by a slow wave + noise, ~10 neighbours per point; the instances are a disc and a
stripe of > 10^5 points each, so the first queue spans > 100 LDS chunks.  python scripts/refine_stress.py --n 1000000"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / '3d-point-cloud-segmentation-using-2d-img-segmentation_amd'))
sys.path.insert(0, str(ROOT / 'tests'))
import f3d                          # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--n', type=int, default=1_000_000)
ap.add_argument('--max-level', type=int, default=50)
ap.add_argument('--runs', type=int, default=10)
ap.add_argument('--repeats', type=int, default=3, help='repetitions of the whole measurement (run-to-run noise)')
ap.add_argument('--color-segment', action='store_true', help='also time f3d_color_segment_dev from the same single seed')
ap.add_argument('--only-color-segment', action='store_true', help='time nothing else (works on a tree without region_grow)')
ap.add_argument('--no-host', action='store_true', help='skip the restatement')
args = ap.parse_args()

import torch                        # noqa: E402

ctx = f3d.default_context()
dev = torch.device('cuda', ctx.device)
n = args.n
rng = np.random.default_rng(11)
xy = rng.uniform(0, 10, (n, 2))
pts = np.stack([xy[:, 0], xy[:, 1], 0.02 * np.sin(xy[:, 0]) + rng.normal(0, 0.004, n)], 1)
col = np.clip(np.stack([xy[:, 0] / 10, xy[:, 1] / 10, np.full(n, 0.5)], 1) + rng.normal(0, 0.02, (n, 3)), 0, 1)
offs, nb = ctx.radius_graph(pts, float(np.sqrt(10.0 / (np.pi * n / 100.0))))
disc = np.nonzero(((xy - 5) ** 2).sum(1) < 4.0)[0]
stripe = np.nonzero(np.abs(xy[:, 0] - 5) < 0.8)[0]
dist = np.abs(pts[:, 2])
picks = np.array([disc[0], disc[len(disc) // 2], disc[-1]])
do, dn = torch.as_tensor(offs, device=dev), torch.as_tensor(nb, device=dev)
ddist, dcol = torch.as_tensor(dist, device=dev), torch.as_tensor(col, device=dev)
stream = torch.cuda.Stream(dev)                                            # the events and the kernels share it


def timed(fn):
    fn()                                                                   # warm-up
    ms = []
    for _ in range(args.runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(min(ms)), float(max(ms))


out = {'n': n, 'edges': int(offs[-1]), 'max_level': args.max_level, 'disc': len(disc), 'stripe': len(stripe)}
if not args.only_color_segment:
    import refinement_ref as R      # noqa: E402
    cluster, count = torch.empty(n, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
    floods = {'depth_floodfill_dl': (ddist, dist, 1, disc, 0.01, True, 'depth_points'),
              'color_floodfill_dl': (dcol, col, 3, stripe, 0.1, True, 'color_points'),
              'depth_floodfill_point': (ddist, dist, 1, picks, 0.01, False, 'depth_point'),
              'color_floodfill_point': (dcol, col, 3, picks[1:2], 0.1, False, 'color_point')}
    for name, (dval, val, nchan, seeds, thr, given, kind) in floods.items():
        ds = torch.as_tensor(seeds, device=dev)
        single = name == 'color_floodfill_point'
        sma0, npts0 = (val[seeds[0]], 0) if single else (np.average(val[seeds], axis=0), len(seeds))

        def run():
            ctx.region_grow_dev(dval.data_ptr(), f3d.F64, nchan, n, do.data_ptr(), dn.data_ptr(), ds.data_ptr(), len(ds), sma0, npts0, thr,
                                args.max_level, cluster.data_ptr(), count.data_ptr(), given, stream.cuda_stream)
        reps = [timed(run) for _ in range(args.repeats)]
        ctx.take_device_error(stream.cuda_stream)
        rec = {'ms_median': [round(r[0], 3) for r in reps], 'ms_min': round(min(r[1] for r in reps), 3),
               'ms_max': round(max(r[2] for r in reps), 3), 'seeds': len(seeds), 'grown': int(count)}
        if not args.no_host:
            t0 = time.perf_counter()
            want = getattr(R, kind)(val, (offs, nb), int(seeds[0]) if single else seeds, thr, args.max_level)
            rec['host_s'] = round(time.perf_counter() - t0, 3)
            rec['equal'] = bool(np.array_equal(cluster[:int(count)].cpu().numpy(), want))
        out[name] = rec
if args.color_segment or args.only_color_segment:
    ids0 = torch.zeros(n, dtype=torch.int64, device=dev)
    ids0[int(picks[1])] = 1
    ids = ids0.clone()
    seed = torch.as_tensor(picks[1:2], device=dev)
    acc = torch.zeros(1, dtype=torch.int64, device=dev)

    def run_cs():
        with torch.cuda.stream(stream):
            ids.copy_(ids0)
            acc.zero_()
        ctx.color_segment_dev(dcol.data_ptr(), f3d.F64, n, do.data_ptr(), dn.data_ptr(), ids.data_ptr(), seed.data_ptr(), 1, 0.1, (0,),
                              args.max_level, acc.data_ptr(), stream.cuda_stream)

    def run_reset():
        with torch.cuda.stream(stream):
            ids.copy_(ids0)
            acc.zero_()
    reps = [timed(run_cs) for _ in range(args.repeats)]
    ctx.take_device_error(stream.cuda_stream)
    accepted = int(acc)
    resets = [timed(run_reset) for _ in range(args.repeats)]
    out['color_segment_single_seed'] = {'ms_median': [round(r[0], 3) for r in reps], 'ms_min': round(min(r[1] for r in reps), 3),
                                        'ms_max': round(max(r[2] for r in reps), 3), 'accepted': accepted,
                                        'reset_ms_median': [round(r[0], 3) for r in resets]}
print(json.dumps(out))
