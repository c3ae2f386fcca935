#!/usr/bin/env python3
"""CVSegmentation at scale (f3d_flood_order_dev, f3d_color_segment_dev): one JSON line per cloud size with the flood-order ms (HIP events,
after a warm-up; the frontier readbacks included), its BFS levels and readbacks, clusters; color_segment ms for the seed list, per
seed and per accepted point; the restatement's host time (tests/cvseg_ref.py, a deque BFS like the reference's list queue) on a
slice of the cloud, scaled linearly to the full size and flagged "extrapolated".

Synthetic cloud: a room of n points (floor, two walls, a long table) with 2 mm noise, its radius graph (radius_adjacency at ~12
neighbours per point), classes in 0.4 m blobs (4 classes, hundreds of clusters, walls hundreds of hops across), colours smooth
along the surfaces.  Run one size per process:  python scripts/cvseg_stress.py --n 1000000"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / '3d-point-cloud-segmentation-using-2d-img-segmentation_amd'))
sys.path.insert(0, str(ROOT / 'tests'))
import f3d                     # noqa: E402
import cvseg_ref as R          # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--n', type=int, default=1_000_000)
ap.add_argument('--seeds', type=int, default=64)
ap.add_argument('--max-level', type=int, default=10)
ap.add_argument('--host-points', type=int, default=100_000, help='slice the restatement is timed on (0: skip)')
args = ap.parse_args()

import torch                   # noqa: E402

ctx = f3d.default_context()
dev = torch.device('cuda', ctx.device)


def room(n, seed=0):
    rng = np.random.default_rng(seed)
    k = rng.choice(4, n, p=[0.4, 0.25, 0.25, 0.1])
    u, v = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
    s = np.sqrt(n / 1e6)                                               # keep the density as n grows
    L, W, H = 12.0 * s, 8.0 * s, 3.0
    p = np.empty((n, 3))
    p[k == 0] = np.stack([u * L, v * W, 0 * u], 1)[k == 0]
    p[k == 1] = np.stack([u * L, 0 * u, v * H], 1)[k == 1]
    p[k == 2] = np.stack([0 * u, u * W, v * H], 1)[k == 2]
    p[k == 3] = np.stack([2 + u * 0.6 * L, 3 + v * 1.2, 0.75 + 0 * u], 1)[k == 3]
    p += rng.normal(0, 0.002, p.shape)
    q = np.floor(p / 0.4).astype(np.int64)
    cls = ((q[:, 0] + 2 * q[:, 1] + 3 * q[:, 2] + k) % 4).astype(np.int64)
    clr = np.stack([0.5 + 0.5 * np.sin(p[:, 0]), 0.5 + 0.5 * np.cos(p[:, 1]), 0.5 + 0.5 * np.sin(0.7 * p[:, 2] + p[:, 0])], 1)
    return p, cls, clr


pts, cls, clr = room(args.n)
area = 12 * 8 * (args.n / 1e6) * 1.1 + (12 + 8) * np.sqrt(args.n / 1e6) * 3
r = float(np.sqrt(12 / np.pi / (args.n / area)))                          # ~12 neighbours per point
offs, nb = f3d.default_context().radius_graph(pts, r)
n = args.n
dc, do, dn = torch.as_tensor(cls, device=dev), torch.as_tensor(offs, device=dev), torch.as_tensor(nb, device=dev)
root, order = torch.empty(n, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.int64, device=dev)
coffs, flags = torch.empty(n + 1, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
stream = torch.cuda.Stream(dev)                                           # a stream of its own: the events and the kernels share it
torch.cuda.synchronize(dev)


def flood():
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    st = ctx.flood_order_dev(dc.data_ptr(), n, do.data_ptr(), dn.data_ptr(), [0, 1, 2, 3], root.data_ptr(), order.data_ptr(), coffs.data_ptr(),
                             flags.data_ptr(), stream.cuda_stream)
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1), st


flood()
fl_ms, fst = min((flood() for _ in range(3)), key=lambda t: t[0])

seeds_np = np.random.default_rng(2).choice(n, args.seeds, replace=False)   # every seed starts in neutral (id 0) space
seeds = torch.as_tensor(seeds_np, device=dev)
ids0 = torch.zeros(n, dtype=torch.int64, device=dev)
ids0[seeds] = torch.arange(1, args.seeds + 1, device=dev)
dclr = torch.as_tensor(clr, device=dev)
acc = torch.zeros(1, dtype=torch.int64, device=dev)


def grow():
    ids = ids0.clone()
    acc.zero_()
    torch.cuda.synchronize(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    ctx.color_segment_dev(dclr.data_ptr(), f3d.F64, n, do.data_ptr(), dn.data_ptr(), ids.data_ptr(), seeds.data_ptr(), len(seeds), 0.05, (0,),
                          args.max_level, acc.data_ptr(), stream.cuda_stream)
    e1.record(stream)
    e1.synchronize()
    ctx.take_device_error(stream.cuda_stream)
    return e0.elapsed_time(e1), int(acc.item())


grow()
cs_ms, accepted = min(grow() for _ in range(3))

out = {'n': n, 'edges': int(offs[-1]), 'radius': r, 'flood_ms': round(fl_ms, 3), 'levels': fst['levels'], 'readbacks': fst['readbacks'],
       'clusters': fst['clusters'], 'color_ms': round(cs_ms, 3), 'seeds': len(seeds_np), 'max_level': args.max_level, 'accepted': accepted,
       'color_us_per_seed': round(1e3 * cs_ms / len(seeds_np), 2), 'color_us_per_point': round(1e3 * cs_ms / max(accepted, 1), 3)}
if args.host_points:
    m = min(args.host_points, n)
    sub = np.arange(m)
    keep = (nb[:offs[m]] < m)
    lens = np.add.reduceat(keep, offs[:m]) if offs[m] else np.zeros(m, np.int64)
    soffs = np.r_[0, np.cumsum(lens)].astype(np.int64)
    snb = nb[:offs[m]][keep]
    t0 = time.perf_counter()
    R.instance_seperate(cls[sub].copy(), (soffs, snb), [0, 1, 2, 3], 1)
    host_is = time.perf_counter() - t0
    t0 = time.perf_counter()
    R.color_segment(None, (offs, nb), clr, ids0.cpu().numpy(), seeds_np, 0.05, (0,), args.max_level)
    host_cs = time.perf_counter() - t0
    out.update({'host_flood_s': round(host_is * n / m, 2), 'host_flood_extrapolated': m < n, 'host_flood_slice': m,
                'host_color_s': round(host_cs, 3), 'host_color_us_per_point': round(1e6 * host_cs / max(accepted, 1), 2)})
print(json.dumps(out), flush=True)
