#!/usr/bin/env python3
"""Radius query of PointCorrespondance (f3d_radius_query_count_dev / _fill_dev): count + fill ms (HIP events, after a warm-up, the nnz
readback included), pairs and pairs/s for 256 frames x 256x192 and 64 frames x 480x640, each against a cloud of 1M points, at
r in {0.02, 0.05, 0.1}; the host algorithm of the reference (sklearn KDTree(dense, leaf_size=2).query_radius(sparse) + the inversion
loop, one process) on a slice of frames, scaled to the capture and flagged "extrapolated"; an A/B of the query order (frame pixel
order as given against the queries sorted by grid cell, the sort itself timed apart).

Synthetic capture: a camera walking down a corridor (walls 2.5 m to either side, a floor 1.2 m below), 0.5 m per frame, depth with
5 % dropouts (their points sit at the camera centre, as unprojected zero depth does).  The cloud: 1M points drawn from the
capture's own points with 5 mm noise (what a fused cloud of it looks like)."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / '3d-point-cloud-segmentation-using-2d-img-segmentation_amd'))
import f3d                     # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--repeats', type=int, default=3)
ap.add_argument('--cloud', type=int, default=1_000_000)
ap.add_argument('--radii', default='0.02,0.05,0.1')
ap.add_argument('--host-frames', type=int, default=1, help='frames of the host baseline slice')
ap.add_argument('--no-host', action='store_true')
args = ap.parse_args()

import torch                   # noqa: E402

ctx = f3d.default_context()
dev = torch.device('cuda', ctx.device)


def capture(F, h, w, seed=0):
    """dense points float64 [F*h*w, 3] on the device; camera j at (0.5 j, 0, 0) looks across the corridor (+z), which runs along +x."""
    g = torch.Generator(device=dev).manual_seed(seed)
    f = 210.0 * w / 256
    v, u = torch.meshgrid(torch.arange(h, device=dev, dtype=torch.float64), torch.arange(w, device=dev, dtype=torch.float64), indexing='ij')
    dx, dy = (u - w / 2) / f, (v - h / 2) / f                       # camera axes: x right, y down, z forward
    z = torch.minimum(torch.full_like(dx, 2.5), torch.where(dy > 1e-9, 1.2 / dy.clamp_min(1e-9), torch.full_like(dy, float('inf'))))
    out = torch.empty((F, h * w, 3), dtype=torch.float64, device=dev)
    for j in range(F):
        zz = z + torch.randn(z.shape, generator=g, device=dev, dtype=torch.float64) * 0.001
        p = torch.stack([dx * zz + 0.5 * j, dy * zz, zz], -1).reshape(-1, 3)
        drop = torch.rand(h * w, generator=g, device=dev) < 0.05
        p[drop] = torch.tensor([0.5 * j, 0.0, 0.0], dtype=torch.float64, device=dev)
        out[j] = p
    return out.reshape(-1, 3)


def cloud_of(dense, n, seed=1):
    g = torch.Generator(device=dev).manual_seed(seed)
    pick = torch.randint(0, len(dense), (n,), generator=g, device=dev)
    return (dense[pick] + torch.randn((n, 3), generator=g, device=dev, dtype=torch.float64) * 0.005).contiguous()


def run(sparse, dense, r):
    """-> (ms of count + fill, nnz, offsets, neighbours)."""
    stream = torch.cuda.current_stream(dev)
    offs = torch.empty(len(dense) + 1, dtype=torch.int64, device=dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    nnz = ctx.radius_query_dev(sparse.data_ptr(), f3d.F64, len(sparse), dense.data_ptr(), f3d.F64, len(dense), r, offs.data_ptr(),
                               stream.cuda_stream)
    nb = torch.empty(nnz, dtype=torch.int32, device=dev)
    ctx.radius_query_fill_dev(dense.data_ptr(), f3d.F64, len(dense), offs.data_ptr(), nb.data_ptr(), stream.cuda_stream)
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1), nnz, offs, nb


def timed(sparse, dense, r):
    run(sparse, dense, r)                                           # warm-up (scratch growth, code load)
    best = None
    for _ in range(args.repeats):
        ms, nnz, offs, nb = run(sparse, dense, r)
        best = ms if best is None else min(best, ms)
    return best, nnz, offs, nb


def cell_order(dense, r):
    lo = dense.amin(0)
    c = ((dense - lo) / (r * 1.000001)).floor().to(torch.int64)
    dim = c.amax(0) + 1
    key = (c[:, 2] * dim[1] + c[:, 1]) * dim[0] + c[:, 0]
    return torch.argsort(key, stable=True)


def host_baseline(sparse, dense, r, nf, hw):
    """KDTree over the dense points of nf frames, queried with every cloud point, inverted with the reference's double loop."""
    from sklearn.neighbors import KDTree
    d = dense[: nf * hw].cpu().numpy()
    s = sparse.cpu().numpy()
    t0 = time.perf_counter()
    tree = KDTree(d, leaf_size=2)
    neighbors = tree.query_radius(s, r=r)
    merge_maps = [[] for _ in range(len(d))]
    for i, pts in enumerate(neighbors):
        for pt in pts:
            merge_maps[pt].append(i)
    np.array(merge_maps, dtype=object)
    return time.perf_counter() - t0, sum(len(m) for m in merge_maps)


results = []
for F, h, w in ((256, 192, 256), (64, 480, 640)):
    dense = capture(F, h, w)
    sparse = cloud_of(dense, args.cloud)
    for r in (float(x) for x in args.radii.split(',')):
        ms, nnz, offs, nb = timed(sparse, dense, r)
        lens = offs[1:] - offs[:-1]
        row = {'frames': F, 'h': h, 'w': w, 'queries': len(dense), 'cloud': len(sparse), 'radius': r, 'ms': round(ms, 2), 'pairs': int(nnz),
               'pairs_per_s': float(nnz) / (ms / 1e3), 'max_row': int(lens.max()), 'rows_over_32': int((lens > 32).sum())}
        # query order A/B: the same queries sorted by grid cell (the result rows permute with them)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        order = cell_order(dense, r)
        sorted_q = dense[order].contiguous()
        torch.cuda.synchronize(dev)
        row['cell_sort_ms'] = round((time.perf_counter() - t0) * 1e3, 2)
        ms2, nnz2, offs2, nb2 = timed(sparse, sorted_q, r)
        assert nnz2 == nnz and torch.equal(offs2[1:] - offs2[:-1], lens[order])
        row['ms_cell_ordered_queries'] = round(ms2, 2)
        del offs2, nb2, sorted_q, order
        if not args.no_host:
            secs, pairs = host_baseline(sparse, dense, r, args.host_frames, h * w)
            row['host_s_extrapolated'] = round(secs * F / args.host_frames, 1)
            row['host_slice'] = {'frames': args.host_frames, 's': round(secs, 2), 'pairs': pairs, 'extrapolated': True}
            row['speedup_extrapolated'] = round(row['host_s_extrapolated'] / (ms / 1e3))
        print(json.dumps(row), flush=True)
        results.append(row)
        del offs, nb, lens
        torch.cuda.empty_cache()
    del dense, sparse
    torch.cuda.empty_cache()
print(json.dumps({'corr_stress': results}))
