#!/usr/bin/env python3
"""extract_planes at scan size: a synthetic box room of 1M and of 4M points with its radius graph, both normal modes.

Per size: the device time of the radius graph (count and fill passes) and of planeUtils.extract_planes on device tensors with the
cloud's normals and with ``normals=None`` (HIP events around the call, median of 5 calls after a warm-up), with the planes found, the
attach rounds and the labelled points of each mode.  The stages this script times itself are the graph's count pass, its fill pass
and the whole extract_planes call.  That call is one C entry, so its own stages (core / union / roots, the two groupings, the plane
sums, the attach rounds, extents) are NOT split here: they come from a kernel trace of a single call, a run of its own,
``rocprofv3 --kernel-trace --stats -- python scripts/planes_stress.py --once --points 1000000``, which lists the k_pl_* kernels and
the rocPRIM sorts by name.  Prints one JSON line per measurement.
"""
import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / '3d-point-cloud-segmentation-using-2d-img-segmentation_amd', ROOT / 'tests'):
    sys.path.insert(0, str(p))


def room(n, size=(8.0, 6.0, 3.0), seed=3):
    """About n points on the six faces of a box (grid of one spacing, 1 mm noise, shuffled) -> (points, unit normals, spacing)."""
    rng = np.random.default_rng(seed)
    lx, ly, lz = size
    spacing = float(np.sqrt(2 * (lx * ly + ly * lz + lx * lz) / n))
    pts, nrm = [], []
    for axis, (la, lb), level in ((2, (lx, ly), 0.0), (2, (lx, ly), lz), (0, (ly, lz), 0.0), (0, (ly, lz), lx), (1, (lx, lz), 0.0), (1, (lx, lz), ly)):
        a, b = np.meshgrid(np.arange(spacing / 2, la, spacing), np.arange(spacing / 2, lb, spacing), indexing='ij')
        face = np.empty((a.size, 3))
        others = [c for c in range(3) if c != axis]
        face[:, others[0]], face[:, others[1]], face[:, axis] = a.reshape(-1), b.reshape(-1), level
        pts.append(face)
        nrm.append(np.tile(np.eye(3)[axis], (a.size, 1)))
    pts, nrm = np.concatenate(pts), np.concatenate(nrm)
    pts = pts + 0.001 * rng.standard_normal(pts.shape)
    nrm = nrm + 0.02 * rng.standard_normal(nrm.shape)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    perm = rng.permutation(len(pts))
    return np.ascontiguousarray(pts[perm]), np.ascontiguousarray(nrm[perm]), spacing


def event_ms(fn, torch, calls):
    fn(); torch.cuda.synchronize()                                    # warm-up (sizes the scratch)
    times = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def device_graph(ctx, torch, x, radius, calls):
    """The radius graph of device points as a device CSR pair, and the times of its two passes."""
    import f3d
    n = len(x)
    offs = torch.zeros(n + 1, dtype=torch.int64, device=x.device)
    nnz = C.c_int64(0)
    st = torch.cuda.current_stream()
    count = lambda: ctx._check(ctx._lib.f3d_radius_graph_count_dev(ctx._h, x.data_ptr(), f3d.F64, n, radius, offs.data_ptr(), C.byref(nnz), st.cuda_stream))
    t_count = event_ms(count, torch, calls)
    nbrs = torch.empty(nnz.value, dtype=torch.int32, device=x.device)
    fill = lambda: ctx._check(ctx._lib.f3d_radius_graph_fill_dev(ctx._h, n, offs.data_ptr(), nbrs.data_ptr(), st.cuda_stream))
    t_fill = event_ms(fill, torch, calls)
    return (offs, nbrs), t_count, t_fill


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--points', type=int, nargs='*', default=[1_000_000, 4_000_000])
    ap.add_argument('--radius-cells', type=float, default=2.5, help='graph radius in grid spacings')
    ap.add_argument('--calls', type=int, default=5)
    ap.add_argument('--once', action='store_true', help='one call per mode after a warm-up: the target of a kernel trace')
    args = ap.parse_args()
    import torch
    import f3d
    from Fusion3DSeg.segUtils import planeUtils as pu
    ctx = f3d.default_context(0)
    with torch.cuda.stream(torch.cuda.Stream()):                      # a stream of the caller's own: no side-stream hand-off per call
        for want in args.points:
            pts, nrm, spacing = room(want)
            radius = args.radius_cells * spacing
            x, nd = torch.as_tensor(pts, device='cuda'), torch.as_tensor(nrm, device='cuda')
            adj, t_count, t_fill = device_graph(ctx, torch, x, radius, 1 if args.once else args.calls)
            meta = {'points': len(pts), 'spacing': round(spacing, 5), 'radius': round(radius, 5), 'edges': int(len(adj[1]))}
            print(json.dumps({'stage': 'radius_graph', 'count_ms': round(t_count, 3), 'fill_ms': round(t_fill, 3), **meta}), flush=True)
            for mode, normals in (('normals', nd), ('pca', None)):
                kw = dict(offset=max(0.01, spacing), dist=0.01, min_points=1000)
                call = lambda: pu.extract_planes(x, adj, normals, **kw)
                ms = event_ms(call, torch, 1 if args.once else args.calls)
                got = call()
                planes, qualifying, rounds, labelled = (int(v) for v in got.counts.tolist())
                print(json.dumps({'stage': 'extract_planes', 'mode': mode, 'device_ms': round(ms, 3), 'planes': planes, 'qualifying': qualifying,
                                  'attach_rounds': rounds, 'labelled': labelled, **meta}), flush=True)


if __name__ == '__main__':
    main()
