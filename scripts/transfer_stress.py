#!/usr/bin/env python3
"""Label transfer at scan size: a 1M-point surface cloud (two 10 m^2 planes, about 390 points within 5 cm of a point), 2M queries made
from cloud points jittered by 1 cm, r = 5 cm, everything on device tensors.

Times ``transfer_labels`` at k = 1 and k = 8 and ``knn_query`` at k = 8 (Context ``*_dev`` calls), and in the same process the only
route to the k = 1 answer without them: ``radius_query`` count + fill on the same inputs, alone and followed by a per-row arg-min
with torch.  HIP events go around the whole call, readback included; each figure is the median of 10 calls after a warm-up,
repeated ``--reps`` times and reported as min-max over the repetitions.  Prints one JSON line per measurement and a summary line.
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / '3d-point-cloud-segmentation-using-2d-img-segmentation_amd'):
    sys.path.insert(0, str(p))


def build(m, n, seed=5):
    rng = np.random.default_rng(seed)
    half = m // 2
    floor = np.stack([rng.uniform(0, 4, half), rng.uniform(0, 2.5, half), rng.normal(0, 0.002, half)], 1)
    wall = np.stack([rng.uniform(0, 4, m - half), rng.normal(0, 0.002, m - half), rng.uniform(0, 2.5, m - half)], 1)
    cloud = np.concatenate([floor, wall])[rng.permutation(m)]
    queries = cloud[rng.integers(0, m, n)] + rng.normal(0, 0.01, (n, 3))
    labels = rng.integers(0, 40, m)
    return cloud, labels, queries


def device_ms(fn, torch, stream, calls=10):
    times = []
    with torch.cuda.stream(stream):                                   # the library's calls and torch's own work on one stream
        fn(); torch.cuda.synchronize()                                # warm-up (sizes the scratch)
        for _ in range(calls):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream); fn(); b.record(stream)
            torch.cuda.synchronize()
            times.append(a.elapsed_time(b))
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--points', type=int, default=1_000_000)
    ap.add_argument('--queries', type=int, default=2_000_000)
    ap.add_argument('--radius', type=float, default=0.05)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--no-argmin', action='store_true', help='skip the torch arg-min over the CSR')
    args = ap.parse_args()
    import torch
    import f3d
    cloud, labels, queries = build(args.points, args.queries)
    d, lab, q = (torch.as_tensor(a, device='cuda') for a in (cloud, labels, queries))
    m, n, r = len(d), len(q), args.radius
    ctx = f3d.default_context(0)
    side = torch.cuda.Stream()                                        # (a null-stream handle would select the context's own stream)
    stream = side.cuda_stream
    out = torch.empty(n, dtype=torch.int64, device='cuda')
    support = torch.empty(n, dtype=torch.int32, device='cuda')
    idx = torch.empty((n, 8), dtype=torch.int32, device='cuda')
    dist2 = torch.empty((n, 8), dtype=torch.float64, device='cuda')
    counts = torch.empty(n, dtype=torch.int32, device='cuda')
    offs = torch.empty(n + 1, dtype=torch.int64, device='cuda')
    csr = {}

    def transfer(k):
        ctx.transfer_labels_dev(d.data_ptr(), f3d.F64, m, lab.data_ptr(), q.data_ptr(), f3d.F64, n, k, r, -1, out.data_ptr(), support.data_ptr(), stream)

    def knn8():
        ctx.knn_query_dev(d.data_ptr(), f3d.F64, m, q.data_ptr(), f3d.F64, n, 8, r, idx.data_ptr(), dist2.data_ptr(), counts.data_ptr(), stream)

    def count_fill():
        nnz = ctx.radius_query_dev(d.data_ptr(), f3d.F64, m, q.data_ptr(), f3d.F64, n, r, offs.data_ptr(), stream)
        nb = csr.get('nb')
        if nb is None or len(nb) != nnz:
            nb = csr['nb'] = torch.empty(nnz, dtype=torch.int32, device='cuda')
        ctx.radius_query_fill_dev(q.data_ptr(), f3d.F64, n, offs.data_ptr(), nb.data_ptr(), stream)

    def count_fill_argmin(rows_per_chunk=100_000):
        count_fill()
        nb_all, big = csr['nb'], torch.iinfo(torch.int64).max
        label = torch.empty(n, dtype=torch.int64, device='cuda')
        for a in range(0, n, rows_per_chunk):                         # in slices of the queries: the pair arrays stay at a few GB
            b = min(a + rows_per_chunk, n)
            lens = offs[a + 1:b + 1] - offs[a:b]
            nb = nb_all[int(offs[a]):int(offs[b])].to(torch.int64)
            rows = torch.repeat_interleave(torch.arange(b - a, device='cuda'), lens)
            t = q[a:b][rows] - d[nb]
            d2 = (t[:, 0] * t[:, 0] + t[:, 1] * t[:, 1]) + t[:, 2] * t[:, 2]
            best = torch.full((b - a,), float('inf'), dtype=torch.float64, device='cuda').scatter_reduce(0, rows, d2, 'amin')
            cand = torch.where(d2 == best[rows], nb, big)
            first = torch.full((b - a,), big, dtype=torch.int64, device='cuda').scatter_reduce(0, rows, cand, 'amin')
            label[a:b] = torch.where(first < m, lab[first.clamp(max=m - 1)], -1)
        csr['label'] = label

    runs = {'transfer_labels_k1': lambda: transfer(1), 'transfer_labels_k8': lambda: transfer(8), 'knn_query_k8': knn8,
            'radius_query_count_fill': count_fill}
    if not args.no_argmin:
        runs['radius_query_count_fill_argmin'] = count_fill_argmin
    ranges = {name: [] for name in runs}
    for rep in range(args.reps):
        for name, fn in runs.items():
            ms = device_ms(fn, torch, side)
            ranges[name].append(ms)
            print(json.dumps({'call': name, 'rep': rep, 'device_ms': round(ms, 3), 'points': m, 'queries': n, 'radius': r}), flush=True)
    if not args.no_argmin:                                            # the two routes give the same k = 1 labels
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            transfer(1)
        torch.cuda.synchronize()
        assert torch.equal(out, csr['label']), 'the fused k = 1 transfer and the CSR arg-min disagree'
    summary = {name: [round(min(v), 3), round(max(v), 3)] for name, v in ranges.items()}
    summary['pairs'] = int(offs[-1])
    summary['fused_k1_not_above_count_fill'] = min(ranges['transfer_labels_k1']) <= max(ranges['radius_query_count_fill'])
    print(json.dumps({'summary_ms_min_max': summary}), flush=True)


if __name__ == '__main__':
    main()
