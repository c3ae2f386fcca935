#!/usr/bin/env python3
"""The face graph at scan-mesh size: the shuffled 2M-triangle grid of scripts/mesh_stress.py (side 1001).

Device time of the ``_dev`` entries on one stream (HIP events, a warm-up, the median of 10 calls, three repetitions in one process):
f3d_mesh_face_frames_dev, f3d_mesh_face_graph_dev ungated and gated at 45 degrees, f3d_smooth_segment_dev over the graph with 134
float64 columns and, for context, f3d_mesh_triangle_clusters_dev on the same mesh (it sorts the same keys).  For scale, the NumPy
restatement tests/face_graph_ref.py on one host core (the sort-based one on the whole mesh, the dictionary on 100k faces).

``--once`` runs every entry twice and exits: the target of ``rocprofv3 --kernel-trace --stats -- python
scripts/face_graph_stress.py --once``, which splits the graph into sort (rocPRIM), run bounds (k_fg_runs), count and fill
(k_fg_rows) and the offsets (rocPRIM scan, k_fg_offsets).  Prints one JSON line per measurement.
"""
import argparse
import json
import math
import os
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / '3d-point-cloud-segmentation-using-2d-img-segmentation_amd', ROOT / 'tests', ROOT / 'scripts'):
    sys.path.insert(0, str(p))


def entries(ctx, torch, verts, tris, ncols):
    """name -> a call that enqueues the entry on `stream`; the outputs live as long as the dictionary."""
    import f3d
    from f3d.tensors import dtype_code, index_code
    dev = tris.device
    nv, nt = len(verts), len(tris)
    i64, f64 = torch.int64, torch.float64
    counts = torch.empty(4, dtype=i64, device=dev)
    normals, centroids = torch.empty((nt, 3), dtype=f64, device=dev), torch.empty((nt, 3), dtype=f64, device=dev)
    areas = torch.empty(nt, dtype=f64, device=dev)
    offsets = torch.empty(nt + 1, dtype=i64, device=dev)
    nbrs = torch.empty(3 * nt, dtype=torch.int32, device=dev)
    clusters = torch.empty(nt, dtype=torch.int32, device=dev)
    cluster_n, cluster_area = torch.empty(nt, dtype=i64, device=dev), torch.empty(nt, dtype=f64, device=dev)
    votes = torch.zeros((nt, ncols), dtype=f64, device=dev)
    votes[torch.arange(nt, device=dev), torch.randint(0, ncols - 1, (nt,), device=dev, generator=torch.Generator(dev).manual_seed(3))] = 8
    classes = torch.empty(nt, dtype=i64, device=dev)
    mesh = (verts.data_ptr(), dtype_code(verts), nv, tris.data_ptr(), index_code(tris), nt)
    cos45 = math.cos(math.radians(45.0))

    gated = torch.empty(nt + 1, dtype=i64, device=dev), torch.empty(3 * nt, dtype=torch.int32, device=dev)

    def graph(gate, s):                                                # the smoothing reads the ungated graph
        o, n = gated if gate else (offsets, nbrs)
        ctx.mesh_face_graph_dev(*mesh, gate, cos45, o.data_ptr(), n.data_ptr(), 3 * nt, counts.data_ptr(), s)

    return {
        'face_frames': lambda s: ctx.mesh_face_frames_dev(*mesh, normals.data_ptr(), centroids.data_ptr(), areas.data_ptr(), counts.data_ptr(), s),
        'face_graph': lambda s: graph(False, s),
        'face_graph_45': lambda s: graph(True, s),
        'smooth_segment_134': lambda s: ctx.smooth_segment_dev(votes.data_ptr(), f3d._vtype(votes), nt, ncols, offsets.data_ptr(), nbrs.data_ptr(),
                                                               None, 0.0, None, f3d.F64, 0.0, 1.0, 1, ncols - 1, 0.5, None, False,
                                                               classes.data_ptr(), s),
        'triangle_clusters': lambda s: ctx.mesh_triangle_clusters_dev(*mesh, clusters.data_ptr(), cluster_n.data_ptr(), cluster_area.data_ptr(),
                                                                      None, counts.data_ptr(), s),
    }, counts


def device_ms(fn, torch, stream, calls=10):
    fn(stream.cuda_stream); stream.synchronize()                       # warm-up (sizes the scratch)
    times = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream); fn(stream.cuda_stream); b.record(stream)
        stream.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--side', type=int, default=1001, help='grid vertices per side (1001 -> 2.0M triangles)')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--cols', type=int, default=134)
    ap.add_argument('--once', action='store_true')
    ap.add_argument('--no-host', action='store_true', help='skip the one-core restatement')
    args = ap.parse_args()
    os.environ.setdefault('OMP_NUM_THREADS', '1')
    import torch
    import f3d
    import face_graph_ref as G
    from mesh_stress import build
    verts, tris, _ = build(args.side)
    ctx = f3d.default_context(0)
    dv, dt = (torch.as_tensor(a, device='cuda') for a in (verts, tris))
    fns, counts = entries(ctx, torch, dv, dt, args.cols)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    meta = {'triangles': len(tris), 'vertices': len(verts)}
    if args.once:
        for _ in range(2):
            for fn in fns.values():
                fn(stream.cuda_stream)
            stream.synchronize()
        print(json.dumps({'once': True, **meta}))
        return
    for rep in range(args.reps):
        for name, fn in fns.items():
            ms = device_ms(fn, torch, stream)
            extra = {'nnz': int(counts[0]), 'boundary_edges': int(counts[3])} if name.startswith('face_graph') else {}
            print(json.dumps({'entry': name, 'rep': rep, 'device_ms': round(ms, 3), **extra, **meta}), flush=True)
    ctx.take_device_error(stream.cuda_stream)
    if not args.no_host:
        t0 = time.perf_counter(); normals = G.face_frames(verts, tris)[0]
        print(json.dumps({'entry': 'face_frames', 'restatement_one_core_s': round(time.perf_counter() - t0, 3), **meta}), flush=True)
        for name, cos_crease in (('face_graph', None), ('face_graph_45', math.cos(math.radians(45.0)))):
            t0 = time.perf_counter(); G.face_graph(tris, normals, cos_crease)
            print(json.dumps({'entry': name, 'restatement_one_core_s': round(time.perf_counter() - t0, 3), **meta}), flush=True)
        t0 = time.perf_counter(); G.face_graph_dict(tris[:100_000])
        print(json.dumps({'entry': 'face_graph', 'dictionary_100k_faces_s': round(time.perf_counter() - t0, 3)}), flush=True)


if __name__ == '__main__':
    main()
