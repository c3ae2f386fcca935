#!/usr/bin/env python3
"""meshUtils at scan-mesh size: a 4M-triangle grid mesh with 5 % of the vertices removed.

Device time of each of the five functions on device tensors (HIP events, median of 10 calls after a warm-up, three
repetitions), against the NumPy / SciPy restatement tests/mesh_ref.py on one host core, and -- with ``--reference DIR`` -- against
the reference's own Python loops (functions 1-3), timed on a 100k-triangle slice and scaled by the triangle count.

``--once`` runs every function once after a warm-up and exits: the target of a kernel trace of its own,
``rocprofv3 --kernel-trace --stats -- python scripts/mesh_stress.py --once``, which splits the time into sort (rocPRIM), union
(k_mesh_union), compress (k_mesh_roots) and compaction (k_mesh_compact / k_mesh_keep_out).
Prints one JSON line per measurement.
"""
import argparse
import ast
import json
import os
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / '3d-point-cloud-segmentation-using-2d-img-segmentation_amd', ROOT / 'tests'):
    sys.path.insert(0, str(p))


def build(side, seed=7):
    import mesh_ref as R
    rng = np.random.default_rng(seed)
    verts, tris = R.grid_mesh(side, side, rng)
    return verts, tris[rng.permutation(len(tris))], rng.random(len(verts)) < 0.05


def functions(mu, verts, tris, mask):
    nv = len(verts)
    return {'vertex_triangle_mapping': lambda: mu.vertex_triangle_mapping(tris, nv),
            'remove_faces_by_vertices': lambda: mu.remove_faces_by_vertices(nv, tris, mask),
            'keep_faces_by_vertices': lambda: mu.keep_faces_by_vertices(verts, tris, mask),
            'get_triangle_clusters': lambda: mu.get_triangle_clusters((verts, tris)),
            'clean_mesh': lambda: mu.clean_mesh(verts, tris, mask, 50)}


def device_ms(fn, torch, calls=10):
    fn(); torch.cuda.synchronize()                                    # warm-up (sizes the scratch)
    times = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def reference_loops(refdir, verts, tris, mask, nslice=100_000):
    """Seconds of the reference's Python loops on the first nslice triangles."""
    src = (Path(refdir) / 'Fusion3DSeg/segUtils/meshUtils.py').read_text()
    names = ['vertex_triangle_mapping', 'remove_faces_by_vertices', 'keep_faces_by_vertices']
    body = [n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name in names]
    ns = {'np': np}
    exec(compile(ast.Module(body=body, type_ignores=[]), 'meshUtils.py', 'exec'), ns)
    t = tris[:nslice]
    out = {}
    for name, call in (('vertex_triangle_mapping', lambda: ns[names[0]](t, len(verts))),
                       ('remove_faces_by_vertices', lambda: ns[names[1]](len(verts), t, mask)),
                       ('keep_faces_by_vertices', lambda: ns[names[2]](verts, t.copy(), mask))):
        t0 = time.perf_counter(); call(); out[name] = time.perf_counter() - t0
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--side', type=int, default=1416, help='grid vertices per side (1416 -> 4.0M triangles)')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--once', action='store_true')
    ap.add_argument('--no-host', action='store_true', help='skip the one-core restatement')
    ap.add_argument('--reference', default=None, help="the reference project's directory (its loops are timed when given)")
    args = ap.parse_args()
    os.environ.setdefault('OMP_NUM_THREADS', '1')
    import torch
    from Fusion3DSeg.segUtils import meshUtils as mu
    import mesh_ref as R
    verts, tris, mask = build(args.side)
    dev = tuple(torch.as_tensor(a, device='cuda') for a in (verts, tris, mask))
    fns = functions(mu, *dev)
    meta = {'triangles': len(tris), 'vertices': len(verts), 'masked': int(mask.sum())}
    if args.once:
        for fn in fns.values():
            fn()
        torch.cuda.synchronize()
        for fn in fns.values():
            fn()
        torch.cuda.synchronize()
        print(json.dumps({'once': True, **meta}))
        return
    for rep in range(args.reps):
        for name, fn in fns.items():
            print(json.dumps({'function': name, 'rep': rep, 'device_ms': round(device_ms(fn, torch), 3), **meta}), flush=True)
    if not args.no_host:
        nv = len(verts)
        host = {'vertex_triangle_mapping': lambda: R.vertex_map(tris, nv), 'remove_faces_by_vertices': lambda: R.remove_faces(nv, tris, mask),
                'keep_faces_by_vertices': lambda: R.keep_faces(verts, tris, mask), 'get_triangle_clusters': lambda: R.clusters(verts, tris),
                'clean_mesh': lambda: R.ref_clean(verts, tris, mask, 50, 0.0)}
        for name, fn in host.items():
            t0 = time.perf_counter(); fn()
            print(json.dumps({'function': name, 'restatement_one_core_s': round(time.perf_counter() - t0, 3), **meta}), flush=True)
    if args.reference:
        for name, sec in reference_loops(args.reference, verts, tris, mask).items():
            print(json.dumps({'function': name, 'reference_loops_100k_s': round(sec, 3),
                              'scaled_to_mesh_s': round(sec * len(tris) / 100_000, 1), **meta}), flush=True)


if __name__ == '__main__':
    main()
