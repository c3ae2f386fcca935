#!/usr/bin/env python3
"""door_window_bbox.generate_mesh at capture size (f3d_door_window_quads_dev): one JSON line per scene with the call's ms (HIP
events, after a warm-up, median of --reps), the points x triangles pairs it evaluates, the largest [M, T, 3] float64 temporary the
reference forms for one instance (point_vecs, :93) and the sum over instances, and the host time of the restatement
(tests/door_window_ref.py, NumPy on one core) on the smallest instance, scaled by points x triangles to the whole scene and flagged
"extrapolated".

Scene: tests/door_window_ref.capture_scene -- --inst door / window instances of 1k .. --largest points (geometric), each a noisy
patch on one of --rect random rectangles (2 triangles each).   python scripts/door_window_stress.py --rect 1000 --inst 40"""
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
import door_window_ref as R    # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--rect', type=int, default=1000, help='rectangles of the mesh (2 triangles each)')
ap.add_argument('--inst', type=int, default=40)
ap.add_argument('--largest', type=int, default=200_000)
ap.add_argument('--reps', type=int, default=10)
ap.add_argument('--host', action='store_true', help='time the restatement on the smallest instance')
args = ap.parse_args()

import torch                   # noqa: E402

ctx = f3d.default_context()
dev = torch.device('cuda', ctx.device)
pts, ids, info, verts, tris = R.capture_scene(ninst=args.inst, nrect=args.rect, largest=args.largest)
entries = np.array([d['id'] for d in info if d['category_id'] in R.DOOR_WINDOW], np.int64)
k, T = len(entries), len(tris)
sizes = np.array([int((ids == e).sum()) for e in entries])
d = {n: torch.as_tensor(a, device=dev) for n, a in (('pts', pts), ('ids', ids), ('inst', entries), ('verts', verts), ('tris', tris))}
quads = torch.empty((k, 4, 3), dtype=torch.float64, device=dev)
status = torch.empty(k, dtype=torch.int32, device=dev)
tri = torch.empty(k, dtype=torch.int32, device=dev)
stream = torch.cuda.Stream(dev)


def call():
    ctx.door_window_quads_dev(d['pts'].data_ptr(), len(pts), d['ids'].data_ptr(), d['inst'].data_ptr(), k, d['verts'].data_ptr(), len(verts),
                              d['tris'].data_ptr(), T, quads.data_ptr(), status.data_ptr(), tri.data_ptr(), None, stream.cuda_stream)


with torch.cuda.stream(stream):
    call()
    ctx.take_device_error(stream.cuda_stream)
    ms = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        call()
        b.record(stream)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ctx.take_device_error(stream.cuda_stream)
st = status.cpu().numpy()
pairs = int(sizes.sum()) * T
out = {'points': len(pts), 'instances': k, 'instance_points': [int(sizes.min()), int(sizes.max()), int(sizes.sum())], 'triangles': T,
       'pairs': pairs, 'gpu_ms_median': float(np.median(ms)), 'gpu_ms_min': float(np.min(ms)),
       'gpairs_per_s': pairs / (np.median(ms) * 1e-3) / 1e9, 'ok': int((st == R.QUAD_OK).sum()),
       'horizontal': int((st == R.QUAD_HORIZONTAL).sum()), 'no_candidate': int((st == R.QUAD_NO_CANDIDATE).sum()),
       'reference_peak_temp_GB': int(sizes.max()) * T * 3 * 8 / 1e9, 'reference_sum_temp_GB': pairs * 3 * 8 / 1e9}
if args.host:
    small = int(np.argmin(sizes))
    p = pts[ids == entries[small]]
    t0 = time.perf_counter()
    R.quad_of(p, np.full(len(p), entries[small]), entries[small], verts, tris, R.normals(verts, tris))
    dt = time.perf_counter() - t0
    out.update(host_s_smallest=dt, host_s_scene_extrapolated=dt * sizes.sum() / sizes[small], host_extrapolated=True)
print(json.dumps(out), flush=True)
