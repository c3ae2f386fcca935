#!/usr/bin/env python3
"""Cloud-to-cloud ICP at size: a 1M-point target (the points of f3d.synth.cloud, each moved onto one of the six faces of its
10 x 10 x 3 m box, with that face's inward normal: a room of about 3100 points per square metre, 1.8 cm apart) and a source of 500k of
its points taken through the inverse of a pose 3 cm and 2 degrees (about the box's centre) off, max_dist 5 cm

  a   one f3d_cloud_icp_dev call of `--rounds` rounds (the target's grid built once, search and sums fused), plane and point mode
  b   what a caller had before: `--rounds` f3d_knn_query_dev(k = 1) calls on the same points; each rebuilds the target's grid,
      writes idx and dist2, and computes no sums, no solve and no update (the queries are not even moved between the calls)

Synchronised host clock around each, after a warm-up, `--repeats` times, a and b alternating; the spread is max - min over the
repeats of one kind in this run.  A round that goes LOST makes every later terms kernel return at once, so the times of a run
whose final status is not OK say nothing: the status and the rounds that ran are printed next to the times, and the script ends
with an error after its JSON line when a mode was lost.  The context is reserved (f3d_ctx_reserve_cloud_icp, f3d_ctx_reserve_knn)
and strict: it must not allocate.  One JSON line.  python scripts/cloud_icp_stress.py [--m 1000000] [--n 500000] [--rounds 20]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / '3d-point-cloud-segmentation-using-2d-img-segmentation_amd'))
import f3d                                        # noqa: E402
from f3d import clouds as CL, synth               # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--m', type=int, default=1_000_000)
ap.add_argument('--n', type=int, default=500_000)
ap.add_argument('--rounds', type=int, default=20)
ap.add_argument('--max-dist', type=float, default=0.05)
ap.add_argument('--repeats', type=int, default=5)
args = ap.parse_args()

import torch                                      # noqa: E402

M, N, ROUNDS, MAX_DIST = args.m, args.n, args.rounds, args.max_dist
rng = np.random.default_rng(7)
target = synth.cloud(M, dtype=np.float32).copy()
LO, HI = np.array([-5.0, -5.0, 0.0], np.float32), np.array([5.0, 5.0, 3.0], np.float32)
face = np.arange(M) % 6                                                        # axis = face // 2, the low or the high side = face % 2
normals = np.zeros((M, 3))
for f in range(6):
    rows = face == f
    target[rows, f // 2] = (HI if f % 2 else LO)[f // 2]
    normals[rows, f // 2] = -1.0 if f % 2 else 1.0
half = np.radians(2.0) / 2
axis = np.array([0.4, -0.7, 0.59]) / np.linalg.norm([0.4, -0.7, 0.59])
q_true = np.concatenate([[np.cos(half)], np.sin(half) * axis])
w, x, y, z = q_true
R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
              [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
centre = np.array([0.0, 0.0, 1.5])
shift = 0.03 * np.array([0.6, -0.5, 0.62]) / np.linalg.norm([0.6, -0.5, 0.62])
picked = rng.permutation(M)[:N]
# the true pose maps s to R (s - centre) + centre + shift; the source is centred on the box's centre, as alignment.register_clouds does
source = (target[picked].astype(np.float64) - centre - shift) @ R
t_true = centre + shift

ctx = f3d.Context(0)
dev = torch.device('cuda', ctx.device)
ctx.reserve_cloud_icp(M, N)
ctx.reserve_knn(M)
ctx.set_strict(True)
work = torch.cuda.Stream(dev)
s = work.cuda_stream
d_src, d_tgt, d_nrm = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (source, target, normals))
pose, stats = torch.empty(7, dtype=torch.float64, device=dev), torch.empty((ROUNDS, 3), dtype=torch.float64, device=dev)
status = torch.empty(1, dtype=torch.int32, device=dev)
idx, dist2 = torch.empty((N, 1), dtype=torch.int32, device=dev), torch.empty((N, 1), dtype=torch.float64, device=dev)
torch.cuda.synchronize(dev)
allocs = ctx.alloc_count
IDENT, START = np.array([1.0, 0.0, 0.0, 0.0]), centre.copy()


def icp(mode):
    CL.cloud_icp_dev(ctx, d_src.data_ptr(), f3d.F64, N, d_tgt.data_ptr(), f3d.F32, M, d_nrm.data_ptr() if mode == f3d.CLOUD_ICP_PLANE else None, mode,
                     IDENT, START, MAX_DIST, ROUNDS, 100, pose.data_ptr(), stats.data_ptr(), status.data_ptr(), s)


def knn():
    for _ in range(ROUNDS):
        ctx.knn_query_dev(d_tgt.data_ptr(), f3d.F32, M, d_src.data_ptr(), f3d.F64, N, 1, MAX_DIST, idx.data_ptr(), dist2.data_ptr(), None, s)


def clocked(fn):
    torch.cuda.synchronize(dev)
    start = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - start) * 1e3


kinds = {'plane': lambda: icp(f3d.CLOUD_ICP_PLANE), 'point': lambda: icp(f3d.CLOUD_ICP_POINT), 'knn': knn}
for fn in kinds.values():
    fn()                                                                       # the warm-up
ms = {k: [] for k in kinds}
for _ in range(args.repeats):                                                  # alternating
    for k, fn in kinds.items():
        ms[k].append(clocked(fn))
out = {}
for name, mode in (('plane', f3d.CLOUD_ICP_PLANE), ('point', f3d.CLOUD_ICP_POINT)):
    icp(mode)
    torch.cuda.synchronize(dev)
    p, st = pose.cpu().numpy(), stats.cpu().numpy()
    qa = p[:4] / np.linalg.norm(p[:4])
    rmse = [float(np.sqrt(st[k, 1] / max(st[k, 0], 1))) for k in (0, -1)]
    out[name] = dict(status=int(status[0]), rounds_ok=int((st[:, 2] == f3d.ICP_OK).sum()), pairs_first_last=[int(st[0, 0]), int(st[-1, 0])], rmse_first_last=rmse,
                     errors_m_rad=[float(np.linalg.norm(p[4:] - t_true)), float(2 * np.arccos(min(1.0, abs(float(qa @ q_true)))))])
assert ctx.alloc_count == allocs, 'the reserved strict context allocated'
summary = {k: dict(best_ms=round(min(v), 3), median_ms=round(float(np.median(v)), 3), spread_ms=round(max(v) - min(v), 3)) for k, v in ms.items()}
print(json.dumps({'m': M, 'n': N, 'rounds': ROUNDS, 'max_dist': MAX_DIST, 'repeats': args.repeats,
                  'cloud_icp_plane': {**summary['plane'], **out['plane']}, 'cloud_icp_point': {**summary['point'], **out['point']},
                  'knn_query_k1_calls': summary['knn'],
                  'icp_not_slower_beyond_spread': {k: summary[k]['median_ms'] <= summary['knn']['median_ms'] + max(summary[k]['spread_ms'],
                                                                                                               summary['knn']['spread_ms'])
                                                   for k in ('plane', 'point')}}))
lost = [k for k in ('plane', 'point') if out[k]['status'] != f3d.ICP_OK]
if lost:
    sys.exit(f'lost in {lost}: the rounds after the lost one did no work, the times above are not those of {ROUNDS} rounds')
