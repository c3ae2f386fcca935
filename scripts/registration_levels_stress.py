#!/usr/bin/env python3
"""Coarse-to-fine registration at size, on the scene of scripts/registration_stress.py: a 256^3 volume of 2 cm voxels holding a box
room integrated from a ring of poses, and a 480 x 640 camera inside it

  halves    one f3d_depth_half_dev and one f3d_maps_half_dev call at 480 x 640 (to 240 x 320): ms each
  icp       one f3d_icp_dev call of 10 rounds at full resolution against one f3d_icp_levels_dev call of 4 + 5 + 10 rounds over three
            levels (the pyramids built beforehand), from a pose 2 cm and 1 degree off: ms, and the pose errors
  pyramid   the two half-samplings of both pyramids (four launches): ms
  track     registration.track_frames over `--track` frames into an empty device volume with levels=1 and with levels=3
            (level_iterations 10, 5, 4): ms per frame by the host clock around the synchronised call

HIP events around every call after a warm-up, best of `--repeats`, on a context of its own that is reserved (f3d_ctx_reserve_icp)
and strict: it must not allocate.  One JSON line.  python scripts/registration_levels_stress.py [--dims 256,256,256] [--hw 480,640]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / '3d-point-cloud-segmentation-using-2d-img-segmentation_amd'))
import f3d                                        # noqa: E402
from f3d import levels as LV                      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--dims', default='256,256,256')
ap.add_argument('--voxel', type=float, default=0.02)
ap.add_argument('--frames', type=int, default=8)
ap.add_argument('--hw', default='480,640')
ap.add_argument('--repeats', type=int, default=3)
ap.add_argument('--track', type=int, default=4)
args = ap.parse_args()

import torch                                      # noqa: E402

DIMS = tuple(int(x) for x in args.dims.split(','))
H, W = (int(x) for x in args.hw.split(','))
VS, F = args.voxel, args.frames
TRUNC, MAX_DEPTH, MAX_WEIGHT, GATE = 4 * VS, 10.0, 64.0, 0.1
ROUNDS = (10, 5, 4)                                                            # finest first
EXT = np.array(DIMS) * VS
LO = -EXT / 2
ROOM_LO, ROOM_HI = LO + 8 * VS, LO + EXT - 8 * VS                              # the walls, eight voxels inside the volume

ctx = f3d.Context(0)
dev = torch.device('cuda', ctx.device)


def rot_to_quat(R):
    w = np.sqrt(max(0.0, 1.0 + R[0, 0] + R[1, 1] + R[2, 2])) / 2
    x = np.sqrt(max(0.0, 1.0 + R[0, 0] - R[1, 1] - R[2, 2])) / 2
    y = np.sqrt(max(0.0, 1.0 - R[0, 0] + R[1, 1] - R[2, 2])) / 2
    z = np.sqrt(max(0.0, 1.0 - R[0, 0] - R[1, 1] + R[2, 2])) / 2
    return np.array([w, np.copysign(x, R[2, 1] - R[1, 2]), np.copysign(y, R[0, 2] - R[2, 0]), np.copysign(z, R[1, 0] - R[0, 1])])


def capture():
    """K, wxyzs, translations, depths float32 [F, H, W]: the room's walls seen from a ring of poses inside it, looking into a corner
    region so that three wall directions are in view."""
    K = np.array([[0.8 * W, 0.0, W / 2.0], [0.0, 0.8 * W, H / 2.0], [0.0, 0.0, 1.0]])
    uu, vv = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    dc = np.stack([(uu - K[0, 2]) / K[0, 0], (vv - K[1, 2]) / K[1, 1], np.ones_like(uu)], -1).reshape(-1, 3)
    qs, ts, depths = [], [], []
    for f in range(F):
        a = 0.25 * f / max(F - 1, 1)
        eye = np.array([0.3 * np.cos(a) - 0.2, 0.3 * np.sin(a) - 0.1, 0.1 * f / F])
        z = np.array([np.cos(0.6 + a), np.sin(0.6 + a), 0.45])
        z /= np.linalg.norm(z)
        x = np.cross(np.array([0.0, 0.0, -1.0]), z)
        x /= np.linalg.norm(x)
        R = np.stack([x, np.cross(z, x), z], axis=1)                            # columns: camera axes in the world (x right, y down)
        D = dc @ R.T
        with np.errstate(divide='ignore'):
            s = np.where(D > 0, (ROOM_HI - eye) / D, (ROOM_LO - eye) / D)
        qs.append(rot_to_quat(R)); ts.append(eye)
        depths.append(s.min(axis=1).reshape(H, W))
    return K, np.array(qs), np.array(ts), np.array(depths, dtype=np.float32)


work = torch.cuda.Stream(dev)


def timed(fn):
    torch.cuda.synchronize(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(work)
    fn()
    e1.record(work)
    e1.synchronize()
    return e0.elapsed_time(e1)


def best(fn):
    fn()
    return min(timed(fn) for _ in range(args.repeats))


def half_K(K):
    K = K.copy()
    K[:2] /= 2.0
    return K


K, q, t, depths = capture()
ctx.reserve_icp(H * W)
ctx.set_strict(True)
s = work.cuda_stream
dd = torch.from_numpy(depths).to(dev)
dviews = torch.from_numpy(f3d.views_build(K, W, H, q, t, MAX_DEPTH)).to(dev)
tsdf, weight = (torch.zeros(DIMS[::-1], dtype=torch.float32, device=dev) for _ in range(2))
f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)      # noqa: E731
sizes = [(H >> l, W >> l) for l in range(3)]
Ks = [K, half_K(K), half_K(half_K(K))]
vertex, normal = [f64(h * w, 3) for h, w in sizes], [f64(h * w, 3) for h, w in sizes]
depth = [dd[0]] + [f64(h * w) for h, w in sizes[1:]]
views = torch.from_numpy(np.concatenate([f3d.views_build(Ks[l], sizes[l][1], sizes[l][0], q[:1], t[:1], MAX_DEPTH) for l in range(3)])).to(dev)
pose, status = f64(7), torch.empty(1, dtype=torch.int32, device=dev)
stats1, stats3 = f64(ROUNDS[0], 3), f64(sum(ROUNDS), 3)
torch.cuda.synchronize(dev)
allocs = ctx.alloc_count
ctx.tsdf_integrate_dev(tsdf.data_ptr(), weight.data_ptr(), DIMS, LO, VS, TRUNC, MAX_WEIGHT, dd.data_ptr(), 1, F, H, W, 1.0, MAX_DEPTH, dviews.data_ptr(), s)
nsteps = int(np.floor(MAX_DEPTH / VS)) + 1
ctx.tsdf_raycast_dev(tsdf.data_ptr(), weight.data_ptr(), DIMS, LO, VS, 1.0, K, q[0], t[0], H, W, 0.0, VS, nsteps, vertex[0].data_ptr(),
                     normal[0].data_ptr(), None, s)


def depth_step(l):
    LV.depth_half_dev(ctx, depth[l].data_ptr(), 1 if l == 0 else 0, *sizes[l], 1.0, MAX_DEPTH, GATE, depth[l + 1].data_ptr(), s)


def maps_step(l):
    LV.maps_half_dev(ctx, vertex[l].data_ptr(), normal[l].data_ptr(), None, *sizes[l], views[l].data_ptr(), GATE, vertex[l + 1].data_ptr(),
                     normal[l + 1].data_ptr(), None, s)


def pyramid():
    for l in range(2):
        depth_step(l)
        maps_step(l)


depth_half_ms, maps_half_ms, pyramid_ms = best(lambda: depth_step(0)), best(lambda: maps_step(0)), best(pyramid)

half = np.radians(1.0) / 2
axis = np.array([0.5, -0.7, 0.4]) / np.linalg.norm([0.5, -0.7, 0.4])
dq, b = np.concatenate([[np.cos(half)], np.sin(half) * axis]), q[0]
q0 = np.array([dq[0] * b[0] - dq[1] * b[1] - dq[2] * b[2] - dq[3] * b[3], dq[0] * b[1] + dq[1] * b[0] + dq[2] * b[3] - dq[3] * b[2],
               dq[0] * b[2] - dq[1] * b[3] + dq[2] * b[0] + dq[3] * b[1], dq[0] * b[3] + dq[1] * b[2] - dq[2] * b[1] + dq[3] * b[0]])
t0 = t[0] + 0.02 * np.array([0.6, -0.55, 0.58]) / np.linalg.norm([0.6, -0.55, 0.58])


def errors():
    p = pose.cpu().numpy()
    qa, qb = p[:4] / np.linalg.norm(p[:4]), q[0] / np.linalg.norm(q[0])
    return float(np.linalg.norm(p[4:] - t[0])), float(2 * np.arccos(min(1.0, abs(float(qa @ qb)))))


one_ms = best(lambda: ctx.icp_dev(dd[0].data_ptr(), 1, H, W, K, q0, t0, vertex[0].data_ptr(), normal[0].data_ptr(), H, W, views[0].data_ptr(), 0.1, 1.0,
                                  MAX_DEPTH, ROUNDS[0], 100, pose.data_ptr(), stats1.data_ptr(), status.data_ptr(), s))
one_err, one_status = errors(), int(status[0])
recs = [dict(depth=depth[l].data_ptr(), depth_type=1 if l == 0 else 0, h=sizes[l][0], w=sizes[l][1], K=Ks[l], model_vertex=vertex[l].data_ptr(),
             model_normal=normal[l].data_ptr(), hm=sizes[l][0], wm=sizes[l][1], model_view=views[l].data_ptr(), max_dist=0.1, iterations=ROUNDS[l],
             min_pairs=max(6, 100 >> (2 * l))) for l in range(3)][::-1]
three_ms = best(lambda: LV.icp_levels_dev(ctx, recs, q0, t0, MAX_DEPTH, pose.data_ptr(), stats3.data_ptr(), status.data_ptr(), stream=s))
three_err, three_status = errors(), int(status[0])
coarse_ms = best(lambda: LV.icp_levels_dev(ctx, [dict(recs[0], iterations=10)], q0, t0, MAX_DEPTH, pose.data_ptr(), stats1.data_ptr(), status.data_ptr(),
                                           stream=s))
torch.cuda.synchronize(dev)
assert ctx.alloc_count == allocs, 'the reserved strict context allocated'
pairs3 = stats3.cpu().numpy()[:, 0]

# track_frames through the module (the default context, one readback per frame): host clock around the synchronised call
from Fusion3DSeg.segUtils import reconstruct, registration      # noqa: E402


def track(**kw):
    vol = reconstruct.TSDFVolume(LO, DIMS, VS, TRUNC)
    vol._to_device()                                                           # the upload of the empty volume is not tracking
    n = args.track
    torch.cuda.synchronize(dev)
    start = time.perf_counter()
    _, _, st = registration.track_frames(vol, dd[:n], K, q[:n], t[:n], max_depth=MAX_DEPTH, **kw)
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - start) * 1e3 / n, st.cpu().numpy().tolist()


track_ms = {}
if args.track > 1:
    for name, kw in (('levels1', {}), ('levels3', dict(levels=3, level_iterations=ROUNDS))):
        track(**kw)
        runs = [track(**kw) for _ in range(args.repeats)]
        track_ms[name] = {'ms_per_frame': round(min(r[0] for r in runs), 3), 'status': runs[0][1]}

print(json.dumps({
    'dims': DIMS, 'voxel': VS, 'hw': [H, W], 'frames_integrated': F,
    'depth_half_ms': round(depth_half_ms, 4), 'maps_half_ms': round(maps_half_ms, 4), 'pyramid_two_steps_ms': round(pyramid_ms, 4),
    'icp_1_level_rounds': ROUNDS[0], 'icp_1_level_ms': round(one_ms, 3), 'icp_1_level_status': one_status,
    'icp_1_level_errors_m_rad': one_err,
    'icp_3_levels_rounds': list(ROUNDS[::-1]), 'icp_3_levels_ms': round(three_ms, 3), 'icp_3_levels_status': three_status,
    'icp_3_levels_errors_m_rad': three_err, 'icp_3_levels_pairs': [int(x) for x in pairs3],
    'icp_coarsest_level_10_rounds_ms': round(coarse_ms, 3),
    'start_errors_m_rad': [0.02, float(np.radians(1.0))], 'track_frames': track_ms,
}))
