#!/usr/bin/env python3
"""Registration with colour at size: the scene of registration_stress.py (a 256^3 volume of 2 cm voxels holding a box room, a
480 x 640 camera inside it), the room's walls textured and the volume built with colour, then

  raycast   one f3d_tsdf_raycast_color_dev call (the five maps) beside one f3d_tsdf_raycast_dev call (three): ms each
  icp       one f3d_icp_color_dev call of 10 rounds beside one f3d_icp_dev call, both from a pose 2 cm and 1 degree off: ms each, and
            what the rounds did to the pose

HIP events around every call after a warm-up, best of `--repeats`, on a context of its own that is reserved
(f3d_ctx_reserve_icp_color) and strict: it must not allocate.  One JSON line.
python scripts/registration_color_stress.py [--dims 256,256,256] [--hw 480,640] [--color-weight 0.1]"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / '3d-point-cloud-segmentation-using-2d-img-segmentation_amd'))
import f3d                                        # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--dims', default='256,256,256')
ap.add_argument('--voxel', type=float, default=0.02)
ap.add_argument('--frames', type=int, default=8)
ap.add_argument('--hw', default='480,640')
ap.add_argument('--rounds', type=int, default=10)
ap.add_argument('--repeats', type=int, default=3)
ap.add_argument('--color-weight', type=float, default=0.1)
args = ap.parse_args()

import torch                                      # noqa: E402

DIMS = tuple(int(x) for x in args.dims.split(','))
H, W = (int(x) for x in args.hw.split(','))
VS, F = args.voxel, args.frames
TRUNC, MAX_DEPTH, MAX_WEIGHT = 4 * VS, 10.0, 64.0
EXT = np.array(DIMS) * VS
LO = -EXT / 2
ROOM_LO, ROOM_HI = LO + 8 * VS, LO + EXT - 8 * VS                              # the walls, eight voxels inside the volume
WAVES = np.array([[1.0, 0.3, 0.2], [-0.4, 1.0, 0.3], [0.7, -0.7, 0.5]])        # one wave vector per channel, wavelength 0.5 m
WAVES /= np.linalg.norm(WAVES, axis=1)[:, None]

ctx = f3d.Context(0)
dev = torch.device('cuda', ctx.device)


def rot_to_quat(R):
    w = np.sqrt(max(0.0, 1.0 + R[0, 0] + R[1, 1] + R[2, 2])) / 2
    x = np.sqrt(max(0.0, 1.0 + R[0, 0] - R[1, 1] - R[2, 2])) / 2
    y = np.sqrt(max(0.0, 1.0 - R[0, 0] + R[1, 1] - R[2, 2])) / 2
    z = np.sqrt(max(0.0, 1.0 - R[0, 0] - R[1, 1] + R[2, 2])) / 2
    return np.array([w, np.copysign(x, R[2, 1] - R[1, 2]), np.copysign(y, R[0, 2] - R[2, 0]), np.copysign(z, R[1, 0] - R[0, 1])])


def capture():
    """K, wxyzs, translations, depths float32 [F, H, W], colours uint8 [F, H, W, 3]: registration_stress.py's frames, and for every pixel
    a sinusoid per channel of the wall point it sees."""
    K = np.array([[0.8 * W, 0.0, W / 2.0], [0.0, 0.8 * W, H / 2.0], [0.0, 0.0, 1.0]])
    uu, vv = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    dc = np.stack([(uu - K[0, 2]) / K[0, 0], (vv - K[1, 2]) / K[1, 1], np.ones_like(uu)], -1).reshape(-1, 3)
    qs, ts, depths, colours = [], [], [], []
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
            s = np.where(D > 0, (ROOM_HI - eye) / D, (ROOM_LO - eye) / D).min(axis=1)
        p = eye[None, :] + D * s[:, None]
        qs.append(rot_to_quat(R)); ts.append(eye)
        depths.append(s.reshape(H, W))
        colours.append(np.clip(np.round(128.0 + 100.0 * np.sin(2.0 * np.pi * (p @ WAVES.T) / 0.5)), 0, 255).astype(np.uint8).reshape(H, W, 3))
    return K, np.array(qs), np.array(ts), np.array(depths, dtype=np.float32), np.array(colours)


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


def errors(p):
    qa, qb = p[:4] / np.linalg.norm(p[:4]), q[0] / np.linalg.norm(q[0])
    return float(np.linalg.norm(p[4:] - t[0])), float(2 * np.arccos(min(1.0, abs(float(qa @ qb)))))


K, q, t, depths, colours = capture()
ctx.reserve_icp_color(H * W)
ctx.set_strict(True)
s = work.cuda_stream
dd, drgb = torch.from_numpy(depths).to(dev), torch.from_numpy(colours).to(dev)
dviews = torch.from_numpy(f3d.views_build(K, W, H, q, t, MAX_DEPTH)).to(dev)
tsdf, weight = (torch.zeros(DIMS[::-1], dtype=torch.float32, device=dev) for _ in range(2))
color = torch.zeros(DIMS[::-1] + (4,), dtype=torch.float32, device=dev)
vertex, normal, rgb = (torch.empty((H * W, 3), dtype=torch.float64, device=dev) for _ in range(3))
zmap, inten = (torch.empty(H * W, dtype=torch.float64, device=dev) for _ in range(2))
plain = [torch.empty((H * W, 3), dtype=torch.float64, device=dev), torch.empty((H * W, 3), dtype=torch.float64, device=dev),
         torch.empty(H * W, dtype=torch.float64, device=dev)]
pose, pose_c = (torch.empty(7, dtype=torch.float64, device=dev) for _ in range(2))
stats, stats_c = (torch.empty((args.rounds, n), dtype=torch.float64, device=dev) for n in (3, 5))
status, status_c = (torch.empty(1, dtype=torch.int32, device=dev) for _ in range(2))
torch.cuda.synchronize(dev)
allocs = ctx.alloc_count
ctx.tsdf_integrate_color_dev(tsdf.data_ptr(), weight.data_ptr(), color.data_ptr(), DIMS, LO, VS, TRUNC, MAX_WEIGHT, dd.data_ptr(), 1, drgb.data_ptr(), F,
                             H, W, H, W, 1.0, MAX_DEPTH, dviews.data_ptr(), s)
nsteps = int(np.floor(MAX_DEPTH / VS)) + 1
ray = (DIMS, LO, VS, 1.0, K, q[0], t[0], H, W, 0.0, VS, nsteps)
ray_ms = best(lambda: ctx.tsdf_raycast_dev(tsdf.data_ptr(), weight.data_ptr(), *ray, *(m.data_ptr() for m in plain), s))
ray_color_ms = best(lambda: ctx.tsdf_raycast_color_dev(tsdf.data_ptr(), weight.data_ptr(), color.data_ptr(), *ray, vertex.data_ptr(), normal.data_ptr(),
                                                       zmap.data_ptr(), rgb.data_ptr(), inten.data_ptr(), s))
torch.cuda.synchronize(dev)
same_maps = all(bool((a.view(torch.int64) == b.view(torch.int64)).all()) for a, b in zip(plain, (vertex, normal, zmap)))
hits, coloured = int((zmap > 0).sum()), int(torch.isfinite(inten).sum())

half = np.radians(1.0) / 2
axis = np.array([0.5, -0.7, 0.4]) / np.linalg.norm([0.5, -0.7, 0.4])
dq, b = np.concatenate([[np.cos(half)], np.sin(half) * axis]), q[0]
q0 = np.array([dq[0] * b[0] - dq[1] * b[1] - dq[2] * b[2] - dq[3] * b[3], dq[0] * b[1] + dq[1] * b[0] + dq[2] * b[3] - dq[3] * b[2],
               dq[0] * b[2] - dq[1] * b[3] + dq[2] * b[0] + dq[3] * b[1], dq[0] * b[3] + dq[1] * b[2] - dq[2] * b[1] + dq[3] * b[0]])
t0 = t[0] + 0.02 * np.array([0.6, -0.55, 0.58]) / np.linalg.norm([0.6, -0.55, 0.58])
icp = (dd[0].data_ptr(), 1, H, W, K, q0, t0, vertex.data_ptr(), normal.data_ptr(), H, W, dviews[0].data_ptr(), 0.1)
icp_ms = best(lambda: ctx.icp_dev(*icp, 1.0, MAX_DEPTH, args.rounds, 100, pose.data_ptr(), stats.data_ptr(), status.data_ptr(), s))
icp_color_ms = best(lambda: ctx.icp_color_dev(*icp, inten.data_ptr(), drgb[0].data_ptr(), H, W, args.color_weight, 1.0, MAX_DEPTH, args.rounds, 100,
                                              pose_c.data_ptr(), stats_c.data_ptr(), status_c.data_ptr(), s))
torch.cuda.synchronize(dev)
assert ctx.alloc_count == allocs, 'the reserved strict context allocated'
st, sc = stats.cpu().numpy(), stats_c.cpu().numpy()
e, ec = errors(pose.cpu().numpy()), errors(pose_c.cpu().numpy())
print(json.dumps({
    'dims': DIMS, 'voxel': VS, 'hw': [H, W], 'frames_integrated': F, 'samples_per_ray': nsteps,
    'raycast_ms': round(ray_ms, 3), 'raycast_color_ms': round(ray_color_ms, 3), 'geometry_maps_equal': same_maps, 'hits': hits, 'coloured_hits': coloured,
    'icp_rounds': args.rounds, 'color_weight': args.color_weight, 'icp_ms': round(icp_ms, 3), 'icp_color_ms': round(icp_color_ms, 3),
    'icp_status': int(status[0]), 'icp_color_status': int(status_c[0]),
    'pairs_last_round': int(st[-1, 0]), 'color_pairs_last_round': [int(sc[-1, 0]), int(sc[-1, 3])],
    'color_rms_first_last': [float(np.sqrt(sc[0, 4] / max(sc[0, 3], 1.0))), float(np.sqrt(sc[-1, 4] / max(sc[-1, 3], 1.0)))],
    'translation_error_m': {'start': 0.02, 'icp': e[0], 'icp_color': ec[0]},
    'rotation_error_rad': {'start': float(np.radians(1.0)), 'icp': e[1], 'icp_color': ec[1]},
}))
