#!/usr/bin/env python3
"""TSDF reconstruction at size: a 512 x 512 x 160 volume of 2 cm voxels (10.24 x 10.24 x 3.2 m), 256 depth frames of 256 x 192
pixels cast analytically inside a box room from a ring of poses.  HIP events around every call after a warm-up, best of
`--repeats`, on a context of its own that is reserved (f3d_ctx_reserve_tsdf) and strict: it must not allocate.

  integrate     one f3d_tsdf_integrate_dev call over all frames on a fresh volume: ms per call, voxel x frames per second
  extract       f3d_tsdf_extract_count_dev + f3d_tsdf_extract_fill_dev on the integrated volume: ms for the pair, vertices, triangles
  torch         the same integrate written in plain torch ops on the same device (float64, one frame at a time over the whole volume,
                no culling), on the first `--torch-frames` frames, beside the kernel on those same frames; the two states are
                compared: voxels_that_differ = other weight or |tsdf difference| > 1e-5 (where a rotation-matrix projection rounds
                across a pixel border or a truncation bound), voxels_not_equal = any difference in value at all
One JSON line.  python scripts/tsdf_stress.py [--dims 512,512,160] [--voxel 0.02] [--frames 256] [--torch-frames 16]"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / '3d-point-cloud-segmentation-using-2d-img-segmentation_amd'))
import f3d                                        # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--dims', default='512,512,160')
ap.add_argument('--voxel', type=float, default=0.02)
ap.add_argument('--frames', type=int, default=256)
ap.add_argument('--hw', default='192,256')
ap.add_argument('--torch-frames', type=int, default=16)
ap.add_argument('--repeats', type=int, default=3)
args = ap.parse_args()

import torch                                      # noqa: E402

DIMS = tuple(int(x) for x in args.dims.split(','))
H, W = (int(x) for x in args.hw.split(','))
VS, F = args.voxel, args.frames
TRUNC, MAX_DEPTH, MAX_WEIGHT = 4 * VS, 10.0, 64.0
EXT = np.array(DIMS) * VS
LO = np.array([-EXT[0] / 2, -EXT[1] / 2, 0.0])
ROOM_LO, ROOM_HI = LO + 6 * VS, LO + EXT - 6 * VS                              # the walls, six voxels inside the volume

ctx = f3d.Context(0)
dev = torch.device('cuda', ctx.device)


def rot_to_quat(R):
    w = np.sqrt(max(0.0, 1.0 + R[0, 0] + R[1, 1] + R[2, 2])) / 2
    x = np.sqrt(max(0.0, 1.0 + R[0, 0] - R[1, 1] - R[2, 2])) / 2
    y = np.sqrt(max(0.0, 1.0 - R[0, 0] + R[1, 1] - R[2, 2])) / 2
    z = np.sqrt(max(0.0, 1.0 - R[0, 0] - R[1, 1] + R[2, 2])) / 2
    return np.array([w, np.copysign(x, R[2, 1] - R[1, 2]), np.copysign(y, R[0, 2] - R[2, 0]), np.copysign(z, R[1, 0] - R[0, 1])])


def capture():
    """K, wxyzs, translations, rotation matrices, depths float32 [F, H, W]: the room's walls seen from a ring of poses inside it."""
    K = np.array([[0.8 * W, 0.0, W / 2.0], [0.0, 0.8 * W, H / 2.0], [0.0, 0.0, 1.0]])
    uu, vv = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    dc = np.stack([(uu - K[0, 2]) / K[0, 0], (vv - K[1, 2]) / K[1, 1], np.ones_like(uu)], -1).reshape(-1, 3)
    centre = (ROOM_LO + ROOM_HI) / 2
    qs, ts, Rs, depths = [], [], [], []
    for f in range(F):
        a = 2 * np.pi * f / F
        eye = centre + np.array([0.2 * EXT[0] * np.cos(a), 0.2 * EXT[1] * np.sin(a), 0.15 * EXT[2] * np.sin(3 * a)])
        z = np.array([np.cos(a + 0.4), np.sin(a + 0.4), 0.25 * np.sin(5 * a)])
        z /= np.linalg.norm(z)
        x = np.cross(np.array([0.0, 0.0, -1.0]), z)
        x /= np.linalg.norm(x)
        R = np.stack([x, np.cross(z, x), z], axis=1)                            # columns: camera axes in the world (x right, y down)
        D = dc @ R.T
        with np.errstate(divide='ignore'):
            s = np.where(D > 0, (ROOM_HI - eye) / D, (ROOM_LO - eye) / D)
        qs.append(rot_to_quat(R)); ts.append(eye); Rs.append(R)
        depths.append(s.min(axis=1).reshape(H, W))
    return K, np.array(qs), np.array(ts), np.array(Rs), np.array(depths, dtype=np.float32)


def timed(fn):
    s = torch.cuda.current_stream(dev)
    torch.cuda.synchronize(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    fn()
    e1.record(s)
    e1.synchronize()
    return e0.elapsed_time(e1)


def torch_integrate(tsdf, weight, depths, K, Rs, ts):
    """The integrate of include/f3d.h in plain torch ops (rotation matrices instead of the quaternion product), in place."""
    nx, ny, nz = DIMS
    ax = [LO[a] + (torch.arange(n, dtype=torch.float64, device=dev) + 0.5) * VS for a, n in enumerate(DIMS)]
    T, Wt = tsdf.reshape(-1), weight.reshape(-1)
    Kt = torch.from_numpy(K).to(dev)
    for f in range(len(depths)):
        M = Kt @ torch.from_numpy(Rs[f].T.copy()).to(dev)
        o = M @ torch.from_numpy(ts[f]).to(dev)
        h = [((M[r, 2] * ax[2])[:, None, None] + (M[r, 1] * ax[1])[None, :, None] + (M[r, 0] * ax[0])[None, None, :] - o[r]).reshape(-1) for r in range(3)]
        px, py = h[0] / h[2], h[1] / h[2]
        ok = (h[2] > 0) & (px >= 0) & (px < W) & (py >= 0) & (py < H)
        idx = torch.where(ok, torch.floor(py) * W + torch.floor(px), torch.zeros_like(px)).to(torch.int64)
        d = depths[f].reshape(-1)[idx].to(torch.float64)
        sdf = d - h[2]
        ok &= (d > 0) & (d <= MAX_DEPTH) & (sdf >= -TRUNC)
        val = torch.clamp(sdf / TRUNC, max=1.0)
        w64 = Wt.to(torch.float64)
        T.copy_(torch.where(ok, ((T.to(torch.float64) * w64 + val) / (w64 + 1.0)).to(torch.float32), T))
        Wt.copy_(torch.where(ok, torch.clamp(w64 + 1.0, max=MAX_WEIGHT).to(torch.float32), Wt))


K, q, t, Rs, depths = capture()
n = DIMS[0] * DIMS[1] * DIMS[2]
ctx.reserve_tsdf(n)
ctx.set_strict(True)
dd = torch.from_numpy(depths).to(dev)
dviews = torch.from_numpy(f3d.views_build(K, W, H, q, t, MAX_DEPTH)).to(dev)
tsdf, weight = (torch.zeros(DIMS[::-1], dtype=torch.float32, device=dev) for _ in range(2))
allocs = ctx.alloc_count
out = {'dims': list(DIMS), 'voxel': VS, 'frames': F, 'hw': [H, W]}

with torch.cuda.stream(torch.cuda.Stream(dev)):
    sh = lambda: torch.cuda.current_stream(dev).cuda_stream                      # noqa: E731

    def integrate(nframes):
        tsdf.zero_(); weight.zero_()
        return timed(lambda: ctx.tsdf_integrate_dev(tsdf.data_ptr(), weight.data_ptr(), DIMS, LO, VS, TRUNC, MAX_WEIGHT, dd.data_ptr(), 1, nframes, H, W, 1.0,
                                                    MAX_DEPTH, dviews.data_ptr(), sh()))

    integrate(F)                                                                 # warm-up
    ms = min(integrate(F) for _ in range(args.repeats))
    out.update(integrate_ms=round(ms, 3), voxel_frames_per_s=round(n * F / (ms * 1e-3), 1), observed=float((weight > 0).float().mean()))

    sizes = {}

    def extract():
        nv, nt = ctx.tsdf_extract_count_dev(tsdf.data_ptr(), weight.data_ptr(), DIMS, 1.0, sh())
        verts = torch.empty((nv, 3), dtype=torch.float64, device=dev)
        tris = torch.empty((nt, 3), dtype=torch.int32, device=dev)
        ctx.tsdf_extract_fill_dev(tsdf.data_ptr(), DIMS, LO, VS, verts.data_ptr(), tris.data_ptr(), sh())
        sizes.update(vertices=nv, triangles=nt)

    timed(extract)
    out.update(extract_ms=round(min(timed(extract) for _ in range(args.repeats)), 3), **sizes)

    tf = min(args.torch_frames, F)
    if tf > 0:
        integrate(tf)
        k_ms = min(integrate(tf) for _ in range(args.repeats))
        k_t, k_w = tsdf.clone(), weight.clone()

        def torch_run():
            tsdf.zero_(); weight.zero_()
            return timed(lambda: torch_integrate(tsdf, weight, dd[:tf], K, Rs, t))

        torch_run()
        t_ms = min(torch_run() for _ in range(args.repeats))
        differ = (k_w != weight) | ((k_t - tsdf).abs() > 1e-5)
        out.update(torch_frames=tf, kernel_ms_on_torch_frames=round(k_ms, 3), torch_ms=round(t_ms, 3), torch_over_kernel=round(t_ms / k_ms, 2),
                   voxels_that_differ=int(differ.sum()), voxels_not_equal=int(((k_t != tsdf) | (k_w != weight)).sum()), max_tsdf_difference_elsewhere=float((k_t - tsdf).abs()[~differ].max()))
out['allocations_while_strict'] = ctx.alloc_count - allocs
print(json.dumps(out), flush=True)
ctx.close()
