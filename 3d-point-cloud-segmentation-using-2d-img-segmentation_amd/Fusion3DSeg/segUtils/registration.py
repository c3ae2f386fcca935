"""Registration: camera poses refined against the model being built (no reference counterpart).

Every other route takes its camera poses as given, from an RTAB-Map or ARKit export; a pose that is off by a centimetre or half a
degree lands the 2D masks on the wrong points at object borders and makes the TSDF average two copies of each surface.  This module
is the producer of poses: ``raycast`` renders a ``TSDFVolume`` from a pose into a vertex map and a normal map, ``icp`` aligns a depth
frame to such maps by projective point-to-plane ICP, ``track_frames`` does both per frame and integrates the frame at the refined
pose (frame-to-model tracking).  All of it runs on the GPU (f3d_tsdf_raycast, f3d_icp_sums, f3d_icp: include/f3d.h states the
contract, tests/icp_ref.py restates it in NumPy).

A pixel (u, v) stands for the ray through (u + 0.5, v + 0.5), the convention of ``TSDFVolume.integrate``.  NumPy arrays in, NumPy
arrays back; device tensors in, or a volume that is on the device, keep everything on the GPU, ordered with torch's current stream.
There is no CPU fallback.  Out of scope: image pyramids, colour or photometric terms, robust weights, loop closure, and
re-unprojecting ``Fusion``'s stored frames at refined poses.
"""
import math

import numpy as np

import f3d
from f3d.tensors import depth_code, on_device, torch_device, work_stream

__all__ = ['raycast', 'icp_sums', 'icp', 'track_frames']


def _positive(name, x):
    x = float(x)
    if not (x > 0.0 and math.isfinite(x)):
        raise ValueError(f'{name} must be finite and positive, got {x}')
    return x


def _pose(K, wxyz, t, what=''):
    K, q, t = np.asarray(K, np.float64), np.asarray(wxyz, np.float64).reshape(-1), np.asarray(t, np.float64).reshape(-1)
    if K.shape != (3, 3) or not np.isfinite(K).all():
        raise ValueError(f'{what}K must be a finite 3 x 3 matrix')
    if q.shape != (4,) or t.shape != (3,) or not np.isfinite(q).all() or not np.isfinite(t).all():
        raise ValueError(f'{what}wxyz must be 4 and {what}t 3 finite numbers')
    if not q.any():
        raise ZeroDivisionError('a zero quaternion is no rotation')
    return np.ascontiguousarray(K), np.ascontiguousarray(q), np.ascontiguousarray(t)


def _min_weight(min_weight):
    min_weight = float(min_weight)
    if not min_weight >= 1.0:
        raise ValueError(f'min_weight must be at least 1, got {min_weight}')
    return min_weight


def _march(volume, near, far, step):
    near, far = float(near), float(far)
    step = _positive('step', volume.voxel if step is None else step)
    if not (near >= 0.0 and math.isfinite(far) and far >= near):
        raise ValueError(f'0 <= near <= far, both finite, expected; got {near} and {far}')
    nsteps = int(math.floor((far - near) / step)) + 1
    if nsteps >= 1 << 31:
        raise ValueError(f'{nsteps} samples per ray are too many')
    return near, step, nsteps


def raycast(volume, K, wxyz, t, hw, min_weight=1, near=0.0, far=10.0, step=None):
    """Model maps of ``volume`` (a ``TSDFVolume``) seen from the camera->world pose (``wxyz``, ``t``) with intrinsics ``K`` in an
    image of ``hw = (h, w)`` pixels -> (vertex float64 [h, w, 3] and unit normal float64 [h, w, 3] in the world frame, depth float64
    [h, w] along the camera z axis).  Rays are sampled every ``step`` (default: the voxel edge) from ``near`` to ``far``; only voxels seen at
    least ``min_weight`` times count.  A pixel without a hit has NaN rows and depth 0.  Device tensors for a volume on the device."""
    K, q, t = _pose(K, wxyz, t)
    h, w = (int(x) for x in hw)
    if h < 1 or w < 1 or h * w >= 1 << 31:
        raise ValueError(f'hw must be two positive sizes with a product below 2^31, got {(h, w)}')
    min_weight = _min_weight(min_weight)
    near, step, nsteps = _march(volume, near, far, step)
    ctx = f3d.default_context()
    if not volume.on_device:
        vertex, normal, depth = ctx.tsdf_raycast(volume.tsdf, volume.weight, volume.lo, volume.voxel, min_weight, K, q, t, h, w, near, step, nsteps)
        return vertex.reshape(h, w, 3), normal.reshape(h, w, 3), depth.reshape(h, w)
    torch, dev = torch_device(ctx, 'raycast')
    with torch.cuda.device(dev), work_stream(dev) as work:
        vertex, normal = (torch.empty((h, w, 3), dtype=torch.float64, device=dev) for _ in range(2))
        depth = torch.empty((h, w), dtype=torch.float64, device=dev)
        ctx.tsdf_raycast_dev(volume.tsdf.data_ptr(), volume.weight.data_ptr(), volume.dims, volume.lo, volume.voxel, min_weight, K, q, t, h, w, near,
                             step, nsteps, vertex.data_ptr(), normal.data_ptr(), depth.data_ptr(), work.cuda_stream)
    for x in (vertex, normal, depth):
        x.record_stream(torch.cuda.current_stream(dev))
    return vertex, normal, depth


def _icp_args(depth, K, wxyz, t, model_vertex, model_normal, model_K, model_wxyz, model_t, max_dist, depth_scale, max_depth):
    """The checked arguments of icp_sums / icp, before any device is touched."""
    if not on_device(depth):
        depth = np.asarray(depth)
    if len(depth.shape) != 2 or int(depth.shape[0]) < 1 or int(depth.shape[1]) < 1:
        raise ValueError(f'depth must be one [h, w] frame with pixels, got {tuple(depth.shape)}')
    code = depth_code(depth)
    model_vertex, model_normal = (a if on_device(a) else np.asarray(a, np.float64) for a in (model_vertex, model_normal))
    K, q, t = _pose(K, wxyz, t)
    mK, mq, mt = _pose(model_K, model_wxyz, model_t, 'model_')
    shape = tuple(int(x) for x in model_vertex.shape)
    if len(shape) != 3 or shape[2] != 3 or shape[0] < 1 or shape[1] < 1 or tuple(int(x) for x in model_normal.shape) != shape:
        raise ValueError(f'model_vertex and model_normal must both be [hm, wm, 3], got {shape} and {tuple(model_normal.shape)}')
    max_dist, depth_scale, max_depth = _positive('max_dist', max_dist), _positive('depth_scale', depth_scale), _positive('max_depth', max_depth)
    view = f3d.views_build(mK, shape[1], shape[0], mq[None], mt[None], max_depth)
    return depth, code, K, q, t, model_vertex, model_normal, shape[0], shape[1], view, max_dist, depth_scale, max_depth


def _rounds(iterations, min_pairs):
    iterations, min_pairs = int(iterations), int(min_pairs)
    if iterations < 1 or min_pairs < 6:
        raise ValueError(f'iterations must be at least 1 and min_pairs at least 6, got {iterations} and {min_pairs}')
    return iterations, min_pairs


def _info(stats, status, xp=np):
    """status, counts and rms per round from the stats rows {count, sum r^2, status}."""
    counts = stats[:, 0]
    return {'status': int(status), 'counts': counts, 'rms': xp.sqrt(stats[:, 1] / xp.where(counts > 0, counts, xp.ones_like(counts)))}


def icp_sums(depth, K, wxyz, t, model_vertex, model_normal, model_K, model_wxyz, model_t, max_dist=0.1, depth_scale=1.0, max_depth=10):
    """The 29 sums of one point-to-plane linearisation, for callers who bring their own solver: the 21 products J_a J_b (a <= b), the
    6 products J_a r, r r and the pair count, over the pixels of the depth frame ``depth`` [h, w] (uint16, float32 or float64) at the
    camera->world pose (``wxyz``, ``t``, intrinsics ``K``) that find a model point within ``max_dist``.  The model is a pair of maps
    ``model_vertex``, ``model_normal`` [hm, wm, 3] in the world frame (NaN = missing; what ``raycast`` returns) seen by the camera
    (``model_K``, ``model_wxyz``, ``model_t``).  -> float64 [29]; a device tensor when any of the arrays is one."""
    depth, code, K, q, t, model_vertex, model_normal, hm, wm, view, max_dist, depth_scale, max_depth = _icp_args(
        depth, K, wxyz, t, model_vertex, model_normal, model_K, model_wxyz, model_t, max_dist, depth_scale, max_depth)
    ctx = f3d.default_context()
    if not (on_device(depth) or on_device(model_vertex) or on_device(model_normal)):
        return ctx.icp_sums(depth, K, q, t, model_vertex, model_normal, hm, wm, view, max_dist, depth_scale, max_depth)
    torch, dev = torch_device(ctx, 'icp_sums')
    h, w = (int(x) for x in depth.shape)
    with torch.cuda.device(dev), work_stream(dev) as work:
        d, mv, mn, dview = _to_device(torch, dev, depth, model_vertex, model_normal, view)
        sums = torch.empty(f3d.ICP_NSUMS, dtype=torch.float64, device=dev)
        ctx.icp_sums_dev(d.data_ptr(), code, h, w, K, q, t, mv.data_ptr(), mn.data_ptr(), hm, wm, dview.data_ptr(), max_dist, depth_scale, max_depth,
                         sums.data_ptr(), work.cuda_stream)
    for x in (d, mv, mn, dview, sums):
        x.record_stream(torch.cuda.current_stream(dev))
    return sums


def _to_device(torch, dev, depth, model_vertex, model_normal, view):
    as_tensor = lambda a: a if on_device(a) else torch.from_numpy(np.ascontiguousarray(a))     # noqa: E731
    d = as_tensor(depth).to(dev).contiguous()
    mv, mn = (as_tensor(a).to(dev, torch.float64).contiguous() for a in (model_vertex, model_normal))
    return d, mv, mn, torch.from_numpy(view).to(dev)


def _icp_device(ctx, torch, dev, work, d, code, K, q, t, mv, mn, hm, wm, dview, max_dist, depth_scale, max_depth, iterations, min_pairs):
    """Enqueues the rounds on `work` -> (pose [7], stats [iterations, 3], status [1]) on the device."""
    pose = torch.empty(7, dtype=torch.float64, device=dev)
    stats = torch.empty((iterations, 3), dtype=torch.float64, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    ctx.icp_dev(d.data_ptr(), code, int(d.shape[0]), int(d.shape[1]), K, q, t, mv.data_ptr(), mn.data_ptr(), hm, wm, dview.data_ptr(), max_dist,
                depth_scale, max_depth, iterations, min_pairs, pose.data_ptr(), stats.data_ptr(), status.data_ptr(), work.cuda_stream)
    return pose, stats, status


def icp(depth, K, wxyz, t, model_vertex, model_normal, model_K, model_wxyz, model_t, max_dist=0.1, depth_scale=1.0, max_depth=10, iterations=10,
        min_pairs=100):
    """``iterations`` rounds of projective point-to-plane ICP of the depth frame against the model maps (the arguments of ``icp_sums``),
    starting from the pose (``wxyz``, ``t``), all on the device with no host round trip between the rounds -> (wxyz [4], t [3], info).
    ``info`` holds the final ``status`` (0 = converging, 1 = lost: fewer than ``min_pairs`` pairs or a degenerate system; the pose of a
    lost call is the one its lost round started from) and ``counts`` and ``rms`` per round, measured before that round's update."""
    depth, code, K, q, t, model_vertex, model_normal, hm, wm, view, max_dist, depth_scale, max_depth = _icp_args(
        depth, K, wxyz, t, model_vertex, model_normal, model_K, model_wxyz, model_t, max_dist, depth_scale, max_depth)
    iterations, min_pairs = _rounds(iterations, min_pairs)
    ctx = f3d.default_context()
    if not (on_device(depth) or on_device(model_vertex) or on_device(model_normal)):
        pose, stats, status = ctx.icp(depth, K, q, t, model_vertex, model_normal, hm, wm, view, max_dist, depth_scale, max_depth, iterations, min_pairs)
        return pose[:4].copy(), pose[4:].copy(), _info(stats, status)
    torch, dev = torch_device(ctx, 'icp')
    with torch.cuda.device(dev), work_stream(dev) as work:
        d, mv, mn, dview = _to_device(torch, dev, depth, model_vertex, model_normal, view)
        pose, stats, status = _icp_device(ctx, torch, dev, work, d, code, K, q, t, mv, mn, hm, wm, dview, max_dist, depth_scale, max_depth, iterations,
                                          min_pairs)
    for x in (d, mv, mn, dview, pose, stats, status):
        x.record_stream(torch.cuda.current_stream(dev))
    return pose[:4].clone(), pose[4:].clone(), _info(stats, status[0], torch)


def track_frames(volume, depths, K, wxyzs, translations, depth_scale=1.0, max_depth=10, max_dist=0.1, iterations=10, min_pairs=100, min_weight=1,
                 integrate=True, colors=None):
    """Frame-to-model tracking of the depth frames ``depths`` [F, h, w] into ``volume`` (a ``TSDFVolume``), in frame order.  A frame
    that meets a volume with no weight is integrated at its given pose.  Every later frame is ray-cast at its given pose, the prior
    (samples every voxel edge up to ``max_depth``), aligned to those maps by ``icp`` starting from the prior, takes the refined pose if
    the status is 0 and the prior otherwise, and is integrated at the pose taken (``integrate=False``: only frames that meet an empty
    volume are integrated).  -> (wxyzs [F, 4], translations [F, 3], status int32 [F]); NumPy arrays, or device tensors when the depths
    or the volume are on the device.  ``colors``: the frames' colour images, uint8 [F, hc, wc, 3], for a volume built with
    ``color=True``; each frame that is integrated hands its image to ``integrate``.

    One host synchronisation per frame: the readback of the 7 doubles of the pose and the status, because ``views_build``, which makes
    the record ``integrate`` projects with, needs the pose on the host.  While the volume is empty its weights are looked at, too."""
    if not on_device(depths):
        depths = np.asarray(depths)
    if len(depths.shape) != 3 or int(depths.shape[1]) < 1 or int(depths.shape[2]) < 1:
        raise ValueError(f'depths must be [F, h, w] with pixels, got {tuple(depths.shape)}')
    code = depth_code(depths)
    F, h, w = (int(x) for x in depths.shape)
    qs, ts = np.asarray(wxyzs, np.float64).reshape(-1, 4), np.asarray(translations, np.float64).reshape(-1, 3)
    if len(qs) != F or len(ts) != F:
        raise ValueError(f'{len(qs)} quaternions and {len(ts)} translations for {F} depth frames')
    poses = [_pose(K, qs[f], ts[f]) for f in range(F)]
    K = np.ascontiguousarray(np.asarray(K, np.float64))
    depth_scale, max_depth, max_dist = _positive('depth_scale', depth_scale), _positive('max_depth', max_depth), _positive('max_dist', max_dist)
    iterations, min_pairs = _rounds(iterations, min_pairs)
    min_weight = _min_weight(min_weight)
    near, step, nsteps = _march(volume, 0.0, max_depth, None)
    out_q, out_t, status = qs.copy(), ts.copy(), np.zeros(F, np.int32)
    if colors is not None:
        colors = volume._color_images(colors, F)
    device = on_device(depths) or volume.on_device or (colors is not None and on_device(colors))
    if F == 0:
        return _tracked(device, out_q, out_t, status)
    ctx = f3d.default_context()
    empty = True
    if not device:
        for f in range(F):
            _, q, t = poses[f]
            empty = empty and not volume.weight.any()
            if not empty:
                view = f3d.views_build(K, w, h, q[None], t[None], max_depth)
                vertex, normal, _ = ctx.tsdf_raycast(volume.tsdf, volume.weight, volume.lo, volume.voxel, min_weight, K, q, t, h, w, near, step, nsteps)
                pose, _, status[f] = ctx.icp(depths[f], K, q, t, vertex, normal, h, w, view, max_dist, depth_scale, max_depth, iterations, min_pairs)
                if status[f] == 0:
                    out_q[f], out_t[f] = pose[:4], pose[4:]
            if empty or integrate:
                volume.integrate(depths[f:f + 1], K, out_q[f:f + 1], out_t[f:f + 1], depth_scale, max_depth,
                                 colors=None if colors is None else colors[f:f + 1])
        return out_q, out_t, status
    torch, dev = torch_device(ctx, 'track_frames')
    volume._to_device()
    d_all = (depths if on_device(depths) else torch.from_numpy(np.ascontiguousarray(depths))).to(dev).contiguous()
    for f in range(F):
        _, q, t = poses[f]
        empty = empty and not bool(volume.weight.any())
        if not empty:
            view = f3d.views_build(K, w, h, q[None], t[None], max_depth)
            with torch.cuda.device(dev), work_stream(dev) as work:
                vertex, normal = (torch.empty((h * w, 3), dtype=torch.float64, device=dev) for _ in range(2))
                ctx.tsdf_raycast_dev(volume.tsdf.data_ptr(), volume.weight.data_ptr(), volume.dims, volume.lo, volume.voxel, min_weight, K, q, t, h, w,
                                     near, step, nsteps, vertex.data_ptr(), normal.data_ptr(), None, work.cuda_stream)
                dview = torch.from_numpy(view).to(dev)
                pose, stats, lost = _icp_device(ctx, torch, dev, work, d_all[f], code, K, q, t, vertex, normal, h, w, dview, max_dist, depth_scale,
                                                max_depth, iterations, min_pairs)
                back = torch.cat([pose, lost.to(torch.float64)])
            for x in (vertex, normal, dview, pose, stats, lost):
                x.record_stream(torch.cuda.current_stream(dev))
            back = back.cpu().numpy()                                  # the one synchronisation of the frame
            status[f] = int(back[7])
            if status[f] == 0:
                out_q[f], out_t[f] = back[:4], back[4:7]
        if empty or integrate:
            volume.integrate(d_all[f:f + 1], K, out_q[f:f + 1], out_t[f:f + 1], depth_scale, max_depth,
                             colors=None if colors is None else colors[f:f + 1])
    return _tracked(True, out_q, out_t, status)


def _tracked(device, out_q, out_t, status):
    if not device:
        return out_q, out_t, status
    ctx = f3d.default_context()
    torch, dev = torch_device(ctx, 'track_frames')
    return tuple(torch.from_numpy(a).to(dev) for a in (out_q, out_t, status))
