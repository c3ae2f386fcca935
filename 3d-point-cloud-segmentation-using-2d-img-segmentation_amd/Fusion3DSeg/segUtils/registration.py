"""Registration: camera poses refined against the model being built (no reference counterpart).

Every other route takes its camera poses as given, from an RTAB-Map or ARKit export; a pose that is off by a centimetre or half a
degree lands the 2D masks on the wrong points at object borders and makes the TSDF average two copies of each surface.  This module
is the producer of poses: ``raycast`` renders a ``TSDFVolume`` from a pose into a vertex map and a normal map, ``icp`` aligns a depth
frame to such maps by projective point-to-plane ICP, ``track_frames`` does both per frame and integrates the frame at the refined
pose (frame-to-model tracking).  All of it runs on the GPU (f3d_tsdf_raycast, f3d_icp_sums, f3d_icp: include/f3d.h states the
contract, tests/icp_ref.py restates it in NumPy).

Depth cannot see a motion that maps the geometry onto itself: along a wall, about the axis of a round object.  The colour images can.
``raycast(..., colors=True)`` renders the colour of a volume built with ``color=True`` along with its maps, ``icp_sums`` / ``icp`` take
a photometric term (``color=``, ``model_intensity=``, ``color_weight=``: the intensity residual between the frame's colour image and
the model's intensity map, weighted into the same 6 x 6 system), and ``track_frames(..., colors=..., color_weight=...)`` uses both
(f3d_tsdf_raycast_color, f3d_icp_color_sums, f3d_icp_color; restated in tests/icp_color_ref.py).

A pixel (u, v) stands for the ray through (u + 0.5, v + 0.5), the convention of ``TSDFVolume.integrate``.  NumPy arrays in, NumPy
arrays back; device tensors in, or a volume that is on the device, keep everything on the GPU, ordered with torch's current stream.
There is no CPU fallback.

A start pose a few centimetres off on a surface with structure near the pixel scale needs ``icp(..., levels=3)``: pyramids of the
depth frame and of the model maps by gated 2 x 2 averages, the rounds chained coarse to fine on the device (f3d_depth_half,
f3d_maps_half, f3d_icp_levels; restated in tests/levels_ref.py).  ``track_frames`` takes the same three arguments.

Out of scope: pyramids of the colour image, robust weights, an intensity-difference gate, exposure compensation, colour from
anything but the volume, loop closure, and re-unprojecting ``Fusion``'s stored frames at refined poses.
"""
import math

import numpy as np

import f3d
from f3d.tensors import depth_code, on_device, torch_device, upload, work_stream

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


def raycast(volume, K, wxyz, t, hw, min_weight=1, near=0.0, far=10.0, step=None, colors=False):
    """Model maps of ``volume`` (a ``TSDFVolume``) seen from the camera->world pose (``wxyz``, ``t``) with intrinsics ``K`` in an
    image of ``hw = (h, w)`` pixels -> (vertex float64 [h, w, 3] and unit normal float64 [h, w, 3] in the world frame, depth float64
    [h, w] along the camera z axis).  Rays are sampled every ``step`` (default: the voxel edge) from ``near`` to ``far``; only voxels seen at
    least ``min_weight`` times count.  A pixel without a hit has NaN rows and depth 0.  Device tensors for a volume on the device.
    ``colors=True``, for a volume built with ``color=True``: two more maps after the three, rgb float64 [h, w, 3] on the 0..255 scale
    and intensity float64 [h, w] = (0.299 R + 0.587 G + 0.114 B) / 255, NaN where a pixel has no hit or its hit no colour."""
    K, q, t = _pose(K, wxyz, t)
    if colors and volume.color is None:
        raise ValueError('colors=True needs a volume built with color=True')
    h, w = (int(x) for x in hw)
    if h < 1 or w < 1 or h * w >= 1 << 31:
        raise ValueError(f'hw must be two positive sizes with a product below 2^31, got {(h, w)}')
    min_weight = _min_weight(min_weight)
    near, step, nsteps = _march(volume, near, far, step)
    ctx = f3d.default_context()
    if not volume.on_device:
        if colors:
            vertex, normal, depth, rgb, intensity = ctx.tsdf_raycast_color(volume.tsdf, volume.weight, volume.color, volume.lo, volume.voxel, min_weight,
                                                                           K, q, t, h, w, near, step, nsteps)
            return vertex.reshape(h, w, 3), normal.reshape(h, w, 3), depth.reshape(h, w), rgb.reshape(h, w, 3), intensity.reshape(h, w)
        vertex, normal, depth = ctx.tsdf_raycast(volume.tsdf, volume.weight, volume.lo, volume.voxel, min_weight, K, q, t, h, w, near, step, nsteps)
        return vertex.reshape(h, w, 3), normal.reshape(h, w, 3), depth.reshape(h, w)
    torch, dev = torch_device(ctx, 'raycast')
    with torch.cuda.device(dev), work_stream(dev) as work:
        vertex, normal = (torch.empty((h, w, 3), dtype=torch.float64, device=dev) for _ in range(2))
        depth = torch.empty((h, w), dtype=torch.float64, device=dev)
        out = (vertex, normal, depth)
        if colors:
            out += (torch.empty((h, w, 3), dtype=torch.float64, device=dev), torch.empty((h, w), dtype=torch.float64, device=dev))
            ctx.tsdf_raycast_color_dev(volume.tsdf.data_ptr(), volume.weight.data_ptr(), volume.color.data_ptr(), volume.dims, volume.lo, volume.voxel,
                                       min_weight, K, q, t, h, w, near, step, nsteps, *(x.data_ptr() for x in out), work.cuda_stream)
        else:
            ctx.tsdf_raycast_dev(volume.tsdf.data_ptr(), volume.weight.data_ptr(), volume.dims, volume.lo, volume.voxel, min_weight, K, q, t, h, w,
                                 near, step, nsteps, vertex.data_ptr(), normal.data_ptr(), depth.data_ptr(), work.cuda_stream)
    for x in out:
        x.record_stream(torch.cuda.current_stream(dev))
    return out


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


def _color_args(color, model_intensity, color_weight, hm, wm):
    """The checked colour arguments of icp_sums / icp, before any device is touched: None when none of the three is given, else
    (color uint8 [hc, wc, 3], model_intensity float64 [hm, wm], color_weight); some but not all of them is a ValueError."""
    given = [x is not None for x in (color, model_intensity, color_weight)]
    if not any(given):
        return None
    if not all(given):
        raise ValueError('color, model_intensity and color_weight go together: pass all three or none')
    color, model_intensity = (a if on_device(a) else np.asarray(a) for a in (color, model_intensity))
    if len(model_intensity.shape) != 2:
        raise ValueError(f'model_intensity must be [hm, wm], got {tuple(model_intensity.shape)}')
    _, _, color_weight = f3d.icp_color_check(model_intensity, color, color_weight, hm, wm)
    return color, model_intensity, color_weight


def _color_to_device(torch, dev, color, model_intensity):
    as_tensor = lambda a: a if on_device(a) else torch.from_numpy(np.ascontiguousarray(a))     # noqa: E731
    return as_tensor(color).to(dev).contiguous(), as_tensor(model_intensity).to(dev).contiguous()


def _rounds(iterations, min_pairs):
    iterations, min_pairs = int(iterations), int(min_pairs)
    if iterations < 1 or min_pairs < 6:
        raise ValueError(f'iterations must be at least 1 and min_pairs at least 6, got {iterations} and {min_pairs}')
    return iterations, min_pairs


def _info(stats, status, xp=np):
    """status, counts and rms per round from the stats rows {count, sum r^2, status}; with the two colour columns {colour count, sum rc^2}
    color_counts and color_rms as well."""
    rms = lambda n, ss: xp.sqrt(ss / xp.where(n > 0, n, xp.ones_like(n)))                      # noqa: E731
    info = {'status': int(status), 'counts': stats[:, 0], 'rms': rms(stats[:, 0], stats[:, 1])}
    if stats.shape[1] == 5:
        info.update(color_counts=stats[:, 3], color_rms=rms(stats[:, 3], stats[:, 4]))
    return info


def icp_sums(depth, K, wxyz, t, model_vertex, model_normal, model_K, model_wxyz, model_t, max_dist=0.1, depth_scale=1.0, max_depth=10, *, color=None,
             model_intensity=None, color_weight=None):
    """The 29 sums of one point-to-plane linearisation, for callers who bring their own solver: the 21 products J_a J_b (a <= b), the
    6 products J_a r, r r and the pair count, over the pixels of the depth frame ``depth`` [h, w] (uint16, float32 or float64) at the
    camera->world pose (``wxyz``, ``t``, intrinsics ``K``) that find a model point within ``max_dist``.  The model is a pair of maps
    ``model_vertex``, ``model_normal`` [hm, wm, 3] in the world frame (NaN = missing; what ``raycast`` returns) seen by the camera
    (``model_K``, ``model_wxyz``, ``model_t``).  -> float64 [29]; a device tensor when any of the arrays is one.

    With the frame's colour image ``color`` (uint8 [hc, wc, 3] of any size), the model's intensity map ``model_intensity`` (float64
    [hm, wm], NaN = missing; ``raycast(..., colors=True)``'s) and ``color_weight`` (all three or none; the weight is not read here)
    -> float64 [58]: the 29 sums above, then the same 29 of the photometric pairs (Jc, rc)."""
    depth, code, K, q, t, model_vertex, model_normal, hm, wm, view, max_dist, depth_scale, max_depth = _icp_args(
        depth, K, wxyz, t, model_vertex, model_normal, model_K, model_wxyz, model_t, max_dist, depth_scale, max_depth)
    col = _color_args(color, model_intensity, color_weight, hm, wm)
    ctx = f3d.default_context()
    if not (on_device(depth) or on_device(model_vertex) or on_device(model_normal) or (col is not None and (on_device(col[0]) or on_device(col[1])))):
        if col is not None:
            return ctx.icp_color_sums(depth, K, q, t, model_vertex, model_normal, hm, wm, view, max_dist, col[1], col[0], col[2], depth_scale, max_depth)
        return ctx.icp_sums(depth, K, q, t, model_vertex, model_normal, hm, wm, view, max_dist, depth_scale, max_depth)
    torch, dev = torch_device(ctx, 'icp_sums')
    h, w = (int(x) for x in depth.shape)
    with torch.cuda.device(dev), work_stream(dev) as work:
        d, mv, mn, dview = _to_device(torch, dev, depth, model_vertex, model_normal, view)
        used = [d, mv, mn, dview]
        if col is None:
            sums = torch.empty(f3d.ICP_NSUMS, dtype=torch.float64, device=dev)
            ctx.icp_sums_dev(d.data_ptr(), code, h, w, K, q, t, mv.data_ptr(), mn.data_ptr(), hm, wm, dview.data_ptr(), max_dist, depth_scale, max_depth,
                             sums.data_ptr(), work.cuda_stream)
        else:
            rgb, mi = _color_to_device(torch, dev, col[0], col[1])
            used += [rgb, mi]
            sums = torch.empty(f3d.ICP_NSUMS_COLOR, dtype=torch.float64, device=dev)
            ctx.icp_color_sums_dev(d.data_ptr(), code, h, w, K, q, t, mv.data_ptr(), mn.data_ptr(), hm, wm, dview.data_ptr(), max_dist, mi.data_ptr(),
                                   rgb.data_ptr(), int(rgb.shape[0]), int(rgb.shape[1]), col[2], depth_scale, max_depth, sums.data_ptr(),
                                   work.cuda_stream)
    for x in used + [sums]:
        x.record_stream(torch.cuda.current_stream(dev))
    return sums


def _maps_to_device(torch, dev, depth, model_vertex, model_normal):
    as_tensor = lambda a: a if on_device(a) else torch.from_numpy(np.ascontiguousarray(a))     # noqa: E731
    d = as_tensor(depth).to(dev).contiguous()
    mv, mn = (as_tensor(a).to(dev, torch.float64).contiguous() for a in (model_vertex, model_normal))
    return d, mv, mn


def _to_device(torch, dev, depth, model_vertex, model_normal, view):
    return _maps_to_device(torch, dev, depth, model_vertex, model_normal) + (upload(view, dev),)


def _icp_device(ctx, torch, dev, work, d, code, K, q, t, mv, mn, hm, wm, dview, max_dist, depth_scale, max_depth, iterations, min_pairs):
    """Enqueues the rounds on `work` -> (pose [7], stats [iterations, 3], status [1]) on the device."""
    pose = torch.empty(7, dtype=torch.float64, device=dev)
    stats = torch.empty((iterations, 3), dtype=torch.float64, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    ctx.icp_dev(d.data_ptr(), code, int(d.shape[0]), int(d.shape[1]), K, q, t, mv.data_ptr(), mn.data_ptr(), hm, wm, dview.data_ptr(), max_dist,
                depth_scale, max_depth, iterations, min_pairs, pose.data_ptr(), stats.data_ptr(), status.data_ptr(), work.cuda_stream)
    return pose, stats, status


def _icp_color_device(ctx, torch, dev, work, d, code, K, q, t, mv, mn, hm, wm, dview, max_dist, mi, rgb, color_weight, depth_scale, max_depth, iterations,
                      min_pairs):
    """_icp_device with the photometric term: mi the model's intensity map, rgb the frame's colour image [hc, wc, 3], both on the device
    -> (pose [7], stats [iterations, 5], status [1])."""
    pose = torch.empty(7, dtype=torch.float64, device=dev)
    stats = torch.empty((iterations, 5), dtype=torch.float64, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    ctx.icp_color_dev(d.data_ptr(), code, int(d.shape[0]), int(d.shape[1]), K, q, t, mv.data_ptr(), mn.data_ptr(), hm, wm, dview.data_ptr(), max_dist,
                      mi.data_ptr(), rgb.data_ptr(), int(rgb.shape[0]), int(rgb.shape[1]), color_weight, depth_scale, max_depth, iterations, min_pairs,
                      pose.data_ptr(), stats.data_ptr(), status.data_ptr(), work.cuda_stream)
    return pose, stats, status


def _levels_plan(levels, level_iterations, gate, iterations, min_pairs, max_dist, shapes):
    """The coarse-to-fine arguments of icp / track_frames, checked before any device call.  None for the single call of today
    (``levels=1`` with the other two ``None``); else (levels, rounds per level finest first, gate, min_pairs per level finest first).
    ``shapes``: (rows, columns) of the frame and of the model image, each of which must survive ``levels - 1`` halvings."""
    levels = int(levels)
    if not 1 <= levels <= f3d.ICP_MAX_LEVELS:
        raise ValueError(f'levels must be in [1, {f3d.ICP_MAX_LEVELS}], got {levels}')
    if levels == 1 and level_iterations is None and gate is None:
        return None
    if level_iterations is None:
        rounds = (iterations,) + (max(1, iterations // 2),) * (levels - 1)
    else:
        rounds = tuple(int(x) for x in level_iterations)
        if len(rounds) != levels or min(rounds) < 1:
            raise ValueError(f'level_iterations must hold {levels} counts of at least 1, finest level first, got {tuple(level_iterations)}')
    gate = _positive('gate', max_dist if gate is None else gate)
    for rows, cols in shapes:
        if min(int(rows), int(cols)) < 1 << (levels - 1):
            raise ValueError(f'{levels} levels need at least {1 << (levels - 1)} rows and columns, got {(int(rows), int(cols))}')
    return levels, rounds, gate, tuple(max(6, min_pairs >> (2 * l)) for l in range(levels))


def _half_K(K):
    """The intrinsics of a half-sampled image: input coordinate x is output coordinate x / 2 (f3d.h), so the first two rows halve."""
    K = np.array(K, np.float64)
    K[:2] /= 2.0
    return K


def _level_cameras(plan, K, hw, mK, mhw, mq, mt, max_depth):
    """Per level, finest first: (K, (h, w), model K, (hm, wm), the model's views_build record)."""
    out = []
    for _ in range(plan[0]):
        out.append((K, hw, mK, mhw, f3d.views_build(mK, mhw[1], mhw[0], mq[None], mt[None], max_depth)))
        K, mK, hw, mhw = _half_K(K), _half_K(mK), (hw[0] // 2, hw[1] // 2), (mhw[0] // 2, mhw[1] // 2)
    return out


def _icp_levels_host(ctx, plan, depth, K, q, t, mv, mn, mi, hm, wm, mK, mq, mt, max_dist, depth_scale, max_depth, rgb, color_weight):
    """The half-samplings and the levelled rounds through the host bindings -> (pose, stats, status) of ``Context.icp_levels``."""
    _, rounds, gate, pairs = plan
    recs = []
    for l, (K_l, _, _, (hm_l, wm_l), view) in enumerate(_level_cameras(plan, K, depth.shape, mK, (hm, wm), mq, mt, max_depth)):
        if l:
            p = recs[-1]
            depth, depth_scale = ctx.depth_half(p['depth'], p['depth_scale'], max_depth, gate), 1.0
            maps = ctx.maps_half(p['model_vertex'], p['model_normal'], p['hm'], p['wm'], p['model_view'], gate, p['model_intensity'])
            mv, mn, mi = maps if mi is not None else maps + (None,)
        recs.append(dict(depth=depth, K=K_l, depth_scale=depth_scale, model_vertex=mv, model_normal=mn, model_intensity=mi, hm=hm_l, wm=wm_l,
                         model_view=view, max_dist=max_dist, iterations=rounds[l], min_pairs=pairs[l]))
    return ctx.icp_levels(recs[::-1], q, t, max_depth, rgb, color_weight)


def _icp_levels_device(ctx, torch, dev, work, plan, d, code, K, q, t, mv, mn, mi, hm, wm, mK, mq, mt, max_dist, depth_scale, max_depth, rgb,
                       color_weight):
    """Enqueues the half-samplings and the levelled rounds on `work`, all inputs on the device -> (pose [7], stats [rounds, 3 or 5],
    status [1], the tensors the launches read).  One upload (every level's view record), no host synchronisation."""
    from f3d import levels as LV
    _, rounds, gate, pairs = plan
    cams = _level_cameras(plan, K, tuple(int(x) for x in d.shape), mK, (hm, wm), mq, mt, max_depth)
    dviews = upload(np.stack([np.asarray(c[4]).reshape(-1) for c in cams]), dev)
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)                    # noqa: E731
    ptr = lambda x: None if x is None else x.data_ptr()                                       # noqa: E731
    keep, recs = [dviews], []
    for l, (K_l, (h_l, w_l), _, (hm_l, wm_l), _) in enumerate(cams):
        if l:
            p = recs[-1]
            d, code, depth_scale = f64(h_l * w_l), 0, 1.0
            LV.depth_half_dev(ctx, p['depth'], p['depth_type'], p['h'], p['w'], p['depth_scale'], max_depth, gate, d.data_ptr(), work.cuda_stream)
            mv, mn, mi = f64(hm_l * wm_l, 3), f64(hm_l * wm_l, 3), None if mi is None else f64(hm_l * wm_l)
            LV.maps_half_dev(ctx, p['model_vertex'], p['model_normal'], p['model_intensity'], p['hm'], p['wm'], p['model_view'], gate, mv.data_ptr(),
                             mn.data_ptr(), ptr(mi), work.cuda_stream)
            keep += [x for x in (d, mv, mn, mi) if x is not None]
        recs.append(dict(depth=d.data_ptr(), depth_type=code, h=h_l, w=w_l, K=K_l, depth_scale=depth_scale, model_vertex=mv.data_ptr(),
                         model_normal=mn.data_ptr(), model_intensity=ptr(mi), hm=hm_l, wm=wm_l, model_view=dviews[l].data_ptr(), max_dist=max_dist,
                         iterations=rounds[l], min_pairs=pairs[l]))
    pose, stats = f64(7), f64(sum(rounds), 3 if rgb is None else 5)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    hc, wc = (0, 0) if rgb is None else (int(rgb.shape[0]), int(rgb.shape[1]))
    LV.icp_levels_dev(ctx, recs[::-1], q, t, max_depth, pose.data_ptr(), stats.data_ptr(), status.data_ptr(), ptr(rgb), hc, wc, color_weight,
                      work.cuda_stream)
    return pose, stats, status, keep


def icp(depth, K, wxyz, t, model_vertex, model_normal, model_K, model_wxyz, model_t, max_dist=0.1, depth_scale=1.0, max_depth=10, iterations=10,
        min_pairs=100, *, color=None, model_intensity=None, color_weight=None, levels=1, level_iterations=None, gate=None):
    """``iterations`` rounds of projective point-to-plane ICP of the depth frame against the model maps (the arguments of ``icp_sums``),
    starting from the pose (``wxyz``, ``t``), all on the device with no host round trip between the rounds -> (wxyz [4], t [3], info).
    ``info`` holds the final ``status`` (0 = converging, 1 = lost: fewer than ``min_pairs`` pairs or a degenerate system; the pose of a
    lost call is the one its lost round started from) and ``counts`` and ``rms`` per round, measured before that round's update.

    With ``color``, ``model_intensity`` and ``color_weight`` (the colour arguments of ``icp_sums``; all three or none) every round
    solves ``A_g + color_weight A_c`` against ``-(b_g + color_weight b_c)``: the intensity residual holds what the geometry lets
    slide.  Intensities are in [0, 1] and distances in metres, so the weight is a squared length: a residual of 1/255 counts as much as
    one of sqrt(color_weight) / 255 metres.  ``info`` then also holds ``color_counts`` and ``color_rms`` per round; whether a round is
    lost is decided by the geometric pairs alone.

    ``levels`` > 1 runs coarse to fine: the frame and the model maps (with the intensity map) are half-sampled ``levels - 1`` times by
    2 x 2 averages that keep to the nearest surface within ``gate`` metres (default ``max_dist``), and the rounds run from the coarsest
    level to the full resolution in one chain on the device.  A surface with structure near the pixel scale (bricks, slats, shelves)
    otherwise pulls a start a few centimetres off into the neighbouring period of that structure, with status 0.
    ``level_iterations``: the rounds per level, finest first (default ``iterations`` at full resolution and half of it, at least 1, on
    every coarser level); level l runs with ``max(6, min_pairs >> 2 l)``.  ``info``'s per-round arrays then hold every level's rounds in
    running order, coarsest first, and ``level_rounds`` the rounds per level in that order.  The colour image is not half-sampled: a
    coarse pixel reads the full image by the pixel rule."""
    depth, code, K, q, t, model_vertex, model_normal, hm, wm, view, max_dist, depth_scale, max_depth = _icp_args(
        depth, K, wxyz, t, model_vertex, model_normal, model_K, model_wxyz, model_t, max_dist, depth_scale, max_depth)
    col = _color_args(color, model_intensity, color_weight, hm, wm)
    iterations, min_pairs = _rounds(iterations, min_pairs)
    plan = _levels_plan(levels, level_iterations, gate, iterations, min_pairs, max_dist, (depth.shape, (hm, wm)))
    ctx = f3d.default_context()
    device = on_device(depth) or on_device(model_vertex) or on_device(model_normal) or (col is not None and (on_device(col[0]) or on_device(col[1])))
    if plan is not None:
        mK, mq, mt = _pose(model_K, model_wxyz, model_t, 'model_')
        rgb, mi, weight = (None, None, None) if col is None else col
        if not device:
            pose, stats, status = _icp_levels_host(ctx, plan, depth, K, q, t, model_vertex, model_normal, mi, hm, wm, mK, mq, mt, max_dist, depth_scale,
                                                   max_depth, rgb, weight)
            return pose[:4].copy(), pose[4:].copy(), dict(_info(stats, status), level_rounds=plan[1][::-1])
        torch, dev = torch_device(ctx, 'icp')
        with torch.cuda.device(dev), work_stream(dev) as work:
            d, mv, mn = _maps_to_device(torch, dev, depth, model_vertex, model_normal)
            used = [d, mv, mn]
            if col is not None:
                rgb, mi = _color_to_device(torch, dev, rgb, mi)
                used += [rgb, mi]
            pose, stats, status, keep = _icp_levels_device(ctx, torch, dev, work, plan, d, code, K, q, t, mv, mn, mi, hm, wm, mK, mq, mt, max_dist,
                                                           depth_scale, max_depth, rgb, weight)
        for x in used + keep + [pose, stats, status]:
            x.record_stream(torch.cuda.current_stream(dev))
        return pose[:4].clone(), pose[4:].clone(), dict(_info(stats, status[0], torch), level_rounds=plan[1][::-1])
    if not device:
        if col is not None:
            pose, stats, status = ctx.icp_color(depth, K, q, t, model_vertex, model_normal, hm, wm, view, max_dist, col[1], col[0], col[2], depth_scale,
                                                max_depth, iterations, min_pairs)
        else:
            pose, stats, status = ctx.icp(depth, K, q, t, model_vertex, model_normal, hm, wm, view, max_dist, depth_scale, max_depth, iterations,
                                          min_pairs)
        return pose[:4].copy(), pose[4:].copy(), _info(stats, status)
    torch, dev = torch_device(ctx, 'icp')
    with torch.cuda.device(dev), work_stream(dev) as work:
        d, mv, mn, dview = _to_device(torch, dev, depth, model_vertex, model_normal, view)
        used = [d, mv, mn, dview]
        if col is None:
            pose, stats, status = _icp_device(ctx, torch, dev, work, d, code, K, q, t, mv, mn, hm, wm, dview, max_dist, depth_scale, max_depth,
                                              iterations, min_pairs)
        else:
            rgb, mi = _color_to_device(torch, dev, col[0], col[1])
            used += [rgb, mi]
            pose, stats, status = _icp_color_device(ctx, torch, dev, work, d, code, K, q, t, mv, mn, hm, wm, dview, max_dist, mi, rgb, col[2],
                                                    depth_scale, max_depth, iterations, min_pairs)
    for x in used + [pose, stats, status]:
        x.record_stream(torch.cuda.current_stream(dev))
    return pose[:4].clone(), pose[4:].clone(), _info(stats, status[0], torch)


def track_frames(volume, depths, K, wxyzs, translations, depth_scale=1.0, max_depth=10, max_dist=0.1, iterations=10, min_pairs=100, min_weight=1,
                 integrate=True, colors=None, color_weight=None, levels=1, level_iterations=None, gate=None):
    """Frame-to-model tracking of the depth frames ``depths`` [F, h, w] into ``volume`` (a ``TSDFVolume``), in frame order.  A frame
    that meets a volume with no weight is integrated at its given pose.  Every later frame is ray-cast at its given pose, the prior
    (samples every voxel edge up to ``max_depth``), aligned to those maps by ``icp`` starting from the prior, takes the refined pose if
    the status is 0 and the prior otherwise, and is integrated at the pose taken (``integrate=False``: only frames that meet an empty
    volume are integrated).  -> (wxyzs [F, 4], translations [F, 3], status int32 [F]); NumPy arrays, or device tensors when the depths
    or the volume are on the device.  ``colors``: the frames' colour images, uint8 [F, hc, wc, 3], for a volume built with
    ``color=True``; each frame that is integrated hands its image to ``integrate``.  ``color_weight`` (with ``colors``): every aligned
    frame is ray-cast with the volume's colour and aligned by ``icp`` with the photometric term at that weight, against the intensity
    of the model as built so far; ``None`` keeps the alignment depth-only.  ``levels``, ``level_iterations``, ``gate``: every aligned
    frame runs ``icp``'s coarse-to-fine rounds, its pyramids built from the frame and from the maps ray-cast at full resolution.

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
    plan = _levels_plan(levels, level_iterations, gate, iterations, min_pairs, max_dist, ((h, w),))
    min_weight = _min_weight(min_weight)
    near, step, nsteps = _march(volume, 0.0, max_depth, None)
    out_q, out_t, status = qs.copy(), ts.copy(), np.zeros(F, np.int32)
    if colors is not None:
        colors = volume._color_images(colors, F)
    if color_weight is not None:
        if colors is None:
            raise ValueError('color_weight needs the colour images (colors=...)')
        color_weight = float(color_weight)
        if not (color_weight >= 0.0 and color_weight < math.inf):
            raise ValueError(f'color_weight must be finite and not negative, got {color_weight}')
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
                if color_weight is None:
                    vertex, normal, _ = ctx.tsdf_raycast(volume.tsdf, volume.weight, volume.lo, volume.voxel, min_weight, K, q, t, h, w, near, step,
                                                         nsteps)
                    intensity = None
                else:
                    vertex, normal, _, _, intensity = ctx.tsdf_raycast_color(volume.tsdf, volume.weight, volume.color, volume.lo, volume.voxel,
                                                                             min_weight, K, q, t, h, w, near, step, nsteps)
                if plan is not None:
                    pose, _, status[f] = _icp_levels_host(ctx, plan, depths[f], K, q, t, vertex, normal, intensity, h, w, K, q, t, max_dist, depth_scale,
                                                          max_depth, None if color_weight is None else colors[f], color_weight)
                elif color_weight is None:
                    pose, _, status[f] = ctx.icp(depths[f], K, q, t, vertex, normal, h, w, view, max_dist, depth_scale, max_depth, iterations, min_pairs)
                else:
                    pose, _, status[f] = ctx.icp_color(depths[f], K, q, t, vertex, normal, h, w, view, max_dist, intensity, colors[f], color_weight,
                                                       depth_scale, max_depth, iterations, min_pairs)
                if status[f] == 0:
                    out_q[f], out_t[f] = pose[:4], pose[4:]
            if empty or integrate:
                volume.integrate(depths[f:f + 1], K, out_q[f:f + 1], out_t[f:f + 1], depth_scale, max_depth,
                                 colors=None if colors is None else colors[f:f + 1])
        return out_q, out_t, status
    torch, dev = torch_device(ctx, 'track_frames')
    volume._to_device()
    d_all = (depths if on_device(depths) else torch.from_numpy(np.ascontiguousarray(depths))).to(dev).contiguous()
    if color_weight is not None:
        rgb_all = (colors if on_device(colors) else torch.from_numpy(np.ascontiguousarray(colors))).to(dev).contiguous()
    for f in range(F):
        _, q, t = poses[f]
        empty = empty and not bool(volume.weight.any())
        if not empty:
            view = f3d.views_build(K, w, h, q[None], t[None], max_depth)
            with torch.cuda.device(dev), work_stream(dev) as work:
                vertex, normal = (torch.empty((h * w, 3), dtype=torch.float64, device=dev) for _ in range(2))
                used = [vertex, normal]
                if plan is None:
                    dview = upload(view, dev)
                    used.append(dview)
                if color_weight is None:
                    ctx.tsdf_raycast_dev(volume.tsdf.data_ptr(), volume.weight.data_ptr(), volume.dims, volume.lo, volume.voxel, min_weight, K, q, t, h,
                                         w, near, step, nsteps, vertex.data_ptr(), normal.data_ptr(), None, work.cuda_stream)
                    if plan is None:
                        pose, stats, lost = _icp_device(ctx, torch, dev, work, d_all[f], code, K, q, t, vertex, normal, h, w, dview, max_dist,
                                                        depth_scale, max_depth, iterations, min_pairs)
                    else:
                        pose, stats, lost, keep = _icp_levels_device(ctx, torch, dev, work, plan, d_all[f], code, K, q, t, vertex, normal, None, h, w,
                                                                     K, q, t, max_dist, depth_scale, max_depth, None, None)
                        used += keep
                    back = torch.cat([pose, lost.to(torch.float64)])
                else:
                    intensity = torch.empty(h * w, dtype=torch.float64, device=dev)
                    used.append(intensity)
                    ctx.tsdf_raycast_color_dev(volume.tsdf.data_ptr(), volume.weight.data_ptr(), volume.color.data_ptr(), volume.dims, volume.lo,
                                               volume.voxel, min_weight, K, q, t, h, w, near, step, nsteps, vertex.data_ptr(), normal.data_ptr(), None,
                                               None, intensity.data_ptr(), work.cuda_stream)
                    if plan is None:
                        pose, stats, lost = _icp_color_device(ctx, torch, dev, work, d_all[f], code, K, q, t, vertex, normal, h, w, dview, max_dist,
                                                              intensity, rgb_all[f], color_weight, depth_scale, max_depth, iterations, min_pairs)
                    else:
                        pose, stats, lost, keep = _icp_levels_device(ctx, torch, dev, work, plan, d_all[f], code, K, q, t, vertex, normal, intensity, h,
                                                                     w, K, q, t, max_dist, depth_scale, max_depth, rgb_all[f], color_weight)
                        used += keep
                    back = torch.cat([pose, lost.to(torch.float64), stats[-1, 3:]])          # the two colour columns ride along
            for x in used + [pose, stats, lost]:
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
