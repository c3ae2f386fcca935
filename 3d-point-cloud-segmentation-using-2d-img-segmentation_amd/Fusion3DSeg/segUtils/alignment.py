"""Bring one point set into the frame of another, on the GPU (no reference counterpart).

``transfer.transfer_labels``, ``clean_mesh_by_points``, ``vertex_mask_from_points`` and ``door_window_bbox.generate_mesh`` all assume
that their two point sets share a frame.  A second capture session, an export written in another world frame, a CAD or PolyFit model
or two TSDF meshes of one room do not; ``registration`` aligns a depth frame to model maps through a camera and cannot pair two
unordered clouds.  ``register_clouds`` can: cloud-to-cloud ICP of libf3d_hip (f3d.h ``f3d_cloud_icp``), which builds the target's
radius grid once per call and runs every round on the device, the nearest-point search fused with the sums.

The pose ``(wxyz, t)`` maps source coordinates into the target's frame: ``transform_points(source, wxyz, t)`` lies on the target.
``method='plane'`` (point-to-plane) needs the target's normals, from ``extract_planes(..., normals_out)``, ``Fusion.fuse`` or a mesh;
``method='point'`` needs none and converges more slowly along flat surfaces.

NumPy arrays in give NumPy arrays out (host-pointer entries).  If the source, the target or the normals is a device tensor, the call
goes through ``f3d.clouds.register_tensors``, which owns the whole hand-off (device, stream, dtypes, centring, readbacks): this module
only recognises a device tensor by its ``is_cuda`` attribute.  The pose and the stats then come out as device tensors, which every
function here takes back as a pose.  ICP is local: the start pose must be within ``max_dist`` of the truth at most points.  No CPU fallback.
"""
import numpy as np

import f3d
from f3d import clouds

__all__ = ['register_clouds', 'evaluate_registration', 'transform_points']

_MODES = {'plane': f3d.CLOUD_ICP_PLANE, 'point': f3d.CLOUD_ICP_POINT}


def _device(*arrays):
    """The device of the first device tensor among `arrays`, or None (the NumPy route)."""
    for a in arrays:
        if getattr(a, 'is_cuda', False):
            return a.device
    return None


def _host_points(a, name):
    p = np.asarray(a.cpu() if hasattr(a, 'cpu') else a)
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError(f'{name} must be [N, 3], got {p.shape}')
    if p.dtype != np.float32:
        p = p.astype(np.float64)
    return np.ascontiguousarray(p)


def _host_vector(x, size):
    """A pose argument (a sequence, a NumPy array or a tensor on any device, as the device route returns them) as float64 [size]."""
    return np.asarray(x.cpu() if hasattr(x, 'cpu') else x, np.float64).reshape(size)


def _stages(max_dist, iterations):
    """(max_dists, iterations) of the stages, coarse to fine: either argument may be one number for all of them."""
    dists = [float(r) for r in np.atleast_1d(np.asarray(max_dist, np.float64))]
    its = [int(i) for i in np.atleast_1d(np.asarray(iterations))]
    if len(dists) == 1:
        dists = dists * len(its)
    if len(its) == 1:
        its = its * len(dists)
    if len(dists) != len(its) or not dists:
        raise ValueError(f'max_dist names {len(dists)} stages and iterations {len(its)}')
    return dists, its


def transform_points(points, wxyz, t):
    """``points`` [N, 3] under the pose: rotate by ``wxyz``, then add ``t`` -> float64 [N, 3], a NumPy array or a tensor as given.
    The pose may be sequences, NumPy arrays or tensors (what ``register_clouds`` returned on either route)."""
    R, t = f3d._quat_matrix(_host_vector(wxyz, 4)), _host_vector(t, 3)
    if hasattr(points, 'is_cuda'):
        import torch
        if points.dim() != 2 or points.shape[1] != 3:
            raise ValueError(f'points must be [N, 3], got {tuple(points.shape)}')
        p = points.to(torch.float64)
        return p @ torch.from_numpy(R.T.copy()).to(p.device) + torch.from_numpy(t).to(p.device)
    p = np.asarray(points, np.float64)
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError(f'points must be [N, 3], got {p.shape}')
    return p @ R.T + t


def register_clouds(source, target, target_normals=None, max_dist=0.1, wxyz=(1, 0, 0, 0), t=(0, 0, 0), iterations=30, min_pairs=100,
                    method='plane', center=True):
    """ICP of ``source`` [n, 3] onto ``target`` [m, 3] from the start pose ``(wxyz, t)`` -> (wxyz float64 [4], t float64 [3], info).

    ``max_dist`` and ``iterations`` may be sequences, coarse to fine: each stage is one library call that starts from the pose the
    stage before left.  ``center``: the increment of a round rotates about ``t``, so the mean of the source is subtracted before the
    calls and folded back into ``t`` after them, which keeps the system well conditioned for a cloud far from its origin.  The start
    pose may be sequences, NumPy arrays or tensors, so a result of either route can be fed back.  ``info``:
    ``count`` (pairs of the last round that ran), ``rmse`` (sqrt of their mean squared residual: along the normal for 'plane', the
    distance for 'point'), ``fitness`` = count / n, ``status`` (``f3d.ICP_LOST`` if any stage was lost: too few pairs, or a geometry that
    does not fix all six degrees of freedom) and ``stats`` [rounds, 3] = count, sum r^2, status per round."""
    if method not in _MODES:
        raise ValueError(f"method must be 'plane' or 'point', got {method!r}")
    mode = _MODES[method]
    if mode == f3d.CLOUD_ICP_PLANE and target_normals is None:
        raise ValueError("method='plane' needs target_normals (extract_planes(..., normals_out), Fusion.fuse, or a mesh); use method='point' without")
    dists, its = _stages(max_dist, iterations)
    q0, t0 = _host_vector(wxyz, 4), _host_vector(t, 3)
    for r, it in zip(dists, its):
        f3d._cloud_icp_check(mode, target_normals is not None, q0, t0, r, it, min_pairs)
    dev = _device(source, target, target_normals)
    if dev is not None:                                                 # tensors: device, stream, centring and readbacks are f3d.clouds'
        q, tr, stats, status, host_stats = clouds.register_tensors(f3d.default_context(dev.index), source, target, target_normals, mode, q0, t0,
                                                                   dists, its, min_pairs, center)
        return q, tr, _info(host_stats, int(host_stats[:, 2].max()), len(source), stats)
    src, tgt = _host_points(source, 'source'), _host_points(target, 'target')
    n = len(src)
    c = src.astype(np.float64).mean(axis=0) if center and n else np.zeros(3)
    if center:
        src = src.astype(np.float64) - c
    ctx = f3d.default_context()
    q, tr = q0, t0 + f3d._quat_matrix(q0) @ c
    rows, lost = [], f3d.ICP_OK
    for r, it in zip(dists, its):
        pose, stats, status = ctx.cloud_icp(src, tgt, target_normals, mode, q, tr, r, it, min_pairs)
        q, tr = pose[:4], pose[4:]
        rows.append(stats)
        lost = max(lost, status)
    tr = tr - f3d._quat_matrix(q) @ c
    return q.copy(), tr, _info(np.concatenate(rows), lost, n)


def _info(stats, status, n, stats_out=None):
    ran = stats[stats[:, 0] > 0]
    count, sum_r2 = (float(ran[-1, 0]), float(ran[-1, 1])) if len(ran) else (0.0, 0.0)
    return dict(count=int(count), rmse=float(np.sqrt(sum_r2 / count)) if count else float('nan'), fitness=count / n if n else 0.0,
                status=int(status), stats=stats if stats_out is None else stats_out)


def evaluate_registration(source, target, max_dist, wxyz, t):
    """How well ``source`` under the pose lies on ``target`` (Open3D's evaluate_registration): one point-mode linearisation
    (f3d.h ``f3d_cloud_icp_sums``) -> dict(fitness = count / n, inlier_rmse = sqrt(mean squared distance of the pairs), count, pairs int32
    [n]: the nearest target of every source point within ``max_dist`` or -1).  A host-pointer call: device tensors (the clouds and the
    pose alike) are copied to the host, the result is NumPy."""
    src, tgt = _host_points(source, 'source'), _host_points(target, 'target')
    sums, pairs = f3d.default_context().cloud_icp_sums(src, tgt, None, f3d.CLOUD_ICP_POINT, _host_vector(wxyz, 4), _host_vector(t, 3), max_dist, pairs=True)
    count, n = float(sums[28]), len(src)
    return dict(fitness=count / n if n else 0.0, inlier_rmse=float(np.sqrt(sums[27] / count)) if count else float('nan'), count=int(count),
                pairs=pairs)
