"""Device-pointer bindings of cloud-to-cloud ICP (f3d.h f3d_cloud_icp_sums_dev, f3d_cloud_icp_dev) and their torch-tensor hand-off.

The host bindings are ``Context.cloud_icp_sums`` and ``Context.cloud_icp``.  Their device-pointer twins are functions of this module
that take the context first, not ``Context.*_dev`` methods, for the reason f3d/levels.py gives: tests/test_route_cases_cpu.py checks
every such method against the table in tests/route_cases.py, and moving these two onto ``Context`` together with their table rows is a
follow-up of its own.  Until then tests/test_cloud_icp_gpu.py carries their stalled-stream and strided-input cases itself.

``register_tensors`` is the hand-off ``Fusion3DSeg.segUtils.alignment`` uses for device tensors: the device, the stream, the dtype codes,
the contiguous copies, the centring of the source and the readbacks of the pose are all here, with f3d.tensors' helpers.

Raw pointers in (``tensor.data_ptr()``); but for the one readback of a call's prepare step (the target's box, the source's non-finite
flag), nothing here synchronises with the host.
"""
import numpy as np

from f3d import CLOUD_ICP_PLANE, _cloud_icp_check, _ptr, _quat_matrix
from f3d.tensors import device_points, dtype_code, torch_device, upload, work_stream

__all__ = ['cloud_icp_sums_dev', 'cloud_icp_dev', 'register_tensors']


def _sizes(n, m):
    n, m = int(n), int(m)
    if not (0 <= n < 2 ** 31 and 0 < m < 2 ** 31):
        raise ValueError(f'n must be in [0, 2^31) and m in [1, 2^31), got {n} and {m}')
    return n, m


def cloud_icp_sums_dev(ctx, source_ptr, source_dtype, n, target_ptr, target_dtype, m, normals_ptr, mode, q_wxyz, t, max_dist, sums_ptr,
                       pairs_ptr=None, stream=None):
    """The 29 sums of one linearisation of cloud-to-cloud ICP on the device: source [n, 3] and target [m, 3] of their dtype codes,
    normals float64 [m, 3] (None in point mode), q_wxyz and t on the host; sums float64 [29], pairs int32 [n] (may be None)."""
    mode, q, t, max_dist = _cloud_icp_check(mode, normals_ptr is not None, q_wxyz, t, max_dist)
    n, m = _sizes(n, m)
    ctx._check(ctx._lib.f3d_cloud_icp_sums_dev(ctx._h, source_ptr, int(source_dtype), n, target_ptr, int(target_dtype), m, normals_ptr, mode, _ptr(q),
                                               _ptr(t), max_dist, sums_ptr, pairs_ptr, stream))


def cloud_icp_dev(ctx, source_ptr, source_dtype, n, target_ptr, target_dtype, m, normals_ptr, mode, q_wxyz, t, max_dist, iterations, min_pairs,
                  pose_ptr, stats_ptr, status_ptr=None, stream=None):
    """`iterations` rounds of cloud-to-cloud ICP on the device, the target's grid built once and no host round trip between the rounds:
    pose float64 [7], stats float64 [iterations, 3], status int32 [1] (may be None)."""
    mode, q, t, max_dist = _cloud_icp_check(mode, normals_ptr is not None, q_wxyz, t, max_dist, iterations, min_pairs)
    n, m = _sizes(n, m)
    ctx._check(ctx._lib.f3d_cloud_icp_dev(ctx._h, source_ptr, int(source_dtype), n, target_ptr, int(target_dtype), m, normals_ptr, mode, _ptr(q),
                                          _ptr(t), max_dist, int(iterations), int(min_pairs), pose_ptr, stats_ptr, status_ptr, stream))


def register_tensors(ctx, source, target, target_normals, mode, q_wxyz, t, max_dists, iterations, min_pairs, center=False):
    """``alignment.register_clouds`` for torch tensors: stage k is one cloud_icp_dev call with max_dists[k] and iterations[k], started
    from the pose the stage before left (read back between the stages: q and t are host arguments).  The tensors are moved to the
    context's device; float32 clouds stay float32, everything else is widened to float64, views are made contiguous.  ``center``: the
    source's mean c is subtracted (in float64) before the stages, the start becomes t + R c and the result t - R' c.
    -> (wxyz float64 [4], t float64 [3], stats float64 [sum of iterations, 3], status int32 [stages]) as tensors on that device, and
    the stats once more as a NumPy array (the pose has been read back by then, so this costs no further wait)."""
    torch, dev = torch_device(ctx, 'register_clouds')
    if len(max_dists) != len(iterations) or not max_dists:
        raise ValueError('max_dist and iterations must name the same stages, at least one')
    for r, it in zip(max_dists, iterations):
        _cloud_icp_check(mode, target_normals is not None, q_wxyz, t, r, it, min_pairs)
    with torch.cuda.device(dev), work_stream(dev) as work:
        s, g = device_points(source, dev, 'source'), device_points(target, dev, 'target')
        nrm = None
        if mode == CLOUD_ICP_PLANE:
            nrm = torch.as_tensor(target_normals).to(dev).to(torch.float64).contiguous()
            if tuple(nrm.shape) != tuple(g.shape):
                raise ValueError(f'the normals must be {tuple(g.shape)} like the target, got {tuple(nrm.shape)}')
        if len(g) == 0:
            raise ValueError('the target is empty')
        c = np.zeros(3)
        if center and len(s):
            s = s.to(torch.float64)                                        # (contiguous: a view and its copy reduce in the same order)
            mean = s.mean(dim=0)
            s = s - mean
            c = mean.cpu().numpy()
        pose = torch.empty(7, dtype=torch.float64, device=dev)
        stats = torch.empty((int(sum(iterations)), 3), dtype=torch.float64, device=dev)
        status = torch.empty(len(max_dists), dtype=torch.int32, device=dev)
        q = np.asarray(q_wxyz, np.float64).reshape(4)
        tr = np.asarray(t, np.float64).reshape(3) + _quat_matrix(q) @ c
        row = 0
        for k, (r, it) in enumerate(zip(max_dists, iterations)):
            if k:
                host = pose.cpu().numpy()
                q, tr = host[:4], host[4:]
            cloud_icp_dev(ctx, s.data_ptr(), dtype_code(s), len(s), g.data_ptr(), dtype_code(g), len(g), None if nrm is None else nrm.data_ptr(),
                          mode, q, tr, r, it, min_pairs, pose.data_ptr(), stats[row:].data_ptr(), status[k:].data_ptr(), work.cuda_stream)
            row += int(it)
        host = pose.cpu().numpy()
        out_t = upload(host[4:] - _quat_matrix(host[:4]) @ c, dev)
        return pose[:4].clone(), out_t, stats, status, stats.cpu().numpy()
