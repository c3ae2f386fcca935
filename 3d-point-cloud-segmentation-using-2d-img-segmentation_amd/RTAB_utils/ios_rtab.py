"""Hot-path slice of the reference's RTAB_utils/ios_rtab.py: depth frame -> world points -> surface normals on the GPU (row (f)#3).

``RTAB2Cache`` itself (pose-file / PNG / JPEG readers, colour resize, the pickle cache) stays out of scope: it is file I/O
around the methods restated here, ``__getRGBP3d`` (:155-177), ``__getModP3d`` (:179-193) and ``surface_normal_estimation``
(:236-248).
"""
import numpy as np

import f3d
from f3d.tensors import torch_device, work_stream


def resize_camera_matrix(intrinsic, scale_x, scale_y):
    """RTAB2Cache.__resize_camera_matrix (:115-131): intrinsics of the depth resolution."""
    K = np.asarray(intrinsic, np.float64)
    return np.array([[K[0, 0] * scale_x, 0., K[0, 2] * scale_x],
                     [0., K[1, 1] * scale_y, K[1, 2] * scale_y],
                     [0., 0., 1.0]])


def frame_points_world(depth, intrinsics_scaled, odo_xyzw, odo_xyz, depth_scale=1000):
    """One frame of ``mod_ptx``: unproject ``depth`` [H,W] with the scaled intrinsics (:171-173), mm -> m (:187), rotate by
    the pose quaternion -- ``odo_xyzw`` is the pose file's (x, y, z, w) row, as the reference indexes it (:190) -- and add
    the translation (:191-192).  Returns float64 [H*W, 3] in row-major pixel order."""
    q = np.asarray(odo_xyzw, np.float64)
    return f3d.default_context().unproject_depth(depth, intrinsics_scaled, q[[3, 0, 1, 2]], odo_xyz, depth_scale)


def frames_points_world(depths, intrinsics_scaled, odo_xyzw, odo_xyz, depth_scale=1000):
    """``RTAB2Cache.__getModP3d`` over all frames: list of [H*W, 3] arrays."""
    return [frame_points_world(d, intrinsics_scaled, q, t, depth_scale) for d, q, t in zip(depths, odo_xyzw, odo_xyz)]


def surface_normal_estimation(points, cam_centre, radius=0.05, max_nn=30):
    """RTAB2Cache.surface_normal_estimation (:236-248): normals of one frame's points [N,3] by Open3D's estimate_normals recipe
    (KDTreeSearchParamHybrid(radius, max_nn), restated in f3d.h), flipped to face ``cam_centre``.  float64 [N,3]."""
    return f3d.default_context().estimate_normals(points, np.asarray(cam_centre, np.float64), radius, max_nn)


def frames_world_dev(depths, intrinsics_scaled, odo_xyzw, odo_xyz, depth_scale=1000, radius=0.05, max_nn=30):
    """``mod_ptx`` and ``modSurfaceNormals`` (:284) of F frames on the device, in one batch each: depths [F,H,W] (NumPy or a
    torch tensor; uint16, float32 or float64) -> (points, normals), float64 torch tensors [F, H*W, 3] on the context's device.
    ``points[j]`` / ``normals[j]`` are what Fusion.from_frames(...).fuse_device takes.  The camera centre of frame j is
    ``odo_xyz[j]``, as the reference passes it (:280-283).  Raises F3DUnavailable without a device."""
    ctx = f3d.default_context()
    torch, dev = torch_device(ctx, 'frames_world_dev')
    q = np.asarray(odo_xyzw, np.float64).reshape(-1, 4)[:, [3, 0, 1, 2]]
    t = np.asarray(odo_xyz, np.float64).reshape(-1, 3)
    if isinstance(depths, torch.Tensor):
        d = depths.to(dev).contiguous()
        code = {torch.int16: 2, torch.float32: 1, torch.float64: 0}.get(d.dtype)
        if code is None and getattr(torch, 'uint16', None) is not None and d.dtype == torch.uint16:
            d, code = d.view(torch.int16), 2
    else:
        a = np.ascontiguousarray(depths)
        code = {np.dtype(np.uint16): 2, np.dtype(np.float32): 1, np.dtype(np.float64): 0}.get(a.dtype)
        d = torch.from_numpy(a.view(np.int16) if code == 2 else a).to(dev) if code is not None else None
    if code is None:
        raise ValueError('depths must be uint16 (int16 bits as a tensor), float32 or float64')
    if d.dim() != 3 or d.shape[0] != len(q) or len(t) != len(q):
        raise ValueError('depths must be [F,H,W] with one pose per frame')
    F, H, W = (int(x) for x in d.shape)
    pts = torch.empty((F, H * W, 3), dtype=torch.float64, device=dev)
    nrm = torch.empty((F, H * W, 3), dtype=torch.float64, device=dev)
    with work_stream(dev) as work:
        ctx.unproject_depth_batch_dev(d.data_ptr(), code, F, H, W, intrinsics_scaled, q, t, pts.data_ptr(), float(depth_scale), work.cuda_stream)
        ctx.estimate_normals_batch_dev(pts.data_ptr(), F, H * W, t, nrm.data_ptr(), radius, max_nn, True, stream=work.cuda_stream)
    return pts, nrm
