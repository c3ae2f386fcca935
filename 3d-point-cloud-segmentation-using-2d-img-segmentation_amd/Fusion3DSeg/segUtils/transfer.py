"""Carry a per-point result from the point set it was computed on to another one, on the GPU (no reference counterpart).

``get3DSeg.remove_classes`` and ``segment`` give one class, id or keep-bit per fused cloud point; ``meshUtils.clean_mesh``,
``remove_faces_by_vertices`` and ``keep_faces_by_vertices`` take one bit per mesh vertex; the dense frames' points and an RTAB
export are point sets of their own.  These functions join them: the hybrid search of libf3d_hip (at most k nearest within a
radius, f3d.h ``f3d_knn_query``) and the label transfer fused with it (``f3d_transfer_labels``), which keeps no [n, k] table.

NumPy arrays in give NumPy arrays out (host-pointer entries); if any point set, label array or mesh is a device tensor, the
others are moved to its device, the result is device tensors, ordered with torch's current stream (``f3d.tensors.work_stream``),
and nothing but the call's one readback (the cloud's box) touches the host.  No CPU fallback.

The search is radius-bounded: a query with no cloud point within ``radius`` has an empty row (``fill`` / ``unmatched``).  Rows are in
(squared distance, cloud index) order, ties in distance go to the lower index; the plurality's ties go to the label that comes
first in the row.  1 <= k <= 32.
"""
import numpy as np

import f3d
from f3d.tensors import device_points, dtype_code, on_device, work_stream
from Fusion3DSeg.segUtils import meshUtils

__all__ = ['nearest_points', 'transfer_labels', 'vertex_mask_from_points', 'clean_mesh_by_points']


def _device_of(*arrays):
    """The device of the first device tensor among `arrays`, or None (the NumPy route)."""
    for a in arrays:
        if on_device(a):
            return a.device
    return None


def _host_points(a, name):
    p = np.asarray(a.cpu() if hasattr(a, 'cpu') else a)
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError(f'{name} must be [N, 3], got {p.shape}')
    if p.dtype != np.float32:
        p = p.astype(np.float64)
    return np.ascontiguousarray(p)


def nearest_points(cloud, queries, radius, k=1):
    """At most ``k`` nearest ``cloud`` points within ``radius`` of every query -> (idx int32 [n, k], dist2 float64 [n, k], counts
    int32 [n]).  Row q lists cloud indices in (squared distance, index) order; the slots past counts[q] hold -1 / +inf."""
    k, r = f3d._knn_k(k), float(radius)
    dev = _device_of(queries, cloud)
    if dev is None:
        return f3d.default_context().knn_query(_host_points(cloud, 'cloud'), _host_points(queries, 'queries'), k, r)
    import torch
    ctx = f3d.default_context(dev.index)
    c, q = device_points(cloud, dev, 'cloud'), device_points(queries, dev, 'queries')
    n = len(q)
    idx = torch.empty((n, k), dtype=torch.int32, device=dev)
    dist2 = torch.empty((n, k), dtype=torch.float64, device=dev)
    counts = torch.empty(n, dtype=torch.int32, device=dev)
    with work_stream(dev) as work:
        ctx.knn_query_dev(c.data_ptr(), dtype_code(c), len(c), q.data_ptr(), dtype_code(q), n, k, r, idx.data_ptr(), dist2.data_ptr(),
                          counts.data_ptr(), work.cuda_stream)
    return idx, dist2, counts


def transfer_labels(cloud, labels, queries, radius, k=1, fill=-1, return_support=False):
    """The plurality label among the at most ``k`` nearest ``cloud`` points within ``radius`` of every query -> out [n] in the
    dtype of ``labels`` (any integer dtype or bool, one entry per cloud point); a query without a neighbour gets ``fill``,
    coerced to that dtype like every other value.  ``return_support``: also support int32 [n], the winner's count (0 for
    ``fill``).  k = 1 is the nearest point's label."""
    k, r = f3d._knn_k(k), float(radius)
    dev = _device_of(queries, cloud, labels)
    if dev is None:
        lab = np.asarray(labels)
        if lab.dtype != bool and not np.issubdtype(lab.dtype, np.integer):
            raise TypeError(f'labels must be an integer or bool array, got {lab.dtype}')
        c = _host_points(cloud, 'cloud')
        if lab.shape != (len(c),):
            raise ValueError(f'labels must have one entry per cloud point ({len(c)}), got shape {lab.shape}')
        fill = int(bool(fill)) if lab.dtype == bool else int(fill)
        out, support = f3d.default_context().transfer_labels(c, lab.astype(np.int64), _host_points(queries, 'queries'), k, r, fill)
        out = out.astype(lab.dtype)
        return (out, support) if return_support else out
    import torch
    ctx = f3d.default_context(dev.index)
    c, q = device_points(cloud, dev, 'cloud'), device_points(queries, dev, 'queries')
    lab = torch.as_tensor(labels).to(dev)
    if lab.dtype.is_floating_point or lab.dtype.is_complex:
        raise TypeError(f'labels must be an integer or bool tensor, got {lab.dtype}')
    if tuple(lab.shape) != (len(c),):
        raise ValueError(f'labels must have one entry per cloud point ({len(c)}), got shape {tuple(lab.shape)}')
    fill = int(bool(fill)) if lab.dtype == torch.bool else int(fill)
    lab64 = lab.to(torch.int64).contiguous()
    n = len(q)
    out = torch.empty(n, dtype=torch.int64, device=dev)
    support = torch.empty(n, dtype=torch.int32, device=dev) if return_support else None
    with work_stream(dev) as work:
        ctx.transfer_labels_dev(c.data_ptr(), dtype_code(c), len(c), lab64.data_ptr(), q.data_ptr(), dtype_code(q), n, k, r, fill,
                                out.data_ptr(), None if support is None else support.data_ptr(), work.cuda_stream)
    out = out.to(lab.dtype)
    return (out, support) if return_support else out


def vertex_mask_from_points(cloud, point_mask, vertices, radius, k=1, unmatched=False):
    """A per-point bit of ``cloud`` carried to mesh vertices -> bool [V]: the transferred bit (the plurality of the at most ``k``
    nearest cloud points within ``radius``), ``unmatched`` for a vertex with no cloud point within ``radius``.  The result is
    what ``meshUtils.clean_mesh``, ``remove_faces_by_vertices`` and ``keep_faces_by_vertices`` take as their mask."""
    if on_device(point_mask):
        import torch
        bits = point_mask.to(torch.bool)
    else:
        bits = np.asarray(point_mask).astype(bool)
    return transfer_labels(cloud, bits, vertices, radius, k=k, fill=bool(unmatched))


def clean_mesh_by_points(vertices, triangles, cloud, remove_point_mask, radius, k=1, min_triangles=1, min_area=0.0):
    """``meshUtils.clean_mesh`` with the vertices to remove chosen by a per-point bit of ``cloud``
    (``vertex_mask_from_points``; a vertex with no cloud point within ``radius`` stays) -> (new_vertices, new_triangles,
    kept_vertex_mask bool [V], kept_triangle_mask bool [M]).  With a device mesh everything runs on its device."""
    dev = _device_of(triangles, vertices)
    if dev is not None:
        vertices = device_points(vertices, dev, 'vertices')
    mask = vertex_mask_from_points(cloud, remove_point_mask, vertices, radius, k=k, unmatched=False)
    if dev is None and on_device(mask):
        mask = mask.cpu().numpy()
    return meshUtils.clean_mesh(vertices, triangles, mask, min_triangles=min_triangles, min_area=min_area)
