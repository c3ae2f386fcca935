"""The reference's Fusion3DSeg/segUtils/refinement.py on the GPU: repair a picked door / window after panoptic segmentation
by growing it over neighbouring points at the same depth off the wall plane, or of the same colour.

The four ``*_floodfill_*`` functions of the reference are one FIFO flood whose acceptance test is a running mean carried
over the whole flood.  Here that flood is f3d_region_grow (csrc/f3d_refine.hip, one GPU workgroup, the reference's queue
order); ``grow_depth`` / ``grow_color`` are its array-level entries and take NumPy arrays or device tensors.  The running
mean's start is ``np.average`` of the seed values, reduced with NumPy on the host (NumPy's summation order), which is the
only thing that leaves the device on the tensor route.  Pinned by tests/golden/refinement.npz.

The public wrappers keep the reference's positional signatures.  No viewer exists here, so the index the reference gets from
``pick_points`` is the keyword ``selected_point`` (an index, or a list whose first entry names the instance; ``None`` raises).
``instance_id`` / ``seg_colors`` / ``seg_points`` pass the segmentation directly instead of the ``ids.npy`` + ``pcd.ply`` the
reference reads under ``outputpath``.  They return ``(instance_id, PointCloud)``.

Two deliberate deviations.  A picked list with a repeated index makes the reference process that point twice and return it
twice; here it is a ``ValueError``.  A negative seed or picked index wraps in the reference's NumPy indexing (and then appears
in its result as a negative number); here every index outside [0, N) is an ``IndexError``.
"""
import os

import numpy as np

import f3d
from f3d.tensors import CSR_ADJACENCY, device_csr, dtype_code, host_csr, on_device, work_stream
from Fusion3DSeg.segUtils.cv import adjacency_to_csr
from RTAB_utils.spatQuad import SpatQuadranion as Quat

_COL = {'Shapeinfo': 0, 'indicies': 1, 'BBoxids': 2, 'BBoxpoints': 3}          # columns of the plane table (planeUtils.Headers)


# ------------------------------------------------------------------------------------------------ array level
def _seeds_host(seeds, n, what):
    sd = np.asarray(seeds)
    if sd.dtype.kind not in 'iu' and sd.size:
        raise TypeError(f'{what}: seeds must be integer indices, got {sd.dtype}')
    sd = np.ascontiguousarray(sd.reshape(-1), dtype=np.int64)
    if len(sd) and (sd.min() < 0 or sd.max() >= n):
        raise IndexError(f'{what}: seed index out of bounds for {n} points')
    if len(np.unique(sd)) != len(sd):
        raise ValueError(f'{what}: a seed is listed twice')
    return sd


def _grow(values, nchan, adj, seeds, threshold, max_level, given, single, what):
    """The flood over `values` ([n] for nchan 1, [n, 3] for nchan 3).  `single`: the reference's one-point colour rule (the mean
    starts as the seed's value and counts no point); otherwise it starts as the seeds' average and counts them."""
    shape = tuple(values.shape)
    n = shape[0] if shape else 0
    if (nchan == 1 and len(shape) != 1) or (nchan == 3 and (len(shape) != 2 or shape[1] != 3)):
        raise ValueError(f'{what}: values must be {"[N]" if nchan == 1 else "[N, 3]"}, got {shape}')
    thr = np.asarray(threshold, dtype=np.float64)
    if thr.ndim and thr.size != nchan:
        raise ValueError(f'{what}: threshold must be a scalar or have {nchan} entries')
    if on_device(values):
        import torch
        dev = values.device
        ok = (torch.float64,) if nchan == 1 else (torch.float64, torch.float32)
        if values.dtype not in ok:
            raise TypeError(f'{what}: values must be {" or ".join(str(t) for t in ok)}, got {values.dtype}')
        offs, nbrs = device_csr(adj, n, dev, 'device values')
        sd = torch.as_tensor(seeds, device=dev)
        if (sd.dtype.is_floating_point or sd.dtype == torch.bool) and sd.numel():
            raise TypeError(f'{what}: seeds must be integer indices, got {sd.dtype}')
        sd = sd.to(torch.int64).reshape(-1).contiguous()
        if not len(sd):
            return torch.zeros(0, dtype=torch.int64, device=dev)
        if n == 0:
            raise IndexError(f'{what}: seed index out of bounds for 0 points')
        val = values.contiguous()
        picked = val[sd.clamp(0, n - 1)].cpu().numpy()                    # the only data that leaves the device
        sma0, npts0 = (picked[0], 0) if single else (np.average(picked, axis=0), len(sd))
        cluster = torch.empty(n, dtype=torch.int64, device=dev)
        count = torch.zeros(1, dtype=torch.int64, device=dev)
        ctx = f3d.default_context(dev.index)
        with work_stream(dev) as work:
            ctx.region_grow_dev(val.data_ptr(), dtype_code(val), nchan, n, offs.data_ptr(),
                                nbrs.data_ptr(), sd.data_ptr(), len(sd), sma0, npts0, thr, max_level, cluster.data_ptr(),
                                count.data_ptr(), given, work.cuda_stream)
            try:
                ctx.take_device_error(work.cuda_stream)                   # synchronises the stream: the results are complete
            except IndexError:                                            # the kernel refused the seeds (nothing ran), or met a bad row
                if bool(((sd < 0) | (sd >= n)).any()):
                    raise IndexError(f'{what}: seed index out of bounds for {n} points') from None
                if len(torch.unique(sd)) != len(sd):
                    raise ValueError(f'{what}: a seed is listed twice') from None
                raise
        return cluster[:int(count)].clone()                               # not a view: the n-entry buffer is released
    val = np.asarray(values)
    ok = (np.float64,) if nchan == 1 else (np.float64, np.float32)
    if val.dtype not in ok:
        raise TypeError(f'{what}: values must be {" or ".join(np.dtype(t).name for t in ok)}, got {val.dtype}')
    if not isinstance(adj, tuple) and n and isinstance(adj[0], (set, frozenset)):
        adj = [list(a) for a in adj]                                      # the reference's list[set]: rows in the sets' iteration order
    offs, nbrs = host_csr(*adjacency_to_csr(adj, n), n, CSR_ADJACENCY)
    sd = _seeds_host(seeds, n, what)
    if not len(sd):
        return np.zeros(0, np.int64)
    picked = val[sd]
    sma0, npts0 = (picked[0], 0) if single else (np.average(picked, axis=0), len(sd))
    return f3d.default_context().region_grow(val, offs, nbrs, sd, sma0, npts0, thr, max_level, given)


def grow_depth(distance, adj, seeds, threshold, max_level=50, given=False):
    """The reference's floodfill_depth_points (``given=True``: the seeds are an instance's points; they are tested and expanded
    but not returned) and floodfill_depth_point (``given=False``: the seeds are picked points and are returned when accepted).
    distance float64 [N]; adj a list of rows or a CSR pair (a device CSR pair for a device tensor); seeds distinct indices in
    queue order.  -> the accepted points int64, in acceptance order (a device tensor for device input).  max_level <= 0: no limit."""
    return _grow(distance, 1, adj, seeds, threshold, max_level, given, False, 'grow_depth')


def grow_color(colors, adj, seeds, threshold, max_level=50, given=False):
    """The reference's floodfill_color_points (seeds = an instance's points, ``given=True``) and floodfill_color_point (seeds = ONE
    index, not a list: the mean starts as that point's colour and counts no point).  A list of picked points with ``given=False`` is
    the colour analogue of floodfill_depth_point.  colors float64 or float32 [N, 3]; threshold a scalar or [r, g, b]."""
    single = np.ndim(seeds) == 0 and not given
    return _grow(colors, 3, adj, seeds, threshold, max_level, given, single, 'grow_color')


def plane_distance(points, plane_point, normal):
    """|(points - plane_point) . normal| on the GPU (f3d_plane_distance), float64 [N]: NumPy array or device tensor.  The sum is
    ((dx nx + dy ny) + dz nz); the reference's einsum adds in another order, so a point whose distance lies within rounding of the
    threshold may fall on the other side of it than in the reference."""
    if on_device(points):
        import torch
        if points.dtype != torch.float64 or points.dim() != 2 or points.shape[1] != 3:
            raise TypeError(f'plane_distance: points must be a float64 [N, 3] tensor, got {points.dtype} {tuple(points.shape)}')
        pts = points.contiguous()
        out = torch.empty(len(pts), dtype=torch.float64, device=pts.device)
        with work_stream(pts.device) as work:
            f3d.default_context(pts.device.index).plane_distance_dev(pts.data_ptr(), len(pts), plane_point, normal, out.data_ptr(),
                                                                     work.cuda_stream)
        return out
    return f3d.default_context().plane_distance(points, plane_point, normal)


# ------------------------------------------------------------------------------------------------ files
def read_ply(path):
    """(xyz float64 [N, 3], colours float64 [N, 3] in [0, 1] or None) of a binary little-endian or ascii PLY with scalar vertex
    properties (what get3DSeg.write_ply writes)."""
    np_t = {'double': '<f8', 'float': '<f4', 'uchar': 'u1', 'float64': '<f8', 'float32': '<f4', 'uint8': 'u1', 'int': '<i4'}
    with open(path, 'rb') as fp:
        props, n, fmt, in_vertex = [], 0, 'ascii', False
        while True:
            line = fp.readline().decode('ascii').strip()
            if line.startswith('format'):
                fmt = line.split()[1]
            elif line.startswith('element'):
                in_vertex = line.split()[1] == 'vertex'
                if in_vertex:
                    n = int(line.split()[-1])
            elif line.startswith('property') and in_vertex and 'list' not in line:
                props.append(line.split()[1:3])
            elif line == 'end_header':
                break
        names = [nm for _, nm in props]
        if fmt == 'ascii':
            data = np.loadtxt(fp, max_rows=n, ndmin=2).reshape(n, len(names))
            rec = {nm: data[:, k] for k, nm in enumerate(names)}
        else:
            rec = np.frombuffer(fp.read(), dtype=[(nm, np_t[t]) for t, nm in props], count=n)
    pts = np.stack([rec['x'], rec['y'], rec['z']], axis=1).astype(np.float64)
    clr = np.stack([rec['red'], rec['green'], rec['blue']], axis=1) / 255.0 if 'red' in names else None
    return pts, clr


def _load_segmentation(outputpath, instance_id, seg_colors, seg_points, points_all):
    """(instance_id, PointCloud of the segmentation): the keywords, or cv_segmentation/ then panoptic_segmentation/ under
    outputpath (reference :136-147).  The cloud's colours are an array of their own: the wrappers write into them."""
    from get3DSeg import PointCloud
    if instance_id is not None:
        if seg_colors is None:
            raise ValueError('instance_id= needs seg_colors= (the segmentation cloud\'s colours)')
        pts = points_all if seg_points is None else np.asarray(seg_points, np.float64)
        return np.asarray(instance_id), PointCloud(pts, np.array(seg_colors, dtype=np.float64))
    cv_seg_path = outputpath + os.sep + 'cv_segmentation'
    os.makedirs(cv_seg_path, exist_ok=True)
    where = cv_seg_path
    if not (os.path.exists(os.path.join(where, 'ids.npy')) and os.path.exists(os.path.join(where, 'pcd.ply'))):
        where = outputpath + os.sep + 'panoptic_segmentation'
    pts, clr = read_ply(os.path.join(where, 'pcd.ply'))
    if clr is None:
        raise ValueError(f'{os.path.join(where, "pcd.ply")} has no colours')
    return np.load(os.path.join(where, 'ids.npy')), PointCloud(pts, clr)


def _picked(selected_point, n):
    if selected_point is None:
        raise ValueError('selected_point= is required: there is no viewer here to pick a point in (the reference calls pick_points)')
    sel = np.asarray(selected_point)
    if sel.dtype.kind not in 'iu':
        raise TypeError(f'selected_point must be an integer index or a list of them, got {sel.dtype}')
    sel = sel.reshape(-1).astype(np.int64)
    if not len(sel):
        raise IndexError('selected_point is empty')                                # selected_point[0] (:165)
    if sel.min() < 0 or sel.max() >= n:
        raise IndexError(f'selected_point out of bounds for {n} points')
    if len(np.unique(sel)) != len(sel):
        raise ValueError('selected_point lists a point twice')
    return sel


def _wall_distance(PlaneswithPoints, Vertex, SelectedPoint, BoundingPoints):
    """dp of the depth wrappers, by the reference's own NumPy expression (:148-157), so that the host route equals the reference."""
    planeidx, _ = GetactualIndex(SelectedPoints=SelectedPoint, PLanewithPoints=PlaneswithPoints, Vertex=Vertex)
    all_ind = planeidx.tolist()
    normal_wall = np.asarray(PlaneswithPoints[all_ind[0], 0].normal)
    points_all = Vertex[:, :3]
    point_wall = BoundingPoints[PlaneswithPoints[0, 2]][0].reshape(1, 3)
    normal_wall = normal_wall.reshape(1, 3)
    point_vectors = points_all[:, None, :] - point_wall[None, :, :]
    dp = np.einsum('nmc, mc -> mn', point_vectors, normal_wall)
    return np.abs(dp[0])


def _apply(cluster, instance_id, seg, door_id, door_palette):
    """The wrappers' ending (:172-181): the grown points take the instance's id and colour; nothing changes for an empty flood."""
    if len(cluster) > 0:
        instance_id[cluster] = door_id
        seg.colors[cluster] = door_palette
    return instance_id, seg


def depth_floodfill_dl(PlaneswithPoints, Vertex, SelectedPoint, BoundingPoints, connected, outputpath, depth_threshold=0.03, max_level=50,
                       viz_ply=False, *, selected_point=None, instance_id=None, seg_colors=None, seg_points=None):
    """Grow the picked instance over the connected points at its depth off the wall plane (reference :84-182).  -> (instance_id,
    PointCloud); instance_id is updated in place."""
    sel = _picked(selected_point, len(Vertex))
    instance_id, seg = _load_segmentation(outputpath, instance_id, seg_colors, seg_points, Vertex[:, :3])
    dp = _wall_distance(PlaneswithPoints, Vertex, SelectedPoint, BoundingPoints)
    door_id, door_palette = instance_id[sel[0]], seg.colors[sel[0]].copy()
    door_points = np.where(instance_id == door_id)[0]
    return _apply(grow_depth(dp, connected, door_points, depth_threshold, max_level, given=True), instance_id, seg, door_id, door_palette)


def depth_floodfill_point(PlaneswithPoints, Vertex, SelectedPoint, BoundingPoints, connected, outputpath, depth_threshold=0.03, max_level=50,
                          viz_ply=False, *, selected_point=None, instance_id=None, seg_colors=None, seg_points=None):
    """Extract a door / window from the wall by depth, from the picked points themselves (reference :185-273)."""
    sel = _picked(selected_point, len(Vertex))
    instance_id, seg = _load_segmentation(outputpath, instance_id, seg_colors, seg_points, Vertex[:, :3])
    dp = _wall_distance(PlaneswithPoints, Vertex, SelectedPoint, BoundingPoints)
    door_id, door_palette = instance_id[sel[0]], seg.colors[sel[0]].copy()
    return _apply(grow_depth(dp, connected, sel, depth_threshold, max_level), instance_id, seg, door_id, door_palette)


def color_floodfill_dl(Vertex, connected, outputpath, color_threshold=0.1, max_level=50, viz_ply=False, *, selected_point=None,
                       instance_id=None, seg_colors=None, seg_points=None):
    """Grow the picked instance over the connected points of its colour (reference :276-353); the colours are Vertex[:, 3:6]."""
    sel = _picked(selected_point, len(Vertex))
    instance_id, seg = _load_segmentation(outputpath, instance_id, seg_colors, seg_points, Vertex[:, :3])
    door_id, door_palette = instance_id[sel[0]], seg.colors[sel[0]].copy()
    door_points = np.where(instance_id == door_id)[0]
    cluster = grow_color(np.ascontiguousarray(Vertex[:, 3:6]), connected, door_points, color_threshold, max_level, given=True)
    return _apply(cluster, instance_id, seg, door_id, door_palette)


def color_floodfill_point(Vertex, connected, outputpath, color_threshold=0.1, max_level=50, viz_ply=False, *, selected_point=None,
                          instance_id=None, seg_colors=None, seg_points=None):
    """Extract a door / window by colour from the first picked point (reference :356-432)."""
    sel = _picked(selected_point, len(Vertex))
    instance_id, seg = _load_segmentation(outputpath, instance_id, seg_colors, seg_points, Vertex[:, :3])
    door_id, door_palette = instance_id[sel[0]], seg.colors[sel[0]].copy()
    cluster = grow_color(np.ascontiguousarray(Vertex[:, 3:6]), connected, int(sel[0]), color_threshold, max_level)
    return _apply(cluster, instance_id, seg, door_id, door_palette)


def save_ids_ply(seg_ply, instance_ids, outputpath):
    """Save the instance ids and the updated cloud under outputpath/cv_segmentation (reference :435-440)."""
    from get3DSeg import write_ply
    cv_seg_path = outputpath + os.sep + 'cv_segmentation'
    os.makedirs(cv_seg_path, exist_ok=True)
    write_ply(cv_seg_path + os.sep + 'pcd.ply', seg_ply)
    np.save(cv_seg_path + os.sep + 'ids.npy', instance_ids)


# ------------------------------------------------------------------------------------------------ host geometry
def ReadVerticesConnectedFiles(file_connected_path):
    """Rows of the connected-graph file (reference :9-13): a header line ``VIDs``, then ``id,neighbour,neighbour,...`` per line ->
    list of neighbour lists."""
    with open(file_connected_path) as fp:
        lines = [ln.rstrip('\n') for ln in fp]
    if not lines or lines[0].strip() != 'VIDs':
        raise KeyError('VIDs')
    return [list(map(int, ln.split(',')[1:])) for ln in lines[1:] if ln.strip()]


def GetactualIndex(SelectedPoints, Vertex, PLanewithPoints, BoundingPoints=None):
    """Rows of the plane table that hold the selected points (reference :16-38): by vertex index when the point is a vertex,
    else by its bounding points.  -> (row indices, the point indices of those rows, repeated as the reference repeats them)."""
    idxlist, indices = [], []
    for pt in SelectedPoints:
        hit = np.where(np.all(Vertex[:, 0:3] == pt, axis=1))[0]
        if len(hit) > 0:
            v = hit[0]
            idx = [i for i, p in enumerate(PLanewithPoints[:, _COL['indicies']]) if p.intersection({v})]
        else:
            idx = [i for i in range(len(PLanewithPoints)) if np.any(np.all(PLanewithPoints[i, _COL['BBoxpoints']] == pt, axis=1))]
        if len(idx) < 1 or idx[0] in idxlist:
            continue
        idxlist.append(idx[0])
        for i in idxlist:
            indices.extend(list(PLanewithPoints[i, _COL['indicies']]))
    return np.array(idxlist), indices


def _foot_on_line(a, b, p):
    """(distance from p to its foot, the foot) on the line through a and b"""
    along = b - a
    foot = a + np.dot(p - a, along) / np.dot(along, along) * along
    return np.linalg.norm(foot - p), foot


def door_updation(outer_poly, inner_poly, normal_wall, max_distance=0.2):
    """Project the door's corners [4, 3] into the wall plane (through outer_poly[0]) and snap each to every wall side whose line
    is nearer than max_distance, side after side: sides 0-1, 1-2, 2-3, then 0-3, and a later side sees the corner where the
    earlier one left it (reference :41-81).  -> the updated corners [4, 3]; the arguments are not written."""
    wall = np.asarray(outer_poly)
    lift = wall[0].dot(normal_wall) - np.einsum('c, nc -> n', normal_wall, inner_poly)
    door = inner_poly + lift[:, None] * normal_wall[None, :]
    last = len(wall) - 1
    sides = [(k, k + 1) for k in range(last)] + [(0, last)]
    for corner in door:                                                    # a row view: a snap is seen by the next side
        for k0, k1 in sides:
            dist, foot = _foot_on_line(wall[k0], wall[k1], corner)
            if dist < max_distance:
                corner[:] = foot
    return door


def _rotate_quad(q, p):
    """q p q* without normalising q (what SpatQuadranion.rotate computes on the GPU for a cloud), on the host: four corners."""
    w, v = q[0], np.asarray(q[1:], np.float64)
    a = w * p + np.cross(v, p)                                   # vector part of q p; its scalar part is -(p . v)
    return (p @ v)[:, None] * v[None, :] + w * a - np.cross(a, v)


def _door_wall_bottom_align(door_BBp, wall_BBp, flip):
    door_BB = door_BBp[door_BBp[:, 2].argsort()]
    door_vector = door_BB[1] - door_BB[0]
    wall_BB = wall_BBp[wall_BBp[:, 2].argsort()]
    wall_vector = wall_BB[1] - wall_BB[0]
    wall_vector = wall_vector / np.linalg.norm(wall_vector)
    door_vector = door_vector / np.linalg.norm(door_vector)
    axis = np.cross(wall_vector, door_vector)
    axis = axis / np.linalg.norm(axis)
    angle = np.arccos(np.dot(wall_vector, door_vector))
    pivot = door_BB[0]
    qt = Quat(axis=axis, angle=angle)
    return _rotate_quad((qt.inverse if flip else qt).q, door_BBp - pivot) + pivot


def door_floor_align(PlaneswithPoints, Vertex, SelectedPoint, BoundingPoints, connected, outputpath, flip=True):
    """Turn the first selected plane's quad (the door) about its lowest corner so that its bottom edge is parallel to the second's
    (the wall's) (reference :443-494).  BoundingPoints is updated in place.  The rotation goes through SpatQuadranion(axis=, angle=),
    whose parity with pyquaternion is unpinned."""
    planeidx, _ = GetactualIndex(SelectedPoints=SelectedPoint, PLanewithPoints=PlaneswithPoints, Vertex=Vertex)
    all_ind = planeidx.tolist()
    door_key = PlaneswithPoints[all_ind[0], _COL['BBoxids']]
    wall_BB = BoundingPoints[PlaneswithPoints[all_ind[1], _COL['BBoxids']]]
    BoundingPoints[door_key] = _door_wall_bottom_align(BoundingPoints[door_key], wall_BB, flip)
    return PlaneswithPoints, Vertex, BoundingPoints
