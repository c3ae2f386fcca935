"""The part of the reference's Fusion3DSeg/segUtils/planeUtils.py that the pipeline needs, and the producer it never shipped.

The reference got its plane table from ``./Executables/ConnectedGraph`` (run_connected_executable) and PolyFit; neither exists.
``extract_planes`` produces the table on the GPU instead (f3d_extract_planes, csrc/f3d_planes.hip: a deterministic plane
segmentation of a cloud over its adjacency; the contract is in include/f3d.h), and ``plane_table`` puts it into the shape
``refinement.py`` indexes (PlaneswithPoints with the columns of ``Headers``, and BoundingPoints).  The legends and column helpers
keep the reference's names and values.  Its path, PLY and CSV helpers and run_connected_executable are not ported.
"""
import math
from collections import namedtuple

import numpy as np

import f3d
from f3d.tensors import CSR_ADJACENCY, device_csr, dtype_code, host_csr, on_device, work_stream
from Fusion3DSeg.segUtils.cv import adjacency_to_csr


# ------------------------------------------------------------------------------------------------ legends
def ObjLegend():
    return {1: 'Walls', 2: 'Ceilings', 3: 'Floors', 4: 'Beams', 5: 'Columns', 6: 'Doors', 7: 'Windows', 8: 'Pipes'}


def getShapelegend():
    return {'Plane': 1, 'Cuboid': 2, 'Cylinders': 3, 'Sphere': 4, 'Cone': 5, 'Unidentified': 0}


def Headers():
    return {'Shapeinfo': 0, 'indicies': 1, 'BBoxids': 2, 'BBoxpoints': 3, 'Hide': 4, 'Category': 5, 'Shape': 6, 'Area': 7}


def revealShape(Category):
    """The shape of an object category: beams and columns are cuboids, the other categories up to windows planes, the rest cylinders."""
    if Category in (4, 5):
        return getShapelegend()['Cuboid']
    if Category in range(1, 8):
        return getShapelegend()['Plane']
    return getShapelegend()['Cylinders']


def Col(str):
    return Headers()[str]


def Obj(str):
    for key, val in ObjLegend().items():
        if val == str:
            return key
    return None


# ------------------------------------------------------------------------------------------------ extraction
PlaneSet = namedtuple('PlaneSet', ['labels', 'planes', 'corners', 'counts'])
PlaneSet.__doc__ = """labels int32 [N] (-1: no plane), planes float64 [P, 8] (normal, -normal . centroid, centroid, rms residual), corners
float64 [P, 4, 3] (the quad (min, min), (max, min), (max, max), (min, max) in the plane's axes), counts int64 [4] (planes written,
qualifying components, attach rounds run, labelled points).  Device tensors for device input."""


class Shapeinfo:
    """A plane of the table: a point on it and its unit normal (what refinement.py reads as ``.normal``)."""
    __slots__ = ('point', 'normal')

    def __init__(self, point, normal):
        self.point, self.normal = point, normal

    def __repr__(self):
        return f'Shapeinfo(point={self.point!r}, normal={self.normal!r})'


def _scalars(angle, offset, dist, max_variation, min_points, max_rounds):
    min_points, max_rounds = int(min_points), int(max_rounds)
    if min_points < 3:
        raise ValueError(f'extract_planes: min_points must be at least 3, got {min_points}')
    if max_rounds < 0:
        raise ValueError(f'extract_planes: max_rounds must not be negative, got {max_rounds}')
    return math.cos(math.radians(float(angle))), float(offset), float(dist), float(max_variation), min_points, max_rounds


def extract_planes(points, adj, normals=None, angle=10.0, offset=0.01, dist=0.01, max_variation=0.01, min_points=50, max_rounds=64):
    """Planes of a cloud over its adjacency (include/f3d.h f3d_extract_planes).  points float64 / float32 [N, 3]; adj a list of rows
    or a CSR pair, symmetric and without duplicate entries (``f3d.Context.radius_graph``); normals float64 [N, 3] unit vectors, or None
    for the PCA of every point's row.  Core points whose normals agree within `angle` degrees and that lie within `offset` of each
    other's tangent plane are joined; components of at least `min_points` are planes; members farther than `dist` from the fitted
    plane are dropped; unlabelled points then join a neighbour's plane within `dist`, in at most `max_rounds` rounds.  Device tensors
    with a device CSR pair stay on the device.  -> PlaneSet.  Every argument is checked before anything is launched."""
    cos_angle, offset, dist, max_variation, min_points, max_rounds = _scalars(angle, offset, dist, max_variation, min_points, max_rounds)
    shape = tuple(points.shape) if hasattr(points, 'shape') else np.shape(points)
    if len(shape) != 2 or shape[1] != 3:
        raise ValueError(f'extract_planes: points must be [N, 3], got {shape}')
    n = shape[0]
    if normals is not None and tuple(normals.shape) != (n, 3):
        raise ValueError(f'extract_planes: normals must be [{n}, 3], got {tuple(normals.shape)}')
    max_planes = n // min_points
    if on_device(points):
        import torch
        dev = points.device
        if points.dtype not in (torch.float64, torch.float32):
            raise TypeError(f'extract_planes: points must be float64 or float32, got {points.dtype}')
        if normals is not None and (not on_device(normals) or normals.dtype != torch.float64):
            raise TypeError('extract_planes: normals must be a float64 device tensor for device points')
        offs, nbrs = device_csr(adj, n, dev, 'device points')
        pts = points.contiguous()
        nrm = None if normals is None else normals.to(dev).contiguous()
        labels = torch.empty(n, dtype=torch.int32, device=dev)
        planes = torch.zeros((max_planes, 8), dtype=torch.float64, device=dev)
        corners = torch.zeros((max_planes, 4, 3), dtype=torch.float64, device=dev)
        counts = torch.zeros(4, dtype=torch.int64, device=dev)
        ctx = f3d.default_context(dev.index)
        with work_stream(dev) as work:
            ctx.extract_planes_dev(pts.data_ptr(), dtype_code(pts), n, offs.data_ptr(), nbrs.data_ptr(), None if nrm is None else nrm.data_ptr(),
                                   cos_angle, offset, dist, max_variation, min_points, max_rounds, max_planes, labels.data_ptr(),
                                   planes.data_ptr(), corners.data_ptr(), counts.data_ptr(), None, work.cuda_stream)
            ctx.take_device_error(work.cuda_stream)                       # synchronises the stream: the results are complete
            written = int(counts[0])
        return PlaneSet(labels, planes[:written].clone(), corners[:written].clone(), counts)
    pts = np.asarray(points)
    if pts.dtype not in (np.float64, np.float32):
        raise TypeError(f'extract_planes: points must be float64 or float32, got {pts.dtype}')
    pts = np.ascontiguousarray(pts)
    if normals is not None:
        if on_device(normals) or np.asarray(normals).dtype != np.float64:
            raise TypeError('extract_planes: normals must be a float64 array for host points')
        normals = np.ascontiguousarray(normals)
    if isinstance(adj, tuple) and any(on_device(a) for a in adj):
        raise TypeError('extract_planes: host points need a host adjacency (a device CSR pair goes with device tensors)')
    offs, nbrs = host_csr(*adjacency_to_csr(adj, n), n, CSR_ADJACENCY)
    return PlaneSet(*f3d.default_context().extract_planes(pts, offs, nbrs, normals, cos_angle, offset, dist, max_variation, min_points,
                                                          max_rounds, max_planes))


def plane_table(planeset):
    """(PlaneswithPoints, BoundingPoints) of a PlaneSet, as refinement.py indexes them.  PlaneswithPoints is an object array [P, 8]
    with the columns of ``Headers``: Shapeinfo (``.point`` = the centroid, ``.normal``), indicies (the ``set`` of member indices),
    BBoxids (the 4 rows of BoundingPoints that hold the plane's quad), BBoxpoints (float64 [4, 3]), Hide 0, Category 0, Shape
    ``getShapelegend()['Plane']``, Area (the quad's area).  BoundingPoints is float64 [4 P, 3].  Device tensors are copied to the host."""
    labels, planes, corners = (np.asarray(a.cpu() if on_device(a) else a) for a in planeset[:3])
    P = len(planes)
    corners = np.ascontiguousarray(corners, dtype=np.float64).reshape(P, 4, 3)
    order = np.argsort(labels, kind='stable')
    cuts = np.searchsorted(labels[order], np.arange(P + 1))
    table = np.empty((P, 8), dtype=object)
    H = Headers()
    for k in range(P):
        quad = corners[k].copy()
        table[k, H['Shapeinfo']] = Shapeinfo(planes[k, 4:7].copy(), planes[k, 0:3].copy())
        table[k, H['indicies']] = set(order[cuts[k]:cuts[k + 1]].tolist())
        table[k, H['BBoxids']] = np.arange(4 * k, 4 * k + 4)
        table[k, H['BBoxpoints']] = quad
        table[k, H['Hide']] = 0
        table[k, H['Category']] = 0
        table[k, H['Shape']] = getShapelegend()['Plane']
        table[k, H['Area']] = float(np.linalg.norm(quad[1] - quad[0]) * np.linalg.norm(quad[3] - quad[0]))
    return table, corners.reshape(4 * P, 3).copy()
