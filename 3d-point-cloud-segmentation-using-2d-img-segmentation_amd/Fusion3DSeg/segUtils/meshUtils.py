"""The mesh-topology part of the reference's Fusion3DSeg/segUtils/meshUtils.py on the GPU, plus ``clean_mesh`` and the face graph
(``face_normals``, ``face_adjacency``, ``segment_faces``: face votes smoothed over the faces' adjacency and split into instances).

Same names and positional signatures as the reference (file:line in each docstring).  NumPy arrays in give NumPy arrays out
(host-pointer entries of libf3d_hip); device tensors in give device tensors out, ordered with torch's current stream
(``f3d.tensors.work_stream``).  The kernel-backed functions have no CPU fallback.

Limits: V < 2^31 vertices, 3 M < 2^31; triangles are int32 or int64 [M, 3].  A vertex index outside [0, V) raises IndexError
and writes nothing -- a stated deviation: the reference's list and NumPy indexing wrap a negative index.

The Open3D / cv2 converters and viewers of the reference file (to_pcd, to_mesh, to_lines, to_uvmesh, to_image, pick_points,
get_roi, read_images, load_o3d_camera_data), generate_texture, uv2rgb and classwise_triangle_colors are not provided.
"""
import math

import numpy as np

import f3d
from f3d.tensors import dtype_code, index_code, on_device, upload, work_stream

__all__ = ['vertex_triangle_mapping', 'remove_faces_by_vertices', 'keep_faces_by_vertices', 'get_triangle_clusters', 'clean_mesh', 'label_faces',
           'face_normals', 'face_adjacency', 'segment_faces_from_votes', 'segment_faces', 'bbox_axes', 'one_to_all_angles', 'VertexTriangleMap']


# ------------------------------------------------------------------------------------------------ argument checks
def _triangles(triangles):
    """int32 / int64 [M, 3], C-contiguous, as given (NumPy array or device tensor)."""
    if on_device(triangles):
        import torch
        if triangles.dtype not in (torch.int32, torch.int64):
            raise TypeError(f'triangles must be int32 or int64, got {triangles.dtype}')
        if triangles.dim() != 2 or triangles.shape[1] != 3:
            raise ValueError(f'triangles must be [M, 3], got {tuple(triangles.shape)}')
        tris = triangles.contiguous()
    else:
        tris = np.asarray(triangles)
        if tris.dtype not in (np.int32, np.int64):
            raise TypeError(f'triangles must be int32 or int64, got {tris.dtype}')
        if tris.ndim != 2 or tris.shape[1] != 3:
            raise ValueError(f'triangles must be [M, 3], got {tris.shape}')
        tris = np.ascontiguousarray(tris)
    if 3 * tris.shape[0] >= 1 << 31:
        raise ValueError('3 * M must be below 2^31')
    return tris


def _nvertices(nvertices):
    nv = int(nvertices)
    if nv < 0 or nv >= 1 << 31:
        raise ValueError(f'nvertices must be in [0, 2^31), got {nv}')
    return nv


def _vertices(vertices, like):
    """float64 / float32 [V, 3] where `like` (the triangles) lives; other dtypes are widened to float64."""
    if on_device(like):
        import torch
        verts = torch.as_tensor(vertices, device=like.device)
        if verts.dtype not in (torch.float64, torch.float32):
            verts = verts.to(torch.float64)
        shape = tuple(verts.shape)
        verts = verts.contiguous()
    else:
        verts = np.asarray(vertices.cpu() if on_device(vertices) else vertices)
        if verts.dtype not in (np.float64, np.float32):
            verts = verts.astype(np.float64)
        shape = verts.shape
        verts = np.ascontiguousarray(verts)
    if len(shape) != 2 or shape[1] != 3:
        raise ValueError(f'vertices must be [V, 3], got {shape}')
    _nvertices(shape[0])
    return verts


def _mask(mask, nv, like, name='mask'):
    """bool [V] where `like` lives."""
    if on_device(like):
        import torch
        m = torch.as_tensor(mask, device=like.device)
        shape = tuple(m.shape)
        m = m.to(torch.bool).contiguous()
    else:
        m = np.asarray(mask.cpu() if on_device(mask) else mask)
        shape = m.shape
        m = np.ascontiguousarray(m, dtype=bool)
    if shape != (nv,):
        raise ValueError(f'{name} must have one entry per vertex ({nv}), got shape {shape}')
    return m


def _ctx(like):
    return f3d.default_context(like.device.index if on_device(like) else None)


def _counts(ctx, counts, work):
    """The one blocking readback of a device call: its output sizes; the IndexError of a bad vertex index is raised here."""
    host = counts.cpu()
    if int(host[2]):
        ctx.take_device_error(work.cuda_stream)
        raise IndexError('mesh: a triangle vertex index is outside [0, nvertices)')
    return int(host[0]), int(host[1])


# ------------------------------------------------------------------------------------------------ 1. vertex -> triangle map
class VertexTriangleMap:
    """What vertex_triangle_mapping returns: ``.csr`` = (offsets int64 [V + 1], tri int32 [3M], pos int8 [3M]), row v =
    ``offsets[v]:offsets[v + 1]``.  It unpacks as the reference's pair ``triangles_of_vertices, position_of_vertices`` (two lists
    of V lists of ints), which are built when first read."""

    def __init__(self, offsets, tri, pos):
        self.csr = (offsets, tri, pos)
        self._lists = None

    def _build(self):
        if self._lists is None:
            offsets, tri, pos = (a.cpu().numpy() if on_device(a) else a for a in self.csr)
            cuts = offsets[1:-1]
            self._lists = ([r.tolist() for r in np.split(tri, cuts)] if len(offsets) > 1 else [],
                           [r.tolist() for r in np.split(pos, cuts)] if len(offsets) > 1 else [])
        return self._lists

    @property
    def triangles_of_vertices(self):
        return self._build()[0]

    @property
    def position_of_vertices(self):
        return self._build()[1]

    def __len__(self):
        return 2

    def __getitem__(self, i):
        return self._build()[i]

    def __iter__(self):
        return iter(self._build())


def vertex_triangle_mapping(triangles, nvertices):
    """For every vertex the triangles that hold it and the corner they hold it at (reference :235-259), as a VertexTriangleMap.

    One stable radix sort of (vertex, slot) pairs, slot = 3 f + j: rows are in ascending slot order, the reference's append
    order; a face (v, v, w) lists f twice in row v, with positions 0 and 1."""
    tris, nv = _triangles(triangles), _nvertices(nvertices)
    ctx = _ctx(tris)
    if not on_device(tris):
        return VertexTriangleMap(*ctx.mesh_vertex_map(tris, nv))
    import torch
    dev, nt = tris.device, tris.shape[0]
    offsets = torch.empty(nv + 1, dtype=torch.int64, device=dev)
    tri = torch.empty(3 * nt, dtype=torch.int32, device=dev)
    pos = torch.empty(3 * nt, dtype=torch.int8, device=dev)
    counts = torch.empty(4, dtype=torch.int64, device=dev)
    with work_stream(dev) as work:
        ctx.mesh_vertex_map_dev(tris.data_ptr(), index_code(tris), nt, nv, offsets.data_ptr(), tri.data_ptr(), pos.data_ptr(), counts.data_ptr(),
                                work.cuda_stream)
        _counts(ctx, counts, work)
    return VertexTriangleMap(offsets, tri, pos)


# ------------------------------------------------------------------------------------------------ 2. remove faces
def remove_faces_by_vertices(nvertices, triangles, mask):
    """Drop every face that touches a masked vertex (reference :262-301) -> (not_removed bool [M], remaining_triangles [Q, 3] in
    the dtype of ``triangles``, oldids2newids int64 [V]).

    oldids2newids is the exclusive scan of ``~mask`` at the kept vertices and 0 at the removed ones; remaining_triangles =
    oldids2newids[triangles[not_removed]], face order kept."""
    tris, nv = _triangles(triangles), _nvertices(nvertices)
    m = _mask(mask, nv, tris)
    ctx = _ctx(tris)
    if not on_device(tris):
        return ctx.mesh_remove_faces(tris, nv, m)
    import torch
    dev, nt = tris.device, tris.shape[0]
    nr = torch.empty(nt, dtype=torch.bool, device=dev)
    rem = torch.empty((nt, 3), dtype=tris.dtype, device=dev)
    o2n = torch.empty(nv, dtype=torch.int64, device=dev)
    counts = torch.empty(4, dtype=torch.int64, device=dev)
    with work_stream(dev) as work:
        ctx.mesh_remove_faces_dev(tris.data_ptr(), index_code(tris), nt, nv, m.data_ptr(), nr.data_ptr(), rem.data_ptr(), o2n.data_ptr(),
                                  counts.data_ptr(), work.cuda_stream)
        q, _ = _counts(ctx, counts, work)
    return nr, rem[:q], o2n


# ------------------------------------------------------------------------------------------------ 3. keep faces
def keep_faces_by_vertices(vertices, triangles, mask):
    """Keep the faces with at least one masked corner and the vertices they use (reference :304-333) -> (remaining_vertices
    [P, 3], remaining_triangles [Q, 3]).

    The vertices are renumbered in order of first appearance over the kept faces (faces in order, corners 0, 1, 2), computed
    data-parallel from per-vertex slot minima, so the result does not depend on thread timing.

    Deviations from the reference: it returns arrays ([P, 3] in the dtype of ``vertices``, [Q, 3] in the dtype of ``triangles``;
    shape (0, 3) when empty) where the reference returns Python lists of rows; and it leaves the caller's ``triangles``
    untouched, where the reference renumbers the caller's array in place (its ``face`` is a view)."""
    tris = _triangles(triangles)
    verts = _vertices(vertices, tris)
    nv, nt = verts.shape[0], tris.shape[0]
    m = _mask(mask, nv, tris)
    ctx = _ctx(tris)
    if not on_device(tris):
        return ctx.mesh_keep_faces(verts, tris, m)
    import torch
    dev = tris.device
    ov = torch.empty((min(3 * nt, nv), 3), dtype=verts.dtype, device=dev)
    ot = torch.empty((nt, 3), dtype=tris.dtype, device=dev)
    counts = torch.empty(4, dtype=torch.int64, device=dev)
    with work_stream(dev) as work:
        ctx.mesh_keep_faces_dev(verts.data_ptr(), dtype_code(verts), nv, tris.data_ptr(), index_code(tris), nt, m.data_ptr(), ov.data_ptr(),
                                ot.data_ptr(), counts.data_ptr(), work.cuda_stream)
        p, q = _counts(ctx, counts, work)
    return ov[:p], ot[:q]


# ------------------------------------------------------------------------------------------------ 4. triangle clusters
def _mesh_parts(mesh):
    if hasattr(mesh, 'vertices') and hasattr(mesh, 'triangles'):
        return mesh.vertices, mesh.triangles
    vertices, triangles = mesh
    return vertices, triangles


def get_triangle_clusters(mesh, return_triangle_areas=False):
    """Connected triangle clusters (reference :360-375, Open3D's cluster_connected_triangles restated; parity with Open3D is
    unpinned) -> (triangle_clusters int32 [M], cluster_n_triangles int64 [P], cluster_area float64 [P]).

    ``mesh`` has ``.vertices`` and ``.triangles`` (get3DSeg.TriangleMesh) or is a ``(vertices, triangles)`` pair.  Two triangles
    are adjacent iff they share an ordered edge (min(a, b), max(a, b)) among their edges (0,1), (0,2), (1,2); sharing only a
    vertex does not connect them, a non-manifold edge connects all its triangles.  Clusters are numbered in ascending order of
    their lowest triangle.  A triangle's area is 0.5 * sqrt((cx*cx + cy*cy) + cz*cz), c = cross(p0 - p1, p0 - p2); a cluster's
    area is a fixed-shape float64 sum (two calls return identical bits).  ``return_triangle_areas`` appends the areas [M]."""
    vertices, triangles = _mesh_parts(mesh)
    tris = _triangles(triangles)
    verts = _vertices(vertices, tris)
    nv, nt = verts.shape[0], tris.shape[0]
    ctx = _ctx(tris)
    if not on_device(tris):
        return ctx.mesh_triangle_clusters(verts, tris, return_triangle_areas)
    import torch
    dev = tris.device
    cl = torch.empty(nt, dtype=torch.int32, device=dev)
    cn = torch.empty(nt, dtype=torch.int64, device=dev)
    ca = torch.empty(nt, dtype=torch.float64, device=dev)
    ta = torch.empty(nt, dtype=torch.float64, device=dev) if return_triangle_areas else None
    counts = torch.empty(4, dtype=torch.int64, device=dev)
    with work_stream(dev) as work:
        ctx.mesh_triangle_clusters_dev(verts.data_ptr(), dtype_code(verts), nv, tris.data_ptr(), index_code(tris), nt, cl.data_ptr(), cn.data_ptr(),
                                       ca.data_ptr(), None if ta is None else ta.data_ptr(), counts.data_ptr(), work.cuda_stream)
        p, _ = _counts(ctx, counts, work)
    out = (cl, cn[:p], ca[:p])
    return out + (ta,) if return_triangle_areas else out


# ------------------------------------------------------------------------------------------------ 5. clean_mesh
def clean_mesh(vertices, triangles, remove_mask=None, min_triangles=1, min_area=0.0):
    """Remove masked vertices and small fragments from a mesh, on the device from end to end (no reference counterpart) ->
    (new_vertices, new_triangles, kept_vertex_mask bool [V], kept_triangle_mask bool [M]).

    1. with ``remove_mask`` (bool [V]): drop every face that touches a masked vertex (remove_faces_by_vertices);
    2. cluster the surviving faces (get_triangle_clusters);
    3. drop the clusters with fewer than ``min_triangles`` triangles or with an area below ``min_area``;
    4. drop the vertices no face references, keeping vertex order, and renumber the faces.

    It is the composition of the functions above and equals it bit for bit; one blocking readback (the output sizes)."""
    tris = _triangles(triangles)
    verts = _vertices(vertices, tris)
    nv, nt = verts.shape[0], tris.shape[0]
    m = None if remove_mask is None else _mask(remove_mask, nv, tris, 'remove_mask')
    ctx = _ctx(tris)
    if not on_device(tris):
        return ctx.mesh_clean(verts, tris, m, min_triangles, min_area)
    import torch
    dev = tris.device
    nvs = torch.empty((nv, 3), dtype=verts.dtype, device=dev)
    nts = torch.empty((nt, 3), dtype=tris.dtype, device=dev)
    kv = torch.zeros(nv, dtype=torch.bool, device=dev)
    kt = torch.zeros(nt, dtype=torch.bool, device=dev)
    counts = torch.empty(4, dtype=torch.int64, device=dev)
    with work_stream(dev) as work:
        ctx.mesh_clean_dev(verts.data_ptr(), dtype_code(verts), nv, tris.data_ptr(), index_code(tris), nt, None if m is None else m.data_ptr(),
                           min_triangles, min_area, nvs.data_ptr(), nts.data_ptr(), kv.data_ptr(), kt.data_ptr(), counts.data_ptr(),
                           work.cuda_stream)
        q, p = _counts(ctx, counts, work)
    return nvs[:p], nts[:q], kv, kt


# ------------------------------------------------------------------------------------------------ 6. face labels
def label_faces(vertices, *args, **kwargs):
    """label_faces(vertices, triangles, K, wxyzs, translations, masks, max_depth=10, nclasses=133, threshold=0.5,
    filter_classes=None, return_votes=False), or with a mesh (``.vertices`` / ``.triangles`` as get3DSeg.TriangleMesh has them, or a
    ``(vertices, triangles)`` pair) in place of the first two arguments.

    Label the faces of a posed mesh from V masks (no reference counterpart): the mesh is rasterised into every view, every covered
    pixel votes for the triangle it sees with its mask label (f3d.h, f3d_vote_faces: the reference's voting direction, one row per
    triangle, a (triangle, label) pair counting once per view), and ``VotingSegmentation.segment`` picks the classes.  masks uint8
    [V,H,W].  Fragments beyond ``max_depth`` are dropped; triangles crossing the camera plane are skipped (no near-plane clipping).

    Returns int64 [M] classes (and float64 [M, nclasses+1] votes).  NumPy in, NumPy out; device tensors in (the triangles decide)
    give device tensors.  A label > nclasses on a covered pixel, or a vertex index outside [0, V), raises IndexError."""
    if isinstance(vertices, tuple) or (hasattr(vertices, 'vertices') and hasattr(vertices, 'triangles')):
        return _label_faces(*_mesh_parts(vertices), *args, **kwargs)
    return _label_faces(vertices, *args, **kwargs)


def _label_faces(vertices, triangles, K, wxyzs, translations, masks, max_depth=10, nclasses=133, threshold=0.5, filter_classes=None,
                 return_votes=False):
    tris = _triangles(triangles)
    if tris.shape[0] >= 1 << 31:
        raise ValueError('M must be below 2^31')
    verts = _vertices(vertices, tris)
    ctx = _ctx(tris)
    device = on_device(tris)
    if not device:
        masks = np.ascontiguousarray(masks.cpu() if on_device(masks) else masks, dtype=np.uint8)
    if masks.ndim != 3:
        raise ValueError('masks must be uint8 [V,H,W]')
    V, H, W = (int(x) for x in masks.shape)
    views = f3d.views_build(K, W, H, wxyzs, translations, max_depth)
    if len(views) != V:
        raise ValueError(f'{len(views)} poses for {V} masks')
    nt, ncols = tris.shape[0], nclasses + 1
    if not device:
        votes = np.zeros((nt, ncols))
        ctx.vote_faces(votes, verts, tris, views, masks, max_depth)
        cls = ctx.segment_votes(votes, nclasses, threshold, filter_classes)
        return (cls, votes) if return_votes else cls
    import torch
    dev = tris.device
    dmasks = torch.as_tensor(masks, device=dev)
    if dmasks.dtype != torch.uint8:
        raise ValueError(f'masks must be uint8, got {dmasks.dtype}')
    dmasks = dmasks.contiguous()
    with torch.cuda.device(dev), work_stream(dev) as work:
        dviews = upload(views, dev)
        votes = torch.zeros((nt, ncols), dtype=torch.float64, device=dev)
        cls = torch.empty(nt, dtype=torch.int64, device=dev)
        ctx.vote_faces_dev(verts.data_ptr(), dtype_code(verts), verts.shape[0], tris.data_ptr(), index_code(tris), nt, dviews.data_ptr(), V,
                           dmasks.data_ptr(), H, W, max_depth, votes.data_ptr(), ncols, 0, work.cuda_stream)
        ctx.segment_votes_dev(votes.data_ptr(), nt, ncols, nclasses, threshold, filter_classes, cls.data_ptr(), work.cuda_stream)
        ctx.take_device_error(work.cuda_stream)                               # the IndexErrors (synchronises)
    for t in (votes, cls):
        t.record_stream(torch.cuda.current_stream(dev))
    return (cls, votes) if return_votes else cls


# ------------------------------------------------------------------------------------------------ 7. face graph
def _is_mesh(x):
    return (isinstance(x, tuple) and len(x) == 2) or (hasattr(x, 'vertices') and hasattr(x, 'triangles'))


def _bad_index(ctx, work):
    ctx.take_device_error(work.cuda_stream)
    raise IndexError('mesh: a triangle vertex index is outside [0, nvertices)')


def face_normals(vertices, *args, **kwargs):
    """face_normals(vertices, triangles, return_centroids=False, return_areas=False), or with a mesh (``.vertices`` /
    ``.triangles``, or a ``(vertices, triangles)`` pair) in place of the first two arguments.

    Unit normals of the faces (f3d.h f3d_mesh_face_frames) -> float64 [M, 3]; with the flags a tuple (normals[, centroids float64
    [M, 3]][, areas float64 [M]]).  normal = c / |c|, c = cross(p0 - p1, p0 - p2), and (0, 0, 0) where |c| is 0 or not finite;
    areas equal get_triangle_clusters' triangle areas bit for bit."""
    if _is_mesh(vertices):
        return _face_normals(*_mesh_parts(vertices), *args, **kwargs)
    return _face_normals(vertices, *args, **kwargs)


def _face_normals(vertices, triangles, return_centroids=False, return_areas=False):
    tris = _triangles(triangles)
    verts = _vertices(vertices, tris)
    nv, nt = verts.shape[0], tris.shape[0]
    ctx = _ctx(tris)
    if not on_device(tris):
        nrm, cen, area = ctx.mesh_face_frames(verts, tris, return_centroids, return_areas)
    else:
        import torch
        dev = tris.device
        nrm = torch.empty((nt, 3), dtype=torch.float64, device=dev)
        cen = torch.empty((nt, 3), dtype=torch.float64, device=dev) if return_centroids else None
        area = torch.empty(nt, dtype=torch.float64, device=dev) if return_areas else None
        counts = torch.empty(4, dtype=torch.int64, device=dev)
        with work_stream(dev) as work:
            ctx.mesh_face_frames_dev(verts.data_ptr(), dtype_code(verts), nv, tris.data_ptr(), index_code(tris), nt, nrm.data_ptr(),
                                     None if cen is None else cen.data_ptr(), None if area is None else area.data_ptr(), counts.data_ptr(),
                                     work.cuda_stream)
            _counts(ctx, counts, work)
    out = (nrm,) + ((cen,) if return_centroids else ()) + ((area,) if return_areas else ())
    return out if len(out) > 1 else nrm


def _crease(max_angle):
    """cos of a crease angle given in degrees in [0, 180], or None."""
    if max_angle is None:
        return None
    angle = float(max_angle)
    if not 0.0 <= angle <= 180.0:
        raise ValueError(f'max_angle must be in [0, 180] degrees, got {max_angle}')
    return math.cos(math.radians(angle))


def face_adjacency(triangles, nvertices=None, vertices=None, max_angle=None, return_stats=False):
    """The faces' adjacency over shared edges as a CSR (f3d.h f3d_mesh_face_graph) -> (offsets int64 [M + 1], neighbours int32
    [nnz]), the pair smooth_votes, smooth_segment, split_into_instances and extract_planes take.  ``triangles`` may be a mesh
    (``.vertices`` / ``.triangles``, or a ``(vertices, triangles)`` pair).

    Row f lists, ascending, every other face that shares an edge (min, max) of the corner pairs (0,1), (0,2), (1,2) with f:
    get_triangle_clusters' edges, so the graph's connected components are its clusters; a non-manifold edge connects all its faces.
    With ``max_angle`` (degrees in [0, 180]; it needs ``vertices``) two faces stay adjacent only through an edge over which their
    dihedral angle is at most max_angle: s * dot(nf, ng) >= cos(max_angle), s = +1 for consistently wound neighbours and -1 for
    inconsistently wound ones, so flipped faces do not cut a flat sheet and a sheet folded back on itself is cut.  Without a
    max_angle ``nvertices`` alone is enough.  ``return_stats`` appends {'nonmanifold_edges', 'boundary_edges'}.

    Room for 3 M entries is allocated; a non-manifold mesh that needs more is run once more with the size the first run found."""
    if _is_mesh(triangles):
        mesh_vertices, triangles = _mesh_parts(triangles)
        vertices = mesh_vertices if vertices is None else vertices
    tris = _triangles(triangles)
    cos_crease = _crease(max_angle)
    gate = cos_crease is not None
    if gate and vertices is None:
        raise ValueError('face_adjacency: a max_angle needs the vertices')
    if vertices is None and nvertices is None:
        raise ValueError('face_adjacency: nvertices or vertices must be given')
    verts = None
    if vertices is not None:
        if gate:
            verts = _vertices(vertices, tris)
            shape = tuple(verts.shape)
        else:
            shape = tuple(vertices.shape) if hasattr(vertices, 'shape') else np.shape(vertices)
            if len(shape) != 2 or shape[1] != 3:
                raise ValueError(f'vertices must be [V, 3], got {shape}')
        if nvertices is not None and int(nvertices) != shape[0]:
            raise ValueError(f'nvertices is {nvertices}, vertices has {shape[0]} rows')
        nvertices = shape[0]
    nv, nt = _nvertices(nvertices), tris.shape[0]
    ctx = _ctx(tris)
    if not on_device(tris):
        offsets, nbrs, counts = ctx.mesh_face_graph(tris, nv, verts, cos_crease)
        if counts[0] > len(nbrs):
            offsets, nbrs, counts = ctx.mesh_face_graph(tris, nv, verts, cos_crease, offsets, np.empty(int(counts[0]), np.int32))
    else:
        import torch
        dev = tris.device
        offsets = torch.empty(nt + 1, dtype=torch.int64, device=dev)
        counts_dev = torch.empty(4, dtype=torch.int64, device=dev)
        cap = 3 * nt
        with work_stream(dev) as work:
            while True:
                nbrs = torch.empty(cap, dtype=torch.int32, device=dev)
                ctx.mesh_face_graph_dev(verts.data_ptr() if gate else None, dtype_code(verts) if gate else f3d.F64, nv, tris.data_ptr(),
                                        index_code(tris), nt, gate, cos_crease if gate else 0.0, offsets.data_ptr(), nbrs.data_ptr() if cap else None,
                                        cap, counts_dev.data_ptr(), work.cuda_stream)
                counts = counts_dev.cpu().numpy()                         # the one blocking readback (two for a non-manifold overflow)
                if counts[2]:
                    _bad_index(ctx, work)
                if counts[0] <= cap:
                    break
                cap = int(counts[0])
    adj = (offsets, nbrs[:int(counts[0])])
    return adj + ({'nonmanifold_edges': int(counts[1]), 'boundary_edges': int(counts[3])},) if return_stats else adj


def segment_faces_from_votes(votes, adj, nclasses=133, threshold=0.5, filter_classes=None, normals=None, angle=None, smooth_iterations=1,
                             self_weight=1.0, instance_classes=None, minimum_faces=1):
    """Face votes -> smoothed classes -> face instances: (classes int64 [M], ids [M], info).

    votes [M, ncols] (label_faces' ``return_votes``), adj the faces' CSR pair (face_adjacency).  With ``smooth_iterations`` > 0 the
    classes are ``voting.smooth_segment``'s over the graph (normals float64 [M, 3] with ``angle`` in degrees gate the sums, as there);
    with 0 they are ``segment``'s of the votes as they are: label_faces' own classes.  ``cv.split_into_instances(classes, adj,
    nclasses, instance_classes, minimum_faces)`` then numbers the connected same-class faces: its updated classes (instances smaller
    than minimum_faces become ``nclasses``), per-face ids and info list ('area' counts faces) are returned.  Device votes and graph
    stay on the device up to that split, which works on host arrays; its outputs are NumPy arrays."""
    from Fusion3DSeg.segUtils import cv, voting
    what = 'segment_faces_from_votes'
    shape = tuple(votes.shape) if hasattr(votes, 'shape') else np.shape(votes)
    if len(shape) != 2:
        raise ValueError(f'{what}: votes must be [M, ncols], got {shape}')
    m = shape[0]
    if not (isinstance(adj, tuple) and len(adj) == 2):
        raise TypeError(f'{what}: adj must be a CSR pair (offsets, neighbours)')
    if len(adj[0]) != m + 1:
        raise ValueError(f'{what}: votes has {m} rows, the adjacency offsets {len(adj[0])} entries ({m + 1} expected)')
    iterations, minimum_faces = int(smooth_iterations), int(minimum_faces)
    if iterations < 0:
        raise ValueError(f'{what}: smooth_iterations must not be negative, got {smooth_iterations}')
    if iterations > 0:
        classes = voting.smooth_segment(votes, adj, nclasses, threshold, filter_classes, False, normals, angle, None, None, self_weight,
                                        iterations)
    elif on_device(votes):
        import torch
        if votes.dtype != torch.float64:
            raise TypeError(f'{what}: device votes must be float64 without smoothing, got {votes.dtype}')
        dev = votes.device
        v = votes.contiguous()
        classes = torch.empty(m, dtype=torch.int64, device=dev)
        ctx = f3d.default_context(dev.index)
        with work_stream(dev) as work:
            ctx.segment_votes_dev(v.data_ptr(), m, shape[1], int(nclasses), float(threshold), filter_classes, classes.data_ptr(), work.cuda_stream)
            ctx.take_device_error(work.cuda_stream)
    else:
        classes = f3d.default_context().segment_votes(np.asarray(votes), nclasses, threshold, filter_classes)
    host = tuple(a.cpu().numpy() if on_device(a) else np.asarray(a) for a in adj)
    classes = classes.cpu().numpy() if on_device(classes) else classes
    _, ids, info, classes = cv.split_into_instances(classes, host, nclasses, instance_classes, minimum_faces)
    return classes, ids, info


def segment_faces(vertices, *args, **kwargs):
    """segment_faces(vertices, triangles, K, wxyzs, translations, masks, max_depth=10, nclasses=133, threshold=0.5,
    filter_classes=None, smooth_iterations=1, angle=None, max_angle=None, self_weight=1.0, instance_classes=None, minimum_faces=1,
    return_votes=False), or with a mesh in place of the first two arguments.

    The mesh route from masks to face instances: ``label_faces(..., return_votes=True)``, ``face_adjacency(..., max_angle=max_angle)``,
    ``face_normals`` when ``angle`` gates the smoothing, then ``segment_faces_from_votes`` -> (classes, ids, info) (+ the votes)."""
    if _is_mesh(vertices):
        return _segment_faces(*_mesh_parts(vertices), *args, **kwargs)
    return _segment_faces(vertices, *args, **kwargs)


def _segment_faces(vertices, triangles, K, wxyzs, translations, masks, max_depth=10, nclasses=133, threshold=0.5, filter_classes=None,
                   smooth_iterations=1, angle=None, max_angle=None, self_weight=1.0, instance_classes=None, minimum_faces=1, return_votes=False):
    tris = _triangles(triangles)
    _crease(max_angle)
    if int(smooth_iterations) < 0:
        raise ValueError(f'segment_faces: smooth_iterations must not be negative, got {smooth_iterations}')
    verts = _vertices(vertices, tris)
    _, votes = _label_faces(verts, tris, K, wxyzs, translations, masks, max_depth, nclasses, threshold, filter_classes, True)
    adj = face_adjacency(tris, vertices=verts, max_angle=max_angle)
    gated = angle is not None and int(smooth_iterations) > 0
    normals = _face_normals(verts, tris) if gated else None
    out = segment_faces_from_votes(votes, adj, nclasses, threshold, filter_classes, normals, angle if gated else None, smooth_iterations,
                                   self_weight, instance_classes, minimum_faces)
    return out + (votes,) if return_votes else out


# ------------------------------------------------------------------------------------------------ 8. host helpers
def bbox_axes(corners):
    """Origin, unit x and y axes and their lengths of an oriented box from its 8 corners in Open3D's order (reference :336-357):
    the x axis is the longest of the three edges at corner 0, the y axis the middle one; the origin is the midpoint of corners
    0 and 3.  NumPy on the host (a handful of vectors)."""
    edges = corners[1:4] - corners[0][None, :]
    lengths = np.linalg.norm(edges, axis=-1)
    by_length = np.argsort(lengths)
    i, li = edges[by_length[2]], lengths[by_length[2]]
    j, lj = edges[by_length[1]], lengths[by_length[1]]
    origin = (corners[0] + corners[3]) / 2
    return origin, i / li, j / lj, li, lj


def one_to_all_angles(vec1, vec2):
    """Angles in degrees between every vector of vec2 [M, 3] and every vector of vec1 [N, 3] -> [M, N] (reference :455-467).
    Both arguments are normalised IN PLACE, as in the reference.  NumPy on the host."""
    vec1 /= np.linalg.norm(vec1, axis=1)[:, None]
    vec2 /= np.linalg.norm(vec2, axis=1)[:, None]
    cos = np.sum(vec1[None, :, :] * vec2[:, None, :], axis=2)
    return np.rad2deg(np.arccos(cos))
