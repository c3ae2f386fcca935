"""Drop-in surface of the reference's Fusion3DSeg/fusion.py for the hot path.

``project_vote_argmax`` is the forward "project every point into every view, sample the mask, vote, segment" composition
the north star names (last row); it runs as ONE fused HIP kernel.

``Fusion`` is the reference's class (fusion.py:80-407): per frame, ``fuse`` culls the fused cloud against the frame's
frustum and projects the survivors (rows a3, a4, a2 -- here ONE launch of the single-view HIP kernel per frame), then
greedily matches depth patches to those points and down-samples what is left (``patch_downsample``).  The greedy part is
a chain of data-dependent decisions (every match removes pixels from later candidates); HIP kernels settle it in data-parallel
rounds with the reference's outcome.  The shuffles are drawn from NumPy's global generator at the same places, so a seeded run
reproduces the reference's output (tests/golden/fuse.npz).  There is one frame loop, ``_DeviceFusion.run``, with the cloud
resident on the GPU: ``fuse_device`` returns its tensors, ``fuse`` is the drop-in with NumPy in and out.
"""
import contextlib
import pickle
import time
from fractions import Fraction
from pathlib import Path

import numpy as np

import f3d
from f3d.tensors import dtype_code, index_code, on_device, torch_device, upload, work_stream


def parse_rts(rts):
    """Camera pickle -> (scaled intrinsics, depth w, depth h, wxyz quaternions, translations) (reference :67-77)."""
    with open(rts, 'rb') as fp:
        d = pickle.load(fp)
    h, w, *_ = d['Depth_res']
    return d['intrinsicScaled'], w, h, d['odo_wxyz'][:, [3, 0, 1, 2]], d['odo_xyz']


def project_vote_argmax(points, K, wxyzs, translations, masks, max_depth=10, nclasses=133, threshold=0.5,
                        filter_classes=None, return_votes=False):
    """Label every point from V posed masks in one pass on the GPU.

    Per view j (reference call sites): the 5 frustum planes of ``Fusion.fuse`` (fusion.py:254-258) ->
    ``point_inside_polyhedra`` (:260) -> ``points2pixel`` (:266) -> samples outside the mask are dropped ->
    ``votes[point, mask_j[v, u]] += 1`` -> ``VotingSegmentation.segment(threshold, filter_classes)``.

    points [N,3] float64 (or float32), K [3,3], wxyzs [V,4] camera->world (w,x,y,z), translations [V,3],
    masks uint8 [V,H,W] (H, W also define the frustum).  Returns int64 [N] (and uint16 [N, nclasses+1] votes).
    """
    masks = np.ascontiguousarray(masks, dtype=np.uint8)
    V, H, W = masks.shape
    views = f3d.views_build(K, W, H, wxyzs, translations, max_depth)
    return f3d.default_context().project_vote_argmax(points, views, masks, nclasses, threshold, filter_classes, return_votes)


def _device_cloud(torch, dev, points):
    """points as a contiguous float64 / float32 [N,3] tensor on `dev` (float32 stays float32, everything else is widened)."""
    pts = points.to(dev)
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise ValueError(f'points must be [N,3], got {tuple(pts.shape)}')
    return (pts if pts.dtype == torch.float32 else pts.to(torch.float64)).contiguous()


def render_lookups(points, K, wxyzs, translations, hw, max_depth=10, splat=0):
    """Per-view depth buffers and ``uv2pt`` lookups of a posed cloud, rendered on the GPU as a point-splat z-buffer.

    For clouds that come without depth frames (an RTAB-Map export, a LiDAR scan, mesh vertices, a reloaded fused cloud) this
    gives what ``Fusion.fuse`` writes per frame (reference fusion.py:105-111, :326-327): pixel -> the point a camera sees there,
    -1 for none.  The lookups feed ``VotingSegmentation`` / ``f3d.Context.vote_uv2pt_batch`` as they are.

    Per view the samples are those of ``project_vote_argmax`` (5 frustum planes, ``points2pixel``, inside the image) with a
    normal positive float32 depth; a point covers the (2 splat + 1)^2 pixels around its pixel; per pixel the nearest point by
    float32 depth wins, ties go to the lowest index (f3d.h, f3d_render_lookups).  ``hw`` = (H, W) of the images.

    Returns depth float32 [V,H,W] (+inf = empty) and uv2pt int32 [V,H*W].  NumPy in, NumPy out; a torch device tensor for
    ``points`` gives device tensors, ordered with torch's current stream, with no host round trip of the cloud."""
    H, W = (int(x) for x in hw)
    views = f3d.views_build(K, W, H, wxyzs, translations, max_depth)
    ctx = f3d.default_context()
    if not on_device(points):
        return ctx.render_lookups(points, views, H, W, splat)
    torch, dev = torch_device(ctx, 'render_lookups')
    pts = _device_cloud(torch, dev, points)
    with torch.cuda.device(dev), work_stream(dev) as work:
        dviews = upload(views, dev)
        depth = torch.empty((len(views), H, W), dtype=torch.float32, device=dev)
        uv2pt = torch.empty((len(views), H * W), dtype=torch.int32, device=dev)
        ctx.render_lookups_dev(pts.data_ptr(), dtype_code(pts), len(pts), dviews.data_ptr(), len(views), H, W, splat, depth.data_ptr(),
                               uv2pt.data_ptr(), work.cuda_stream)
    for t in (depth, uv2pt):                                                  # allocated on the work stream, handed to the caller's
        t.record_stream(torch.cuda.current_stream(dev))
    return depth, uv2pt


def project_vote_argmax_visible(points, K, wxyzs, translations, masks, max_depth=10, nclasses=133, threshold=0.5,
                                filter_classes=None, return_votes=False, splat=1, depth_tol=0.05):
    """``project_vote_argmax`` with an occlusion test: a point votes in a view only when that view sees it.

    The cloud is rendered into every view as for ``render_lookups`` (``splat``); a sample votes iff its float32 depth is within
    ``depth_tol`` of the nearest depth rendered into its pixel (f3d.h, f3d_vote_visible), so a point behind a wall no longer
    collects the wall's label from the cameras in front of it.  ``depth_tol`` defaults to the project's fusion radius
    (``Fusion.fuse``); with ``depth_tol=inf`` the votes are those of ``project_vote_argmax``.  A label > nclasses on a visible
    sample raises IndexError.

    Returns int64 [N] (and float64 [N, nclasses+1] votes, the layout of ``VotingSegmentation``).  NumPy in, NumPy out; torch device
    tensors for ``points`` and ``masks`` give device tensors, ordered with torch's current stream, with no host round trip."""
    ctx = f3d.default_context()
    device = on_device(points) or on_device(masks)
    if not device:
        masks = np.ascontiguousarray(masks, dtype=np.uint8)
    if masks.ndim != 3:
        raise ValueError('masks must be uint8 [V,H,W]')
    V, H, W = (int(x) for x in masks.shape)
    views = f3d.views_build(K, W, H, wxyzs, translations, max_depth)
    if len(views) != V:
        raise ValueError(f'{len(views)} poses for {V} masks')
    if not device:
        votes = np.zeros((len(points), nclasses + 1))
        ctx.vote_visible(votes, points, views, masks, splat, depth_tol)
        cls = ctx.segment_votes(votes, nclasses, threshold, filter_classes)
        return (cls, votes) if return_votes else cls
    torch, dev = torch_device(ctx, 'project_vote_argmax_visible')
    to_t = lambda a: a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))   # noqa: E731
    pts = _device_cloud(torch, dev, to_t(points))
    dmasks = to_t(masks).to(dev)
    if dmasks.dtype != torch.uint8:
        raise ValueError(f'masks must be uint8, got {dmasks.dtype}')
    dmasks = dmasks.contiguous()
    with torch.cuda.device(dev), work_stream(dev) as work:
        dviews = upload(views, dev)
        votes = torch.zeros((len(pts), nclasses + 1), dtype=torch.float64, device=dev)
        cls = torch.empty(len(pts), dtype=torch.int64, device=dev)
        ctx.vote_visible_dev(pts.data_ptr(), dtype_code(pts), len(pts), dviews.data_ptr(), V, dmasks.data_ptr(), H, W, splat, depth_tol,
                             votes.data_ptr(), nclasses + 1, 0, work.cuda_stream)
        ctx.segment_votes_dev(votes.data_ptr(), len(pts), nclasses + 1, nclasses, threshold, filter_classes, cls.data_ptr(), work.cuda_stream)
        ctx.take_device_error(work.cuda_stream)                               # the IndexError of a label > nclasses (synchronises)
    for t in (votes, cls):
        t.record_stream(torch.cuda.current_stream(dev))
    return (cls, votes) if return_votes else cls


def _device_mesh(torch, dev, vertices, triangles):
    """(vertices float64 / float32 [V,3], triangles int64 / int32 [M,3]) as contiguous tensors on `dev`."""
    to_t = lambda a: a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))   # noqa: E731
    verts = _device_cloud(torch, dev, to_t(vertices))
    tris = to_t(triangles).to(dev)
    if tris.dtype not in (torch.int32, torch.int64):
        raise TypeError(f'triangles must be int32 or int64, got {tris.dtype}')
    if tris.dim() != 2 or tris.shape[1] != 3:
        raise ValueError(f'triangles must be [M,3], got {tuple(tris.shape)}')
    return verts, tris.contiguous()


def render_mesh_lookups(vertices, triangles, K, wxyzs, translations, hw, max_depth=10):
    """Per-view depth buffers and pixel -> triangle lookups of a posed triangle mesh, rasterised on the GPU.

    What ``render_lookups`` gives for a cloud, from a watertight surface: no splat size to choose, no gaps for the surface behind to
    show through.  A pixel is covered when its centre lies inside a triangle's projection (edges inclusive, evaluated so that the two
    triangles sharing an edge never both miss it); the depth is perspective-correct; per pixel the nearest float32 depth wins, ties
    go to the lowest triangle index; fragments beyond ``max_depth`` are dropped (f3d.h, f3d_render_mesh_lookups).  There is no
    near-plane clipping: a triangle that crosses the camera plane is skipped and counted in ``straddling`` -- subdivide coarse meshes.

    Returns depth float32 [V,H,W] (+inf = empty), uv2tri int32 [V,H*W] (-1 = empty), straddling int64 [V].  NumPy in, NumPy out;
    torch device tensors for the mesh give device tensors, ordered with torch's current stream."""
    H, W = (int(x) for x in hw)
    views = f3d.views_build(K, W, H, wxyzs, translations, max_depth)
    ctx = f3d.default_context()
    if not (on_device(vertices) or on_device(triangles)):
        return ctx.render_mesh_lookups(vertices, triangles, views, H, W, max_depth)
    torch, dev = torch_device(ctx, 'render_mesh_lookups')
    verts, tris = _device_mesh(torch, dev, vertices, triangles)
    with torch.cuda.device(dev), work_stream(dev) as work:
        dviews = upload(views, dev)
        depth = torch.empty((len(views), H, W), dtype=torch.float32, device=dev)
        uv2tri = torch.empty((len(views), H * W), dtype=torch.int32, device=dev)
        straddling = torch.empty(len(views), dtype=torch.int64, device=dev)
        ctx.render_mesh_lookups_dev(verts.data_ptr(), dtype_code(verts), len(verts), tris.data_ptr(), index_code(tris), len(tris), dviews.data_ptr(),
                                    len(views), H, W, max_depth, depth.data_ptr(), uv2tri.data_ptr(), straddling.data_ptr(), work.cuda_stream)
        ctx.take_device_error(work.cuda_stream)                               # the IndexError of a bad vertex index (synchronises)
    for t in (depth, uv2tri, straddling):
        t.record_stream(torch.cuda.current_stream(dev))
    return depth, uv2tri, straddling


def project_vote_argmax_occluded(points, vertices, triangles, K, wxyzs, translations, masks, max_depth=10, nclasses=133, threshold=0.5,
                                 filter_classes=None, return_votes=False, depth_tol=0.05):
    """``project_vote_argmax_visible`` with a triangle mesh of the scene as the occluder instead of a splat of the cloud itself.

    The mesh is rasterised into every view as for ``render_mesh_lookups``; a point's sample votes iff its float32 depth is within
    ``depth_tol`` of the mesh depth of its pixel, and a pixel no triangle covers hides nothing (f3d.h, f3d_vote_visible_mesh).  A mesh
    neither leaks between the cloud's points nor fattens silhouettes.  With ``depth_tol=inf`` the votes are those of
    ``project_vote_argmax``.  A label > nclasses on a visible sample, or a vertex index outside the mesh, raises IndexError.

    Returns int64 [N] (and float64 [N, nclasses+1] votes).  NumPy in, NumPy out; torch device tensors for ``points``, ``masks`` or the
    mesh give device tensors, ordered with torch's current stream, with no host round trip."""
    ctx = f3d.default_context()
    device = on_device(points) or on_device(masks) or on_device(vertices) or on_device(triangles)
    if not device:
        masks = np.ascontiguousarray(masks, dtype=np.uint8)
    if masks.ndim != 3:
        raise ValueError('masks must be uint8 [V,H,W]')
    V, H, W = (int(x) for x in masks.shape)
    views = f3d.views_build(K, W, H, wxyzs, translations, max_depth)
    if len(views) != V:
        raise ValueError(f'{len(views)} poses for {V} masks')
    if not device:
        votes = np.zeros((len(points), nclasses + 1))
        ctx.vote_visible_mesh(votes, points, vertices, triangles, views, masks, max_depth, depth_tol)
        cls = ctx.segment_votes(votes, nclasses, threshold, filter_classes)
        return (cls, votes) if return_votes else cls
    torch, dev = torch_device(ctx, 'project_vote_argmax_occluded')
    to_t = lambda a: a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))   # noqa: E731
    pts = _device_cloud(torch, dev, to_t(points))
    verts, tris = _device_mesh(torch, dev, vertices, triangles)
    dmasks = to_t(masks).to(dev)
    if dmasks.dtype != torch.uint8:
        raise ValueError(f'masks must be uint8, got {dmasks.dtype}')
    dmasks = dmasks.contiguous()
    with torch.cuda.device(dev), work_stream(dev) as work:
        dviews = upload(views, dev)
        votes = torch.zeros((len(pts), nclasses + 1), dtype=torch.float64, device=dev)
        cls = torch.empty(len(pts), dtype=torch.int64, device=dev)
        ctx.vote_visible_mesh_dev(pts.data_ptr(), dtype_code(pts), len(pts), verts.data_ptr(), dtype_code(verts), len(verts), tris.data_ptr(),
                                  index_code(tris), len(tris), dviews.data_ptr(), V, dmasks.data_ptr(), H, W, max_depth, depth_tol,
                                  votes.data_ptr(), nclasses + 1, 0, work.cuda_stream)
        ctx.segment_votes_dev(votes.data_ptr(), len(pts), nclasses + 1, nclasses, threshold, filter_classes, cls.data_ptr(), work.cuda_stream)
        ctx.take_device_error(work.cuda_stream)                               # the IndexErrors (synchronises)
    for t in (votes, cls):
        t.record_stream(torch.cuda.current_stream(dev))
    return (cls, votes) if return_votes else cls


def radius_adjacency(points, ds_radius, as_csr=False):
    """The adjacency ``Fusion.save_data`` stores in fusion/adj.pkl (reference :373-377):
    ``KDTree(points).query_radius(points, r=2 * ds_radius)``, built on the GPU with a uniform grid.

    Returns what the reference pickles -- an object array of int64 index arrays, one per point, itself included -- or,
    with ``as_csr``, the (offsets int64 [N+1], neighbours int32 [E]) pair that ``split_into_instances`` also accepts
    (no Python objects, what a 10M-point cloud wants).  Row order: by grid cell, then ascending index (sklearn's order is
    the tree traversal's, unspecified)."""
    if ds_radius is None:
        return None                                                            # reference :371-372
    offs, nbrs = f3d.default_context().radius_graph(points, 2 * ds_radius)
    if as_csr:
        return offs, nbrs
    out = np.empty(len(offs) - 1, dtype=object)
    wide = nbrs.astype(np.int64)
    for i in range(len(out)):
        out[i] = wide[offs[i]:offs[i + 1]]
    return out


class FrameData:
    """Per-frame pickles listed by the tof pickle (reference :17-60): item i -> (frame name, world points [h*w,3], normals,
    colours, validity mask)."""

    def __init__(self, tof, point_range=None, decimation=1, depth_hw=(256, 192)):
        self.point_range, self.decimation, self.depth_hw = point_range, decimation, depth_hw
        root = Path(str(tof).split('PointcloudMergeResults')[0])
        with open(tof, 'rb') as fp:
            self.tofcamedata = [root / entry['fileName'].strip() for entry in pickle.load(fp)]

    def __len__(self):
        return len(self.tofcamedata)

    @staticmethod
    def get_valid(points, mindist, maxdist):
        depth = points[:, 2]
        return (depth > mindist) & (depth <= maxdist)

    def __getitem__(self, i):
        with open(self.tofcamedata[i], 'rb') as fp:
            d = pickle.load(fp)
        pts = np.array(d['modPoints'])
        if self.point_range is None:
            ok = np.ones(len(pts), bool)
        else:
            ok = self.get_valid(np.array(d['orgPoints']), self.point_range[0], self.point_range[1])
        if self.decimation > 1:                                               # keep one pixel per decimation x decimation block
            drop = np.ones(self.depth_hw, bool)
            drop[::self.decimation, ::self.decimation] = False
            ok[drop.reshape(-1)] = False
        return str(d['frameNumber']), pts, np.array(d['modSurfaceNormals']), np.array(d['orgColorPoints']), ok


def _row_norms(rows):
    """np.linalg.norm(v) of every row, with the bits of the reference's per-vector call: for a 1-D vector NumPy takes
    sqrt(v.dot(v)), and that dot is BLAS ddot (FMA, kernel dependent), unlike the axis=-1 form.  ``np.vecdot`` runs the same
    kernel on the builds seen so far; it is used for large inputs only after it reproduced the per-vector results on the first
    rows of THIS input."""
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    head = min(len(rows), 1024)
    sq = np.empty(len(rows))
    sq[:head] = [v.dot(v) for v in rows[:head]]
    if head < len(rows):
        fast = getattr(np, 'vecdot', None)
        if fast is not None and np.array_equal(fast(rows[:head], rows[:head]), sq[:head]):
            sq[head:] = fast(rows[head:], rows[head:])
        else:
            sq[head:] = [v.dot(v) for v in rows[head:]]
    return np.sqrt(sq)


def _fma(a, b, c):
    """a * b + c rounded once (exact rational arithmetic, then one rounding to float64)."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def _norm_probe_vectors(n=64, seed=20260917):
    """Vectors on which the plain order (x*x + y*y) + z*z and the FMA chain fma(z,z, fma(y,y, x*x)) round differently."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        x, y, z = (float(c) for c in rng.normal(size=3))
        if (x * x + y * y) + z * z != _fma(z, z, _fma(y, y, x * x)):
            out.append((x, y, z))
    return np.array(out)


def _classify_dot(values, vectors):
    """Which order produced `values` = v.dot(v) of every probe vector: f3d.NORM_FMA, f3d.NORM_PLAIN, or f3d.NORM_HOST (neither)."""
    values = np.asarray(values, np.float64)
    fma = np.array([_fma(z, z, _fma(y, y, x * x)) for x, y, z in vectors])
    plain = (vectors[:, 0] * vectors[:, 0] + vectors[:, 1] * vectors[:, 1]) + vectors[:, 2] * vectors[:, 2]
    if np.array_equal(values, fma):
        return f3d.NORM_FMA
    if np.array_equal(values, plain):
        return f3d.NORM_PLAIN
    return f3d.NORM_HOST


def _probe_norm_mode(dot=None):
    """The order in which this process's NumPy takes the 1-D ``v.dot(v)`` of ``_row_norms`` (BLAS ddot: the kernel OpenBLAS picks for
    the CPU decides it), as the mode the fusion kernels take: both that dot and ``np.vecdot`` (which ``_row_norms`` uses for long
    inputs) must agree with one order, else NORM_HOST (the host normalises).  ``dot``: classify that function instead."""
    vectors = _norm_probe_vectors()
    if dot is not None:
        return _classify_dot([dot(v) for v in vectors], vectors)
    mode = _classify_dot([v.dot(v) for v in vectors], vectors)
    fast = getattr(np, 'vecdot', None)
    if fast is not None and _classify_dot(fast(vectors, vectors), vectors) != mode:
        return f3d.NORM_HOST
    return mode


_NORM_MODE = []


def _norm_mode():
    """``_probe_norm_mode()``, probed once per process."""
    if not _NORM_MODE:
        _NORM_MODE.append(_probe_norm_mode())
    return _NORM_MODE[0]


def _mergeable(seed_pt, seed_normal, cand_pts, cand_normals, max_distance, min_cosine):
    """The reference's merge criterion (:165-170, :223-228): closer than max_distance AND normals within the angle."""
    near = np.linalg.norm(cand_pts - seed_pt[None, :], axis=-1) < max_distance
    return near & (np.einsum('ij, j -> i', cand_normals, seed_normal) > min_cosine)


def _unusable(points, normals, min_cosine):
    """Pixels that would not accept themselves as a seed (zero / NaN normal: np.einsum's dot, the order of _mergeable) or hold a
    non-finite point; the reference then averages an empty set and leaves the pixel to later seeds."""
    own_cos = np.einsum('ij,ij->i', normals, normals)
    return ~((own_cos > min_cosine) & np.isfinite(points).all(axis=1))


class Fusion:
    def __init__(self, tof, rts, point_range=None, decimation=1, save_lookups=True):
        K, w, h, wxyzs, translations = parse_rts(rts)
        lookup_dir = None
        if save_lookups:
            lookup_dir = Path(str(tof).split('PointcloudMergeResults')[0]) / 'fusion' / 'uv2pt'
            lookup_dir.mkdir(exist_ok=True, parents=True)
        self._setup(K, w, h, wxyzs, translations, FrameData(tof, point_range, decimation, (h, w)), save_lookups, lookup_dir)

    @classmethod
    def from_frames(cls, K, w, h, wxyzs, translations, frames, lookup_dir=None, lookup_sink=None):
        """The same object without the file readers: ``frames[i]`` = (name, points, normals, colours, valid).  Per-frame
        lookups go to ``lookup_dir`` (as .npy, like the reference) and/or to ``lookup_sink(name, uv2pt)``: a NumPy int32 [h*w] from
        ``fuse``; from ``fuse_device`` a fresh int32 CUDA tensor [h*w], what ``f3d_vote_uv2pt_batch_dev`` consumes (complete once
        ``fuse_device`` has returned, in the order of the caller's stream).  ``fuse_device`` also accepts frames of torch device
        tensors."""
        self = object.__new__(cls)
        self._setup(K, w, h, wxyzs, translations, frames, lookup_dir is not None or lookup_sink is not None, lookup_dir)
        self._lookup_sink = lookup_sink
        return self

    def _setup(self, K, w, h, wxyzs, translations, frames, save_lookups, lookup_dir):
        self.K, self.w, self.h = np.asarray(K, np.float64), int(w), int(h)
        self.xyzws, self.translations = np.asarray(wxyzs, np.float64), np.asarray(translations, np.float64)   # (w,x,y,z): quirk Q9
        self.frames, self.nframes, self.npts = frames, len(frames), int(h) * int(w)
        self.ds_radius, self.ds_angle = None, None
        self.eyes, self.lookats, self.frustum_spoke_origins, self.frutsum_face_normals = self._get_frustum_data(
            self.K, self.w, self.h, self.xyzws, self.translations, np.arange(self.nframes))
        self.pcdimg = np.arange(self.npts).reshape(self.h, self.w)
        self.pt2u = (np.arange(self.npts) % self.w).astype(np.int32)
        self.pt2v = (np.arange(self.npts) // self.w).astype(np.int32)
        self.save_lookups, self.uv2pt_dir, self._lookup_sink = save_lookups, lookup_dir, None

    @staticmethod
    def _get_frustum_data(K, w, h, xyzws, translations, frame_ids=None):
        """eyes [F,3], lookats [F,3], spoke origins [F,4,3], face normals [F,4,3] (reference :119-132), computed by the
        library's host code.  With ``frame_ids`` the reference indexes the eyes twice for the spoke origins; kept."""
        eyes, lookats, normals = f3d.frustum_data(K, w, h, xyzws, translations)
        ids = np.arange(len(eyes)) if frame_ids is None else np.asarray(frame_ids)
        eyes, lookats = eyes[ids], lookats[ids]
        return eyes, lookats, np.repeat(eyes[ids][:, None, :], 4, axis=1), normals[ids]

    @classmethod
    def patch_downsample(cls, points, normals, colors, height, width, stride, max_distance, min_cosine,
                         pcdimg, pt2u, pt2v, non_merged=None):
        """One frame -> representative points (reference :134-210): visit the pixels in a random order; a pixel that is still
        free becomes a seed, absorbs the free pixels of its (stride x stride) window that satisfy the merge criterion and
        is replaced by their mean.  Returns (points, normals, colours, uv2pt int32 [h*w] with -1 = none, merge counts).

        "Still free when visited" is the only sequential coupling, and it is local: pixel p is a seed iff no EARLIER seed whose
        window covers it accepts it.  The frame goes through the down-sampling step of ``fuse`` (``_DeviceFusion.downsample``) into an
        empty resident cloud: HIP kernels settle the seeds in a few data-parallel rounds, add the members of every seed in the
        reference's order and write the new rows in visiting order."""
        order = np.arange(len(points))
        np.random.shuffle(order)                                              # the global generator, as the reference (:172)
        free = np.ones((height, width), dtype=bool) if non_merged is None else non_merged   # updated in place, like the reference
        half = stride // 2
        points, normals = np.asarray(points, np.float64), np.asarray(normals, np.float64)
        flat_free = free.reshape(-1)
        if len(points) != height * width or not (max_distance > 0) or (flat_free & _unusable(points, normals, min_cosine)).any():
            # a free pixel that would not accept itself: keep the reference's literal order of events for such frames
            return cls._patch_downsample_sequential(order, points, normals, colors, height, width, half, max_distance, min_cosine,
                                                    pcdimg, pt2u, pt2v, free)
        with _DeviceFusion.on_stream('Fusion.patch_downsample', height, width, pcdimg, pt2u, pt2v) as df:
            frame = df.frame((None, points, normals, colors, flat_free))
            df.free.copy_(frame[4])
            df.order_stage.numpy()[:] = order
            uv2pt = df.torch.full((height * width,), -1, dtype=df.torch.int32, device=df.dev)
            df.downsample(order, frame, half, max_distance, min_cosine, False, height * width, 0, uv2pt)
            k = int(df.count_dev.item())
            out_p, out_n, out_c, n_take = (t[:k].cpu().numpy() for t in df.cloud[:4])
            df.consume(free)
            uv2pt = uv2pt.cpu().numpy()
        if not k:
            return np.array([]), np.array([]), np.array([]), uv2pt, np.array([])
        return out_p, out_n, out_c, uv2pt, n_take

    @staticmethod
    def _patch_downsample_sequential(order, points, normals, colors, height, width, half, max_distance, min_cosine, pcdimg, pt2u, pt2v, free):
        """The literal order of events of reference :176-208 (used only for frames the data-parallel form does not cover)."""
        uv2pt = np.full(height * width, -1, np.int32)
        left = height * width
        out_p, out_n, out_c, out_m = [], [], [], []
        for seed in order:
            su, sv = pt2u[seed], pt2v[seed]
            if not free[sv, su]:
                continue
            if not left:
                break
            win = np.s_[max(0, sv - half):sv + half + 1, max(0, su - half):su + half + 1]
            cand = pcdimg[win].reshape(-1)[free[win].reshape(-1)]           # row-major window order, free pixels only
            take = _mergeable(points[seed], normals[seed], points[cand], normals[cand], max_distance, min_cosine)
            members = cand[take]
            left -= take.sum()
            out_p.append(np.mean(points[cand][take], axis=0))
            out_c.append(np.mean(colors[cand][take], axis=0))
            nsum = np.mean(normals[cand][take], axis=0)
            out_n.append(nsum / np.linalg.norm(nsum))
            out_m.append(take.sum())
            uv2pt[members] = len(out_m) - 1
            free[pt2v[members], pt2u[members]] = False
        return np.array(out_p), np.array(out_n), np.array(out_c), uv2pt, np.array(out_m)

    def _frame_view(self, j, max_depth):
        return f3d.views_build(self.K, self.w, self.h, self.xyzws[j:j + 1], self.translations[j:j + 1], max_depth)[0]

    def fuse(self, radius=0.05, angle=10, stride=None, max_depth=10, skip=1, verbose=False):
        """Fuse + down-sample the frames into one sparse cloud (reference :212-324) -> (points, normals, colours float64 [M,3],
        nmerges int64 [M], occurences uint32 [M]) as NumPy arrays; per-frame ``uv2pt`` lookups (NumPy int32 [h*w]) are saved when
        requested.  The loop of ``fuse_device`` with NumPy in and out: like the reference, it consumes the ``valid`` masks of NumPy
        frames in place (written through ``valid.reshape(h, w)`` after every fused frame)."""
        with _DeviceFusion.on_stream('Fusion.fuse', self.h, self.w, self.pcdimg, self.pt2u, self.pt2v) as df:
            out = tuple(t.cpu().numpy() for t in df.run(self, radius, angle, stride, max_depth, skip, verbose, host_io=True))
        if not len(out[0]):                                                   # no valid pixel anywhere: patch_downsample's empty arrays
            return np.array([]), np.array([]), np.array([]), np.array([]), np.ones(0, np.uint32)
        return out

    def fuse_device(self, radius=0.05, angle=10, stride=None, max_depth=10, skip=1, verbose=False):
        """``fuse`` with the cloud and the lookups left on the GPU -> (points, normals, colours float64 [M,3], nmerges int64 [M],
        occurences uint32 [M]) as torch tensors on the context's device, the bits ``fuse`` returns on the same frames under the same
        seeded global NumPy generator (lookups and the generator's final state included).

        Frames: ``self.frames[i]`` may hold NumPy arrays (uploaded once per frame through a pinned staging buffer) or torch device
        tensors (points / normals / colours float64 [h*w,3] contiguous, valid bool or uint8 [h*w]), used in place.  The frame's
        ``valid`` is copied into a free-pixel buffer of this call and never written; ``fuse`` instead consumes the masks of NumPy
        frames in place.  Lookups: ``lookup_dir`` gets the same .npy bytes as ``fuse`` writes; ``lookup_sink(name, uv2pt)`` gets a
        fresh int32 device tensor [h*w] per frame (what ``f3d_vote_uv2pt_batch_dev`` consumes).

        Work goes on the caller's current torch stream (a side stream ordered behind it when that is the null stream); the caller's
        stream waits for it before this returns.  Per frame the host still sees: the shuffle (drawn on the host from the global
        generator, h*w int64 uploaded, drawn while the GPU matches); two small readbacks (hits / valid pixels / cloud rows after the
        projection, free pixels / sequential flag after the matching); for NumPy frames the frame upload and the free mask, on which
        the host takes patch_downsample's own test for the sequential loop; the per-round counter of the seed resolution; the
        lookups when written to disk.  Nothing per seed comes back, except on the two host paths counted in
        ``self.fuse_device_stats`` (``fuse`` fills it too): frames patch_downsample hands to its sequential loop
        ('sequential_frames'), and rows normalised on the host when this process's BLAS dot matches neither kernel order
        ('host_normalised')."""
        with _DeviceFusion.on_stream('Fusion.fuse_device', self.h, self.w, self.pcdimg, self.pt2u, self.pt2v) as df:
            out = df.run(self, radius, angle, stride, max_depth, skip, verbose)
            if df.stream != df.caller:
                for t in out:
                    t.record_stream(df.caller)
        return out

    def reconstruct_mesh(self, voxel, lo=None, dims=None, trunc=None, max_weight=64, max_depth=10, min_weight=1, skip=1, points=None, colors=False):
        """A triangle mesh of the capture by TSDF reconstruction (``segUtils.reconstruct``): the frames' world points go back to
        camera-z depth images (``depth_images``, pixels that are not ``valid`` or not finite are holes), which are integrated into a
        volume of ``voxel`` edge and extracted by surface nets -> (vertices float64 [V, 3], triangles int32 [M, 3]), ready for
        ``render_mesh_lookups``, ``project_vote_argmax_occluded``, ``meshUtils.label_faces`` / ``face_adjacency`` and
        ``write_triangle_mesh``.  Without ``lo`` and ``dims`` the volume is the box of the fused cloud ``points`` (as ``fuse``
        returned it; without it, of the frames' valid points, which contains that box) grown by ``trunc`` (default 4 voxels) on
        every side.  Frames of device tensors give device tensors.  ``fuse`` consumes the ``valid`` masks of NumPy frames, so call
        this first, or on a copy of the frames.  With ``colors`` the frames' colours (``fr[3]``, float [h*w, 3] in [0, 1], made uint8
        by ``round(clip(c, 0, 1) * 255)`` with NaN as 0, the rule of ``write_triangle_mesh``) are integrated with the depths ->
        (vertices, triangles, vertex_colors float64 [V, 3] in [0, 1]), ready for ``TriangleMesh``; a vertex without a colour is black."""
        from Fusion3DSeg.segUtils.reconstruct import TSDFVolume, depth_images
        ids = np.arange(0, self.nframes, skip)
        frames = [self.frames[int(i)] for i in ids]
        if not frames:
            raise ValueError('reconstruct_mesh: no frames')
        if on_device(frames[0][1]):
            import torch
            pts = torch.stack([fr[1].reshape(self.h, self.w, 3) for fr in frames])
            valid = torch.stack([fr[4].reshape(self.h, self.w).to(torch.bool) for fr in frames])
            good = valid & torch.isfinite(pts).all(dim=-1)
            cloud = pts[good].cpu().numpy() if points is None and (lo is None or dims is None) else None
        else:
            pts = np.stack([np.asarray(fr[1], np.float64).reshape(self.h, self.w, 3) for fr in frames])
            valid = np.stack([np.asarray(fr[4], bool).reshape(self.h, self.w) for fr in frames])
            cloud = pts[valid & np.isfinite(pts).all(axis=-1)]
        if not bool(valid.any()):
            raise ValueError('reconstruct_mesh: no frame has a valid pixel (fuse consumes the valid masks of NumPy frames: call this first, or on a copy)')
        voxel = float(voxel)
        trunc = 4.0 * voxel if trunc is None else float(trunc)
        if lo is None or dims is None:
            cloud = cloud if points is None else np.asarray(points.cpu() if on_device(points) else points, np.float64).reshape(-1, 3)
            if not len(cloud):
                raise ValueError('reconstruct_mesh: no valid point to take the bounds from')
            lo = cloud.min(axis=0) - trunc if lo is None else np.asarray(lo, np.float64)
            dims = np.maximum(1, np.ceil((cloud.max(axis=0) + trunc - lo) / voxel)).astype(np.int64)
        depths = depth_images(pts, self.xyzws[ids], self.translations[ids], valid)
        vol = TSDFVolume(lo, dims, voxel, trunc, max_weight, color=bool(colors))
        if not colors:
            return vol.integrate(depths, self.K, self.xyzws[ids], self.translations[ids], 1.0, max_depth).extract_mesh(min_weight)
        if on_device(frames[0][3]):
            import torch
            rgb = torch.stack([torch.round(torch.clip(torch.nan_to_num(fr[3].to(torch.float64)), 0.0, 1.0) * 255.0).to(torch.uint8).reshape(self.h, self.w, 3)
                               for fr in frames])
        else:
            rgb = np.stack([np.round(np.clip(np.nan_to_num(np.asarray(fr[3], np.float64)), 0.0, 1.0) * 255.0).astype(np.uint8).reshape(self.h, self.w, 3)
                            for fr in frames])
        vol.integrate(depths, self.K, self.xyzws[ids], self.translations[ids], 1.0, max_depth, colors=rgb)
        verts, tris, vrgb, _ = vol.extract_mesh(min_weight, colors=True)
        if on_device(vrgb):                                             # a tensor divisor: torch multiplies by the reciprocal of a host scalar
            import torch
            return verts, tris, vrgb.to(torch.float64) / torch.full((), 255.0, dtype=torch.float64, device=vrgb.device)
        return verts, tris, vrgb.astype(np.float64) / 255.0

    @staticmethod
    def filter(values, threshold, data=None, less_than=False):
        mask = values <= threshold if less_than else values >= threshold
        return (mask, None) if data is None else (mask, [d[mask] for d in data])

    def dump_data(self, dirname, points, normals=None, colors=None, nmerges=None, occurences=None, compute_adjacency=True,
                  verbose=False):
        """fusion/fusion_data.pkl, fusion/adj.pkl and the .ply of the fused cloud (reference :349-387); the adjacency is the
        GPU radius graph (``radius_adjacency``) instead of sklearn's KD-tree."""
        dirname = Path(dirname)
        (dirname / 'fusion').mkdir(exist_ok=True, parents=True)
        if verbose:
            print(f'writing fusion data into "{dirname}" directory')
        record = {'points': points, 'normals': normals, 'colors': colors, 'nmerges': nmerges, 'occurences': occurences,
                  'nframes': self.nframes, 'depth_hw': (self.h, self.w)}
        with (dirname / 'fusion' / 'fusion_data.pkl').open('wb') as fp:
            pickle.dump(record, fp)
        if compute_adjacency:
            if verbose:
                print('computing adjacency ...')
            adj = radius_adjacency(points, self.ds_radius)
            with (dirname / 'fusion' / 'adj.pkl').open('wb') as fp:
                pickle.dump(None if adj is None else np.array(adj, dtype=object), fp)
        from get3DSeg import PointCloud, write_ply
        tag = str(self.ds_radius).replace('.', '_')
        write_ply(dirname / 'fusion' / f'fusion_{tag}_{self.ds_angle}.ply', PointCloud(points, colors, normals))

    @classmethod
    def load_data(cls, dirname):
        """points, normals, colors, nmerges, occurences, nframes, depth_hw, adj (reference :389-407)."""
        dirname = Path(dirname)
        with open(dirname / 'fusion' / 'fusion_data.pkl', 'rb') as fp:
            d = pickle.load(fp)
        adj = None
        if (dirname / 'fusion' / 'adj.pkl').is_file():
            with open(dirname / 'fusion' / 'adj.pkl', 'rb') as fp:
                adj = pickle.load(fp)
        return [d['points'], d['normals'], d['colors'], d['nmerges'], d['occurences'], d['nframes'], d['depth_hw'], adj]


class _DeviceFusion:
    """The frame loop of Fusion.fuse / fuse_device and the down-sampling step of Fusion.patch_downsample: the resident cloud
    (capacity doubling), the per-frame buffers and the steps, for frames of h x w pixels."""

    def __init__(self, h, w, pcdimg, pt2u, pt2v, ctx, torch, dev, stream, caller):
        self.ctx, self.torch, self.dev, self.stream, self.sh, self.caller = ctx, torch, dev, stream, stream.cuda_stream, caller
        self.h, self.w, self.npx = h, w, h * w
        self.pcdimg, self.pt2u, self.pt2v = pcdimg, pt2u, pt2v
        self.mode = _norm_mode()
        self.stats = {'frames': 0, 'sequential_frames': 0, 'host_normalised': 0, 'rounds': 0, 'shuffle_s': 0.0, 'draws_undone': 0,
                      'capacity_growths': 0}
        T, n = torch, self.npx
        self.cap = 0
        self.count_dev = T.zeros(1, dtype=T.int64, device=dev)
        self.free = T.zeros(n, dtype=T.uint8, device=dev)
        self.owner = T.empty(n, dtype=T.int32, device=dev)
        self.prio = T.empty(n, dtype=T.int32, device=dev)
        self.order = T.empty(n, dtype=T.int64, device=dev)
        self.px_sums = T.empty((n, 9), dtype=T.float64, device=dev)
        self.px_counts = T.empty(n, dtype=T.int32, device=dev)
        self.stats_dev = T.zeros(3, dtype=T.int64, device=dev)
        self.check_dev = T.zeros(2, dtype=T.int64, device=dev)
        self.stage = [T.empty((n, 3), dtype=T.float64, pin_memory=True) for _ in range(3)] + [T.empty(n, dtype=T.uint8, pin_memory=True)]
        self.order_stage = T.empty(n, dtype=T.int64, pin_memory=True)
        self.frame_buf = [T.empty((n, 3), dtype=T.float64, device=dev) for _ in range(3)] + [T.empty(n, dtype=T.uint8, device=dev)]

    @classmethod
    @contextlib.contextmanager
    def on_stream(cls, what, h, w, pcdimg, pt2u, pt2v):
        """An instance working on the stream ``f3d.tensors.work_stream`` gives for the caller's current torch stream."""
        ctx = f3d.default_context()
        torch, dev = torch_device(ctx, what)
        caller = torch.cuda.current_stream(dev)
        with torch.cuda.device(dev), work_stream(dev) as work:
            yield cls(h, w, pcdimg, pt2u, pt2v, ctx, torch, dev, work, caller)

    # ---------------------------------------------------------------- storage
    def reserve(self, rows):
        """Capacity for `rows` cloud rows (doubling, device-to-device copy of what is there)."""
        if rows <= self.cap:
            return
        T, dev = self.torch, self.dev
        cap = max(rows, 2 * self.cap, 4096)
        new = [T.zeros((cap, 3), dtype=T.float64, device=dev) for _ in range(3)] + [T.zeros(cap, dtype=T.int64, device=dev)]
        occ = T.zeros(cap, dtype=T.int32, device=dev)                     # uint32 bits (returned as a uint32 view)
        if self.cap:
            for a, b in zip(new + [occ], self.cloud + [self.occ]):
                a[:self.cap].copy_(b)
            self.stats['capacity_growths'] += 1
        self.cloud, self.occ, self.cap = new, occ, cap
        self.uv_all = T.empty((2, cap), dtype=T.int32, device=dev)
        self.inside = T.empty(cap, dtype=T.uint8, device=dev)
        self.ids = T.empty(cap, dtype=T.int32, device=dev)
        self.uv = T.empty(2 * cap, dtype=T.int32, device=dev)
        self.hit_pts = T.empty((cap, 3), dtype=T.float64, device=dev)
        self.hit_nrm = T.empty((cap, 3), dtype=T.float64, device=dev)
        self.sums = T.empty((cap, 9), dtype=T.float64, device=dev)
        self.counts = T.empty(cap, dtype=T.int32, device=dev)

    def cloud_ptrs(self):
        return tuple(t.data_ptr() for t in self.cloud + [self.occ])

    # ---------------------------------------------------------------- frames
    def frame(self, fetched):
        """A fetched frame (name, points, normals, colours, valid) -> (name, points, normals, colours, valid uint8) on the device, plus
        the host arrays of a NumPy frame (else None)."""
        T = self.torch
        name, pts, nrm, clr, valid = fetched
        if isinstance(pts, T.Tensor):
            for t in (pts, nrm, clr):
                if t.device != self.dev or t.dtype != T.float64 or tuple(t.shape) != (self.npx, 3) or not t.is_contiguous():
                    raise ValueError(f'fuse_device: frame tensors must be float64 [{self.npx},3] contiguous on {self.dev}')
            if valid.device != self.dev or valid.dtype not in (T.bool, T.uint8) or valid.numel() != self.npx or not valid.is_contiguous():
                raise ValueError(f'fuse_device: valid must be bool or uint8 [{self.npx}] on {self.dev}')
            return name, pts, nrm, clr, valid.reshape(-1).view(T.uint8), None
        host = [np.asarray(pts, np.float64).reshape(self.npx, 3), np.asarray(nrm, np.float64).reshape(self.npx, 3),
                np.asarray(clr, np.float64).reshape(self.npx, 3), np.asarray(valid).reshape(self.npx)]
        for src, stage, buf in zip(host, self.stage, self.frame_buf):      # the previous upload has completed (a readback followed it)
            np.copyto(stage.numpy(), src, casting='unsafe')
            buf.copy_(stage, non_blocking=True)
        return (name, *self.frame_buf, host)

    def draw(self):
        """np.random.shuffle(np.arange(h*w)) of the global generator, into the pinned staging buffer."""
        t0 = time.perf_counter()
        order = self.order_stage.numpy()
        order[:] = np.arange(self.npx)
        np.random.shuffle(order)
        self.stats['shuffle_s'] += time.perf_counter() - t0
        return order

    def consume(self, mask):
        """Pixels of the NumPy `mask` that the free buffer no longer holds are set to False, written through mask.reshape(h, w):
        how the reference consumes a frame's mask in place."""
        mask = mask.reshape(self.h, self.w)
        mask[(mask != 0) & (self.free.cpu().numpy() == 0).reshape(self.h, self.w)] = False

    # ---------------------------------------------------------------- steps
    def host_normalise(self, rows):
        """Normals of the given cloud rows (device int64 tensor) normalised with _row_norms on the host."""
        if not len(rows):
            return
        nrm = self.cloud[1]
        ns = nrm[rows].cpu().numpy()
        nrm[rows] = self.torch.from_numpy(ns / _row_norms(ns)[:, None]).to(self.dev)
        self.stats['host_normalised'] += len(ns)

    def downsample(self, order, frame, half, radius, min_cosine, fallback, nfree, count, uv2pt):
        """patch_downsample of the frame's `nfree` free pixels, appended to the cloud at row `count` -> the new row count (or a bound)."""
        T, ctx, sh, h, w, npx = self.torch, self.ctx, self.sh, self.h, self.w, self.npx
        name, dp, dn, dc, dv, host = frame
        self.reserve(count + npx)
        if fallback:                                                         # the reference's own order of events, on the host
            self.stats['sequential_frames'] += 1
            if host is None:
                host = [dp.cpu().numpy(), dn.cpu().numpy(), dc.cpu().numpy()]
            free = self.free.cpu().numpy().astype(bool).reshape(h, w)
            with np.errstate(all='ignore'):
                n_pts, n_nrm, n_clr, n_uv, n_mrg = Fusion._patch_downsample_sequential(
                    order, host[0], host[1], host[2], h, w, half, radius, min_cosine, self.pcdimg, self.pt2u, self.pt2v, free)
            k = len(n_mrg)
            if k:
                for buf, rows in zip(self.cloud[:3], (n_pts, n_nrm, n_clr)):
                    buf[count:count + k].copy_(T.from_numpy(np.ascontiguousarray(rows, np.float64).reshape(k, 3)))
                self.cloud[3][count:count + k].copy_(T.from_numpy(np.asarray(n_mrg, np.int64)))
                self.occ[count:count + k].fill_(1)
            fresh = T.from_numpy(n_uv).to(self.dev)
            uv2pt.copy_(T.where(fresh != -1, fresh + count, uv2pt))
            self.free.copy_(T.from_numpy(free.reshape(-1).astype(np.uint8)))
            self.count_dev.fill_(count + k)
            return count + k
        self.order.copy_(self.order_stage, non_blocking=True)                # the stage is rewritten only after a later readback
        ctx.fusion_prio_dev(self.order.data_ptr(), npx, self.prio.data_ptr(), sh)
        self.stats['rounds'] += ctx.patch_seeds_sums_dev(dp.data_ptr(), dn.data_ptr(), dc.data_ptr(), self.prio.data_ptr(), self.free.data_ptr(),
                                                         h, w, half, radius, min_cosine, self.owner.data_ptr(), self.px_sums.data_ptr(),
                                                         self.px_counts.data_ptr(), sh)
        p, n, c, m, o = self.cloud_ptrs()
        ctx.fusion_new_seeds_dev(self.owner.data_ptr(), self.prio.data_ptr(), self.px_sums.data_ptr(), self.px_counts.data_ptr(), npx, self.mode,
                                 self.count_dev.data_ptr(), self.cap, p, n, c, m, o, uv2pt.data_ptr(), self.free.data_ptr(), sh)
        if self.mode == f3d.NORM_HOST:
            new = int(self.count_dev.item())
            self.host_normalise(T.arange(count, new, device=self.dev))
            return new
        return count + nfree

    def finish(self, fu, name, uv2pt, mask, host_io):
        """A fused frame's end: ``fuse`` consumes the NumPy mask the free buffer stands for, then the lookup goes to fu's lookup_dir /
        lookup_sink (a NumPy array for ``fuse``, the device tensor for ``fuse_device``)."""
        self.stats['frames'] += 1
        if mask is not None:
            self.consume(mask)
        if not fu.save_lookups:
            return
        host = uv2pt.cpu().numpy() if host_io or fu.uv2pt_dir is not None else None
        if fu.uv2pt_dir is not None:
            np.save(Path(fu.uv2pt_dir) / f'{name}.npy', host)
        if fu._lookup_sink is not None:
            if not host_io and self.stream != self.caller:
                uv2pt.record_stream(self.caller)
            fu._lookup_sink(name, host if host_io else uv2pt)

    def check(self, frame, radius, min_cosine):
        """-> (free pixels, sequential flag) of the current free buffer against the frame (one readback).  A NumPy frame's flag is
        patch_downsample's own test, taken on the host: k_fu_check adds the normal's squared length in another order than np.einsum,
        and a normal whose squared length lies within an ulp of min_cosine can fall on the other side."""
        _, dp, dn, _, _, host = frame
        self.ctx.fusion_frame_check_dev(self.free.data_ptr(), dp.data_ptr(), dn.data_ptr(), self.npx, radius, min_cosine,
                                        self.check_dev.data_ptr(), self.sh)
        nfree, fallback = self.check_dev.tolist()
        if host is not None and nfree:
            free = np.flatnonzero(self.free.cpu().numpy())
            fallback = not (radius > 0) or _unusable(host[0][free], host[1][free], min_cosine).any()
        return nfree, fallback

    def add_free(self, frame, half, radius, min_cosine, count, uv2pt, undo):
        """The frame's free pixels down-sampled onto the cloud at row `count` -> the new row count (or a bound).  The shuffle is drawn
        while the GPU matches; with `undo` it is taken back when no pixel is free (the reference then calls no patch_downsample)."""
        state = np.random.get_state()
        order = self.draw()
        nfree, fallback = self.check(frame, radius, min_cosine)
        if nfree or not undo:
            return self.downsample(order, frame, half, radius, min_cosine, fallback, nfree, count, uv2pt)
        np.random.set_state(state)
        self.stats['draws_undone'] += 1
        return count

    # ---------------------------------------------------------------- the loop of Fusion.fuse
    def run(self, fu, radius, angle, stride, max_depth, skip, verbose, host_io=False):
        """The frames of `fu` fused into the resident cloud -> (points, normals, colours, nmerges, occurences) device tensors.
        ``host_io``: lookups go out as NumPy arrays and the masks of NumPy frames are consumed in place, as ``fuse`` does."""
        T, ctx, sh, npx = self.torch, self.ctx, self.sh, self.npx
        fu.ds_radius, fu.ds_angle, fu.fuse_device_stats = radius, angle, self.stats
        stride = max(10, int(radius * 200)) if stride is None else stride
        half, min_cosine = stride // 2, np.cos(np.deg2rad(angle))
        for first in range(0, fu.nframes):                                  # first frame with any valid pixel seeds the cloud
            fetched = fu.frames[first]
            if bool(fetched[4].any()):
                break
        self.reserve(npx)
        frame = self.frame(fetched)
        mask = fetched[4] if host_io and frame[5] is not None else None   # the NumPy mask the free buffer stands for
        self.free.copy_(frame[4])
        uv2pt = T.full((npx,), -1, dtype=T.int32, device=self.dev)
        count_bound = self.add_free(frame, half, radius, min_cosine, 0, uv2pt, undo=False)
        self.finish(fu, frame[0], uv2pt, mask, host_io)
        have_free, prev_hits = False, npx
        for j in range(first + 1, fu.nframes, skip):
            fetched = fu.frames[j]
            frame = self.frame(fetched)
            name, dp, dn, dc, dv, _ = frame
            p, n, c, m, o = self.cloud_ptrs()                               # rows < count_bound <= capacity
            ctx.project_view_dev(p, f3d.F64, count_bound, fu._frame_view(j, max_depth), self.uv_all.data_ptr(), self.inside.data_ptr(), sh)
            ctx.fusion_hits_dev(self.inside.data_ptr(), self.uv_all.data_ptr(), count_bound, self.count_dev.data_ptr(), p, n, dv.data_ptr(), npx,
                                self.ids.data_ptr(), self.uv.data_ptr(), self.hit_pts.data_ptr(), self.hit_nrm.data_ptr(),
                                self.stats_dev.data_ptr(), sh)
            hits, nvalid, count = self.stats_dev.tolist()
            if verbose:
                print(f'fusing frame: {j + 1}, total points = {count}, previous intersections = {prev_hits}')
            count_bound = count
            if not nvalid:
                continue
            prev_hits = hits
            uv2pt = T.empty(npx, dtype=T.int32, device=self.dev)
            if hits:
                self.free.copy_(dv)                                         # the frame's mask, copied: the caller's tensors stay as they are
                have_free = True
                mask = fetched[4] if host_io and frame[5] is not None else None
                ctx.patch_match_dev(self.uv.data_ptr(), hits, self.h, self.w, half, radius, min_cosine, self.hit_pts.data_ptr(),
                                    self.hit_nrm.data_ptr(), dp.data_ptr(), dn.data_ptr(), dc.data_ptr(), self.free.data_ptr(),
                                    self.owner.data_ptr(), self.sums.data_ptr(), self.counts.data_ptr(), sh)
                ctx.fusion_seed_update_dev(self.ids.data_ptr(), hits, self.sums.data_ptr(), self.counts.data_ptr(), self.mode, p, n, c, m, o, sh)
                if self.mode == f3d.NORM_HOST:
                    took = self.counts[:hits] > 0
                    self.host_normalise(self.ids[:hits][took].long())
                ctx.fusion_lookup_dev(self.owner.data_ptr(), self.ids.data_ptr(), npx, uv2pt.data_ptr(), self.free.data_ptr(), sh)
            else:
                uv2pt.fill_(-1)
                if not have_free:                                          # the reference's `free` was never assigned
                    raise UnboundLocalError("local variable 'free' referenced before assignment (the first fused frame has no hits)")
            # the reference calls patch_downsample with 2 * stride, whose half window is then (2 * stride) // 2
            count_bound = self.add_free(frame, (2 * stride) // 2, radius, min_cosine, count, uv2pt, undo=True)
            self.finish(fu, name, uv2pt, mask, host_io)
        total = int(self.count_dev.item())
        pts, nrm, clr, nmerges = (t[:total] for t in self.cloud[:4])
        return pts, nrm, clr, nmerges, self.occ[:total].view(T.uint32)
