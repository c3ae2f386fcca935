"""One case per public device route, shared by the tests that run every hand-off between torch and the library under some condition
(tests/test_route_streams_gpu.py: stalled streams; tests/test_route_layouts_gpu.py: strided, offset and retyped tensors).  A route is a
public function or class of Fusion3DSeg/, RTAB_utils/ or get2DSeg.py that calls ``on_device``, ``torch_device`` or ``work_stream`` or
hands over a ``.cuda_stream``, itself or through a private helper of its module (tests/test_route_cases_cpu.py walks the sources).

A case is a function of a seed -> (inputs, call, want, check, rows):
  inputs  dict name -> packed NumPy array: the tensor arguments of the route;
  call    call(tensors, between=nop) hands device tensors of those names to the public route and returns its results as they come
          (tensors, arrays, scalars, in tuples / lists / dicts); a stateful route calls ``between()`` between its steps;
  want    what the restatement says (tests/*_ref.py, oracle/np_ref.py), never a second run of the library;
  check   check(got, want) on the results copied to the host: the comparison of that family in tests/family_cases.py or in the
          family's own GPU test, no new tolerance;
  rows    a reference output whose rows differ between two seeds.
Two seeds give the same input shapes and dtypes: seed A is the scene, seed B the decoy, and both are valid inputs (valid CSR, in-range
labels and indices), so nothing that reads the decoy can fault.  Inputs that must keep a size that depends on the data (the entries of
a radius graph) are one base scene under a permutation of its points drawn from the seed.  Shapes are those of family_cases.  This is no
test module: it holds no test."""
import collections
import functools
import math
from types import SimpleNamespace

import numpy as np

import f3d
import cvseg_ref
import door_window_ref
import face_graph_ref
import family_cases as F
import features_ref
import fused_families
import fusion_scenes
import icp_color_ref
import icp_ref
import knn_ref
import lift_ref
import mesh_ref
import normals_ref
import planes_ref
import point_voting_ref
import quad_scenes
import raster_ref
import refinement_ref
import render_ref
import smooth_ref
import sort_ref
import tsdf_color_ref
import tsdf_ref
from oracle import np_ref as O

N, H, W = F.N, F.H, F.W
SEED, OTHER_SEED = F.SEED, F.OTHER_SEED
SU = 'Fusion3DSeg/segUtils/'
FU = 'Fusion3DSeg/fusion.py::'

Route = collections.namedtuple('Route', 'case routes entries syncs stateful inplace alt names owned')
TABLE = {}


def route(name, routes=(), entries=(), syncs=False, stateful=False, inplace=(), alt=None, names=None, owned=()):
    """Registers a case: the public routes it drives, the ``*_dev`` entries of f3d.Context it reaches, ``syncs`` (the route reads back by
    contract: count passes, take_device_error, the cloud's box, icp's status), ``stateful`` (it calls ``between()``), the inputs the route documents as updated in place, the other dtypes the route documents per
    input, the word an error message uses for an input (its name else), and the inputs that are state the route's object owns, not
    arguments (the layout lens leaves them as they are)."""
    def deco(fn):
        TABLE[name] = Route(fn, tuple(routes), tuple(entries), syncs, stateful, tuple(inplace), dict(alt or {}), dict(names or {}), tuple(owned))
        return fn
    return deco


def nop():
    pass


def f32_exact(a):
    """`a` rounded to values float32 holds: the library widens float32 inputs exactly, so the float32 variant has the same reference."""
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


F32 = [np.float32]


@functools.lru_cache(maxsize=None)
def prepared(name, seed):
    """(inputs, call, want, check, rows) of a case and seed, built once; the arrays are read-only."""
    inputs, call, want, check, rows = TABLE[name].case(seed)
    for a in inputs.values():
        a.setflags(write=False)
    return inputs, call, want, check, rows


def _ctx():
    return f3d.default_context()


def direct(fn):
    """A ``*_dev`` entry driven directly goes through the same protocol as a route: inside ``f3d.tensors.work_stream``."""
    @functools.wraps(fn)
    def call(t, between=nop):
        import torch
        from f3d.tensors import work_stream
        dev = next(iter(t.values())).device
        with torch.cuda.device(dev), work_stream(dev) as work:
            out = fn(t, torch, dev, work.cuda_stream)
        for x in out if isinstance(out, (tuple, list)) else (out,):
            if hasattr(x, 'record_stream'):
                x.record_stream(torch.cuda.current_stream(dev))
        return out
    return call


# ---- scenes that keep their sizes under a new seed ----------------------------------------------------------------------------------------
def permutation(seed, n):
    """(perm, inv): row i of the permuted scene is row perm[i] of the base scene, inv[perm[i]] = i."""
    perm = np.random.default_rng(7000 + seed).permutation(n)
    inv = np.empty(n, np.int64)
    inv[perm] = np.arange(n)
    return perm, inv


def permuted_csr(offs, nbrs, perm, inv):
    """The CSR of the permuted scene: the same graph, every row ascending."""
    lens = np.diff(offs)[perm]
    new_offs = np.zeros(len(perm) + 1, np.int64)
    np.cumsum(lens, out=new_offs[1:])
    rows = [np.sort(inv[nbrs[offs[p]:offs[p + 1]]]) for p in perm]
    return new_offs, np.concatenate(rows).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _blob_base():
    return F.blob_scene(SEED)


def blob(seed):
    """family_cases.blob_scene of the base seed with its points permuted: (points, colours, classes, (offsets, neighbours))."""
    pts, colors, classes, (offs, nbrs) = _blob_base()
    perm, inv = permutation(seed, N)
    return pts[perm].copy(), colors[perm].copy(), classes[perm].copy(), permuted_csr(offs, nbrs, perm, inv)


def _adj(t):
    return t['offsets'], t['neighbours']


# ---- refinement -----------------------------------------------------------------------------------------------------------------------------
PP, NR = np.array([0.5, 0.5, 0.5]), np.array([0.3, -0.5, 0.81]) / np.linalg.norm([0.3, -0.5, 0.81])
NSEEDS = 24


def _plane_dist(pts):
    return np.abs(((pts[:, 0] - PP[0]) * NR[0] + (pts[:, 1] - PP[1]) * NR[1]) + (pts[:, 2] - PP[2]) * NR[2])


@route('plane_distance', [SU + 'refinement.py::plane_distance'], ['plane_distance_dev'])
def case_plane_distance(seed):
    """refinement.plane_distance within refinement_ref.plane_distance_bound of the extended-precision value."""
    pts = F.cloud(np.random.default_rng(seed))
    L = np.longdouble
    d = pts.astype(L) - PP.astype(L)
    exact = np.abs(d[:, 0] * L(NR[0]) + d[:, 1] * L(NR[1]) + d[:, 2] * L(NR[2]))

    def call(t, between=nop):
        from Fusion3DSeg.segUtils import refinement
        return refinement.plane_distance(t['points'], PP, NR)

    def check(got, want):
        assert got.dtype == np.float64 and got.shape == (N,)
        assert (np.abs(got.astype(L) - want).astype(np.float64) <= refinement_ref.plane_distance_bound(pts, PP, NR)).all()
    return dict(points=pts), call, exact, check, exact.astype(np.float64)


def _grow_case(seed, colour):
    pts, colors, _, adj = blob(seed)
    dist = _plane_dist(pts)
    inst = np.nonzero(dist < 0.01)[0][:NSEEDS]
    assert len(inst) == NSEEDS
    if colour:
        want = refinement_ref.color_points(colors, adj, inst, 0.45, 50)
    else:
        want = refinement_ref.depth_points(dist, adj, inst, 0.05, 50)

    def call(t, between=nop):
        from Fusion3DSeg.segUtils import refinement
        if colour:
            return refinement.grow_color(t['values'], _adj(t), t['seeds'], 0.45, 50, given=True)
        return refinement.grow_depth(t['values'], _adj(t), t['seeds'], 0.05, 50, given=True)

    def check(got, want):
        F.same(got, want)
        assert len(want) > 100
    return dict(values=colors if colour else dist, offsets=adj[0], neighbours=adj[1], seeds=inst), call, want, check, want


@route('grow_depth', [SU + 'refinement.py::grow_depth'], ['region_grow_dev'], syncs=True,
       alt={'offsets': [np.int32], 'neighbours': [np.int64], 'seeds': [np.int32]}, names={'offsets': 'CSR', 'neighbours': 'CSR'})
def case_grow_depth(seed):
    """refinement.grow_depth (an instance's points as seeds) against refinement_ref.depth_points, acceptance order included."""
    return _grow_case(seed, False)


@route('grow_color', [SU + 'refinement.py::grow_color'], ['region_grow_dev'], syncs=True,
       alt={'offsets': [np.int32], 'neighbours': [np.int64], 'seeds': [np.int32]}, names={'offsets': 'CSR', 'neighbours': 'CSR'})
def case_grow_color(seed):
    """refinement.grow_color against refinement_ref.color_points, acceptance order included."""
    return _grow_case(seed, True)


# ---- transfer ---------------------------------------------------------------------------------------------------------------------------------
def _knn_scene(seed):
    rng = np.random.default_rng(seed)
    return f32_exact(F.cloud(rng)), f32_exact(F.cloud(rng)), rng.integers(-3, 9, N), 8, 0.12


@route('nearest_points', [SU + 'transfer.py::nearest_points'], ['knn_query_dev'], syncs=True, alt={'cloud': F32, 'queries': F32})
def case_nearest_points(seed):
    """transfer.nearest_points against knn_ref.knn, exactly."""
    data, queries, _, k, r = _knn_scene(seed)
    want = knn_ref.knn(data, queries, k, r)[:3]

    def call(t, between=nop):
        from Fusion3DSeg.segUtils import transfer
        return transfer.nearest_points(t['cloud'], t['queries'], r, k)
    return dict(cloud=data, queries=queries), call, want, F.all_same, want[0]


@route('transfer_labels', [SU + 'transfer.py::transfer_labels', SU + 'transfer.py::vertex_mask_from_points'], ['transfer_labels_dev'], syncs=True,
       alt={'labels': [np.int32], 'cloud': F32, 'queries': F32})
def case_transfer_labels(seed):
    """transfer.transfer_labels (with support) and vertex_mask_from_points against knn_ref.knn / plurality, exactly."""
    data, queries, labels, k, r = _knn_scene(seed)
    rows = knn_ref.knn(data, queries, k, r)[:3]
    bits = labels > 3
    want = knn_ref.plurality(rows[0], labels, -5) + (knn_ref.plurality(rows[0], bits.astype(np.int64), 0)[0].astype(bool),)

    def call(t, between=nop):
        from Fusion3DSeg.segUtils import transfer
        out, support = transfer.transfer_labels(t['cloud'], t['labels'], t['queries'], r, k, fill=-5, return_support=True)
        return out, support, transfer.vertex_mask_from_points(t['cloud'], t['labels'] > 3, t['queries'], r, k)

    def check(got, want):
        F.same(got[0].astype(np.int64), want[0]); F.same(got[1], want[1]); F.same(got[2], want[2])
    return dict(cloud=data, labels=labels, queries=queries), call, want, check, np.stack([want[0], want[1]], axis=1)


# ---- lifting ----------------------------------------------------------------------------------------------------------------------------------
def _lift_check_instances(got, want):
    for name in ('ids', 'support', 'seen', 'seg2inst', 'inst_points'):
        F.same(got[name], getattr(want, name))


@route('segment_overlaps', [SU + 'lifting.py::segment_overlaps'], ['lift_overlaps_dev'], syncs=True)
def case_segment_overlaps(seed):
    """lifting.segment_overlaps against lift_ref, exactly."""
    luts, inst = lift_ref.random_scene(seed, N, 6, H * W, 12, skew=1.0)
    want = lift_ref.segment_overlaps(luts, inst, N, 12)

    def call(t, between=nop):
        from Fusion3DSeg.segUtils import lifting
        return lifting.segment_overlaps(t['luts'], t['inst'], N, 12)
    return dict(luts=np.ascontiguousarray(luts, np.int32), inst=np.ascontiguousarray(inst, np.uint16)), call, want, F.all_same, want[0]


@route('lift_instances', [SU + 'lifting.py::lift_instances'], ['lift_instances_dev'], syncs=True)
def case_lift_instances(seed):
    """lifting.lift_instances against lift_ref, exactly."""
    luts, inst = lift_ref.random_scene(seed, N, 6, H * W, 12, skew=1.0)
    want = lift_ref.lift_instances(luts, inst, N, 12)

    def call(t, between=nop):
        from Fusion3DSeg.segUtils import lifting
        return vars(lifting.lift_instances(t['luts'], t['inst'], N, 12))
    return (dict(luts=np.ascontiguousarray(luts, np.int32), inst=np.ascontiguousarray(inst, np.uint16)), call, want, _lift_check_instances,
            np.stack([want.ids, want.support, want.seen], axis=1))


# ---- planes -----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _corner_base():
    pts, nrm, _ = planes_ref.room_corner(np.random.default_rng(SEED))
    pts = f32_exact(pts)
    return pts, nrm, planes_ref.radius_csr(pts, 0.05)


@route('extract_planes', [SU + 'planeUtils.py::extract_planes'], ['extract_planes_dev'], syncs=True,
       alt={'offsets': [np.int32], 'neighbours': [np.int64], 'points': F32}, names={'offsets': 'CSR', 'neighbours': 'CSR'})
def case_extract_planes(seed):
    """planeUtils.extract_planes on the room corner against planes_ref.extract: labels and counts exactly."""
    pts, nrm, (offs, nbrs) = _corner_base()
    perm, inv = permutation(seed, len(pts))
    pts, nrm = pts[perm].copy(), nrm[perm].copy()
    offs, nbrs = permuted_csr(offs, nbrs, perm, inv)
    want = planes_ref.extract(pts, offs, nbrs, nrm)

    def call(t, between=nop):
        from Fusion3DSeg.segUtils import planeUtils
        return tuple(planeUtils.extract_planes(t['points'], _adj(t), t['normals']))

    def check(got, want):
        labels, planes, corners, counts = got
        assert want.margin >= 1e-6, want.margin
        F.same(counts, want.counts); F.same(labels, want.labels)
        assert planes.shape == (want.counts[0], 8) and corners.shape == (want.counts[0], 4, 3) and np.isfinite(planes).all()
    return dict(points=pts, offsets=offs, neighbours=nbrs, normals=nrm), call, want, check, want.labels


# ---- features ---------------------------------------------------------------------------------------------------------------------------------
def _feature_scene(seed, nviews):
    from f3d import synth
    pts = f32_exact(synth.cloud(N, seed=seed))
    K, q, t, _, _ = F.ring_scene(seed, nviews)
    feats = np.random.default_rng(seed).standard_normal((nviews, 12, 10, 20), dtype=np.float32)
    return pts, K, q, t, feats


@route('fuse_features', [SU + 'features.py::fuse_features'], ['fuse_features_dev'], alt={'points': F32})
def case_fuse_features(seed):
    """features.fuse_features of 3 views against features_ref.fuse, bit for bit."""
    pts, K, q, t, feats = _feature_scene(seed, 3)
    want = features_ref.fuse(pts, K, q, t, feats, (H, W), 10, 1, 0.05)

    def call(tt, between=nop):
        from Fusion3DSeg.segUtils import features
        return features.fuse_features(tt['points'], K, q, t, tt['features'], (H, W), 10, 1, 0.05)

    def check(got, want):
        F.same_bits(got[0], want[0]); F.same_bits(got[1], want[1])
    return dict(points=pts, features=feats), call, want, check, render_ref.lookups(pts, K, q, t, (H, W), 10, 1)[0].reshape(3 * H, W)


@route('FeatureFusion', [SU + 'features.py::FeatureFusion'], ['fuse_features_dev', 'features_finalize_dev'], stateful=True)
def case_feature_fusion(seed):
    """features.FeatureFusion fed 40 views in two chunks, then features(), against features_ref.fuse / finalize, bit for bit."""
    pts, K, q, t, feats = _feature_scene(seed, 40)
    sums, counts = features_ref.fuse(pts, K, q, t, feats, (H, W), 10, 1, 0.05)
    want = (sums, counts, features_ref.finalize(sums, counts))

    def call(tt, between=nop):
        from Fusion3DSeg.segUtils import features
        ff = features.FeatureFusion(tt['points'], (H, W), 10, 1, 0.05)
        ff.add(K, q[:20], t[:20], tt['features'][:20])
        between()
        ff.add(K, q[20:], t[20:], tt['features'][20:])
        between()
        return ff.sums, ff.counts, ff.features()

    def check(got, want):
        for g, w in zip(got, want):
            F.same_bits(g, w)
    return dict(points=pts, features=feats), call, want, check, want[0]


# ---- door / window quads ------------------------------------------------------------------------------------------------------------------------
NQUADS = 200


@route('door_window_quads', [SU + 'door_window_bbox.py::door_window_quads'], ['door_window_quads_dev'], syncs=True,
       alt={'triangles': [np.int32], 'points': F32, 'vertices': F32})
def case_door_window_quads(seed):
    """door_window_bbox.door_window_quads for the instances the restatement gives a candidate, against door_window_ref.generate, exactly."""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(2, 4, NQUADS).tolist()
    pts, ids, inst, verts, tris = quad_scenes.shuffled(quad_scenes.rect_scene(150, sizes, seed=seed, nother=N - sum(sizes)), seed)
    pts, verts = f32_exact(pts), f32_exact(verts)
    _, status, _, _ = door_window_ref.quads(pts, ids, inst, verts, tris)
    info = [{'id': int(i), 'isthing': True, 'category_id': int(door_window_ref.DOOR_WINDOW[k % 3]), 'area': 1, 'hexcolor': f'#{(37 * k) % 256:02x}80ff'}
            for k, i in enumerate(inst) if status[k] != door_window_ref.QUAD_NO_CANDIDATE]
    want = door_window_ref.generate(pts, ids, info, verts, tris)

    def call(t, between=nop):
        from Fusion3DSeg.segUtils import door_window_bbox
        return door_window_bbox.door_window_quads(t['points'], t['ids'], info, t['vertices'], t['triangles'])

    def check(got, want):
        assert len(got) == 4 and len(want[0]) >= 60
        F.same(got[0], want[0])
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])
    return (dict(points=pts, ids=np.ascontiguousarray(ids, np.int64), vertices=verts, triangles=np.ascontiguousarray(tris, np.int64)), call, want, check,
            np.pad(want[1], ((0, 4 * NQUADS - len(want[1])), (0, 0))))


# ---- correspondance ---------------------------------------------------------------------------------------------------------------------------
@route('PointCorrespondance', [SU + 'correspondance.py::PointCorrespondance'], ['radius_query_dev', 'radius_query_fill_dev'], syncs=True,
       alt={'sparse': F32, 'dense': F32})
def case_point_correspondance(seed):
    """PointCorrespondance on tensors (float32-exact sparse points) against brute-force radius rows, and get_point against a gather of them."""
    rng = np.random.default_rng(seed)
    sparse, dense = f32_exact(F.cloud(rng)), f32_exact(F.cloud(rng, 2 * 24 * 28))
    r = 0.08
    offs, nb = F.radius_rows(sparse, dense, r)
    images, coords = np.array([0, 1, 1, 0]), np.array([[3, 5], [27, 23], [0, 0], [14, 9]])
    rows = [nb[offs[p]:offs[p + 1]] for p in images * 24 * 28 + coords[:, 1] * 28 + coords[:, 0]]
    want = (offs, nb, np.concatenate(rows), np.array([len(x) for x in rows], np.int64))

    def call(t, between=nop):
        from Fusion3DSeg.segUtils.correspondance import PointCorrespondance
        pc = PointCorrespondance(t['sparse'], t['dense'], r, 2, (24, 28))
        return tuple(pc.csr) + tuple(pc.get_point(images, coords))
    return dict(sparse=sparse, dense=dense), call, want, F.all_same, F.csr_rows(offs, nb)


# ---- CVSegmentation ---------------------------------------------------------------------------------------------------------------------------
@route('instance_seperate', [SU + 'cv.py::CVSegmentation', SU + 'cv.py::Boundaries'], ['flood_order_dev'], syncs=True, inplace=('classes',),
       alt={'offsets': [np.int32], 'neighbours': [np.int64]}, names={'offsets': 'CSR', 'neighbours': 'CSR'})
def case_instance_seperate(seed):
    """CVSegmentation.instance_seperate on device classes against cvseg_ref, by cvseg_ref.same_instances; the classes are rewritten in place."""
    _, _, classes, adj = blob(seed)
    want_classes = classes.copy()
    want = cvseg_ref.instance_seperate(want_classes, adj, [3, 1, 0], 5)

    def call(t, between=nop):
        from Fusion3DSeg.segUtils.cv import CVSegmentation
        got = CVSegmentation(t['classes'], _adj(t)).instance_seperate([3, 1, 0], 5)
        return list(got[:4]) + [[got[4][i] for i in range(len(got[4]))]], t['classes']

    def check(got, want):
        F.same(got[1], want_classes)
        cvseg_ref.same_instances(got[0], (len(want[0]), want[1], want[2], want[3], list(want[4])))
        assert len(got[0][3]) > 10
    return dict(classes=classes, offsets=adj[0], neighbours=adj[1]), call, want, check, want[1]


@route('color_segment', [SU + 'cv.py::CVSegmentation'], ['color_segment_dev'], syncs=True, inplace=('ids',),
       alt={'offsets': [np.int32], 'neighbours': [np.int64], 'seeds': [np.int32]},
       names={'offsets': 'CSR', 'neighbours': 'CSR', 'colors': 'colours'})
def case_color_segment(seed):
    """CVSegmentation.color_segment on device ids (float32-exact colours) against cvseg_ref.color_segment, exactly; ids are updated in place."""
    _, colors, classes, adj = blob(seed)
    colors = colors.astype(np.float32).astype(np.float64)
    offs, nbrs = adj
    _, ids, info, _, _ = cvseg_ref.instance_seperate(classes.copy(), adj, None, 1)
    ids = np.asarray(ids).copy()
    ids[np.isin(ids, [i for i, d in enumerate(info) if d['category_id'] == 1])] = 0
    touch = np.add.reduceat((ids == 0)[nbrs].astype(np.int64), offs[:-1]) > 0
    seeds = np.random.default_rng(seed).choice(np.nonzero((ids != 0) & touch)[0], 40, replace=False)
    want = cvseg_ref.color_segment(None, adj, colors, ids.copy(), seeds, 0.3, (0,), 10)

    def call(t, between=nop):
        from Fusion3DSeg.segUtils.cv import CVSegmentation
        return CVSegmentation(t['ids'], _adj(t)).color_segment(t['colors'], t['ids'], t['seeds'], 0.3, (0,), 10)

    def check(got, want):
        F.same(got, want)
        assert (want != ids).sum() > 50
    return dict(colors=colors, ids=ids, offsets=offs, neighbours=nbrs, seeds=seeds), call, want, check, want


# ---- meshUtils --------------------------------------------------------------------------------------------------------------------------------
def _mesh_scene(seed):
    rng = np.random.default_rng(seed)
    verts, tris = mesh_ref.grid_mesh(40, 41, rng)
    tris = np.ascontiguousarray(tris[rng.permutation(len(tris))][:3001]).astype(np.int64)
    return f32_exact(verts), tris, rng.random(len(verts)) < 0.1


MESH_ALT = {'triangles': [np.int32], 'mask': [np.uint8], 'vertices': F32}


@route('mesh_maps', [SU + 'meshUtils.py::vertex_triangle_mapping', SU + 'meshUtils.py::VertexTriangleMap', SU + 'meshUtils.py::remove_faces_by_vertices',
                     SU + 'meshUtils.py::keep_faces_by_vertices'], ['mesh_vertex_map_dev', 'mesh_remove_faces_dev', 'mesh_keep_faces_dev'],
       syncs=True, alt=MESH_ALT)
def case_mesh_maps(seed):
    """vertex_triangle_mapping, remove_faces_by_vertices and keep_faces_by_vertices on a device mesh against mesh_ref, exactly."""
    verts, tris, mask = _mesh_scene(seed)
    want = (mesh_ref.vertex_map(tris, len(verts)), mesh_ref.remove_faces(len(verts), tris, mask), mesh_ref.keep_faces(verts, tris, mask))

    def call(t, between=nop):
        from Fusion3DSeg.segUtils import meshUtils
        vmap = meshUtils.vertex_triangle_mapping(t['triangles'], len(verts))
        return (vmap.csr, meshUtils.remove_faces_by_vertices(len(verts), t['triangles'], t['mask']),
                meshUtils.keep_faces_by_vertices(t['vertices'], t['triangles'], t['mask']))

    def check(got, want):
        F.all_same(got[0], want[0])
        nr, rem, o2n = got[1]
        F.same(nr, want[1][0]); F.same(rem.astype(np.int64), want[1][1]); F.same(o2n, want[1][2])
        F.same(got[2][0].astype(np.float64), want[2][0]); F.same(got[2][1].astype(np.int64), want[2][1])      # (vertices come back in their dtype)
    return dict(vertices=verts, triangles=tris, mask=mask), call, want, check, want[0][1].reshape(-1, 3)


@route('mesh_clusters', [SU + 'meshUtils.py::get_triangle_clusters', SU + 'meshUtils.py::clean_mesh', SU + 'meshUtils.py::face_normals',
                         SU + 'meshUtils.py::face_adjacency'],
       ['mesh_triangle_clusters_dev', 'mesh_clean_dev', 'mesh_face_frames_dev', 'mesh_face_graph_dev'], syncs=True, alt=MESH_ALT)
def case_mesh_clusters(seed):
    """get_triangle_clusters (areas within mesh_ref.area_bound), clean_mesh (mesh_ref.ref_clean), face_normals and face_adjacency
    (face_graph_ref) on a device mesh, exactly."""
    verts, tris, mask = _mesh_scene(seed)
    want = (mesh_ref.clusters(verts, tris), mesh_ref.ref_clean(verts, tris, mask, 3, 0.0), face_graph_ref.face_frames(verts, tris),
            face_graph_ref.graph_of(verts, tris, 30)[:2])

    def call(t, between=nop):
        from Fusion3DSeg.segUtils import meshUtils
        mesh = (t['vertices'], t['triangles'])
        return (meshUtils.get_triangle_clusters(mesh, True), meshUtils.clean_mesh(t['vertices'], t['triangles'], t['mask'], 3, 0.0),
                meshUtils.face_normals(mesh, return_centroids=True, return_areas=True), meshUtils.face_adjacency(mesh, max_angle=30))

    def check(got, want):
        (cl, n, ca, ta), (wcl, wn, wca, wta) = got[0], want[0]
        F.same(cl, wcl); F.same(n, wn); F.same(ta, wta)
        assert ca.dtype == np.float64 and ca.shape == wca.shape and np.all(np.abs(ca - wca) <= mesh_ref.area_bound(wn, wca))
        for g, w in zip(got[1], want[1]):
            assert np.array_equal(np.asarray(g), np.asarray(w)) and g.shape == np.asarray(w).shape
        F.all_same(got[2], want[2]); F.all_same(got[3], want[3])
    return dict(vertices=verts, triangles=tris, mask=mask), call, want, check, want[2][0]


def _raster_scene(seed):
    from f3d import synth
    verts, tris = raster_ref.scene_mesh(N, seed)
    K, q, t, masks, _ = F.ring_scene(seed, 2)
    return f32_exact(verts), np.ascontiguousarray(tris, np.int64), f32_exact(synth.cloud(N, seed=seed + 100)), K, q, t, masks


@route('label_faces', [SU + 'meshUtils.py::label_faces', SU + 'meshUtils.py::segment_faces_from_votes', SU + 'meshUtils.py::segment_faces'],
       ['vote_faces_dev', 'segment_votes_dev', 'smooth_segment_dev', 'mesh_face_graph_dev'], syncs=True, alt={'triangles': [np.int32], 'vertices': F32})
def case_label_faces(seed):
    """label_faces (votes against raster_ref.face_votes, classes against the oracle's segment), segment_faces_from_votes without smoothing
    and segment_faces with one smoothing pass (smooth_ref over face_graph_ref's graph) on a device mesh, exactly."""
    verts, tris, _, K, q, t, masks = _raster_scene(seed)
    _, uv2tri, _ = raster_ref.lookups(verts, tris, K, q, t, (H, W), 10)
    votes = raster_ref.face_votes(uv2tri, masks, len(tris))
    offs, nbrs = face_graph_ref.graph_of(verts, tris, None)[:2]
    plain = O.segment(votes, 133, 0.5)
    smooth = smooth_ref.smooth_segment(votes, offs, nbrs, 133, 0.5)
    want = (plain, votes, (plain, face_graph_ref.components(offs, nbrs, plain)), (smooth, face_graph_ref.components(offs, nbrs, smooth)))

    def call(tt, between=nop):
        from Fusion3DSeg.segUtils import meshUtils
        cls, dvotes = meshUtils.label_faces(tt['vertices'], tt['triangles'], K, q, t, tt['masks'], 10, 133, 0.5, None, True)
        adj = meshUtils.face_adjacency(tt['triangles'], vertices=tt['vertices'])
        return (cls, dvotes, meshUtils.segment_faces_from_votes(dvotes, adj, 133, 0.5, smooth_iterations=0),
                meshUtils.segment_faces(tt['vertices'], tt['triangles'], K, q, t, tt['masks'], 10, 133, 0.5))

    def check(got, want):
        F.same(got[0], want[0]); F.same(got[1], want[1])
        for (classes, ids, info), (wclasses, (count, lab)) in zip(got[2:], want[2:]):          # as tests/test_face_graph_gpu.py: the classes exactly,
            F.same(classes, wclasses)                                                          #   one record per instance id
            expected = np.where(wclasses == 133, count, lab)                                   # the unclassified faces are one semantic record,
            assert planes_ref.same_partition(ids, expected)                                    #   every other class splits into its components
            assert len(info) == len(np.unique(expected)) and [r['area'] for r in info] == np.bincount(ids).tolist()
    return dict(vertices=verts, triangles=tris, masks=masks), call, want, check, uv2tri.reshape(2 * H, W)


# ---- voting -----------------------------------------------------------------------------------------------------------------------------------
@route('vote_frames', [SU + 'voting.py::PointVotingSegmentation'], ['point_vote_frames_dev'], syncs=True, alt={'frames': F32}, names={'frames': 'points'})
def case_vote_frames(seed):
    """PointVotingSegmentation.vote_frames on device frames against point_voting_ref.vote: integer counts, exact."""
    rng = np.random.default_rng(seed)
    pts, r = F.cloud(rng), 0.06
    frames = f32_exact(rng.uniform(0.0, 1.0, (2, H * W, 3)))
    masks = rng.integers(0, 8, (2, H * W)).astype(np.uint8)
    want = point_voting_ref.vote(np.zeros((N, 9)), pts, frames, masks, r)

    def call(t, between=nop):
        from Fusion3DSeg.segUtils.voting import PointVotingSegmentation
        return PointVotingSegmentation(None, pts, (H, W), None, 8).vote_frames(t['frames'], t['masks'], r)
    return dict(frames=frames, masks=masks), call, want, F.same, want


SMOOTH_ANGLE = 78.0


def _smooth_scene(seed):
    pts, _, _, (offs, nbrs) = blob(seed)
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 9, (N, 70)).astype(np.float64)
    u = rng.integers(0, 65536, (N, 70)).astype(np.uint16)
    nrm = rng.standard_normal((N, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return v, u, nrm, offs, nbrs, dict(normals=nrm, cos_angle=math.cos(math.radians(SMOOTH_ANGLE)), self_weight=2.0, iterations=2)


SMOOTH_ALT = {'offsets': [np.int32], 'neighbours': [np.int64]}


@route('smooth_votes', [SU + 'voting.py::smooth_votes'], ['smooth_votes_dev'], syncs=True, alt=SMOOTH_ALT, names={'offsets': 'CSR', 'neighbours': 'CSR'})
def case_smooth_votes(seed):
    """voting.smooth_votes (float64 gated by normals, two iterations; uint16) on device votes against smooth_ref.smooth, exactly."""
    v, u, nrm, offs, nbrs, kw = _smooth_scene(seed)
    want = (smooth_ref.smooth(v, offs, nbrs, **kw), smooth_ref.smooth(u, offs, nbrs))

    def call(t, between=nop):
        from Fusion3DSeg.segUtils import voting
        return (voting.smooth_votes(t['votes'], _adj(t), normals=t['normals'], angle=SMOOTH_ANGLE, self_weight=2.0, iterations=2),
                voting.smooth_votes(t['counts'], _adj(t)))
    return dict(votes=v, counts=u, normals=nrm, offsets=offs, neighbours=nbrs), call, want, F.all_same, want[1]


@route('smooth_segment', [SU + 'voting.py::smooth_segment'], ['smooth_segment_dev'], syncs=True, alt=SMOOTH_ALT, names={'offsets': 'CSR', 'neighbours': 'CSR'})
def case_smooth_segment(seed):
    """voting.smooth_segment on device votes against smooth_ref.smooth_segment, exactly."""
    v, _, nrm, offs, nbrs, kw = _smooth_scene(seed)
    want = smooth_ref.smooth_segment(v, offs, nbrs, 69, 0.3, **kw)

    def call(t, between=nop):
        from Fusion3DSeg.segUtils import voting
        return voting.smooth_segment(t['votes'], _adj(t), 69, 0.3, normals=t['normals'], angle=SMOOTH_ANGLE, self_weight=2.0, iterations=2)
    return dict(votes=v, normals=nrm, offsets=offs, neighbours=nbrs), call, want, F.same, smooth_ref.smooth(v, offs, nbrs, **kw)


# ---- fusion.py: z-buffer renders ------------------------------------------------------------------------------------------------------------------
def _render_scene(seed):
    from f3d import synth
    K, q, t, masks, _ = F.ring_scene(seed, 3)
    return f32_exact(synth.cloud(N, seed=seed)), K, q, t, masks


@route('render_lookups', [FU + 'render_lookups'], ['render_lookups_dev'], alt={'points': F32})
def case_render_lookups(seed):
    """fusion.render_lookups (splat 1) on a device cloud against render_ref.lookups, exactly."""
    pts, K, q, t, _ = _render_scene(seed)
    want = render_ref.lookups(pts, K, q, t, (H, W), 10, 1)

    def call(tt, between=nop):
        from Fusion3DSeg import fusion
        return fusion.render_lookups(tt['points'], K, q, t, (H, W), 10, 1)
    return dict(points=pts), call, want, F.all_same, want[0].reshape(3 * H, W)


@route('vote_visible', [FU + 'project_vote_argmax_visible'], ['vote_visible_dev', 'segment_votes_dev'], syncs=True, alt={'points': F32})
def case_vote_visible(seed):
    """fusion.project_vote_argmax_visible on device tensors against render_ref.visible_votes and the oracle's segment, exactly."""
    pts, K, q, t, masks = _render_scene(seed)
    votes = render_ref.visible_votes(pts, K, q, t, masks, 10, 1, 0.05)
    want = (O.segment(votes, 133, 0.5), votes)

    def call(tt, between=nop):
        from Fusion3DSeg import fusion
        return fusion.project_vote_argmax_visible(tt['points'], K, q, t, tt['masks'], 10, 133, 0.5, None, True, 1, 0.05)
    return dict(points=pts, masks=masks), call, want, F.all_same, render_ref.lookups(pts, K, q, t, (H, W), 10, 1)[0].reshape(3 * H, W)


@route('render_mesh_lookups', [FU + 'render_mesh_lookups'], ['render_mesh_lookups_dev'], syncs=True, alt={'triangles': [np.int32], 'vertices': F32})
def case_render_mesh_lookups(seed):
    """fusion.render_mesh_lookups on a device mesh against raster_ref.lookups, exactly."""
    verts, tris, _, K, q, t, _ = _raster_scene(seed)
    want = raster_ref.lookups(verts, tris, K, q, t, (H, W), 10)

    def call(tt, between=nop):
        from Fusion3DSeg import fusion
        return fusion.render_mesh_lookups(tt['vertices'], tt['triangles'], K, q, t, (H, W), 10)
    return dict(vertices=verts, triangles=tris), call, want, F.all_same, want[0].reshape(2 * H, W)


@route('vote_occluded', [FU + 'project_vote_argmax_occluded'], ['vote_visible_mesh_dev', 'segment_votes_dev'], syncs=True,
       alt={'triangles': [np.int32], 'vertices': F32, 'points': F32})
def case_vote_occluded(seed):
    """fusion.project_vote_argmax_occluded on device tensors against raster_ref.visible_votes and the oracle's segment, exactly."""
    verts, tris, pts, K, q, t, masks = _raster_scene(seed)
    depth, _, _ = raster_ref.lookups(verts, tris, K, q, t, (H, W), 10)
    votes = raster_ref.visible_votes(pts, depth, K, q, t, masks, 10, 0.05)
    want = (O.segment(votes, 133, 0.5), votes)

    def call(tt, between=nop):
        from Fusion3DSeg import fusion
        return fusion.project_vote_argmax_occluded(tt['points'], tt['vertices'], tt['triangles'], K, q, t, tt['masks'], 10, 133, 0.5, None, True, 0.05)
    return dict(points=pts, vertices=verts, triangles=tris, masks=masks), call, want, F.all_same, depth.reshape(2 * H, W)


# ---- fusion.py: the frame loop, feeding a voting session through its lookup_sink ------------------------------------------------------------------
NFRAMES = 4
FUSION_ENTRIES = ['project_view_dev', 'fusion_hits_dev', 'patch_match_dev', 'fusion_seed_update_dev', 'fusion_lookup_dev', 'fusion_frame_check_dev',
                  'fusion_prio_dev', 'patch_seeds_sums_dev', 'fusion_new_seeds_dev']


@route('fuse_device_votes', [FU + 'Fusion', SU + 'voting.py::VotingSegmentation'], FUSION_ENTRIES + ['vote_uv2pt_batch_dev'], syncs=True, stateful=True,
       names={f'{what}{j}': 'valid' if what == 'valid' else 'frame tensors' for j in range(NFRAMES) for what in ('points', 'normals', 'colors', 'valid')})
def case_fuse_device_votes(seed):
    """Fusion.fuse_device on frames of device tensors against the oracle's fuse, bit for bit (cloud, lookups in order, the generator's next
    draw), while its lookup_sink feeds every frame's device lookup to the voting session of VotingSegmentation.vote (voting._DeviceVotes, one
    add_frames per frame): the downloaded votes against the oracle's vote_frame over the oracle's lookups, exactly."""
    params = (0.03, 15, None, 10, 1)
    K, q, tr, frames = fusion_scenes.curved_capture(H, W, NFRAMES, seed, quirks=False)
    masks = np.random.default_rng(seed).integers(0, 133, (NFRAMES, H * W)).astype(np.uint8)
    fused = fusion_scenes.run_fuse(K, W, H, q, tr, fusion_scenes.copy_frames(frames), params, 5, 'oracle')
    slot = {fr[0]: j for j, fr in enumerate(frames)}
    votes = np.zeros((NFRAMES * H * W, 134))
    for name, lut in fused[1]:
        O.vote_frame(votes, lut, masks[slot[name]])
    inputs = {'masks': masks}
    for j, (_, p, n, c, v) in enumerate(frames):
        inputs.update({f'points{j}': p, f'normals{j}': n, f'colors{j}': c, f'valid{j}': v})

    def call(t, between=nop):
        from Fusion3DSeg.fusion import Fusion
        from Fusion3DSeg.segUtils import voting
        session = voting._DeviceVotes(_ctx(), np.zeros((NFRAMES * H * W, 134)))
        lookups = []

        def sink(name, lut):
            lookups.append((name, lut.clone()))
            session.add_frames([lut], [t['masks'][slot[name]]], H, W)
            between()
        dev_frames = [(fr[0], t[f'points{j}'], t[f'normals{j}'], t[f'colors{j}'], t[f'valid{j}']) for j, fr in enumerate(frames)]
        fu = Fusion.from_frames(K, W, H, q, tr, dev_frames, lookup_sink=sink)
        np.random.seed(5)
        out = fu.fuse_device(*params)
        after = np.random.random()
        return list(out), lookups, after, session.download()

    def check(got, want):
        fusion_scenes.assert_same_fuse(tuple(got[:3]) + (None,), want[0])
        F.same(got[3], want[1])
        assert want[1].sum() > 1000
    return inputs, call, (fused, votes), check, fused[0][0]


# ---- merge_intersecting_bb.HipCloud ----------------------------------------------------------------------------------------------------------------
def _corner_sets_equal(a, b, tol=1e-8):
    """Two boxes' corners as sets within 1e-8: the comparison of tests/test_mirror_gpu.py (the corner order is a convention)."""
    d = np.abs(a[:, None, :] - b[None, :, :]).max(-1)
    return (d.min(1) < tol).all() and (d.min(0) < tol).all()


@route('HipCloud', ['Fusion3DSeg/merge_intersecting_bb.py::HipCloud'],
       ['group_by_id_dev', 'obb_extremes_dev', 'obb_hull_filter_dev', 'obb_candidates_dev', 'gather_points_dev', 'obb_fit_dev', 'points_in_obb_dev',
        'relabel_dev'], syncs=True, inplace=('ids',), names={'points': 'cloud'})
def case_hip_cloud(seed):
    """HipCloud on a resident cloud and resident ids, in the order merge_bb uses it: group, extremes, hull_filter, candidates_and_boxes,
    cooccurrence, relabel, fit_indices -- by the properties of family_cases.case_obb (the grouping exactly; extremes are members with the
    extreme float32 dot; survivors and candidates are members and hold every hull vertex), the boxes as corner sets within 1e-8 of the
    oracle's box of all members, the co-occurrences and the relabelled ids exactly."""
    from scipy.spatial import ConvexHull
    from Fusion3DSeg import merge_intersecting_bb as M
    rng = np.random.default_rng(seed)
    nids = 6
    ids = rng.integers(-1, nids + 1, N).astype(np.int64)
    ids[ids == 2] = 3
    ids[ids < 0] = nids                                                          # resident ids lie in [0, 2^30): strays get an id past nids
    centres = rng.uniform(-4, 4, (nids + 1, 3))
    pts = centres[np.clip(ids, 0, nids)] + rng.normal(size=(N, 3)) * [0.4, 0.2, 0.1]
    axes = np.linalg.qr(rng.standard_normal((5, 3, 3)))[0]
    bc, be = centres[rng.integers(0, nids, 5)] + rng.normal(0, 0.2, (5, 3)), rng.uniform(0.4, 1.5, (5, 3))
    packed = np.concatenate([bc, axes.reshape(5, 9), be], axis=1)
    inside = np.stack([O.points_in_obb(pts, bc[b], axes[b], be[b]) for b in range(5)], axis=1)
    want = F.grouping(ids, nids) + ((inside[:, :, None] & inside[:, None, :]).any(axis=0).astype(np.uint8), np.where(ids == 3, 5, ids))

    def call(t, between=nop):
        cloud = M.HipCloud(t['points'])
        order, starts = cloud.group(t['ids'], nids)
        assert order is None
        ext = cloud.extremes()
        fstart, eqs, margin = np.zeros(nids + 1, np.int32), [], np.zeros(nids)
        for k in range(nids):
            e = np.unique(ext[k][ext[k] >= 0])
            if len(e) >= 4 and k != 4:
                eqs.append(ConvexHull(pts[e]).equations)
                fstart[k + 1] = len(eqs[-1])
                margin[k] = 1e-9 * (np.abs(pts[e]).max() + 1)
        np.cumsum(fstart, out=fstart)
        survivors = cloud.hull_filter(fstart, np.concatenate(eqs), margin)
        boxes = cloud.candidates_and_boxes(256)
        cooc = cloud.cooccurrence(packed)
        cloud.relabel(t['ids'], 3, 5)
        refit = cloud.fit_indices([np.flatnonzero((ids == 3) | (ids == 5)).astype(np.int32)])      # as merge_bb refits after an absorb
        return cloud.d_order, starts, ext, fstart, survivors, boxes, cooc, t['ids'], refit

    def check(got, want):
        order, starts, ext, fstart, (cand, cnt), (dcand, dcs, boxes, status), cooc, relabelled, (rbox, rstatus) = got
        F.same(order, want[0]); F.same(starts, want[1]); F.same(cooc, want[2]); F.same(relabelled, want[3])
        F.check_extremes(ids, pts, ext, nids)
        assert (ext[2] == -1).all() and dcs[0] == 0 and (np.diff(dcs) >= 0).all()
        dropped = 0
        for k in range(nids):
            mem = np.flatnonzero(ids == k)
            c = np.sort(cand[starts[k]:starts[k] + cnt[k]])
            dc = dcand[dcs[k]:dcs[k + 1]]
            assert set(c.tolist()) <= set(mem.tolist()) and np.array_equal(dc, np.sort(dc)) and set(dc.tolist()) <= set(mem.tolist()), k
            if len(mem) == 0:
                continue
            if fstart[k + 1] == fstart[k]:
                assert np.array_equal(c, mem), k
            hull = set(mem[ConvexHull(pts[mem]).vertices].tolist())
            assert hull <= set(c.tolist()) and hull <= set(dc.tolist()), k
            for some in (c, dc):
                for a, b in zip(O.obb_from_points(pts[some]), O.obb_from_points(pts[mem])):
                    assert np.array_equal(a, b), k
            assert status[k] == f3d.OBB_OK, (k, status[k])
            assert _corner_sets_equal(M.obb_corners(boxes[k, 0:3], boxes[k, 3:12].reshape(3, 3), boxes[k, 12:15]),
                                      M.obb_corners(*O.obb_from_points(pts[mem]))), k
            dropped += len(mem) - len(dc)
        assert dropped > 0
        merged = pts[(ids == 3) | (ids == 5)]
        assert rstatus[0] == f3d.OBB_OK
        assert _corner_sets_equal(M.obb_corners(rbox[0, 0:3], rbox[0, 3:12].reshape(3, 3), rbox[0, 12:15]), M.obb_corners(*O.obb_from_points(merged)))
    return dict(points=pts, ids=ids), call, want, check, np.stack([want[0], want[3].astype(np.int32)], axis=1)


# ---- reconstruct ------------------------------------------------------------------------------------------------------------------------------
TSDF_DIMS, TSDF_VS, TSDF_LO, TSDF_TRUNC, TSDF_MAX_DEPTH = (37, 29, 21), 0.05, np.array([-0.9, -0.7, 0.55]), 0.2, 4.0


@route('TSDFVolume', [SU + 'reconstruct.py::TSDFVolume'],
       ['tsdf_integrate_dev', 'tsdf_integrate_color_dev', 'tsdf_extract_count_dev', 'tsdf_extract_fill_dev', 'tsdf_extract_colors_dev'], syncs=True,
       stateful=True, alt={'depths': [np.float32]})
def case_tsdf_volume(seed):
    """TSDFVolume on the device: integrate in two calls -> extract_mesh against tsdf_ref (tsdf, weight and vertices bit for bit, triangles
    exactly), and a colour volume -> extract_mesh(colors=True) against tsdf_color_ref.  The depths are float32-exact."""
    rng = np.random.default_rng(seed)
    eyes = np.array([(0.0, 0.0, 0.0), (-0.5, 0.3, 0.8), (0.6, -0.4, 0.3)]) + rng.uniform(-0.05, 0.05, (3, 3))
    K, q, t, depths = tsdf_ref.scene([tuple(e) for e in eyes], [(0.0, 0.0, 1.0), (0.05, 0.0, 1.2), (0.0, 0.0, 1.1)], H, W)
    depths[0, 5:9, 7:12] = 0.0
    depths[1, 11:14, 20:26] = np.inf
    depths = depths.astype(np.float32).astype(np.float64)
    rgb = rng.integers(0, 256, (3, 24, 28, 3)).astype(np.uint8)
    z = np.zeros(TSDF_DIMS[::-1], np.float32)
    tsdf, weight = tsdf_ref.integrate(z, z, TSDF_LO, TSDF_VS, TSDF_TRUNC, 64, depths, K, q, t, 1.0, TSDF_MAX_DEPTH)
    ct, cw, color = tsdf_color_ref.integrate_color(z, z, np.zeros(TSDF_DIMS[::-1] + (4,), np.float32), TSDF_LO, TSDF_VS, TSDF_TRUNC, 64, depths, rgb, K, q, t,
                                                   1.0, TSDF_MAX_DEPTH)
    mesh = tuple(tsdf_ref.extract(tsdf, weight, TSDF_LO, TSDF_VS, 1.0))
    want = (tsdf, weight) + mesh + (color,) + mesh + tuple(tsdf_color_ref.vertex_colors(ct, cw, color, 1.0))

    def call(tt, between=nop):
        from Fusion3DSeg.segUtils.reconstruct import TSDFVolume
        vol = TSDFVolume(TSDF_LO, TSDF_DIMS, TSDF_VS, TSDF_TRUNC, 64, device=True)
        vol.integrate(tt['depths'][:2], K, q[:2], t[:2], 1.0, TSDF_MAX_DEPTH)
        between()
        vol.integrate(tt['depths'][2:], K, q[2:], t[2:], 1.0, TSDF_MAX_DEPTH)
        between()
        plain = vol.extract_mesh(1.0)
        cvol = TSDFVolume(TSDF_LO, TSDF_DIMS, TSDF_VS, TSDF_TRUNC, 64, device=True, color=True)
        cvol.integrate(tt['depths'], K, q, t, 1.0, TSDF_MAX_DEPTH, colors=tt['colors'])
        between()
        return (vol.tsdf, vol.weight) + tuple(plain) + (cvol.color,) + tuple(cvol.extract_mesh(1.0, colors=True))

    def check(got, want):
        assert len(got) == len(want) == 9
        for k in (0, 1, 2, 4, 5):
            F.same_bits(got[k], want[k])
        for k in (3, 6, 7, 8):
            F.same(got[k], want[k])
        assert len(want[3]) > 100 and want[8].sum() > 100
    return dict(depths=depths, colors=rgb), call, want, check, want[0].reshape(-1, TSDF_DIMS[0])


@route('depth_images', [SU + 'reconstruct.py::depth_images'], ['rotate_dev'], alt={'valid': [np.uint8]})
def case_depth_images(seed):
    """reconstruct.depth_images on device frames against the oracle's rotate of (p - t) by the inverse pose, exactly."""
    rng = np.random.default_rng(seed)
    _, q, t = F.cameras(rng, 2)
    pts = rng.uniform(0.0, 1.0, (2, 24, 28, 3))
    pts[0, 3, 5, 1] = np.nan
    valid = rng.random((2, 24, 28)) > 0.1
    want = np.zeros((2, 24, 28))
    for f in range(2):
        cam = O.rotate(f3d.quat_inverse(q[f]), (pts[f] - t[f]).reshape(-1, 3))[:, 2].reshape(24, 28)
        ok = np.isfinite(pts[f]).all(axis=-1) & valid[f]
        want[f][ok] = cam[ok]

    def call(tt, between=nop):
        from Fusion3DSeg.segUtils import reconstruct
        return reconstruct.depth_images(tt['frame_points'], q, t, tt['valid'])
    return dict(frame_points=pts, valid=valid), call, want, F.same, want.reshape(-1, 28)


# ---- registration -------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reg_scene(seed):
    """The sphere-and-wall scene of icp_ref: a coloured volume integrated from four of its six frames drawn from the seed, the five model
    maps ray-cast from the first of them, and another of its frames (with holes) at a start pose moved off its true one."""
    I = icp_ref
    K, q, t, depths = tsdf_ref.scene(I.EYES, [(0.05, -0.02, 1.0)] * 6, I.H, I.W)
    rgbs = icp_color_ref.textured_images(K, q, t, depths)
    rng = np.random.default_rng(seed)
    sel = np.sort(rng.permutation(6)[:4])
    z = np.zeros(I.DIMS[::-1], np.float32)
    tsdf, weight, color = tsdf_color_ref.integrate_color(z, z, np.zeros(I.DIMS[::-1] + (4,), np.float32), I.LO, I.VS, I.TRUNC, 64, depths[sel], rgbs[sel],
                                                         K, q[sel], t[sel], 1.0, I.MAX_DEPTH)
    nsteps = int(np.floor(I.MAX_DEPTH / I.VS)) + 1
    m, f = int(sel[0]), int(sel[1])
    maps = icp_color_ref.raycast_color(tsdf, weight, color, I.LO, I.VS, 1.0, K, q[m], t[m], I.H, I.W, 0.0, I.VS, nsteps)
    depth = f32_exact(depths[f])
    depth.reshape(-1)[3::41] = 0.0
    depth.reshape(-1)[11::67] = np.nan
    q0, t0 = I.moved(q[f], t[f], (0.2, 0.9, -0.3), 0.7, rng.uniform(-0.01, 0.01, 3))
    qr, tr = I.moved(q[m], t[m], (0.5, -0.7, 0.4), 2.0, rng.uniform(-0.05, 0.05, 3))
    s = dict(K=K, q=q, t=t, depths=depths, rgbs=rgbs, sel=sel, tsdf=tsdf, weight=weight, color=color, nsteps=nsteps, qm=q[m], tm=t[m], depth=depth,
             rgb=rgbs[f], q0=q0, t0=t0, qr=qr, tr=tr, vertex=maps[0], normal=maps[1], intensity=maps[4])
    for a in s.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return s


def _bits_all(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        F.same_bits(np.asarray(g).reshape(np.shape(w)), w)


@route('raycast', [SU + 'registration.py::raycast'], ['tsdf_raycast_dev', 'tsdf_raycast_color_dev'], owned=('tsdf', 'weight', 'color'))
def case_raycast(seed):
    """registration.raycast of a device volume, with and without colour, against icp_ref.raycast / icp_color_ref.raycast_color, bit for bit."""
    I, s = icp_ref, reg_scene(seed)
    hw = (I.H + 3, I.W - 5)
    ray = (I.LO, I.VS, 1.0, s['K'], s['qr'], s['tr'], hw[0], hw[1], 0.0, I.VS, s['nsteps'])
    want = tuple(I.raycast(s['tsdf'], s['weight'], *ray)) + tuple(icp_color_ref.raycast_color(s['tsdf'], s['weight'], s['color'], *ray))

    def call(t, between=nop):
        from Fusion3DSeg.segUtils import registration
        from Fusion3DSeg.segUtils.reconstruct import TSDFVolume
        vol = TSDFVolume(I.LO, I.DIMS, I.VS, I.TRUNC, 64, color=True)
        vol.tsdf, vol.weight, vol.color = t['tsdf'], t['weight'], t['color']
        args = (vol, s['K'], s['qr'], s['tr'], hw, 1, 0.0, I.MAX_DEPTH, None)
        return tuple(registration.raycast(*args)) + tuple(registration.raycast(*args, colors=True))

    def check(got, want):
        _bits_all(got, want)
        assert (want[2] > 0).sum() > 100
    return dict(tsdf=np.array(s['tsdf']), weight=np.array(s['weight']), color=np.array(s['color'])), call, want, check, want[0]


def _model_inputs(s):
    I = icp_ref
    return dict(depth=np.array(s['depth']), vertex=s['vertex'].reshape(I.H, I.W, 3).copy(), normal=s['normal'].reshape(I.H, I.W, 3).copy(),
                intensity=s['intensity'].reshape(I.H, I.W).copy(), color=np.array(s['rgb']))


ICP_ALT = {'depth': [np.float32]}
ICP_NAMES = {'vertex': 'model_vertex', 'normal': 'model_normal', 'intensity': 'model_intensity'}


@route('icp_sums', [SU + 'registration.py::icp_sums'], ['icp_sums_dev', 'icp_color_sums_dev'], alt=ICP_ALT, names=ICP_NAMES)
def case_icp_sums(seed):
    """registration.icp_sums on device maps, with and without the photometric term, against icp_ref / icp_color_ref, bit for bit."""
    I, s = icp_ref, reg_scene(seed)
    model = (s['vertex'], s['normal'])
    tail = (I.H, I.W, s['K'], s['qm'], s['tm'], 0.1)
    want = (I.icp_sums(s['depth'], s['K'], s['q0'], s['t0'], 1.0, I.MAX_DEPTH, *model, *tail),
            icp_color_ref.icp_color_sums(s['depth'], s['rgb'], s['K'], s['q0'], s['t0'], 1.0, I.MAX_DEPTH, *model, s['intensity'], *tail))

    def call(t, between=nop):
        from Fusion3DSeg.segUtils import registration
        args = (t['depth'], s['K'], s['q0'], s['t0'], t['vertex'], t['normal'], s['K'], s['qm'], s['tm'], 0.1, 1.0, I.MAX_DEPTH)
        return registration.icp_sums(*args), registration.icp_sums(*args, color=t['color'], model_intensity=t['intensity'], color_weight=0.1)

    def check(got, want):
        _bits_all(got, want)
        assert want[0][28] > 500 and want[1][29 + 28] > 100
    return _model_inputs(s), call, want, check, np.stack([s['vertex'][:, 0], s['depth'].reshape(-1)], axis=1)


@route('icp', [SU + 'registration.py::icp'], ['icp_dev', 'icp_color_dev'], syncs=True, alt=ICP_ALT, names=ICP_NAMES)
def case_icp(seed):
    """registration.icp (three rounds) on device maps, with and without the photometric term, against icp_ref.icp / icp_color_ref.icp_color:
    pose and per-round statistics bit for bit."""
    I, s = icp_ref, reg_scene(seed)
    model = (s['vertex'], s['normal'])
    tail = (I.H, I.W, s['K'], s['qm'], s['tm'], 0.1)
    want = (I.icp(s['depth'], s['K'], s['q0'], s['t0'], 1.0, I.MAX_DEPTH, *model, *tail, 3, 100),
            icp_color_ref.icp_color(s['depth'], s['rgb'], s['K'], s['q0'], s['t0'], 1.0, I.MAX_DEPTH, *model, s['intensity'], *tail, 0.1, 3, 100))

    def call(t, between=nop):
        from Fusion3DSeg.segUtils import registration
        args = (t['depth'], s['K'], s['q0'], s['t0'], t['vertex'], t['normal'], s['K'], s['qm'], s['tm'], 0.1, 1.0, I.MAX_DEPTH, 3, 100)
        return registration.icp(*args), registration.icp(*args, color=t['color'], model_intensity=t['intensity'], color_weight=0.1)

    def check(got, want):
        for (gq, gt, info), (pose, stats, status) in zip(got, want):
            F.same_bits(gq, pose[:4]); F.same_bits(gt, pose[4:])
            assert info['status'] == status == I.OK
            F.same_bits(info['counts'], np.ascontiguousarray(stats[:, 0]))
            with np.errstate(all='ignore'):
                F.same_bits(info['rms'], np.sqrt(stats[:, 1] / np.where(stats[:, 0] > 0, stats[:, 0], 1.0)))
        F.same_bits(got[1][2]['color_counts'], np.ascontiguousarray(want[1][1][:, 3]))
    return _model_inputs(s), call, want, check, np.stack([s['vertex'][:, 0], s['depth'].reshape(-1)], axis=1)


@route('track_frames', [SU + 'registration.py::track_frames'], ['tsdf_raycast_dev', 'icp_dev', 'tsdf_integrate_dev'], syncs=True, stateful=True)
def case_track_frames(seed):
    """registration.track_frames of three device frames into an empty device volume (between() before every integrate) against
    icp_ref.track_frames: poses, status and the volume bit for bit."""
    I, s = icp_ref, reg_scene(seed)
    sel = s['sel'][:3]
    depths = np.ascontiguousarray(s['depths'][sel])
    pq, pt = I.tracking_priors(s['q'][sel], s['t'][sel], seed)
    z = np.zeros(I.DIMS[::-1], np.float32)
    want = I.track_frames(z, z, I.LO, I.VS, I.TRUNC, 64, depths, s['K'], pq, pt, 1.0, I.MAX_DEPTH, 0.1, 3, 100)

    def call(t, between=nop):
        from Fusion3DSeg.segUtils import registration
        from Fusion3DSeg.segUtils.reconstruct import TSDFVolume
        vol = TSDFVolume(I.LO, I.DIMS, I.VS, I.TRUNC, 64, device=True)
        integrate = vol.integrate

        def stalled_integrate(*a, **k):
            between()
            return integrate(*a, **k)
        vol.integrate = stalled_integrate
        return tuple(registration.track_frames(vol, t['depths'], s['K'], pq, pt, 1.0, I.MAX_DEPTH, 0.1, 3, 100)) + (vol.tsdf, vol.weight)

    def check(got, want):
        _bits_all(got, want)
        assert (want[2] == I.OK).all()
    return dict(depths=depths), call, want, check, want[3].reshape(-1, I.DIMS[0])


# ---- RTAB_utils and get2DSeg -------------------------------------------------------------------------------------------------------------------
@route('frames_world_dev', ['RTAB_utils/ios_rtab.py::frames_world_dev'], ['unproject_depth_batch_dev', 'estimate_normals_batch_dev'], syncs=True)
def case_frames_world(seed):
    """ios_rtab.frames_world_dev of two uint16 depth frames: the points against the oracle's unproject_depth, exactly; the normals by
    normals_ref (rows with a clear eigen-gap within 1e-6 rad of the oracle's, unit length) and facing their camera."""
    rng = np.random.default_rng(seed)
    h, w, r, max_nn = 24, 28, 0.12, 16
    K = np.array([[0.9 * w, 0.0, w / 2.0 - 0.5], [0.0, 0.9 * w, h / 2.0 + 0.25], [0.0, 0.0, 1.0]])
    uu, vv = np.meshgrid(np.arange(w), np.arange(h))
    depth = np.stack([1000.0 + 6.0 * uu + 4.0 * vv + 30.0 * np.sin(0.5 * uu + f) + rng.normal(0, 1.0, (h, w)) for f in range(2)]).astype(np.uint16)
    depth[rng.random(depth.shape) < 0.05] = 0
    xyzw = np.tile([0.0, 0.0, 0.0, 1.0], (2, 1)) + rng.uniform(-0.03, 0.03, (2, 4))
    xyzw /= np.linalg.norm(xyzw, axis=1, keepdims=True)
    xyz = rng.uniform(-0.1, 0.1, (2, 3))
    pts = np.stack([O.unproject_depth(depth[f], K, xyzw[f][[3, 0, 1, 2]], xyz[f]) for f in range(2)])
    refs = [normals_ref.normals(pts[f], r, max_nn) for f in range(2)]

    def call(t, between=nop):
        from RTAB_utils import ios_rtab
        return ios_rtab.frames_world_dev(t['depths'], K, xyzw, xyz, 1000, r, max_nn)

    def check(got, want):
        gp, gn = got
        F.same(gp, want)
        compared = 0
        for f, (wn, gap, degenerate, nb) in enumerate(refs):
            scale = np.array([np.mean(np.einsum('ij,ij->i', pts[f][k], pts[f][k])) if len(k) else 0.0 for k in nb])
            ok = ~degenerate & (gap >= 1e-8 * scale)
            ang = normals_ref.angle(gn[f][ok], wn[ok])
            assert ang.max(initial=0.0) <= 1e-6, ang.max()
            assert np.abs(np.linalg.norm(gn[f], axis=1) - 1.0).max() <= 1e-14
            dots = normals_ref.orient_dots(pts[f], gn[f], xyz[f])
            assert (dots[np.abs(dots) >= 1e-12] < 0).all()
            compared += int(ok.sum())
        assert compared >= h * w
    return dict(depths=depth), call, pts, check, pts.reshape(-1, 3)


def _logits(seed):
    return (np.random.default_rng(seed).standard_normal((2, 21, H, W)) * 3).astype(np.float32)


@route('sem_to_mask_device', ['get2DSeg.py::sem_to_mask_device'], ['sem_logits_to_masks_dev'], inplace=('out',))
def case_sem_to_mask(seed):
    """get2DSeg.sem_to_mask_device of a batch of two logit maps into two planes of a mask tensor against the oracle, exactly."""
    sem = _logits(seed)
    want = np.stack([O.sem_logits_to_mask(sem[b], 0.017, 133) for b in range(2)]).astype(np.uint8)

    def call(t, between=nop):
        import get2DSeg
        return get2DSeg.sem_to_mask_device(t['sem'], t['out'], 0.017, 133)
    return dict(sem=sem, out=np.full((2, H, W), 255, np.uint8)), call, want, F.same, want.reshape(-1, W)


# ---- entries no route of the packages reaches with device tensors: driven directly, through the same protocol ---------------------------------------
def _fused_scene(seed):
    from f3d import synth
    _, K, q, t, max_depth, w, h, _ = fused_families.family('base')
    pts = synth.cloud(N, seed=seed)
    masks = synth.masks(len(t), h, w, 'iid', seed=seed)
    views = f3d.views_build(K, w, h, q, t, max_depth)
    with np.errstate(all='ignore'):
        votes = O.forward_votes(pts, K, q, t, masks, max_depth, ncols=134)
    return pts, masks, views, votes


FUSED_SETTINGS = ((0.5, None), (0.0, [86, 114, 115]))


@route('project_vote_argmax_dev', [], ['project_vote_argmax_dev'])
def case_fused(seed):
    """project_vote_argmax_dev (labels and the vote matrix, with and without a filter) on the base cameras of fused_families against the
    oracle, bit for bit."""
    pts, masks, views, votes = _fused_scene(seed)
    want = (votes,) + tuple(O.segment(votes, 133, thr, flt) for thr, flt in FUSED_SETTINGS)

    @direct
    def call(t, torch, dev, sh):
        ctx, (V, h, w) = _ctx(), masks.shape
        out = []
        for thr, flt in FUSED_SETTINGS:
            cls = torch.full((N,), -7, dtype=torch.int64, device=dev)
            dv = torch.full((N, 134), 0xFFFF, dtype=torch.uint16, device=dev)
            ctx.project_vote_argmax_dev(t['points'].data_ptr(), f3d.F64, N, t['views'].data_ptr(), V, t['masks'].data_ptr(), h, w, 133, thr, flt,
                                        cls.data_ptr(), dv.data_ptr(), sh)
            out += [cls, dv]
        return out

    def check(got, want):
        for k, w_labels in enumerate(want[1:]):
            F.same(got[2 * k], w_labels)
            assert got[2 * k + 1].dtype == np.uint16 and np.array_equal(got[2 * k + 1], want[0])
    return dict(points=pts, views=np.ascontiguousarray(views), masks=masks), call, want, check, want[0]


@route('fuse_chunks', [], ['mask_presence_dev', 'fuse_chunked_begin_dev', 'fuse_chunk_dev', 'code_planes_dev', 'fuse_chunk_coded_dev'], stateful=True)
def case_fuse_chunks(seed):
    """The view-chunked fused call as f3d.sharding.HipChunkEngine drives it (presence, begin, two chunks; then begin, code, two coded
    chunks) against the oracle's labels, exactly; the labels present against np.unique."""
    pts, masks, views, votes = _fused_scene(seed)
    want = (O.segment(votes, 133, 0.5, None), np.unique(masks))

    def call(t, between=nop):
        import torch
        from f3d import sharding
        from f3d.tensors import work_stream
        ctx, dev, (V, h, w) = _ctx(), t['points'].device, masks.shape
        out = []
        with torch.cuda.device(dev), work_stream(dev):
            for coded in (False, True):
                cls = torch.full((N,), -7, dtype=torch.int64, device=dev)
                eng = sharding.HipChunkEngine(ctx, t['points'], f3d.F64, N, t['views'], h, w, 133, 0.5, None, cls)
                eng.begin(eng.presence(t['masks']))
                planes = t['masks']
                if coded:
                    planes = torch.full((V, eng.coded_plane_bytes()), 0xEE, dtype=torch.uint8, device=dev)
                    eng.code(t['masks'], planes)
                for a, b in ((0, V // 2), (V // 2, V)):
                    between()
                    (eng.chunk_coded if coded else eng.chunk)(a, b, planes)
                out += [cls, eng.present]
            for x in out:
                x.record_stream(torch.cuda.current_stream(dev))
        return out

    def check(got, want):
        for k in (0, 2):
            F.same(got[k], want[0])
            F.same(np.flatnonzero(got[k + 1]), want[1].astype(np.int64))
    return dict(points=pts, views=np.ascontiguousarray(views), masks=masks), call, want, check, votes


@route('cloud_sort_cells_dev', [], ['cloud_sort_cells_dev'])
def case_sort(seed):
    """cloud_sort_cells_dev (sentinel-filled outputs) against the stable argsort of sort_ref's keys; the sorted copy is x[perm]."""
    from f3d import synth
    x = synth.cloud(N, seed=seed)
    want = sort_ref.expected_perm(x)

    @direct
    def call(t, torch, dev, sh):
        perm = torch.full((N,), -1, dtype=torch.int32, device=dev)
        xs = torch.full_like(t['points'], float('nan'))
        _ctx().cloud_sort_cells_dev(t['points'].data_ptr(), f3d.F64, N, xs.data_ptr(), perm.data_ptr(), sh)
        return perm, xs

    def check(got, want):
        F.same(got[0], want)
        F.same_bits(got[1], x[want])
    return dict(points=x), call, want, check, want


@route('render_counts_dev', [], ['render_counts_dev'], syncs=True)
def case_render_counts(seed):
    """render_counts_dev (a diagnostic; it synchronises): the samples are those of render_ref.view_samples, exactly; the cells they cover
    lie between the cells render_ref.lookups fills and 9 per sample (splat 1)."""
    pts, K, q, t, _ = _render_scene(seed)
    views = f3d.views_build(K, W, H, q, t, 10)
    ppts, pnrm = O.frustum_planes(K, W, H, q, t, 10)
    samples = sum(len(render_ref.view_samples(pts, K, q[j], t[j], ppts[j], pnrm[j], H, W)[0]) for j in range(3))
    filled = int(np.isfinite(render_ref.lookups(pts, K, q, t, (H, W), 10, 1)[0]).sum())

    @direct
    def call(tt, torch, dev, sh):
        return _ctx().render_counts_dev(tt['points'].data_ptr(), f3d.F64, N, tt['views'].data_ptr(), 3, H, W, 1, sh)

    def check(got, want):
        assert got['samples'] == want[0] and want[1] <= got['cells'] <= 9 * want[0], (got, want)
    return dict(points=pts, views=np.ascontiguousarray(views)), call, (samples, filled), check, pts


@route('raster_counts_dev', [], ['raster_counts_dev'], syncs=True)
def case_raster_counts(seed):
    """raster_counts_dev (a diagnostic; it synchronises): the depth and lookups it renders against raster_ref.lookups, exactly; every
    (triangle, view) pair is walked by at most one tier."""
    verts, tris, _, K, q, t, _ = _raster_scene(seed)
    views = f3d.views_build(K, W, H, q, t, 10)
    want = raster_ref.lookups(verts, tris, K, q, t, (H, W), 10)[:2]

    @direct
    def call(tt, torch, dev, sh):
        depth = torch.full((2, H, W), float('nan'), dtype=torch.float32, device=dev)
        lut = torch.full((2, H * W), -7, dtype=torch.int32, device=dev)
        counts = _ctx().raster_counts_dev(tt['vertices'].data_ptr(), f3d.F64, len(verts), tt['triangles'].data_ptr(), f3d.I64, len(tris),
                                          tt['views'].data_ptr(), 2, H, W, 10, 0, depth.data_ptr(), lut.data_ptr(), sh)
        return depth, lut, counts

    def check(got, want):
        F.same(got[0], want[0]); F.same(got[1], want[1])
        c = got[2]
        assert 0 < c['small'] + c['medium'] + c['huge'] + c['overflow'] <= 2 * len(tris), c
    return dict(vertices=verts, triangles=tris, views=np.ascontiguousarray(views)), call, want, check, want[0].reshape(2 * H, W)


@route('kernels_dev', [], ['segment_votes_lastcol_dev', 'sem_logits_to_mask_dev', 'vote_uv2pt_dev'])
def case_kernels_dev(seed):
    """segment_votes_lastcol_dev against point_voting_ref.segment, sem_logits_to_mask_dev and vote_uv2pt_dev against the oracle, exactly."""
    rng = np.random.default_rng(seed)
    votes = (rng.integers(1, 6, (N, 134)) * (rng.random((N, 134)) < 0.03)).astype(np.float64)
    votes[:, -1] = votes[:, :-1].sum(axis=1)
    lut = rng.integers(-1, N, H * W).astype(np.int32)
    mask = rng.integers(0, 133, H * W).astype(np.uint8)
    sem = _logits(seed)[0]
    want = (point_voting_ref.segment(votes, 133, 0.3), O.sem_logits_to_mask(sem, 0.017, 133).astype(np.uint8), O.vote_frame(np.zeros((N, 134)), lut, mask))

    @direct
    def call(t, torch, dev, sh):
        ctx = _ctx()
        cls = torch.full((N,), -7, dtype=torch.int64, device=dev)
        ctx.segment_votes_lastcol_dev(t['votes'].data_ptr(), N, 134, 133, 0.3, None, cls.data_ptr(), sh)
        out = torch.full((H, W), 255, dtype=torch.uint8, device=dev)
        ctx.sem_logits_to_mask_dev(t['sem'].data_ptr(), 21, H * W, 0.017, 133, out.data_ptr(), sh)
        voted = torch.zeros((N, 134), dtype=torch.float64, device=dev)
        ctx.vote_uv2pt_dev(t['lut'].data_ptr(), t['mask'].data_ptr(), H * W, voted.data_ptr(), N, 134, sh)
        return cls, out, voted
    return dict(votes=votes, sem=sem, lut=lut, mask=mask), call, want, F.all_same, want[2]


@route('tsdf_integrate', [SU + 'reconstruct.py::TSDFVolume'], ['tsdf_integrate_dev', 'tsdf_integrate_color_dev'], stateful=True, alt={'depths': F32})
def case_tsdf_integrate(seed):
    """TSDFVolume.integrate alone, which reads nothing back: a device volume fed in two calls and a colour volume fed in one, against
    tsdf_ref.integrate / tsdf_color_ref.integrate_color, bit for bit.  The whole case is enqueued behind the caller's stall."""
    inputs, _, want, _, rows = TABLE['TSDFVolume'].case(seed)
    rng = np.random.default_rng(seed)
    eyes = np.array([(0.0, 0.0, 0.0), (-0.5, 0.3, 0.8), (0.6, -0.4, 0.3)]) + rng.uniform(-0.05, 0.05, (3, 3))
    K, q, t, _ = tsdf_ref.scene([tuple(e) for e in eyes], [(0.0, 0.0, 1.0), (0.05, 0.0, 1.2), (0.0, 0.0, 1.1)], H, W)

    def call(tt, between=nop):
        from Fusion3DSeg.segUtils.reconstruct import TSDFVolume
        vol = TSDFVolume(TSDF_LO, TSDF_DIMS, TSDF_VS, TSDF_TRUNC, 64, device=True)
        vol.integrate(tt['depths'][:2], K, q[:2], t[:2], 1.0, TSDF_MAX_DEPTH)
        between()
        vol.integrate(tt['depths'][2:], K, q[2:], t[2:], 1.0, TSDF_MAX_DEPTH)
        cvol = TSDFVolume(TSDF_LO, TSDF_DIMS, TSDF_VS, TSDF_TRUNC, 64, device=True, color=True)
        cvol.integrate(tt['depths'], K, q, t, 1.0, TSDF_MAX_DEPTH, colors=tt['colors'])
        return vol.tsdf, vol.weight, cvol.tsdf, cvol.weight, cvol.color

    def check(got, want):
        for g, w in zip(got, (want[0], want[1], want[0], want[1], want[4])):
            F.same_bits(g, w)
        assert (want[1] > 0).sum() > 1000 and (want[4][..., 3] > 0).sum() > 1000
    return inputs, call, want, check, rows


@route('icp_dev', [], ['icp_dev', 'icp_color_dev'])
def case_icp_dev(seed):
    """icp_dev and icp_color_dev (three rounds) driven directly, the view record a device input: nothing is read back, so the rounds are
    enqueued behind the caller's stall.  Pose, statistics and status against icp_ref.icp / icp_color_ref.icp_color, bit for bit."""
    I, s = icp_ref, reg_scene(seed)
    model = (s['vertex'], s['normal'])
    tail = (I.H, I.W, s['K'], s['qm'], s['tm'], 0.1)
    want = (I.icp(s['depth'], s['K'], s['q0'], s['t0'], 1.0, I.MAX_DEPTH, *model, *tail, 3, 100),
            icp_color_ref.icp_color(s['depth'], s['rgb'], s['K'], s['q0'], s['t0'], 1.0, I.MAX_DEPTH, *model, s['intensity'], *tail, 0.1, 3, 100))
    view = f3d.views_build(s['K'], I.W, I.H, s['qm'][None], s['tm'][None], I.MAX_DEPTH)

    @direct
    def call(t, torch, dev, sh):
        ctx, out = _ctx(), []
        for colour in (False, True):
            pose = torch.full((7,), float('nan'), dtype=torch.float64, device=dev)
            stats = torch.full((3, 5 if colour else 3), float('nan'), dtype=torch.float64, device=dev)
            status = torch.full((1,), -7, dtype=torch.int32, device=dev)
            head = (t['depth'].data_ptr(), 0, I.H, I.W, s['K'], s['q0'], s['t0'], t['vertex'].data_ptr(), t['normal'].data_ptr(), I.H, I.W,
                    t['view'].data_ptr(), 0.1)
            ends = (1.0, I.MAX_DEPTH, 3, 100, pose.data_ptr(), stats.data_ptr(), status.data_ptr(), sh)
            if colour:
                ctx.icp_color_dev(*head, t['intensity'].data_ptr(), t['color'].data_ptr(), I.H, I.W, 0.1, *ends)
            else:
                ctx.icp_dev(*head, *ends)
            out += [pose, stats, status]
        return out

    def check(got, want):
        for k, (pose, stats, status) in enumerate(want):
            F.same_bits(got[3 * k], pose); F.same_bits(got[3 * k + 1], stats)
            assert got[3 * k + 2].tolist() == [status] == [I.OK]
    return dict(_model_inputs(s), view=np.ascontiguousarray(view)), call, want, check, np.stack([s['vertex'][:, 0], s['depth'].reshape(-1)], axis=1)


# ---- the tables -------------------------------------------------------------------------------------------------------------------------------------
ROUTES = {}
DEV_ENTRIES = {}
for _name, _r in TABLE.items():
    for _route in _r.routes:
        ROUTES.setdefault(_route, []).append(_name)
    for _entry in _r.entries:
        DEV_ENTRIES.setdefault(_entry, []).append(_name)

# What the lens leaves out, each with its reason: a route ('file::name') or a ``*_dev`` method of f3d.Context (at most 8 of those, and
# never the multi-operation entries NEVER_LEFT_OUT names).
NOT_COVERED = {
    SU + 'features.py::classify_features': 'torch.matmul on the current stream of the tensors; no library call and no stream of its own',
    SU + 'lifting.py::split_by_lift': 'torch.unique on the current stream of the tensors; no library call and no stream of its own',
    SU + 'lifting.py::lift_from_dirs': 'reads lookups and maps from files into NumPy arrays: it has no tensor argument (lift_instances is covered)',
    SU + 'planeUtils.py::plane_table': 'copies a PlaneSet to the host (.cpu() on the current stream); no library call (extract_planes is covered)',
    SU + 'transfer.py::clean_mesh_by_points': 'vertex_mask_from_points followed by meshUtils.clean_mesh, both covered; it adds no hand-off',
}
NEVER_LEFT_OUT = ('project_vote_argmax_dev', 'fuse_chunk', 'radius_query', 'estimate_normals_batch_dev', 'tsdf_', 'icp')
MAX_ENTRIES_LEFT_OUT = 8


# ---- what both lenses do with a case -----------------------------------------------------------------------------------------------------------
def upload(inputs, dev):
    """The inputs as fresh device tensors (uploaded through writable copies on the current stream)."""
    import torch
    return {k: torch.from_numpy(np.array(a)).to(dev) for k, a in inputs.items()}


def map_tensors(x, fn):
    """The results of a call with `fn` applied to every tensor in them (tuples, lists, dicts and namespaces are walked)."""
    if hasattr(x, 'is_cuda'):
        return fn(x)
    if isinstance(x, dict):
        return {k: map_tensors(v, fn) for k, v in x.items()}
    if isinstance(x, SimpleNamespace):
        return {k: map_tensors(v, fn) for k, v in vars(x).items()}
    if isinstance(x, (tuple, list)):
        return [map_tensors(v, fn) for v in x]
    return x


def clone_tree(x):
    return map_tensors(x, lambda t: t.clone())


def to_host(x):
    return map_tensors(x, lambda t: t.cpu().numpy())
