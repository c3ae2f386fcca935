"""The face graph on the GPU (f3d_mesh_face_frames, f3d_mesh_face_graph, meshUtils.face_normals / face_adjacency / segment_faces*):
array_equal against the restatement tests/face_graph_ref.py throughout."""
import functools

import numpy as np
import pytest

import f3d
import face_graph_ref as G
import mesh_ref as R
import smooth_ref as S
from oracle.np_ref import segment

pytestmark = pytest.mark.gpu
FILL = -7


def MU():
    from Fusion3DSeg.segUtils import meshUtils
    return meshUtils


def _np(x):
    return x.cpu().numpy() if hasattr(x, 'cpu') else x


def _dev(*arrays):
    import torch
    return tuple(torch.as_tensor(a, device='cuda') for a in arrays)


def _same(got, want):
    got = _np(got)
    assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), (got.dtype, got.shape, want.dtype, want.shape)


def _same_graph(got, want):
    _same(got[0], want[0]); _same(got[1], want[1])
    if len(got) > 2:
        assert got[2] == want[2], (got[2], want[2])


def _cos(angle):
    return None if angle is None else float(np.cos(np.radians(float(angle))))


def _graph_dev(ctx, tris, nv, verts=None, cos_crease=None, cap=None):
    """f3d_mesh_face_graph_dev on sentinel-filled outputs -> (offsets, neighbours, counts) as NumPy arrays."""
    import torch
    from f3d.tensors import dtype_code, index_code
    dt = torch.as_tensor(tris, device='cuda')
    dv = None if verts is None else torch.as_tensor(verts, device='cuda')
    nt = len(tris)
    cap = 3 * nt if cap is None else cap
    offs = torch.full((nt + 1,), FILL, dtype=torch.int64, device='cuda')
    nb = torch.full((cap,), FILL, dtype=torch.int32, device='cuda')
    counts = torch.full((4,), FILL, dtype=torch.int64, device='cuda')
    st = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    ctx.mesh_face_graph_dev(None if dv is None else dv.data_ptr(), f3d.F64 if dv is None else dtype_code(dv), nv, dt.data_ptr(), index_code(dt), nt,
                            cos_crease is not None, cos_crease or 0.0, offs.data_ptr(), nb.data_ptr() if cap else None, cap, counts.data_ptr(), st)
    torch.cuda.synchronize()
    return offs.cpu().numpy(), nb.cpu().numpy(), counts.cpu().numpy()


def _frames_dev(ctx, verts, tris):
    import torch
    from f3d.tensors import dtype_code, index_code
    dv, dt = _dev(verts, tris)
    nt = len(tris)
    nrm = torch.full((nt, 3), float(FILL), dtype=torch.float64, device='cuda')
    cen = torch.full((nt, 3), float(FILL), dtype=torch.float64, device='cuda')
    area = torch.full((nt,), float(FILL), dtype=torch.float64, device='cuda')
    counts = torch.full((4,), FILL, dtype=torch.int64, device='cuda')
    st = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    ctx.mesh_face_frames_dev(dv.data_ptr(), dtype_code(dv), len(verts), dt.data_ptr(), index_code(dt), nt, nrm.data_ptr(), cen.data_ptr(),
                             area.data_ptr(), counts.data_ptr(), st)
    torch.cuda.synchronize()
    return nrm.cpu().numpy(), cen.cpu().numpy(), area.cpu().numpy(), counts.cpu().numpy()


def _all_routes(verts, tris, max_angle, want):
    """Host entry == _dev entry == tensor route == the restatement `want` = (offsets, neighbours, stats)."""
    mu, ctx = MU(), f3d.default_context()
    kw = {} if max_angle is None else {'max_angle': max_angle}
    host = mu.face_adjacency(tris, vertices=verts, return_stats=True, **kw)
    _same_graph(host, want)
    dev = mu.face_adjacency(_dev(tris)[0], vertices=_dev(verts)[0], return_stats=True, **kw)
    assert dev[0].is_cuda and dev[1].is_cuda
    _same_graph(dev, want)
    offs, nb, counts = _graph_dev(ctx, tris, len(verts), None if max_angle is None else verts, _cos(max_angle))
    nnz = len(want[1])
    assert counts.tolist() == [nnz, want[2]['nonmanifold_edges'], 0, want[2]['boundary_edges']]
    if nnz <= len(nb):
        _same(offs, want[0]); _same(nb[:nnz], want[1])
        assert (nb[nnz:] == FILL).all()
    return host


# ------------------------------------------------------------------------------------------------ sizes, dtypes, routes
SIZES = [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 4097]                           # the mesh block holds 256 threads


def _crease(m):
    """A crease angle that cuts some of the mesh's edges and keeps others: the strips (odd m) are nearly flat."""
    return 1 if m % 2 else 20


@functools.lru_cache(maxsize=None)
def _sized(m):
    """(vertices, triangles, {max_angle: restatement}) of the mesh of m faces; built once, never modified."""
    verts, tris = G.sized_mesh(m, np.random.default_rng(1000 + m))
    want = {a: G.graph_of(verts, tris, a) for a in (None, _crease(m))}
    for a in (verts, tris) + tuple(x for w in want.values() for x in w[:2]):
        a.setflags(write=False)
    return verts, tris, want


@pytest.mark.parametrize('m', SIZES)
def test_sizes_dtypes_and_routes(m):
    mu = MU()
    verts, tris, want = _sized(m)
    crease = _crease(m)
    for angle in (None, crease):
        first = _all_routes(verts, tris, angle, want[angle])
        _same_graph(_all_routes(verts, tris.astype(np.int32), angle, want[angle]), first)          # int32 == int64
        again = mu.face_adjacency(tris, vertices=verts, max_angle=angle)                            # equal bits on a repeated call
        assert again[0].tobytes() == first[0].tobytes() and again[1].tobytes() == first[1].tobytes()
    if m >= 63:
        assert 0 < len(want[crease][1]) < len(want[None][1])                                        # the gate cuts some edges, not all
    v32 = verts.astype(np.float32)
    wide = G.graph_of(v32.astype(np.float64), tris, crease)
    _same_graph(_all_routes(v32, tris, crease, wide), wide)                                             # float32 == its widened float64
    _same_graph(mu.face_adjacency(tris, len(verts)), want[None][:2])                                # nvertices alone
    _same_graph(mu.face_adjacency((verts, tris)), want[None][:2])                                   # a mesh pair


def test_mesh_larger_than_one_sweep_of_the_slot_loops():
    """717,602 faces: 3 M = 2,152,806 slots, more than the 8192 x 256 threads of one sweep of the slot loops (the index check, the run
    bounds).  The per-face loops would wrap only beyond 2,097,152 faces, more than a test here should carry; their stride is the same
    macro."""
    rng = np.random.default_rng(7)
    verts, tris = R.grid_mesh(600, 600, rng)
    tris = G.flipped(tris, rng)
    assert 3 * len(tris) > 8192 * 256
    for angle in (None, 20):
        want = G.graph_of(verts, tris, angle)
        got = MU().face_adjacency(_dev(tris)[0], vertices=_dev(verts)[0], max_angle=angle, return_stats=True)
        _same_graph(got, want)
    assert want[2] == {'nonmanifold_edges': 0, 'boundary_edges': 4 * 599}


def test_keys_at_full_width():
    big = [0, 1, 1 << 30, (1 << 31) - 2]
    tris = np.array([[big[0], big[1], big[2]], [big[1], big[2], big[3]], [big[0], big[3], big[1]], [big[2], big[3], big[0]],
                     [big[3], big[3], big[2]]], np.int64)
    want = G.face_graph(tris)
    assert np.diff(want[0]).tolist() == [3, 4, 3, 4, 2]
    nv = (1 << 31) - 1
    _same_graph(MU().face_adjacency(tris, nv, return_stats=True), want)
    _same_graph(MU().face_adjacency(_dev(tris.astype(np.int32))[0], nv, return_stats=True), want)
    with pytest.raises(IndexError):
        MU().face_adjacency(tris, nv - 1)


# ------------------------------------------------------------------------------------------------ non-manifold, duplicates
@pytest.mark.parametrize('k', [3, 4, 33, 70, 300])
def test_book_of_k_faces(k):
    import torch
    mu, ctx = MU(), f3d.default_context()
    verts, tris = G.book(k, np.random.default_rng(k))
    want = G.face_graph(tris)
    assert np.array_equal(np.diff(want[0]), np.full(k, k - 1)) and want[2] == {'nonmanifold_edges': 1, 'boundary_edges': 2 * k}
    for t in (tris, _dev(tris)[0]):                                             # the wrapper's second call makes room
        _same_graph(mu.face_adjacency(t, len(verts), return_stats=True), want)
    gated = G.graph_of(verts, tris, 30)
    assert 0 < len(gated[1]) < len(want[1]) or k < 33
    _same_graph(mu.face_adjacency(tris, vertices=verts, max_angle=30, return_stats=True), gated)
    # at the Context level a capacity of 3 M is too small from k = 5 on: neighbours keeps its sentinel, the counts are right
    nbrs = np.full(3 * k, FILL, np.int32)
    offs, nbrs, counts = ctx.mesh_face_graph(tris, len(verts), neighbours=nbrs)
    assert counts.tolist() == [k * (k - 1), 1, 0, 2 * k] and np.array_equal(offs, want[0])
    offs_d, nbrs_d, counts_d = _graph_dev(ctx, tris, len(verts))
    assert counts_d.tolist() == counts.tolist() and np.array_equal(offs_d, want[0])
    if k * (k - 1) > 3 * k:
        assert (nbrs == FILL).all() and (nbrs_d == FILL).all()
    else:
        assert np.array_equal(nbrs[:len(want[1])], want[1]) and np.array_equal(nbrs_d[:len(want[1])], want[1])
    torch.cuda.synchronize()


def test_duplicates_and_degenerates():
    rng = np.random.default_rng(11)
    verts = rng.uniform(-1, 1, (9, 3))
    tris = np.array([[0, 1, 2], [2, 0, 1], [1, 0, 2],                           # one triple three times, corners permuted
                     [3, 3, 4], [3, 3, 3], [4, 3, 3], [3, 3, 5],                # (v, v, w), (v, v, v); [3, 3, 5] shares only (3, 3)
                     [6, 7, 8], [5, 4, 8]], np.int64)
    want = G.face_graph_dict(tris)
    assert np.diff(want[0]).tolist() == [2, 2, 2, 3, 3, 3, 3, 0, 0]
    assert want[1][want[0][6]:want[0][7]].tolist() == [3, 4, 5]
    _all_routes(verts, tris, None, want)
    normals = G.face_frames(verts, tris)[0]
    assert not normals[3:7].any()                                               # degenerate faces: normal 0, so dot = 0
    for angle in (0, 60, 90, 91, 180):
        _all_routes(verts, tris, angle, G.face_graph_dict(tris, normals, _cos(angle)))


# ------------------------------------------------------------------------------------------------ errors
@pytest.mark.parametrize('bad', [9, -1], ids=['index_V', 'index_minus_1'])
def test_index_error_writes_nothing(bad):
    mu, ctx = MU(), f3d.default_context()
    verts, tris = R.grid_mesh(3, 3, np.random.default_rng(0))
    wrong = tris.copy()
    wrong[5, 2] = bad
    for t, v in ((wrong, verts), _dev(wrong, verts)):
        with pytest.raises(IndexError):
            mu.face_adjacency(t, len(verts))
        with pytest.raises(IndexError):
            mu.face_adjacency(t, vertices=v, max_angle=30)
        with pytest.raises(IndexError):
            mu.face_normals(v, t)
    st = __import__('torch').cuda.current_stream().cuda_stream
    for gate in (None, 0.5):
        offs, nb, counts = _graph_dev(ctx, wrong, len(verts), verts if gate else None, gate)
        assert counts.tolist() == [0, 0, 1, 0] and (offs == FILL).all() and (nb == FILL).all()
        with pytest.raises(IndexError, match='vertex index'):
            ctx.take_device_error(st)
    nrm, cen, area, counts = _frames_dev(ctx, verts, wrong)
    assert counts.tolist() == [0, 0, 1, 0] and (nrm == FILL).all() and (cen == FILL).all() and (area == FILL).all()
    with pytest.raises(IndexError, match='vertex index'):
        ctx.take_device_error(st)
    ctx.take_device_error(st)                                                   # taken: the next read is clean
    _same_graph(mu.face_adjacency(tris, len(verts)), G.face_graph(tris)[:2])


# ------------------------------------------------------------------------------------------------ the gate
def test_gate_on_the_cube():
    verts, tris = G.cube()
    for angle, comps in ((45, 6), (91, 1), (None, 1)):
        want = G.graph_of(verts, tris, angle)
        assert G.components(*want[:2])[0] == comps
        _all_routes(verts, tris, angle, want)
        _all_routes(verts, G.flipped(tris, np.random.default_rng(4)), angle, want)      # whatever the windings


def test_gate_at_an_exact_right_angle_and_on_a_flat_grid():
    ctx = f3d.default_context()
    verts = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])
    tris = np.array([[0, 1, 2], [0, 2, 3]], np.int64)                           # normals (0, 0, 1) and (1, 0, 0): dot is exactly 0
    nrm = G.face_frames(verts, tris)[0]
    assert np.array_equal(nrm, [[0, 0, 1], [1, 0, 0]])
    offs, nbrs, counts = ctx.mesh_face_graph(tris, 4, verts, 0.0)
    assert counts.tolist() == [2, 0, 0, 4] and offs.tolist() == [0, 1, 2] and nbrs[:2].tolist() == [1, 0]
    offs, nbrs, counts = ctx.mesh_face_graph(tris, 4, verts, float(np.nextafter(0, 1)))
    assert counts.tolist() == [0, 0, 0, 4] and offs.tolist() == [0, 0, 0]
    gv, gt = R.grid_mesh(9, 7)                                                  # integer coordinates: every normal is (0, 0, +-1)
    want = G.face_graph(gt)
    offs, nbrs, counts = ctx.mesh_face_graph(gt, len(gv), gv, 1.0)
    assert counts[0] == len(want[1]) and np.array_equal(offs, want[0]) and np.array_equal(nbrs[:counts[0]], want[1])
    mixed = G.flipped(gt, np.random.default_rng(2))                             # a random half of the faces flipped
    assert (mixed != gt).any()
    _same_graph(MU().face_adjacency(mixed, vertices=gv, max_angle=10), want[:2])
    _same_graph(MU().face_adjacency(_dev(mixed)[0], vertices=_dev(gv)[0], max_angle=10), want[:2])


@pytest.mark.parametrize('first', [False, True])
@pytest.mark.parametrize('second', [False, True])
def test_a_sheet_folded_onto_itself_is_cut(first, second):
    verts, tris = G.folded_pair(first, second)
    for angle in (0, 45, 90, 135, 179.9):
        offs, nbrs = MU().face_adjacency(tris, vertices=verts, max_angle=angle)
        assert offs.tolist() == [0, 0, 0] and len(nbrs) == 0, angle
    for kw in ({'max_angle': 180}, {}):
        offs, nbrs = MU().face_adjacency(tris, vertices=verts, **kw)
        assert offs.tolist() == [0, 1, 2] and nbrs.tolist() == [1, 0]


def test_a_nan_vertex_isolates_its_faces_when_gated():
    verts, tris = R.grid_mesh(8, 8)
    verts = verts.copy()
    verts[27, 1] = np.nan
    touched = (tris == 27).any(axis=1)
    assert touched.sum() == 6
    plain = G.face_graph(tris)
    _all_routes(verts, tris, None, plain)                                       # ungated: the coordinates play no part
    want = G.graph_of(verts, tris, 45)
    got = _all_routes(verts, tris, 45, want)
    assert (np.diff(got[0])[touched] == 0).all() and (np.diff(got[0])[~touched] > 0).all()
    assert not np.isin(got[1], np.nonzero(touched)[0]).any()


# ------------------------------------------------------------------------------------------------ properties
@pytest.mark.parametrize('name', ['random', 'grid'])
def test_rows_components_and_areas(name):
    rng = np.random.default_rng(21)
    if name == 'random':
        verts, tris = R.random_mesh(400, 3000, rng)
    else:
        verts, tris = R.grid_mesh(40, 40, rng)
        tris = tris[rng.permutation(len(tris))][:2500]
    mu = MU()
    offs, nbrs, stats = mu.face_adjacency(tris, vertices=verts, return_stats=True)
    _same_graph((offs, nbrs, stats), G.face_graph(tris))
    m = len(tris)
    rows = np.repeat(np.arange(m), np.diff(offs))
    flat = rows * m + nbrs
    assert (np.diff(flat) > 0).all() and (rows != nbrs).all()                   # strictly ascending rows, never the face itself
    assert np.array_equal(np.sort(nbrs.astype(np.int64) * m + rows), flat)      # symmetric
    clusters, cluster_n, _, tri_area = mu.get_triangle_clusters((verts, tris), True)
    count, lab = G.components(offs, nbrs)
    assert count == len(cluster_n) and np.array_equal(lab, clusters)
    normals, centroids, areas = mu.face_normals(verts, tris, True, True)
    assert areas.tobytes() == tri_area.tobytes()
    want = G.face_frames(verts, tris)
    _same(normals, want[0]); _same(centroids, want[1]); _same(areas, want[2])


# ------------------------------------------------------------------------------------------------ face_normals
def test_face_normals_against_the_restatement():
    mu = MU()
    rng = np.random.default_rng(31)
    verts, tris = R.random_mesh(500, 4097, rng)
    tris[7] = [3, 3, 9]                                                         # a repeated vertex
    for v in (verts, verts.astype(np.float32)):
        want = G.face_frames(v, tris)
        for vx, tx in ((v, tris), (v, tris.astype(np.int32)), _dev(v, tris)):
            got = mu.face_normals(vx, tx, True, True)
            for g, w in zip(got, want):
                _same(g, w)
        _same(mu.face_normals((v, tris)), want[0])
        _same(mu.face_normals(v, tris, return_areas=True)[1], want[2])
    repeated = (tris[:, 0] == tris[:, 1]) | (tris[:, 0] == tris[:, 2]) | (tris[:, 1] == tris[:, 2])
    assert repeated[7] and not want[0][repeated].any() and np.allclose(np.linalg.norm(want[0][~repeated], axis=1), 1.0)
    ctx = f3d.default_context()
    nrm, cen, area, counts = _frames_dev(ctx, verts, tris)                      # host entry == _dev entry
    want = G.face_frames(verts, tris)
    _same(nrm, want[0]); _same(cen, want[1]); _same(area, want[2])
    assert counts.tolist() == [0, 0, 0, 0]


def test_face_normals_where_the_length_underflows_or_overflows():
    base = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.5]])
    tris = np.array([[0, 1, 2], [1, 3, 2]], np.int64)
    for scale, area in ((1e-160, 0.0), (1e150, np.inf)):
        want = G.face_frames(base * scale, tris)
        assert not want[0].any() and (want[2] == area).all()
        got = MU().face_normals(base * scale, tris, True, True)
        for g, w in zip(got, want):
            _same(g, w)
    got = MU().face_normals(base, tris)
    _same(got, G.face_frames(base, tris)[0])
    assert got[0].tolist() == [0, 0, 1]


# ------------------------------------------------------------------------------------------------ strict context
def test_strict_context_after_reserve():
    import torch
    from f3d.tensors import dtype_code, index_code
    verts, tris, want = _sized(4097)
    nv, nt = len(verts), len(tris)
    ctx = f3d.Context(0)
    ctx.reserve_mesh(nv, nt)
    dv, dt = _dev(verts, tris)
    offs = torch.empty(nt + 1, dtype=torch.int64, device='cuda')
    nb = torch.empty(3 * nt, dtype=torch.int32, device='cuda')
    nrm = torch.empty((nt, 3), dtype=torch.float64, device='cuda')
    counts = torch.empty(4, dtype=torch.int64, device='cuda')
    st = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    ctx.set_strict(True)
    before = ctx.alloc_count
    ctx.mesh_face_frames_dev(dv.data_ptr(), dtype_code(dv), nv, dt.data_ptr(), index_code(dt), nt, nrm.data_ptr(), None, None, counts.data_ptr(), st)
    ctx.mesh_face_graph_dev(dv.data_ptr(), dtype_code(dv), nv, dt.data_ptr(), index_code(dt), nt, True, _cos(1), offs.data_ptr(), nb.data_ptr(),
                            3 * nt, counts.data_ptr(), st)
    ctx.take_device_error(st)
    assert ctx.alloc_count == before
    nnz = int(counts[0])
    _same(offs, want[1][0]); _same(nb[:nnz], want[1][1]); _same(nrm, G.face_frames(verts, tris)[0])
    ctx.close()
    small = f3d.Context(0)
    small.reserve_mesh(16, 16)
    small.set_strict(True)
    with pytest.raises(MemoryError, match='strict context'):
        small.mesh_face_graph_dev(None, f3d.F64, nv, dt.data_ptr(), index_code(dt), nt, False, 0.0, offs.data_ptr(), nb.data_ptr(), 3 * nt,
                                  counts.data_ptr(), st)
    small.close()


# ------------------------------------------------------------------------------------------------ segment_faces_from_votes
def _records(info):
    return [(r['isthing'], r['category_id'], r['area']) for r in info]


def test_segment_faces_from_votes_sheet():
    """Scene 1, with the outcome tests/test_face_graph_cpu.py::test_sheet_scene_outcome fixes from the restatements."""
    mu = MU()
    verts, tris, votes, truth = G.sheet()
    adj = mu.face_adjacency(tris, vertices=verts)
    _same_graph(adj, G.face_graph(tris)[:2])
    want = S.smooth_segment(votes, adj[0], adj[1], G.NCLASSES, 0.5)
    for v, a in ((votes, adj), (_dev(votes)[0], _dev(*adj))):
        classes, ids, info = mu.segment_faces_from_votes(v, a, G.NCLASSES, minimum_faces=G.SHEET_MIN_FACES)
        _same(classes, want)
        assert [r[:2] for r in _records(info)] == [(True, 1), (True, 2)]        # exactly two instances, no "small" bucket
        assert [r['area'] for r in info] == np.bincount(want)[1:3].tolist() and sum(r['area'] for r in info) == 4800
        assert np.array_equal(ids, want - 1) and (classes != truth).mean() < 0.02
        raw, raw_ids, raw_info = mu.segment_faces_from_votes(v, a, G.NCLASSES, smooth_iterations=0)
        _same(raw, segment(votes, G.NCLASSES, 0.5))                             # label_faces' own classes
        assert len(raw_info) > 500 and len(np.unique(raw_ids)) == len(raw_info)
        folded, _, folded_info = mu.segment_faces_from_votes(v, a, G.NCLASSES, smooth_iterations=0, minimum_faces=G.SHEET_MIN_FACES)
        bucket = [r for r in folded_info if r['category_id'] == G.NCLASSES]
        assert len(bucket) == 1 and bucket[0]['area'] > 500 and (folded == G.NCLASSES).sum() == bucket[0]['area']


def test_segment_faces_from_votes_corner():
    """Scene 2, with the outcome tests/test_face_graph_cpu.py::test_corner_scene_outcome fixes from the restatements."""
    mu = MU()
    verts, tris, votes, surface = G.corner()
    truth = np.where(surface == 0, *G.CORNER_CLASSES)
    sizes = np.bincount(surface).tolist()
    for v, t, x in ((verts, tris, votes), _dev(verts, tris, votes)):
        adj = mu.face_adjacency(t, vertices=v)
        plain, _, _ = mu.segment_faces_from_votes(x, adj, G.NCLASSES)
        leaked = plain != truth
        assert leaked.sum() == 12 and (surface[leaked] == 1).all() and (plain[leaked] == G.CORNER_CLASSES[0]).all()
        gated, ids, info = mu.segment_faces_from_votes(x, adj, G.NCLASSES, normals=mu.face_normals(v, t), angle=30)
        _same(gated, truth)                                                     # angle = 30 leaks into no face
        assert _records(info) == [(True, 1, sizes[0]), (True, 2, sizes[1])] and np.array_equal(ids, surface)
        cut = mu.face_adjacency(t, vertices=v, max_angle=45)
        _same_graph(cut, G.graph_of(verts, tris, 45)[:2])
        apart, ids, info = mu.segment_faces_from_votes(x, cut, G.NCLASSES)      # max_angle = 45 alone keeps the instances apart
        _same(apart, truth)
        assert _records(info) == [(True, 1, sizes[0]), (True, 2, sizes[1])] and np.array_equal(ids, surface)


def test_segment_faces_end_to_end():
    """Two quads facing one camera, the mask split down the middle between them."""
    import raster_ref as M
    import render_ref
    mu = MU()
    hw = (24, 40)
    K = render_ref.pinhole(*hw)                                                 # u = 16 x + 20, v = 16 y + 12 at z = 2
    q, t = M.IDENTITY
    verts = np.array([[-1, -0.5, 2], [0, -0.5, 2], [1, -0.5, 2], [-1, 0.5, 2], [0, 0.5, 2], [1, 0.5, 2]], np.float64)
    tris = np.array([[0, 1, 4], [0, 4, 3], [1, 2, 5], [1, 5, 4]], np.int64)
    masks = np.full((1, *hw), 5, np.uint8)
    masks[:, :, 20:] = 9
    own, votes = mu.label_faces(verts, tris, K, q, t, masks, return_votes=True)
    assert own.tolist() == [5, 5, 9, 9] and votes.sum() == 4                    # a (triangle, label) pair counts once per view
    for v, f, m in ((verts, tris, masks), _dev(verts, tris, masks)):
        for kw in ({}, {'angle': 30}, {'max_angle': 45}, {'smooth_iterations': 0}, {'smooth_iterations': 2, 'self_weight': 2.0}):
            classes, ids, info, got_votes = mu.segment_faces(v, f, K, q, t, m, return_votes=True, **kw)
            _same(classes, own); _same(got_votes, votes)
            assert ids.tolist() == [0, 0, 1, 1] and _records(info) == [(True, 5, 2), (True, 9, 2)]
        classes, ids, info = mu.segment_faces((v, f), K, q, t, m, minimum_faces=3)             # a mesh pair; both instances too small
        assert (classes == 133).all() and _records(info) == [(True, 133, 4)] and (ids == 0).all()
