"""planeUtils without a GPU: the NumPy restatement of f3d_extract_planes on the room corner (both normal modes, the margin condition),
plane_table against refinement.py's indexing, the legends, and the argument errors, which are raised before any device call."""
import functools

import numpy as np
import pytest

import planes_ref as R


def PU():
    from Fusion3DSeg.segUtils import planeUtils
    return planeUtils


@functools.lru_cache(maxsize=None)
def _room():
    pts, nrm, face = R.room_corner(np.random.default_rng(1))
    offs, nbrs = R.radius_csr(pts, 0.05)
    return pts, nrm, face, offs, nbrs


@functools.lru_cache(maxsize=None)
def _room_result(with_normals):
    pts, nrm, _, offs, nbrs = _room()
    return R.extract(pts, offs, nbrs, nrm if with_normals else None)


# ------------------------------------------------------------------------------------------------ the restatement
def test_room_corner_with_normals_finds_four_planes_of_900():
    r = _room_result(True)
    face = _room()[2]
    assert r.counts.tolist() == [4, 4, r.counts[2], 3600] and (r.labels >= 0).all()
    assert np.bincount(r.labels).tolist() == [900] * 4
    assert R.same_partition(r.labels, face)
    first = [int(np.flatnonzero(r.labels == k)[0]) for k in range(4)]
    assert first == sorted(first)                                                  # numbered by ascending root
    assert np.allclose(np.linalg.norm(r.planes[:, :3], axis=1), 1.0, atol=1e-12) and (r.planes[:, 7] < 0.002).all()


def test_room_corner_without_normals_finds_the_three_faces():
    """PCA mode: a point whose row mixes two surfaces is not core, so every face loses a strip along the edges it shares; the attach
    rounds give the strips back, except that a first-row point within `dist` of the neighbouring face may go to the lower plane.  So
    a face keeps at least 900 - 2 * 30 of its points in one plane, and each of the three faces has a plane of its own."""
    r = _room_result(False)
    face = _room()[2]
    owner = []
    for f in range(3):
        got = np.bincount(r.labels[face == f] + 1, minlength=r.counts[0] + 1)[1:]
        assert got.max() >= 840, (f, got)
        owner.append(int(got.argmax()))
    assert len(set(owner)) == 3
    for f, k in enumerate(owner):                                                  # the plane's normal is the face's axis
        axis = np.eye(3)[[2, 0, 1][f]]
        assert abs(r.planes[k, :3] @ axis) > 0.999


@pytest.mark.parametrize('with_normals', [True, False], ids=['normals', 'pca'])
def test_room_corner_margin_condition(with_normals):
    assert _room_result(with_normals).margin >= 1e-6


@pytest.mark.parametrize('name', list(R.EDGE_SHEETS))
def test_chunk_edge_sheets_are_one_plane_of_that_many_members_with_margin(name):
    """The scenes tests/test_planes_gpu.py compares exactly at the edges of a 4096-member chunk are fit for it under the restatement
    alone: one plane that holds every point, fitted on exactly nx * ny core members, and the margin condition."""
    nx, ny, _ = R.EDGE_SHEETS[name]
    pts, nrm = R.edge_sheet(name)
    assert len(pts) == nx * ny == int(name[5:])
    r = R.extract(pts, *R.radius_csr(pts, 0.05), nrm)
    assert r.counts.tolist()[:2] == [1, 1] and r.counts[3] == nx * ny and len(r.members[0]) == nx * ny
    assert r.margin >= 1e-6, r.margin


def test_restated_sums_have_the_contract_shape():
    x = np.random.default_rng(0).standard_normal(4900)
    lanes = [0.0] * 64
    for i, v in enumerate(x[:4096]):
        lanes[i % 64] = lanes[i % 64] + float(v)
    for off in (32, 16, 8, 4, 2, 1):
        lanes = [lanes[l] + lanes[l ^ off] for l in range(64)]
    assert R.wave_sum(x[:4096]) == lanes[0]
    assert R.shaped_sum(x) == R.wave_sum([R.wave_sum(x[:4096]), R.wave_sum(x[4096:])])
    assert R.shaped_sum(x[:0]) == 0.0 and R.shaped_sum(x[:1]) == x[0]


def test_restated_jacobi_diagonalises():
    a = np.random.default_rng(3).standard_normal((3, 3))
    a = a @ a.T
    w, V = R.jacobi3(a[0, 0], a[0, 1], a[0, 2], a[1, 1], a[1, 2], a[2, 2])
    V = np.array(V)
    assert np.allclose(V @ np.diag(w) @ V.T, a, atol=1e-13) and np.allclose(V.T @ V, np.eye(3), atol=1e-14)
    assert np.allclose(sorted(w), np.linalg.eigvalsh(a), atol=1e-13)


# ------------------------------------------------------------------------------------------------ plane_table
def _table():
    r = _room_result(True)
    return r, PU().plane_table(PU().PlaneSet(r.labels, r.planes, r.corners, r.counts))


def test_plane_table_shape_and_columns():
    r, (table, bounding) = _table()
    H = PU().Headers()
    assert table.shape == (4, 8) and table.dtype == object and bounding.shape == (16, 3) and bounding.dtype == np.float64
    for k in range(4):
        info = table[k, H['Shapeinfo']]
        assert np.array_equal(info.normal, r.planes[k, :3]) and np.array_equal(info.point, r.planes[k, 4:7])
        assert isinstance(table[k, H['indicies']], set) and table[k, H['indicies']] == set(np.flatnonzero(r.labels == k).tolist())
        assert table[k, H['BBoxids']].tolist() == [4 * k, 4 * k + 1, 4 * k + 2, 4 * k + 3]
        assert table[k, H['BBoxpoints']].shape == (4, 3) and np.array_equal(bounding[table[k, H['BBoxids']]], r.corners[k])
        assert table[k, H['Hide']] == 0 and table[k, H['Category']] == 0 and table[k, H['Shape']] == PU().getShapelegend()['Plane']
        # a 0.58 m square with 1 mm noise; its in-plane axes are those of a near-isotropic covariance, so the quad may stand
        # at any angle to the sides: between the square's area and twice that
        assert 0.57 ** 2 < table[k, H['Area']] < 2 * 0.6 ** 2
    assert np.array_equal(bounding[table[0, 2]][0], r.corners[0, 0])               # refinement._wall_distance's indexing


def test_plane_table_feeds_refinement():
    from Fusion3DSeg.segUtils import refinement
    r, (table, bounding) = _table()
    vertex = np.hstack([_room()[0], np.zeros((3600, 3))])
    pick = int(np.flatnonzero(r.labels == 2)[5])
    rows, indices = refinement.GetactualIndex(SelectedPoints=[vertex[pick, :3]], Vertex=vertex, PLanewithPoints=table)
    assert rows.tolist() == [2] and set(indices) == table[2, 1]
    rows, _ = refinement.GetactualIndex(SelectedPoints=[r.corners[3, 1]], Vertex=vertex, PLanewithPoints=table)
    assert rows.tolist() == [3]
    picks = [vertex[int(np.flatnonzero(r.labels == k)[0]), :3] for k in (1, 0)]
    before = bounding.copy()
    _, _, after = refinement.door_floor_align(table, vertex, picks, bounding, None, None)
    assert after is bounding and np.isfinite(after).all()
    assert np.array_equal(after[8:], before[8:]) and np.array_equal(after[:4], before[:4]) and not np.array_equal(after[4:8], before[4:8])


def test_plane_table_of_no_planes():
    table, bounding = PU().plane_table(PU().PlaneSet(np.full(5, -1, np.int32), np.zeros((0, 8)), np.zeros((0, 4, 3)), np.zeros(4, np.int64)))
    assert table.shape == (0, 8) and bounding.shape == (0, 3)


# ------------------------------------------------------------------------------------------------ legends
def test_legends():
    pu = PU()
    assert pu.ObjLegend() == {1: 'Walls', 2: 'Ceilings', 3: 'Floors', 4: 'Beams', 5: 'Columns', 6: 'Doors', 7: 'Windows', 8: 'Pipes'}
    assert pu.getShapelegend() == {'Plane': 1, 'Cuboid': 2, 'Cylinders': 3, 'Sphere': 4, 'Cone': 5, 'Unidentified': 0}
    assert pu.Headers() == {'Shapeinfo': 0, 'indicies': 1, 'BBoxids': 2, 'BBoxpoints': 3, 'Hide': 4, 'Category': 5, 'Shape': 6, 'Area': 7}
    assert [pu.revealShape(c) for c in range(0, 10)] == [3, 1, 1, 1, 2, 2, 1, 1, 3, 3]
    assert pu.Col('BBoxids') == 2 and pu.Col('Area') == 7 and pu.Obj('Doors') == 6 and pu.Obj('Walls') == 1 and pu.Obj('Stairs') is None
    with pytest.raises(KeyError):
        pu.Col('nothing')


# ------------------------------------------------------------------------------------------------ argument errors
class _FakeDeviceTensor:
    """What planeUtils looks at before it touches a device: is_cuda, shape, dtype."""
    is_cuda = True

    def __init__(self, shape, dtype):
        self.shape, self.dtype, self.device = shape, dtype, None


def test_argument_errors_come_before_any_device_call():
    pts = np.zeros((6, 3))
    adj = (np.arange(7, dtype=np.int64), np.arange(6, dtype=np.int32))
    ex = PU().extract_planes
    with pytest.raises(ValueError, match='min_points'):
        ex(pts, adj, min_points=2)
    with pytest.raises(ValueError, match='max_rounds'):
        ex(pts, adj, max_rounds=-1)
    with pytest.raises(ValueError, match=r'\[N, 3\]'):
        ex(np.zeros((6, 2)), adj, min_points=3)
    with pytest.raises(ValueError, match=r'\[N, 3\]'):
        ex(np.zeros(6), adj, min_points=3)
    with pytest.raises(ValueError, match='normals'):
        ex(pts, adj, normals=np.zeros((5, 3)), min_points=3)
    with pytest.raises(TypeError, match='float64 or float32'):
        ex(np.zeros((6, 3), np.int64), adj, min_points=3)
    with pytest.raises(TypeError, match='float64 or float32'):
        ex(np.zeros((6, 3), np.float16), adj, min_points=3)
    with pytest.raises(TypeError, match='normals'):
        ex(pts, adj, normals=np.zeros((6, 3), np.float32), min_points=3)
    with pytest.raises(ValueError, match='offsets'):
        ex(pts, (adj[0][:-1], adj[1]), min_points=3)
    with pytest.raises(ValueError, match='offsets'):
        ex(pts, (adj[0], adj[1][:-1]), min_points=3)
    import torch
    with pytest.raises(TypeError, match='device CSR'):
        ex(_FakeDeviceTensor((6, 3), torch.float64), adj, min_points=3)
    with pytest.raises(TypeError, match='float64 or float32'):
        ex(_FakeDeviceTensor((6, 3), torch.int32), adj, min_points=3)
