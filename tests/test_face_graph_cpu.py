"""The face graph without a GPU: the new C-ABI names are bound, every argument error is raised before the library is reached, and
the restatement tests/face_graph_ref.py gives the known answers and, on the two scenes, exactly the outcome that
tests/test_face_graph_gpu.py asserts of the library."""
import ctypes

import numpy as np
import pytest

import f3d
import face_graph_ref as G
import mesh_ref as R
import smooth_ref as S
from Fusion3DSeg.segUtils import meshUtils as MU
from oracle.np_ref import segment

ENTRIES = {'f3d_mesh_face_frames': 11, 'f3d_mesh_face_frames_dev': 12, 'f3d_mesh_face_graph': 13, 'f3d_mesh_face_graph_dev': 14}


def test_symbols_are_bound_with_argtypes():
    lib = f3d.library()
    for name, nargs in ENTRIES.items():
        fn = getattr(lib, name)
        assert name in lib._f3d_symbols and fn.argtypes is not None and len(fn.argtypes) == nargs, name
    graph = lib.f3d_mesh_face_graph_dev.argtypes
    assert graph[8] is ctypes.c_double and graph[11] is ctypes.c_int64                      # cos_crease, cap
    for name in ('face_normals', 'face_adjacency', 'segment_faces_from_votes', 'segment_faces'):
        assert name in MU.__all__ and callable(getattr(MU, name))
    for name in ('mesh_face_frames', 'mesh_face_frames_dev', 'mesh_face_graph', 'mesh_face_graph_dev'):
        assert callable(getattr(f3d.Context, name))


def test_argument_checks_run_before_the_library():
    tris = np.zeros((4, 3), np.int64)
    verts = np.zeros((5, 3))
    with pytest.raises(ValueError, match='max_angle needs the vertices'):
        MU.face_adjacency(tris, 5, max_angle=30)
    for bad in (-1, 180.5, float('nan')):
        with pytest.raises(ValueError, match=r'\[0, 180\]'):
            MU.face_adjacency(tris, vertices=verts, max_angle=bad)
        with pytest.raises(ValueError, match=r'\[0, 180\]'):
            MU.segment_faces(verts, tris, np.eye(3), [[1, 0, 0, 0]], [[0, 0, 0]], np.zeros((1, 4, 4), np.uint8), max_angle=bad)
    with pytest.raises(ValueError, match='nvertices or vertices'):
        MU.face_adjacency(tris)
    with pytest.raises(ValueError, match='nvertices is 6'):
        MU.face_adjacency(tris, 6, verts)
    with pytest.raises(ValueError, match='nvertices'):
        MU.face_adjacency(tris, 1 << 31)
    with pytest.raises(TypeError, match='int32 or int64'):
        MU.face_adjacency(tris.astype(np.int16), 5)
    with pytest.raises(TypeError, match='int32 or int64'):
        MU.face_normals(verts, tris.astype(np.float32))
    with pytest.raises(ValueError, match=r'\[M, 3\]'):
        MU.face_adjacency(np.zeros((4, 2), np.int64), 5)
    with pytest.raises(ValueError, match=r'\[M, 3\]'):
        MU.face_normals((verts, np.zeros(12, np.int64)))
    with pytest.raises(ValueError, match=r'\[V, 3\]'):
        MU.face_normals(np.zeros((5, 2)), tris)
    with pytest.raises(ValueError, match=r'\[V, 3\]'):
        MU.face_adjacency(tris, vertices=np.zeros(15))
    with pytest.raises(ValueError, match=r'\[V, 3\]'):
        MU.face_adjacency(tris, vertices=np.zeros((5, 4)), max_angle=10)
    votes = np.zeros((4, 5))
    adj = (np.zeros(5, np.int64), np.zeros(0, np.int32))
    with pytest.raises(ValueError, match=r'\[M, ncols\]'):
        MU.segment_faces_from_votes(np.zeros(4), adj, 4)
    with pytest.raises(ValueError, match='votes has 3 rows'):
        MU.segment_faces_from_votes(votes[:3], adj, 4)
    with pytest.raises(ValueError, match='offsets 4 entries'):
        MU.segment_faces_from_votes(votes, (adj[0][:4], adj[1]), 4)
    with pytest.raises(TypeError, match='CSR pair'):
        MU.segment_faces_from_votes(votes, [[1], [0], [], []], 4)
    with pytest.raises(ValueError, match='smooth_iterations'):
        MU.segment_faces_from_votes(votes, adj, 4, smooth_iterations=-1)
    with pytest.raises(ValueError, match='CSR adjacency'):                                  # offsets that do not end at len(neighbours)
        MU.segment_faces_from_votes(votes, (np.arange(5, dtype=np.int64), np.zeros(3, np.int32)), 4)
    with pytest.raises(ValueError, match='normals and angle go together'):
        MU.segment_faces_from_votes(votes, adj, 4, angle=30)
    with pytest.raises(ValueError, match=r'normals must be \[4, 3\]'):
        MU.segment_faces_from_votes(votes, adj, 4, normals=np.zeros((3, 3)), angle=30)
    with pytest.raises(TypeError, match='float64 or uint16'):
        MU.segment_faces_from_votes(votes.astype(np.float32), adj, 4)
    with pytest.raises(ValueError, match='self_weight'):
        MU.segment_faces_from_votes(votes, adj, 4, self_weight=-1.0)


def test_restatement_on_a_cube():
    verts, tris = G.cube()
    normals, centroids, areas = G.face_frames(verts, tris)
    assert np.array_equal(areas, np.full(12, 0.5)) and np.array_equal(np.abs(normals).sum(1), np.ones(12))
    assert np.array_equal(normals[::2], normals[1::2])                                      # the two faces of a side
    assert np.array_equal(np.sign(normals[::2].sum(1)), [-1, 1, -1, 1, -1, 1])              # outward
    assert np.allclose(centroids.mean(0), 0.5)
    offsets, nbrs, stats = G.face_graph(tris)
    assert len(offsets) == 13 and np.array_equal(np.diff(offsets), np.full(12, 3)) and stats == {'nonmanifold_edges': 0, 'boundary_edges': 0}
    assert G.components(offsets, nbrs)[0] == 1
    o45, n45, _ = G.graph_of(verts, tris, 45)
    count, lab = G.components(o45, n45)
    assert count == 6 and np.array_equal(lab, np.repeat(np.arange(6), 2)) and np.array_equal(np.diff(o45), np.ones(12))
    o91, n91, _ = G.graph_of(verts, tris, 91)
    assert np.array_equal(o91, offsets) and np.array_equal(n91, nbrs)
    o90, n90, _ = G.graph_of(verts, tris, 90)                                               # cos(90 degrees) is 6e-17, not 0: cut
    assert np.array_equal(n90, n45)
    flipped = G.flipped(tris, np.random.default_rng(3))                                     # the winding plays no part
    assert (flipped != tris).any() and np.array_equal(G.graph_of(verts, flipped, 45)[1], n45)


def test_the_two_restatements_agree():
    rng = np.random.default_rng(5)
    meshes = [G.sized_mesh(m, rng) for m in (0, 1, 2, 3, 64, 257)] + [R.random_mesh(30, 300, rng), G.book(33, rng), G.cube()]
    meshes.append((rng.uniform(-1, 1, (6, 3)), np.array([[0, 1, 2], [2, 0, 1], [1, 0, 2], [3, 3, 4], [3, 3, 3], [4, 3, 3], [3, 3, 5]], np.int64)))
    for verts, tris in meshes:
        normals = G.face_frames(verts, tris)[0]
        for cos_crease in (None, 1.0, 0.9, 0.0, -1.0):
            a, b = G.face_graph(tris, normals, cos_crease), G.face_graph_dict(tris, normals, cos_crease)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2], (len(tris), cos_crease)
            rows = np.repeat(np.arange(len(tris)), np.diff(a[0]))
            pairs = set(zip(rows.tolist(), a[1].tolist()))
            assert all((g, f) in pairs for f, g in pairs) and all(f != g for f, g in pairs)            # symmetric, no self


def test_folded_and_flipped_sheets():
    for first in (False, True):
        for second in (False, True):
            verts, tris = G.folded_pair(first, second)
            assert [len(G.graph_of(verts, tris, a)[1]) for a in (0, 45, 90, 135, 179.9, 180)] == [0, 0, 0, 0, 0, 2]
            assert len(G.face_graph(tris)[1]) == 2
    verts, tris = R.grid_mesh(9, 7)
    want = G.face_graph(tris)
    got = G.graph_of(verts, G.flipped(tris, np.random.default_rng(2)), 10)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def _instances(offsets, nbrs, classes, minimum):
    """(instances of at least `minimum` faces, faces in smaller ones) over the same-class components."""
    sizes = np.bincount(G.components(offsets, nbrs, classes)[1])
    return int((sizes >= minimum).sum()), int(sizes[sizes < minimum].sum())


def test_sheet_scene_outcome():
    """What test_face_graph_gpu.py::test_segment_faces_from_votes_sheet asserts of the library, from the restatements."""
    verts, tris, votes, truth = G.sheet()
    assert len(tris) == 4800 and 0.13 < ((votes > 0).sum(1) == 2).mean() < 0.17 and 0.04 < (votes.sum(1) == 0).mean() < 0.06
    offsets, nbrs, stats = G.face_graph(tris)
    assert stats == {'nonmanifold_edges': 0, 'boundary_edges': 200}
    raw = segment(votes, G.NCLASSES, 0.5)
    assert _instances(offsets, nbrs, raw, 1)[0] > 500                                       # unsmoothed: many same-class components
    assert _instances(offsets, nbrs, raw, G.SHEET_MIN_FACES)[1] > 500
    smoothed = S.smooth_segment(votes, offsets, nbrs, G.NCLASSES, 0.5)
    assert _instances(offsets, nbrs, smoothed, 1) == (2, 0) and _instances(offsets, nbrs, smoothed, G.SHEET_MIN_FACES) == (2, 0)
    assert sorted(np.unique(smoothed)) == list(G.SHEET_CLASSES) and (smoothed != truth).mean() < 0.02
    # a typical draw: one iteration removes all but a handful of the stray components
    _, tris0, votes0, _ = G.sheet(0)
    o0, n0, _ = G.face_graph(tris0)
    before = _instances(o0, n0, segment(votes0, G.NCLASSES, 0.5), 1)[0]
    after = _instances(o0, n0, S.smooth_segment(votes0, o0, n0, G.NCLASSES, 0.5), 1)[0]
    assert before > 500 and 2 < after < 30


def test_corner_scene_outcome():
    """What test_face_graph_gpu.py::test_segment_faces_from_votes_corner asserts of the library, from the restatements."""
    verts, tris, votes, surface = G.corner()
    truth = np.where(surface == 0, *G.CORNER_CLASSES)
    offsets, nbrs, _ = G.face_graph(tris)
    normals = G.face_frames(verts, tris)[0]
    assert set(map(tuple, normals[surface == 0])) == {(0.0, 0.0, 1.0)} and set(map(tuple, normals[surface == 1])) == {(1.0, 0.0, 0.0)}
    plain = S.smooth_segment(votes, offsets, nbrs, G.NCLASSES, 0.5)
    leaked = plain != truth
    assert leaked.sum() == 12 and (surface[leaked] == 1).all() and (plain[leaked] == G.CORNER_CLASSES[0]).all()
    gated = S.smooth_segment(votes, offsets, nbrs, G.NCLASSES, 0.5, normals=normals, cos_angle=np.cos(np.radians(30.0)))
    assert np.array_equal(gated, truth)
    o45, n45, _ = G.graph_of(verts, tris, 45)
    assert len(nbrs) - len(n45) == 24 and G.components(o45, n45)[0] == 2 and G.components(offsets, nbrs)[0] == 1
    cut = S.smooth_segment(votes, o45, n45, G.NCLASSES, 0.5)
    assert np.array_equal(cut, truth) and _instances(o45, n45, cut, 1) == (2, 0)
