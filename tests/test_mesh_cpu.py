"""meshUtils without a GPU: the restatement tests/mesh_ref.py equals the reference golden exactly, the argument checks that run
before the library is reached, the lazy list view of the CSR, and the two host helpers."""
import numpy as np
import pytest

import mesh_ref as R
from Fusion3DSeg.segUtils import meshUtils as MU

SCENES = ['some', 'none', 'all', 'odd', 'empty', 'corners']


def _scene(g, s):
    return g[f'{s}_vertices'], g[f'{s}_triangles'], g[f'{s}_mask']


def test_golden_lists_every_scene(golden):
    assert list(golden('mesh')['scenes']) == SCENES


@pytest.mark.parametrize('s', SCENES)
def test_restatement_equals_reference_golden(golden, s):
    g = golden('mesh')
    verts, tris, mask = _scene(g, s)
    offsets, tri, pos = R.vertex_map(tris, len(verts))
    assert np.array_equal(offsets, g[f'{s}_offsets']) and np.array_equal(tri, g[f'{s}_tov']) and np.array_equal(pos, g[f'{s}_pov'])
    nr, rem, o2n = R.remove_faces(len(verts), tris, mask)
    assert np.array_equal(nr, g[f'{s}_not_removed']) and np.array_equal(o2n, g[f'{s}_old2new'])
    assert rem.dtype == tris.dtype and rem.shape == g[f'{s}_remaining'].shape and np.array_equal(rem, g[f'{s}_remaining'])
    kv, kt = R.keep_faces(verts, tris, mask)
    assert kv.shape == g[f'{s}_kept_vertices'].shape and np.array_equal(kv, g[f'{s}_kept_vertices'])
    assert kt.dtype == tris.dtype and kt.shape == g[f'{s}_kept_triangles'].shape and np.array_equal(kt, g[f'{s}_kept_triangles'])


@pytest.mark.parametrize('s', SCENES)
def test_lazy_list_view_equals_reference_lists(golden, s):
    g = golden('mesh')
    offsets = g[f'{s}_offsets']
    vmap = MU.VertexTriangleMap(offsets, g[f'{s}_tov'].astype(np.int32), g[f'{s}_pov'].astype(np.int8))
    assert vmap._lists is None and vmap.csr[0] is offsets              # nothing is built until it is read
    tov, pov = vmap
    assert tov == R.lists_of(offsets, g[f'{s}_tov']) and pov == R.lists_of(offsets, g[f'{s}_pov'])
    assert len(tov) == len(offsets) - 1 and all(isinstance(x, int) for row in tov for x in row)
    assert len(vmap) == 2 and vmap[0] is tov and vmap.position_of_vertices is pov


def test_restated_clusters_known_answers():
    # two fans that meet at vertex 0 only -> 2 clusters; three triangles on the edge (0, 1) -> 1 cluster
    fans = np.array(R.fan(0, [1, 2, 3, 4]) + R.fan(0, [5, 6, 7]), np.int64)
    verts = np.random.default_rng(1).uniform(-1, 1, (8, 3))
    cl, n, a, area = R.clusters(verts, fans)
    assert cl.tolist() == [0, 0, 0, 1, 1] and n.tolist() == [3, 2]
    assert np.allclose(a, [area[:3].sum(), area[3:].sum()], rtol=1e-15)
    cl, n, _, _ = R.clusters(verts, np.array([[0, 1, 2], [1, 0, 3], [4, 0, 1]], np.int64))
    assert cl.tolist() == [0, 0, 0] and n.tolist() == [3]
    # numbering by lowest triangle index; a (v, v, w) face joins through its (v, w) edge
    cl, n, _, _ = R.clusters(verts, np.array([[5, 6, 7], [0, 1, 2], [7, 6, 4], [2, 2, 1]], np.int64))
    assert cl.tolist() == [0, 1, 0, 1] and n.tolist() == [2, 2]


def test_argument_checks_run_before_the_library():
    tris = np.zeros((4, 3), np.int64)
    verts = np.zeros((5, 3))
    mask = np.zeros(5, bool)
    with pytest.raises(ValueError, match=r'\[M, 3\]'):
        MU.vertex_triangle_mapping(np.zeros((4, 4), np.int64), 5)
    with pytest.raises(ValueError, match=r'\[M, 3\]'):
        MU.remove_faces_by_vertices(5, np.zeros(12, np.int64), mask)
    with pytest.raises(TypeError, match='int32 or int64'):
        MU.vertex_triangle_mapping(tris.astype(np.float64), 5)
    with pytest.raises(TypeError, match='int32 or int64'):
        MU.keep_faces_by_vertices(verts, tris.astype(np.int16), mask)
    with pytest.raises(ValueError, match='nvertices'):
        MU.vertex_triangle_mapping(tris, -1)
    with pytest.raises(ValueError, match='nvertices'):
        MU.remove_faces_by_vertices(1 << 31, tris, mask)
    with pytest.raises(ValueError, match='one entry per vertex'):
        MU.remove_faces_by_vertices(5, tris, np.zeros(4, bool))
    with pytest.raises(ValueError, match='one entry per vertex'):
        MU.keep_faces_by_vertices(verts, tris, np.zeros((5, 1), bool))
    with pytest.raises(ValueError, match=r'\[V, 3\]'):
        MU.keep_faces_by_vertices(np.zeros((5, 2)), tris, mask)
    with pytest.raises(ValueError, match=r'\[V, 3\]'):
        MU.get_triangle_clusters((np.zeros(15), tris))
    with pytest.raises(ValueError, match='remove_mask'):
        MU.clean_mesh(verts, tris, np.zeros(6, bool))


def test_host_helpers_equal_reference_golden(golden):
    g = golden('mesh')
    origin, i, j, li, lj = MU.bbox_axes(g['box_corners'])
    assert np.array_equal(origin, g['box_origin']) and np.array_equal(i, g['box_i']) and np.array_equal(j, g['box_j'])
    assert li == g['box_li'] and lj == g['box_lj']
    v1, v2 = g['ang_vec1'].copy(), g['ang_vec2'].copy()
    angles = MU.one_to_all_angles(v1, v2)
    assert angles.shape == (5, 4) and np.array_equal(angles, g['ang_angles'])
    assert np.array_equal(v1, g['ang_vec1_after']) and np.array_equal(v2, g['ang_vec2_after'])    # normalised in place
