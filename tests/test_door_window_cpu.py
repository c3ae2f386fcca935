"""door_window_bbox.generate_mesh without a GPU: the restatement tests/door_window_ref.py against the reference golden, the OFF
reader and the triangle-mesh PLY writer, and the argument checks that run before the library is reached."""
import json

import numpy as np
import pytest

import door_window_ref as R


def _scene(g, name):
    return g[f'{name}_points'], g[f'{name}_ids'], json.loads(str(g[f'{name}_info'])), g[f'{name}_vertices'], g[f'{name}_triangles']


@pytest.mark.parametrize('name', ['a', 'c'])
def test_restatement_matches_reference_golden(golden, name):
    g = golden('door_window')
    pts, ids, info, verts, tris = _scene(g, name)
    assert np.array_equal(R.normals(verts, tris), g[f'{name}_normals'])
    tid, qv, qt, qc = R.generate(pts, ids, info, verts, tris)
    assert tid.dtype == np.int32 and np.array_equal(tid, g[f'{name}_triangle_ids'])
    assert np.array_equal(qv, g[f'{name}_quad_vertices'])                  # bit for bit (NaN never occurs here)
    assert np.array_equal(qt, g[f'{name}_quad_triangles'])
    assert np.array_equal(qc, g[f'{name}_quad_colors'])


def test_golden_covers_the_stated_cases(golden):
    g = golden('door_window')
    pts, ids, info, verts, tris = _scene(g, 'a')
    entries = [d for d in info if d['category_id'] in R.DOOR_WINDOW]
    q, st, tri, nrm = R.quads(pts, ids, [d['id'] for d in entries], verts, tris)
    assert (st == R.QUAD_HORIZONTAL).sum() == 1 and (st == R.QUAD_OK).sum() == len(entries) - 1
    sizes = sorted(int((ids == d['id']).sum()) for d in entries)
    assert sizes[0] == 1 and sizes[-1] >= 3000
    assert any(abs(abs(nrm[t][2]) - 1) <= 1e-5 and nrm[t][2] < 0 for t in tri[st == R.QUAD_OK])   # the other basis branch
    # coplanar candidates with equal distance sums (exact ties in argmin), decided by the inside counts
    tv = verts[tris]
    p = pts[ids == 12]
    td = R.tri_dist(p, tv[:, 0], nrm)
    cand = np.nonzero(td < td.min() + 0.05 * td.min())[0]
    assert len(cand) >= 2 and (td[cand] == td.min()).all()
    counts = [R.inside_count(p - nrm[t] * R._perp(p, tv[t, 0], nrm[t])[:, None], tv[t]) for t in cand]
    assert counts.count(max(counts)) >= 2                                  # a tie in argmax: the first candidate wins
    assert str(g['b_raises']) == 'attempt to get argmax of an empty sequence'
    b = _scene(g, 'b')
    with pytest.raises(ValueError, match='argmax of an empty sequence'):
        R.generate(*b)


def test_off_reader_fans_polygons_and_skips_comments(tmp_path, golden):
    from Fusion3DSeg.segUtils.door_window_bbox import read_off
    g = golden('door_window')
    (tmp_path / 'a.off').write_text(str(g['a_off']))
    v, t = read_off(tmp_path / 'a.off')
    assert v.dtype == np.float64 and t.dtype == np.int64
    assert np.array_equal(v, g['a_vertices']) and np.array_equal(t, g['a_triangles'])
    (tmp_path / 'b.off').write_text('OFF\n# a pentagon\n5 1 0\n0 0 0\n1 0 0\n2 1 0\n1 2 0\n0 1 0\n5 0 1 2 3 4\n')
    v, t = read_off(tmp_path / 'b.off')
    assert t.tolist() == [[0, 1, 2], [0, 2, 3], [0, 3, 4]] and v.shape == (5, 3)
    (tmp_path / 'c.off').write_text('OFF\n3 1 0\n0 0 0\n1 0 0\n')
    with pytest.raises(ValueError, match='malformed'):
        read_off(tmp_path / 'c.off')
    (tmp_path / 'd.off').write_text('PLY\n')
    with pytest.raises(ValueError, match='not an OFF'):
        read_off(tmp_path / 'd.off')


def test_triangle_mesh_ply_round_trip(tmp_path):
    from get3DSeg import TriangleMesh, read_triangle_mesh_ply, write_triangle_mesh
    rng = np.random.default_rng(3)
    v = rng.normal(size=(8, 3))
    f = np.vstack([np.array([[0, 1, 2], [2, 3, 0]]) + 4 * b for b in range(2)])
    c = np.repeat(rng.integers(0, 256, (2, 3)), 4, axis=0) / 255
    mesh = TriangleMesh(v, f, c)
    assert mesh.triangles.dtype == np.int32
    write_triangle_mesh(tmp_path / 'm.ply', mesh)
    head = (tmp_path / 'm.ply').read_bytes().split(b'end_header\n')[0].decode()
    assert 'element face 4' in head and 'property list uchar int vertex_indices' in head and 'property uchar red' in head
    back = read_triangle_mesh_ply(tmp_path / 'm.ply')
    assert np.array_equal(back.vertices, v) and np.array_equal(back.triangles, f) and np.array_equal(back.vertex_colors, c)
    write_triangle_mesh(tmp_path / 'n.ply', TriangleMesh(v, f))
    assert read_triangle_mesh_ply(tmp_path / 'n.ply').vertex_colors is None


def test_arguments_are_checked_before_the_library(golden):
    from Fusion3DSeg.segUtils.door_window_bbox import door_window_quads
    g = golden('door_window')
    pts, ids, info, verts, tris = _scene(g, 'a')
    with pytest.raises(ValueError, match=r'points must be \[N, 3\]'):
        door_window_quads(pts[:, :2], ids, info, verts, tris)
    with pytest.raises(ValueError, match='ids for'):
        door_window_quads(pts, ids[:-1], info, verts, tris)
    with pytest.raises(ValueError, match=r'triangles must be \[T, 3\]'):
        door_window_quads(pts, ids, info, verts, tris[:, :2])
    with pytest.raises(ValueError, match='argmin of an empty sequence'):            # an empty mesh
        door_window_quads(pts, ids, info, verts, np.zeros((0, 3), np.int64))
    with pytest.raises(ValueError, match='need at least one array'):               # no door or window at all
        door_window_quads(pts, ids, [d for d in info if d['category_id'] not in R.DOOR_WINDOW], verts, tris)
