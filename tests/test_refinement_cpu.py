"""segUtils/refinement.py without a GPU: the restatement against the reference golden, the host geometry, argument errors."""
import numpy as np
import pytest

import f3d
import refinement_ref as R


def test_restatement_matches_reference_golden(golden):
    g = golden('refinement')
    assert int(g['ncases']) >= 31
    kinds, empties = set(), 0
    for k in range(int(g['ncases'])):
        kind, adj, val, seeds, thr, ml, want = R.golden_case(g, k)
        got = getattr(R, kind)(val, adj, seeds, thr, ml)
        assert got.dtype == np.int64 and np.array_equal(got, want), (k, kind)
        kinds.add(kind)
        empties += len(want) == 0
    assert kinds == {'depth_points', 'depth_point', 'color_points', 'color_point'} and empties >= 4


def test_door_updation_matches_reference_golden(golden):
    from Fusion3DSeg.segUtils.refinement import door_updation
    g = golden('refinement')
    moved = 0
    for k in range(int(g['ndoors'])):
        inner = g[f'd{k}_inner'].copy()
        out = door_updation(g['wall_quad'], inner, g['wall_normal'], float(g[f'd{k}_max_distance']))
        assert np.array_equal(out, g[f'd{k}_out']), k                      # NumPy only: bit for bit
        assert np.array_equal(inner, g[f'd{k}_inner'])                      # the caller's corners are not written
        moved += int((np.abs(out - inner).max(axis=1) > 0.06).sum())        # beyond the 0.05 projection into the plane
    assert 0 < moved < 4 * int(g['ndoors'])


def test_door_floor_align_matches_reference_golden(golden):
    """The golden ran the reference with a restated axis-angle quaternion constructor (parity unpinned).  Tolerance: the result is a
    chain of fewer than 64 float64 roundings (normalisations, cross products, two quaternion products) on intermediates no larger
    than 4 x the largest coordinate, so it differs from another evaluation order by less than 64 * 4 * 2^-53 * max|coordinate|."""
    from Fusion3DSeg.segUtils.refinement import door_floor_align
    g = golden('refinement')
    tol = 64 * 4 * 2.0 ** -53 * float(np.abs(g['align_quad']).max())
    quads = np.stack([g['wall_quad'], g['align_quad']])
    vertex = np.hstack([g['points'], g['colors']])
    for j, flip in enumerate((True, False)):
        table, bounding = R.plane_table(g['plane_normals'], g['plane_index_offsets'], g['plane_index_values'], quads)
        t2, v2, b2 = door_floor_align(table, vertex, list(g['align_selected']), bounding, None, '', flip=flip)
        assert t2 is table and b2 is bounding
        err = float(np.abs(b2[1] - g[f'a{j}_out']).max())
        print(f'door_floor_align flip={flip}: max abs difference {err:.3e} (tolerance {tol:.3e})')
        assert err <= tol
        assert np.array_equal(b2[0], g['wall_quad'])
    assert not np.allclose(g['a0_out'], g['a1_out'])


def test_get_actual_index_and_connected_file(tmp_path, golden):
    from Fusion3DSeg.segUtils.refinement import GetactualIndex, ReadVerticesConnectedFiles
    g = golden('refinement')
    table, _ = R.plane_table(g['plane_normals'], g['plane_index_offsets'], g['plane_index_values'], np.stack([g['wall_quad'], g['align_quad']]))
    vertex = np.hstack([g['points'], g['colors']])
    door, wall = g['align_selected']
    idx, indices = GetactualIndex([door, wall, door], vertex, table)
    assert idx.tolist() == [1, 0]
    n1, n0 = len(table[1, 1]), len(table[0, 1])
    assert len(indices) == n1 + (n1 + n0)                                  # the reference re-appends every row found so far
    idx, _ = GetactualIndex([g['align_quad'][2]], vertex, table)            # not a vertex: found through the bounding points
    assert idx.tolist() == [1]
    idx, _ = GetactualIndex([np.array([1e3, 1e3, 1e3])], vertex, table)
    assert len(idx) == 0
    path = tmp_path / 'connected.csv'
    path.write_text('VIDs\n0,1,2\n1,0\n2,0\n3\n')
    assert ReadVerticesConnectedFiles(str(path)) == [[1, 2], [0], [0], []]


def test_read_ply_returns_colours(tmp_path):
    from get3DSeg import PointCloud, write_ply, read_ply_points
    from Fusion3DSeg.segUtils.refinement import read_ply, save_ids_ply
    rng = np.random.default_rng(3)
    pts, clr = rng.normal(size=(50, 3)), rng.integers(0, 256, (50, 3)) / 255.0
    save_ids_ply(PointCloud(pts, clr), np.arange(50), str(tmp_path))
    p, c = read_ply(tmp_path / 'cv_segmentation' / 'pcd.ply')
    assert np.array_equal(p, pts) and np.array_equal(c, np.clip(clr * 255.0, 0, 255).astype(np.uint8) / 255.0)
    assert np.array_equal(np.load(tmp_path / 'cv_segmentation' / 'ids.npy'), np.arange(50))
    assert np.array_equal(read_ply_points(tmp_path / 'cv_segmentation' / 'pcd.ply'), pts)
    write_ply(tmp_path / 'bare.ply', PointCloud(pts))
    assert read_ply(tmp_path / 'bare.ply')[1] is None


def test_argument_errors_raise_before_any_device_call(monkeypatch, golden, tmp_path):
    from Fusion3DSeg.segUtils import refinement as M

    def no_device(*a, **k):
        raise AssertionError('a device call was made')
    monkeypatch.setattr(f3d, 'default_context', no_device)
    g = golden('refinement')
    adj = R.golden_graph(g, 0)
    dist, col = g['dist'], g['colors']
    n = len(dist)
    vertex = np.hstack([g['points'], col])
    ids, seg = g['ids'].copy(), g['seg_colors'].copy()
    table, bounding = R.plane_table(g['plane_normals'], g['plane_index_offsets'], g['plane_index_values'], g['plane_quads'])
    sel = list(g['selected_vertices'])
    for fn, args in ((M.depth_floodfill_dl, (table, vertex, sel, bounding, adj, str(tmp_path))),
                     (M.depth_floodfill_point, (table, vertex, sel, bounding, adj, str(tmp_path))),
                     (M.color_floodfill_dl, (vertex, adj, str(tmp_path))), (M.color_floodfill_point, (vertex, adj, str(tmp_path)))):
        with pytest.raises(ValueError, match='no viewer'):
            fn(*args, instance_id=ids, seg_colors=seg)
        with pytest.raises(ValueError, match='twice'):
            fn(*args, selected_point=[5, 9, 5], instance_id=ids, seg_colors=seg)
        with pytest.raises(IndexError):
            fn(*args, selected_point=[n], instance_id=ids, seg_colors=seg)
        with pytest.raises(TypeError):
            fn(*args, selected_point=[1.5], instance_id=ids, seg_colors=seg)
    with pytest.raises(ValueError, match='twice'):
        M.grow_depth(dist, adj, [3, 4, 3], 0.01)
    with pytest.raises(IndexError):
        M.grow_depth(dist, adj, [n], 0.01)
    with pytest.raises(IndexError):
        M.grow_color(col, adj, -1, 0.1)
    with pytest.raises(TypeError):
        M.grow_depth(dist.astype(np.float32), adj, [3], 0.01)
    with pytest.raises(TypeError):
        M.grow_color((col * 255).astype(np.uint8), adj, 3, 0.1)
    with pytest.raises(TypeError):
        M.grow_depth(dist, adj, [3.0], 0.01)
    with pytest.raises(ValueError):
        M.grow_depth(col, adj, [3], 0.01)
    with pytest.raises(ValueError):
        M.grow_color(dist, adj, 3, 0.1)
    with pytest.raises(ValueError):
        M.grow_color(col, adj, 3, [0.1, 0.1])
    with pytest.raises(ValueError):
        M.grow_depth(dist, (adj[0][:-1], adj[1]), [3], 0.01)
    assert len(M.grow_depth(dist, adj, [], 0.01)) == 0                      # nothing to grow from: no device call either


def test_library_declares_region_grow():
    lib = f3d.library()
    for name in ('f3d_region_grow', 'f3d_region_grow_dev', 'f3d_plane_distance', 'f3d_plane_distance_dev', 'f3d_ctx_reserve_refine'):
        assert name in lib._f3d_symbols and hasattr(lib, name)
