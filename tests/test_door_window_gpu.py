"""door_window_bbox.generate_mesh on the GPU (f3d_door_window_quads): bit-exact against the reference golden and, at capture size
(40 instances of 1k-200k points against 2 000 triangles), against the restatement tests/door_window_ref.py; the pipeline's own
files, device tensors, and every ValueError of the reference."""
import json
import multiprocessing as mp
import types

import numpy as np
import pytest

import f3d
import door_window_ref as R

pytestmark = pytest.mark.gpu


def _scene(g, name):
    return g[f'{name}_points'], g[f'{name}_ids'], json.loads(str(g[f'{name}_info'])), g[f'{name}_vertices'], g[f'{name}_triangles']


def _same(got, g, name):
    tid, qv, qt, qc = got
    assert tid.dtype == np.int32 and np.array_equal(tid, g[f'{name}_triangle_ids'])
    assert qv.dtype == np.float64 and np.array_equal(qv, g[f'{name}_quad_vertices'])
    assert np.array_equal(qt, g[f'{name}_quad_triangles'])
    assert np.array_equal(qc, g[f'{name}_quad_colors'])


@pytest.mark.parametrize('name', ['a', 'c'])
def test_bit_identical_to_reference_golden(golden, name):
    from Fusion3DSeg.segUtils.door_window_bbox import door_window_quads
    g = golden('door_window')
    pts, ids, info, verts, tris = _scene(g, name)
    _same(door_window_quads(pts, ids, info, verts, tris), g, name)
    entries = [d['id'] for d in info if d['category_id'] in R.DOOR_WINDOW]
    q, st, tri, nrm = f3d.default_context().door_window_quads(pts, ids, entries, verts, tris)
    wq, wst, wtri, wnrm = R.quads(pts, ids, entries, verts, tris)
    assert np.array_equal(nrm, g[f'{name}_normals']) and np.array_equal(nrm, wnrm)
    assert np.array_equal(st, wst) and np.array_equal(tri, wtri)
    assert np.array_equal(q, wq, equal_nan=True)


def _ref_one(args):
    pts, inst_id, verts, tris, nrm = args
    return R.quad_of(pts, np.full(len(pts), inst_id), inst_id, verts, tris, nrm)


def test_capture_size_matches_restatement():
    pts, ids, info, verts, tris = R.capture_scene()
    entries = [d['id'] for d in info if d['category_id'] in R.DOOR_WINDOW]
    ctx = f3d.default_context()
    q, st, tri, nrm = ctx.door_window_quads(pts, ids, entries, verts, tris)
    assert np.array_equal(nrm, R.normals(verts, tris))
    jobs = [(pts[ids == e], e, verts, tris, nrm) for e in entries]
    jobs.sort(key=lambda j: -len(j[0]))                                   # the largest first
    order = sorted(range(len(entries)), key=lambda k: -int((ids == entries[k]).sum()))
    with mp.get_context('spawn').Pool(8) as pool:                        # fresh interpreters: no GPU state in the workers
        res = pool.map(_ref_one, jobs, chunksize=1)
    for k, (wst, wtri, wq) in zip(order, res):
        assert st[k] == wst and tri[k] == wtri, (k, st[k], wst, tri[k], wtri)
        if wq is not None:
            assert np.array_equal(q[k], wq), k
    assert (st == R.QUAD_OK).sum() >= 30 and (st == R.QUAD_HORIZONTAL).sum() >= 1


def test_generate_mesh_on_pipeline_output(tmp_path, golden):
    from Fusion3DSeg.fusion import Fusion
    from Fusion3DSeg.segUtils.door_window_bbox import generate_mesh
    from get3DSeg import panoptic_viz, read_triangle_mesh_ply
    g = golden('door_window')
    pts, ids, info, verts, tris = _scene(g, 'a')
    cat = {d['id']: d['category_id'] for d in info}
    idinfo = [{'id': i, 'isthing': cat.get(i, 133) != 133, 'category_id': cat.get(i, 133), 'area': int((ids == i).sum())}
              for i in range(int(ids.max()) + 1)]
    owner = types.SimpleNamespace(nframes=1, h=4, w=4, ds_radius=0.05, ds_angle=10)
    Fusion.dump_data(owner, tmp_path, pts, colors=np.zeros_like(pts), compute_adjacency=False)
    np.random.seed(5)
    panoptic_viz(pts, ids, idinfo, tmp_path / 'panoptic_segmentation')
    (tmp_path / 'polyfit').mkdir()
    (tmp_path / 'polyfit' / 'building.off').write_text(str(g['a_off']))
    tid, mesh = generate_mesh(tmp_path)
    written = json.loads((tmp_path / 'panoptic_segmentation' / 'info.json').read_text())
    wtid, wv, wt, wc = R.generate(pts, ids, written, g['a_vertices'], g['a_triangles'])
    assert np.array_equal(tid, wtid) and np.array_equal(mesh.vertices, wv) and np.array_equal(mesh.triangles, wt)
    assert np.array_equal(mesh.vertex_colors, wc)
    assert np.array_equal(np.load(tmp_path / 'panoptic_segmentation' / 'triangle_ids.npy'), tid)
    back = read_triangle_mesh_ply(tmp_path / 'panoptic_segmentation' / 'door_window_mesh.ply')
    assert np.array_equal(back.vertices, wv) and np.array_equal(back.triangles, wt) and np.array_equal(back.vertex_colors, wc)


def test_device_tensors(golden):
    import torch
    from Fusion3DSeg.segUtils.door_window_bbox import door_window_quads
    g = golden('door_window')
    pts, ids, info, verts, tris = _scene(g, 'c')
    dev = torch.device('cuda', 0)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        dp = torch.as_tensor(pts, device=dev)
        di = torch.as_tensor(ids, device=dev)
        got = door_window_quads(dp, di, info, torch.as_tensor(verts, device=dev), torch.as_tensor(tris, device=dev))
    _same(got, g, 'c')
    got = door_window_quads(torch.as_tensor(pts, device=dev), torch.as_tensor(ids, device=dev).int(), info, verts, tris)
    _same(got, g, 'c')                                                    # the legacy default stream, int32 ids, host mesh


def test_strict_context_after_reserve(golden):
    g = golden('door_window')
    pts, ids, info, verts, tris = _scene(g, 'a')
    entries = [d['id'] for d in info if d['category_id'] in R.DOOR_WINDOW]
    ctx = f3d.Context(0)
    ctx.reserve_quads(len(pts), len(entries), len(tris))
    ctx.door_window_quads(pts, ids, entries, verts, tris)                # sizes the host entry's staging slots
    ctx.set_strict(True)
    allocs = ctx.alloc_count
    q, st, tri, _ = ctx.door_window_quads(pts, ids, entries, verts, tris)
    assert ctx.alloc_count == allocs
    wq, wst, wtri, _ = R.quads(pts, ids, entries, verts, tris)
    assert np.array_equal(st, wst) and np.array_equal(tri, wtri) and np.array_equal(q, wq, equal_nan=True)
    with pytest.raises(MemoryError, match='strict context'):
        ctx.door_window_quads(pts, ids, entries, verts, np.concatenate([tris] * 4))
    ctx.close()


def test_every_value_error_of_the_reference(golden):
    from Fusion3DSeg.segUtils.door_window_bbox import door_window_quads
    g = golden('door_window')
    with pytest.raises(ValueError, match=str(g['b_raises'])):             # points exactly in a mesh plane: minimum 0
        door_window_quads(*_scene(g, 'b'))
    pts, ids, info, verts, tris = _scene(g, 'a')
    ghost = info + [{'id': 999, 'isthing': True, 'category_id': 86, 'area': 0, 'hexcolor': '#000000'}]
    with pytest.raises(ValueError, match='argmax of an empty sequence'):   # an instance without points
        door_window_quads(pts, ids, ghost, verts, tris)
    bad = pts.copy()
    bad[np.nonzero(ids == 3)[0][7]] = [np.nan, 0.0, 0.0]
    with pytest.raises(ValueError, match='argmax of an empty sequence'):   # a NaN distance sum
        door_window_quads(bad, ids, info, verts, tris)
    with pytest.raises(ValueError, match='argmin of an empty sequence'):   # an empty mesh
        door_window_quads(pts, ids, info, verts, np.zeros((0, 3), np.int64))
    roof = [d for d in info if d['id'] == 9 or d['category_id'] not in R.DOOR_WINDOW]
    assert [d['category_id'] in R.DOOR_WINDOW for d in roof].count(True) == 1
    with pytest.raises(ValueError, match='need at least one array'):       # every quad skipped as horizontal
        door_window_quads(pts, ids, roof, verts, tris)
    with pytest.raises(IndexError, match='vertex index'):
        f3d.default_context().door_window_quads(pts, ids, [7], verts, np.array([[0, 1, len(verts)]]))
    q, st, tri, _ = f3d.default_context().door_window_quads(pts, ids, [7], verts, tris)       # the context recovers
    assert st[0] == R.QUAD_OK
