#!/usr/bin/env python3
"""Golden vectors of the reference's Fusion3DSeg/segUtils/refinement.py, run from the reference.

Run where the reference checkout that make_golden.REF names is present: ``python tests/golden/make_golden_refinement.py``.
The functions are compiled from the reference's file by ``ast`` at generation time; nothing of them is copied.
* The four nested floods (floodfill_depth_points / _point, floodfill_color_points / _point) use only NumPy: they are lifted out
  of their enclosing functions with ``ast.walk`` and run directly.
* The four public functions, GetactualIndex, door_updation and door_floor_align are run end to end in a temporary directory.
  Stand-ins (no Open3D, no viewer here): ``o3d.io.read_point_cloud`` returns the cloud this script registered for that path,
  ``to_pcd`` builds the same kind of object, ``pick_points`` returns the fixture's picked indices, ``Putil.Col`` is the column map
  of planeUtils.Headers.  ``Quat`` is the reference's SpatQuadranion over a base class that restates pyquaternion's
  ``axis=, angle=`` constructor (cos(a/2), sin(a/2) axis/|axis|) and ``.inverse``: that piece is "parity unpinned".
* tests/refinement_ref.py (the restatement) is asserted equal to the reference on every flood case.

The cloud: 4 000 points on a 10 x 10 wall, lifted off it by 0.02 sin(x) + noise, turned and shifted so that the plane distance is
a general dot product; a radius graph (sklearn KDTree, r = 0.3, rows in the tree's order) and the same graph with every row
reordered (refinement_ref.shuffled_csr).  Every flood case is either meant to return nothing (level limit 1, 2 for the instance variants, or a threshold no seed
meets), or the one seed alone (floodfill_color_point at level limit 2), or must accept some and reject some of the points a threshold-free flood with the same level limit reaches.
"""
import os
import sys
import tempfile
import types
import ast
from collections import deque
from pathlib import Path

import numpy as np
from sklearn.neighbors import KDTree

OUT = Path(__file__).resolve().parent
sys.path.insert(0, str(OUT))
sys.path.insert(0, str(OUT.parent))
from make_golden import REF, _defs_from, _QuaternionBase  # noqa: E402
import refinement_ref as R  # noqa: E402

RELPATH = 'Fusion3DSeg/segUtils/refinement.py'
FLOODS = ['floodfill_depth_points', 'floodfill_depth_point', 'floodfill_color_points', 'floodfill_color_point']


def nested_defs(names, ns):
    tree = ast.parse((REF / RELPATH).read_text())
    keep = [n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name in names]
    assert sorted(n.name for n in keep) == sorted(names)
    exec(compile(ast.Module(body=keep, type_ignores=[]), str(REF / RELPATH), 'exec'), ns)
    return ns


class _AxisAngle(_QuaternionBase):
    """pyquaternion's constructor forms the reference uses: a 4-sequence, or axis= / angle=."""

    def __init__(self, seq=None, axis=None, angle=None):
        if axis is not None:
            axis = np.asarray(axis, np.float64)
            half = float(angle) / 2.0
            seq = np.concatenate([[np.cos(half)], np.sin(half) * axis / np.linalg.norm(axis)])
        super().__init__(seq)


class _Cloud:
    def __init__(self, points, colors):
        self.points, self.colors = np.array(points, np.float64), np.array(colors, np.float64)


def reachable(rows, seeds, max_level, given):
    """points a threshold-free flood accepts: everything enqueued below the level limit (without the seeds when they are given)"""
    seen = np.zeros(len(rows), bool)
    seen[list(seeds)] = True
    todo = deque((int(s), 1) for s in seeds)
    cnt = 0
    while todo:
        p, lv = todo.popleft()
        if lv == max_level:
            continue
        cnt += not (given and lv == 1)
        for q in rows[p]:
            if not seen[q]:
                seen[q] = True
                todo.append((int(q), lv + 1))
    return cnt


def main():
    rng = np.random.default_rng(20261016)
    n = 4000
    xy = rng.uniform(0, 10, (n, 2))
    lift = 0.02 * np.sin(xy[:, 0]) + rng.normal(0, 0.004, n)
    a = 0.7
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]])
    Rx = np.array([[1.0, 0, 0], [0, np.cos(1.1), -np.sin(1.1)], [0, np.sin(1.1), np.cos(1.1)]])
    rot, shift = Rz @ Rx, np.array([1.5, -2.25, 0.75])
    points = np.stack([xy[:, 0], xy[:, 1], lift], 1) @ rot.T + shift
    normal = rot @ np.array([0.0, 0.0, 1.0])
    wall_quad = np.array([[0, 0, 0], [10, 0, 0], [10, 10, 0], [0, 10, 0.0]]) @ rot.T + shift
    colors = np.clip(np.stack([xy[:, 0] / 10, xy[:, 1] / 10, np.full(n, 0.5)], 1) + rng.normal(0, 0.02, (n, 3)), 0, 1)
    rows0 = [r.astype(np.int64) for r in KDTree(xy).query_radius(xy, r=0.3)]
    offs0 = np.concatenate([[0], np.cumsum([len(r) for r in rows0])]).astype(np.int64)
    offs1, nb1 = R.shuffled_csr(offs0, np.concatenate(rows0))          # graph 1 is derived from graph 0, not stored
    rows1 = [nb1[offs1[i]:offs1[i + 1]].astype(np.int64) for i in range(n)]
    assert sum((a != b).any() for a, b in zip(rows0, rows1)) > n // 2
    graphs = [rows0, rows1]
    # the reference's own expression for the distance to the wall (refinement.py:153-157)
    pv = points[:, None, :] - wall_quad[0].reshape(1, 3)[None, :, :]
    dist = np.abs(np.einsum('nmc, mc -> mn', pv, normal.reshape(1, 3))[0])

    ns = nested_defs(FLOODS, {'np': np})
    centre = ((xy - 5) ** 2).sum(1)
    inst_small = np.nonzero(centre < 1.0)[0]                        # an instance whose points all sit at one depth
    inst_wide = np.nonzero(((xy - [3.0, 5.0]) ** 2).sum(1) < 4.0)[0]  # one that spans the sine: part of it fails the threshold
    pick1 = [int(inst_small[0])]
    far = int(np.argmax(np.where(centre < 4.0, np.abs(dist - dist[inst_small[0]]), -1)))     # a pick at another depth
    pick3 = [int(inst_small[0]), far, int(inst_small[5])]
    col32 = colors.astype(np.float32)
    t3 = np.array([0.1, 0.1, 0.1])
    values = {'dist': dist, 'col': colors, 'col32': col32}
    cases = []                                                       # (kind, graph, values, seeds, threshold, max_level, want_empty)
    for ml in (0, 1, 2, 5, 50):
        cases.append(('depth_points', 0, 'dist', inst_small, 0.01, ml, ml in (1, 2)))
        cases.append(('depth_point', 0, 'dist', pick1 if ml != 2 else pick3, 0.01, ml, ml == 1))
        cases.append(('color_points', 0, 'col', inst_small, t3, ml, ml in (1, 2)))
        # one seed at level limit 2 returns the seed alone: a declared 'seed only' case (it cannot reject a reachable point)
        cases.append(('color_point', 0, 'col', pick1[0], t3, ml, 'seed' if ml == 2 else ml == 1))
    cases.append(('depth_point', 0, 'dist', pick3, 0.01, 50, False))
    cases.append(('depth_point', 1, 'dist', pick3, 0.01, 5, False))
    cases.append(('depth_points', 0, 'dist', inst_wide, 0.01, 50, False))           # given seeds that do not expand
    cases.append(('color_points', 0, 'col', inst_wide, np.array([0.05, 0.2, 0.2]), 50, False))
    cases.append(('depth_points', 1, 'dist', inst_small, 0.01, 50, False))           # shuffled rows
    cases.append(('color_points', 1, 'col', inst_small, t3, 5, False))
    cases.append(('color_point', 1, 'col', pick1[0], t3, 50, False))
    cases.append(('color_points', 0, 'col32', inst_small, t3, 50, False))           # float32 colours
    cases.append(('color_point', 0, 'col32', pick1[0], t3, 5, False))
    cases.append(('color_point', 1, 'col32', far, np.array([0.05, 0.1, 0.3]), 0, False))
    cases.append(('depth_points', 0, 'dist', inst_wide, 1e-7, 50, True))            # no seed meets the threshold
    g = {'points': points, 'colors': colors, 'dist': dist, 'wall_normal': normal, 'wall_quad': wall_quad, 'ncases': np.array(len(cases))}
    g['g0_offsets'], g['g0_neighbours'] = offs0, np.concatenate(rows0).astype(np.int32)
    for k, (kind, gi, vname, seeds, thr, ml, want_empty) in enumerate(cases):
        rows, val = graphs[gi], values[vname]
        if kind == 'color_point':
            want = ns['floodfill_color_point'](int(seeds), n, [list(r) for r in rows], val, thr, ml)
            mine = R.color_point(val, rows, seeds, thr, ml)
            given, sd = False, [int(seeds)]
        else:
            sd = np.asarray(seeds) if kind.endswith('points') else list(seeds)
            want = ns['floodfill_' + kind](sd, n, [list(r) for r in rows], val, thr, ml)
            mine = getattr(R, kind)(val, rows, seeds, thr, ml)
            given = kind.endswith('points')
        want = np.asarray(want, np.int64).reshape(-1)
        assert np.array_equal(mine, want), (k, kind)
        reach = reachable(rows, list(np.asarray(sd).reshape(-1)), ml, given)
        if want_empty == 'seed':
            assert want.tolist() == [int(seeds)] and reach == 1, (k, kind, want)
        elif want_empty:
            assert len(want) == 0, (k, kind, len(want))
        else:
            assert 0 < len(want) < reach, (k, kind, len(want), reach)
        if given and not want_empty:
            sma0 = np.average(val[np.asarray(sd)], axis=0)
            failing = int((np.abs(sma0 - val[np.asarray(sd)]) > thr).reshape(len(sd), -1).any(1).sum())
            g[f'c{k}_seeds_failing'] = np.array(failing)
        print(f'case {k:2d} {kind:13s} graph {gi} {vname:5s} max_level {ml:2d} seeds {len(np.asarray(sd).reshape(-1)):4d} '
              f'-> {len(want):4d} of {reach}')
        g[f'c{k}_kind'], g[f'c{k}_graph'], g[f'c{k}_values'] = np.array(kind), np.array(gi), np.array(vname)
        g[f'c{k}_seeds'], g[f'c{k}_threshold'], g[f'c{k}_max_level'] = np.asarray(seeds, np.int64), np.asarray(thr, np.float64), np.array(ml)
        g[f'c{k}_cluster'] = want
    assert any(int(g[f'c{k}_seeds_failing']) > 0 for k in range(len(cases)) if f'c{k}_seeds_failing' in g)

    # ---- the public functions, end to end
    clouds, picked = {}, {}
    o3d = types.SimpleNamespace(io=types.SimpleNamespace(read_point_cloud=lambda path: clouds[os.path.normpath(path)]))
    ns_q = {'np': np, 'Quaternion': _AxisAngle}
    _defs_from('RTAB_utils/spatQuad.py', ['SpatQuadranion'], ns_q)
    pub = {'np': np, 'os': os, 'o3d': o3d, 'Quat': ns_q['SpatQuadranion'],
           'to_pcd': lambda points, colors=None, **kw: _Cloud(points, colors),
           'pick_points': lambda pcd: list(picked['now']),
           'Putil': types.SimpleNamespace(Col=lambda s: {'Shapeinfo': 0, 'indicies': 1, 'BBoxids': 2, 'BBoxpoints': 3}[s]),
           'print': lambda *a, **k: None}
    _defs_from(RELPATH, ['GetactualIndex', 'door_updation', 'depth_floodfill_dl', 'depth_floodfill_point', 'color_floodfill_dl',
                         'color_floodfill_point', 'door_floor_align'], pub)
    ids = np.zeros(n, np.int64)
    ids[inst_wide] = 4
    ids[inst_small] = 7                                               # the door; where the two overlap the door wins
    palette = np.array([[200, 200, 200], [0, 0, 0], [0, 0, 0], [0, 0, 0], [30, 144, 255], [0, 0, 0], [0, 0, 0], [255, 99, 71]]) / 255.0
    seg_colors = palette[ids]
    assert np.array_equal(np.clip(seg_colors * 255.0, 0, 255).astype(np.uint8) / 255.0, seg_colors)      # survives a uchar PLY
    vertex = np.hstack([points, colors])
    door_quad = np.array([[4, 4, 0], [6, 4, 0], [6, 6, 0], [4, 6, 0.0]]) @ rot.T + shift
    plane_normals = np.stack([normal, normal])
    plane_sets = [np.setdiff1d(np.arange(n), inst_small), inst_small]           # row 0 = the wall, row 1 = the door
    quads = np.stack([wall_quad, door_quad])
    g.update(ids=ids, seg_colors=seg_colors, plane_normals=plane_normals, plane_quads=quads,
             plane_index_offsets=np.array([0, len(plane_sets[0]), len(plane_sets[0]) + len(plane_sets[1])], np.int64),
             plane_index_values=np.concatenate(plane_sets).astype(np.int64))
    wall_sel = [points[int(plane_sets[0][0])]]                        # a selected vertex of the wall: the wall's normal is used
    g['selected_vertices'] = np.array(wall_sel)
    runs = [('depth_floodfill_dl', 'panoptic_segmentation', pick1, dict(depth_threshold=0.01, max_level=50)),
            ('depth_floodfill_point', 'panoptic_segmentation', pick3, dict(depth_threshold=0.01, max_level=50)),
            ('color_floodfill_dl', 'cv_segmentation', pick1, dict(color_threshold=0.1, max_level=5)),
            ('color_floodfill_point', 'panoptic_segmentation', pick1, dict(color_threshold=0.1)),
            ('depth_floodfill_dl', 'panoptic_segmentation', pick1, dict(depth_threshold=0.01, max_level=2)),       # unchanged
            ('depth_floodfill_dl', 'panoptic_segmentation', [int(inst_wide[3])], {})]                              # the defaults
    g['nruns'] = np.array(len(runs))
    adj0 = [r.tolist() for r in rows0]          # lists, as ReadVerticesConnectedFiles returns them: a set would iterate in hash order
    with tempfile.TemporaryDirectory() as tmp:
        for k, (name, where, pick, kw) in enumerate(runs):
            d = Path(tmp) / f'run{k}'
            (d / where).mkdir(parents=True)
            np.save(d / where / 'ids.npy', ids)
            (d / where / 'pcd.ply').write_bytes(b'')                  # must exist for the cv_segmentation branch; read by the stand-in
            clouds[os.path.normpath(str(d / where / 'pcd.ply'))] = _Cloud(points, seg_colors)
            picked['now'] = pick
            table, bounding = R.plane_table(plane_normals, g['plane_index_offsets'], g['plane_index_values'], quads)
            if name.startswith('depth'):
                out_ids, out_pcd = pub[name](table, vertex.copy(), wall_sel, bounding, adj0, str(d), **kw)
            else:
                out_ids, out_pcd = pub[name](vertex.copy(), adj0, str(d), **kw)
            changed = int((out_ids != ids).sum())
            print(f'run {k} {name} pick {pick} {kw}: {changed} ids changed')
            assert (changed == 0) == (k == 4), (k, changed)
            g[f'r{k}_name'], g[f'r{k}_where'], g[f'r{k}_pick'] = np.array(name), np.array(where), np.array(pick, np.int64)
            g[f'r{k}_kw_names'] = np.array(list(kw.keys()), dtype='U32')
            g[f'r{k}_kw_values'] = np.array(list(kw.values()), np.float64)
            g[f'r{k}_ids'], g[f'r{k}_colors'] = np.asarray(out_ids), np.asarray(out_pcd.colors)

    # ---- door_updation: corners nearer and farther than max_distance from one and from two wall sides
    outer = wall_quad
    flat = lambda q: np.array(q, np.float64) @ rot.T + shift + 0.05 * normal     # noqa: E731  (off the wall plane: projected first)
    doors = [flat([[4, 0.1, 0], [6, 0.1, 0], [6, 3, 0], [4, 3, 0]]),            # two corners near one side
             flat([[0.1, 0.15, 0], [2, 0.15, 0], [2, 3, 0], [0.1, 3, 0]]),      # one corner near two sides, two near one
             flat([[4, 4, 0], [6, 4, 0], [6, 6, 0], [4, 6, 0]]),                # none near
             flat([[9.9, 9.85, 0], [9.9, 5, 0], [5, 5, 0], [5, 9.85, 0]])]      # the far corner of the wall
    g['ndoors'] = np.array(len(doors) * 2)
    for k, dq in enumerate(doors):
        for j, md in enumerate((0.2, 0.12)):
            g[f'd{2 * k + j}_inner'], g[f'd{2 * k + j}_max_distance'] = dq, np.array(md)
            g[f'd{2 * k + j}_out'] = pub['door_updation'](outer, dq, normal, md)
    assert not np.allclose(g['d0_out'], g['d4_out'])
    # ---- door_floor_align: the door's quad turned by 0.2 rad about the wall normal
    c, s = np.cos(0.2), np.sin(0.2)
    tilted = (np.array([[4, 4, 0], [6, 4, 0], [6, 6, 0], [4, 6, 0.0]]) - [4, 4, 0]) @ np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]]).T + [4, 4, 0]
    tilted = tilted @ rot.T + shift
    for j, flip in enumerate((True, False)):
        table, bounding = R.plane_table(plane_normals, g['plane_index_offsets'], g['plane_index_values'], np.stack([wall_quad, tilted]))
        sel = [points[int(plane_sets[1][0])], points[int(plane_sets[0][0])]]    # the door first, then the wall
        _, _, b = pub['door_floor_align'](table, vertex, sel, bounding, adj0, '', flip=flip)
        g[f'a{j}_out'] = np.array(b[1])
    g['align_quad'], g['align_selected'] = tilted, np.array(sel)
    np.savez_compressed(OUT / 'refinement.npz', **g)
    print('wrote', OUT / 'refinement.npz', (OUT / 'refinement.npz').stat().st_size, 'bytes')


if __name__ == '__main__':
    main()
