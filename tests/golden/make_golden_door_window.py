#!/usr/bin/env python3
"""Golden vectors of the reference's Fusion3DSeg/segUtils/door_window_bbox.py (generate_mesh), run from the reference.

Run where the reference checkout that make_golden.REF names is present: ``python tests/golden/make_golden_door_window.py``.
Like make_golden.py, the functions are compiled from the reference's file by ``ast``; nothing of them is copied.  Open3D is not
installed, so the namespace holds a stand-in ``o3d`` whose rules are the ones the port states (unpinned):
* read_triangle_mesh of an OFF file: polygon faces as fans (f0, fj, fj+1);
* compute_triangle_normals: cross(v1 - v0, v2 - v0) / sqrt((x*x + y*y) + z*z), left as it is when the squared norm is 0, and
  (0, 0, 1) when x is NaN;
* write_triangle_mesh only records the mesh.
Everything else (np.dot through this host's BLAS, einsum, argmin / argmax, the horizontal test) is the reference's own code.

Scenes (one directory each, written with the reference's file layout):
* ``a_*``: a building of 4-gon, 5-gon and split coplanar faces; doors / windows on an axis-aligned wall split in two quads (the
  inside count decides between coplanar candidates, exact ties in argmin and argmax), on a slanted wall, on the pentagon (points
  exactly on the fan's diagonal edge), one of 1 point and one of 3 000 points, one by the roof (skipped: horizontal) and one by the
  floor (the normal is -z: _get_perpendicular_vectors takes its other branch); the cloud is shuffled;
* ``c_*``: the same scene turned about z by an irrational angle, with float64 noise (no exact arithmetic anywhere);
* ``b_*``: a window whose points lie exactly in a mesh plane (minimum 0: no candidate, ValueError).
"""
import json
import pickle
import sys
import tempfile
import types
from pathlib import Path

import numpy as np

OUT = Path(__file__).resolve().parent
sys.path.insert(0, str(OUT))
from make_golden import _defs_from  # noqa: E402


def read_off(path):
    """OFF -> (vertices float64 [V, 3], triangles int64 [T, 3]); polygon faces as fans (f0, fj, fj+1)."""
    toks = []
    for line in Path(path).read_text().splitlines():
        line = line.split('#', 1)[0].strip()
        if line:
            toks += line.split()
    assert toks[0] == 'OFF'
    nv, nf = int(toks[1]), int(toks[2])
    at = 4
    verts = np.array(toks[at:at + 3 * nv], dtype=np.float64).reshape(nv, 3)
    at += 3 * nv
    tris = []
    for _ in range(nf):
        m = int(toks[at])
        f = [int(x) for x in toks[at + 1:at + 1 + m]]
        at += 1 + m
        tris += [[f[0], f[j], f[j + 1]] for j in range(1, m - 1)]
    return verts, np.array(tris, dtype=np.int64).reshape(-1, 3)


def normals_of(verts, tris):
    tv = verts[tris]
    a, b = tv[:, 1] - tv[:, 0], tv[:, 2] - tv[:, 0]
    c = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)
    nn = (c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]
    with np.errstate(invalid='ignore', divide='ignore'):
        n = np.where((nn > 0)[:, None], c / np.sqrt(nn)[:, None], c)
    n[np.isnan(n[:, 0])] = [0.0, 0.0, 1.0]
    return n


class _Mesh:
    def __init__(self):
        self.vertices = self.triangles = self.vertex_colors = self.triangle_normals = None

    def compute_triangle_normals(self):
        self.triangle_normals = normals_of(np.asarray(self.vertices), np.asarray(self.triangles))
        return self


def _o3d(written):
    def read_triangle_mesh(path):
        m = _Mesh()
        m.vertices, m.triangles = read_off(path)
        return m

    def write_triangle_mesh(filename, mesh):
        written[filename] = mesh
        return True

    return types.SimpleNamespace(
        geometry=types.SimpleNamespace(TriangleMesh=_Mesh),
        utility=types.SimpleNamespace(Vector3dVector=lambda a: np.asarray(a, np.float64), Vector3iVector=lambda a: np.asarray(a, np.int32)),
        io=types.SimpleNamespace(read_triangle_mesh=read_triangle_mesh, write_triangle_mesh=write_triangle_mesh))


# the building: 0 <= x <= 8, 0 <= y <= 6, 0 <= z <= 3; the wall x = 0 leans in to x = 1 at the top; the wall x = 8 is a gable
BUILDING_V = [[0, 0, 0], [4, 0, 0], [8, 0, 0], [8, 6, 0], [0, 6, 0],          # 0-4 floor corners (+ the split point of y = 0)
              [1, 0, 3], [4, 0, 3], [8, 0, 3], [8, 6, 3], [1, 6, 3],          # 5-9 top corners
              [8, 3, 4]]                                                      # 10 gable apex
BUILDING_F = [[0, 1, 6, 5], [1, 2, 7, 6],            # wall y = 0 in two coplanar quads
              [2, 3, 8, 10, 7],                      # gable wall x = 8 (a pentagon)
              [3, 4, 9, 8],                          # wall y = 6
              [4, 0, 5, 9],                          # the slanted wall
              [6, 7, 8, 9, 5],                       # roof z = 3 (a pentagon with a collinear vertex, not in any fan triangle)
              [1, 0, 4, 3, 2]]                       # floor z = 0, facing down


def off_text(verts, faces):
    lines = ['OFF', '# building', f'{len(verts)} {len(faces)} 0']
    lines += [' '.join(repr(float(c)) for c in v) for v in verts]
    lines += [' '.join(str(x) for x in [len(f)] + list(f)) for f in faces]
    return '\n'.join(lines) + '\n'


def lattice(rng, n, lo, hi, q=64):
    return np.round(rng.uniform(lo, hi, (n, len(lo))) * q) / q


def scene_a(rng):
    parts = []                                         # (points, id, category)
    p = lattice(rng, 3000, [3.0, -0.125, 0.0], [5.0, 0.125, 2.25])
    parts.append((p, 7, 86))                           # door across the two coplanar quads of y = 0
    p = lattice(rng, 64, [1.0, -0.0625, 0.5], [7.0, 0.0625, 1.0])
    p[:, 0] = np.where(np.arange(64) % 2 == 0, 2.0, 6.0) + p[:, 0] / 1024
    parts.append((p, 12, 115))                         # even split between the two quads: ties in the inside counts
    t = rng.uniform(0.5, 1.5, (500, 2))
    p = np.stack([t[:, 1] / 3 + rng.normal(0, 0.02, 500), rng.uniform(2.0, 4.0, 500), t[:, 1]], 1)
    parts.append((p, 3, 116))                          # window on the slanted wall
    s = np.round(rng.uniform(0.5, 2.5, 200) * 16) / 16
    p = np.stack([np.full(200, 8.0), 2 * s, s], 1)     # on the fan's diagonal (8,0,0)-(8,6,3) of the gable ...
    p[::2, 0] += np.round(rng.uniform(-0.25, 0.25, 100) * 64) / 64
    parts.append((p, 21, 115))                         # ... half of them off the wall
    parts.append((np.array([[2.5, 6.25, 1.5]]), 30, 86))            # a single point by the wall y = 6
    p = lattice(rng, 120, [2.0, 2.0, 2.875], [5.0, 4.0, 3.125])
    parts.append((p, 9, 115))                          # by the roof: horizontal, skipped
    p = lattice(rng, 150, [2.0, 1.0, -0.125], [6.0, 5.0, 0.0625])
    parts.append((p, 14, 116))                         # by the floor (normal -z)
    p = lattice(rng, 400, [0.5, 0.5, 0.0], [7.5, 5.5, 3.0])
    parts.append((p, 2, 50))                           # not a door or a window
    p = lattice(rng, 600, [0.0, 0.0, 0.0], [8.0, 6.0, 3.0])
    parts.append((p, 0, 133))                          # the rest
    return parts


def assemble(rng, parts, turn=None, noise=0.0):
    pts = np.concatenate([p for p, _, _ in parts])
    ids = np.concatenate([np.full(len(p), i, np.int64) for p, i, _ in parts])
    verts = np.array(BUILDING_V, np.float64)
    if turn is not None:
        c, s = np.cos(turn), np.sin(turn)
        R = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
        pts, verts = pts @ R.T + np.array([0.3, -1.7, 0.2]), verts @ R.T + np.array([0.3, -1.7, 0.2])
    pts = pts + rng.normal(0, noise, pts.shape) if noise else pts
    perm = rng.permutation(len(pts))
    info = []
    for _, i, cat in parts:
        clr = rng.integers(0, 256, 3)
        info.append({'id': int(i), 'isthing': cat != 133, 'category_id': int(cat), 'area': int((ids == i).sum()),
                     'hexcolor': '#' + ''.join(f'{int(x):02x}' for x in clr)})
    order = rng.permutation(len(info))
    return pts[perm], ids[perm], [info[k] for k in order], verts


def run(ns, written, root, pts, ids, info, verts):
    d = Path(root)
    (d / 'fusion').mkdir(parents=True)
    (d / 'panoptic_segmentation').mkdir()
    (d / 'polyfit').mkdir()
    with open(d / 'fusion' / 'fusion_data.pkl', 'wb') as fp:
        pickle.dump({'points': pts, 'colors': np.zeros_like(pts)}, fp)
    np.save(d / 'panoptic_segmentation' / 'ids.npy', ids)
    (d / 'panoptic_segmentation' / 'info.json').write_text(json.dumps(info))
    text = off_text(verts, BUILDING_F)
    (d / 'polyfit' / 'building.off').write_text(text)
    v, t = read_off(d / 'polyfit' / 'building.off')
    rec = {'points': pts, 'ids': ids, 'info': np.array(json.dumps(info)), 'off': np.array(text), 'vertices': v, 'triangles': t,
           'normals': normals_of(v, t)}
    try:
        tid, mesh = ns['generate_mesh'](str(d))
    except ValueError as exc:
        rec['raises'] = np.array(str(exc))
        return rec
    rec.update(triangle_ids=tid, quad_vertices=np.asarray(mesh.vertices), quad_triangles=np.asarray(mesh.triangles),
               quad_colors=np.asarray(mesh.vertex_colors))
    assert list(written) == [str(d / 'panoptic_segmentation' / 'door_window_mesh.ply')]
    assert np.array_equal(np.load(d / 'panoptic_segmentation' / 'triangle_ids.npy'), tid)
    written.clear()
    return rec


def main():
    rng = np.random.default_rng(20261016)
    written = {}
    ns = {'np': np, 'json': json, 'pickle': pickle, 'Path': Path, 'o3d': _o3d(written)}
    _defs_from('Fusion3DSeg/segUtils/door_window_bbox.py',
               ['_get_door_window_mesh', '_hex_to_rgb', '_point_in_triangle', '_get_perpendicular_vectors', 'generate_mesh'], ns)
    g = {}
    with tempfile.TemporaryDirectory() as tmp:
        scenes = {'a': assemble(rng, scene_a(rng)),
                  'c': assemble(rng, scene_a(rng), turn=np.sqrt(2.0), noise=1e-3)}
        flat = [(lattice(rng, 40, [1.0, 6.0, 0.5], [3.0, 6.0, 2.5]), 5, 116), (lattice(rng, 30, [0.0, 0.0, 0.0], [8.0, 6.0, 3.0]), 0, 133)]
        scenes['b'] = assemble(rng, flat)
        for name, (pts, ids, info, verts) in scenes.items():
            rec = run(ns, written, Path(tmp) / name, pts, ids, info, verts)
            g.update({f'{name}_{k}': v for k, v in rec.items()})
            print(name, len(pts), 'points', len(rec['triangles']), 'triangles',
                  'raises: ' + str(rec['raises']) if 'raises' in rec else f"{len(rec['triangle_ids']) // 2} quads {rec['triangle_ids'].tolist()}")
    assert 'raises' not in {k.split('_', 1)[1] for k in g if k[0] in 'ac'} and 'b_raises' in g
    np.savez_compressed(OUT / 'door_window.npz', **g)
    print('door_window.npz', (OUT / 'door_window.npz').stat().st_size, 'bytes')


if __name__ == '__main__':
    main()
