#!/usr/bin/env python3
"""Golden vectors of the reference's mesh-topology functions (Fusion3DSeg/segUtils/meshUtils.py), run from the reference.

Run in the build container (the reference is mounted at /root/reference): ``python tests/golden/make_golden_mesh.py``.
The module itself cannot be imported without cv2 / open3d, so -- like the other makers -- vertex_triangle_mapping,
remove_faces_by_vertices, keep_faces_by_vertices, bbox_axes and one_to_all_angles are compiled from the reference's file by
``ast``; nothing of it is copied.  The fixture holds arrays only.

``scenes`` lists the scene names.  Per scene ``<s>``: ``<s>_vertices`` [V, 3], ``<s>_triangles`` [M, 3] (int64 or int32), ``<s>_mask``
[V] and
* ``<s>_tov`` / ``<s>_pov`` / ``<s>_offsets``: the two lists of lists of vertex_triangle_mapping, rows concatenated;
* ``<s>_not_removed``, ``<s>_remaining``, ``<s>_old2new``: remove_faces_by_vertices(V, triangles, mask);
* ``<s>_kept_vertices`` [P, 3], ``<s>_kept_triangles`` [Q, 3]: keep_faces_by_vertices(vertices, copy of triangles, mask), its lists
  of rows stacked.
Scenes: ``some`` / ``none`` / ``all`` (one random mesh of 40 vertices and 60 faces, a mask of some, no and all vertices); ``odd`` (int32;
30 vertices of which 5 are unreferenced, faces with a repeated vertex, duplicated faces); ``empty`` (M = 0); ``corners`` (a face
whose only masked vertex is its last corner; a vertex first seen in corner 2 of one face and in corner 0 of a later one; an
unkept face).
``box_corners`` [8, 3] -> ``box_origin``, ``box_i``, ``box_j``, ``box_li``, ``box_lj`` (bbox_axes); ``ang_vec1`` [4, 3], ``ang_vec2`` [5, 3] ->
``ang_angles`` [5, 4] and the two arguments as one_to_all_angles leaves them, ``ang_vec1_after`` / ``ang_vec2_after``.
"""
import sys
from pathlib import Path

import numpy as np

OUT = Path(__file__).resolve().parent
sys.path.insert(0, str(OUT))
from make_golden import _defs_from  # noqa: E402

NAMES = ['vertex_triangle_mapping', 'remove_faces_by_vertices', 'keep_faces_by_vertices', 'bbox_axes', 'one_to_all_angles']


def scenes(rng):
    verts = rng.uniform(-1, 1, (40, 3))
    tris = rng.integers(0, 40, (60, 3)).astype(np.int64)
    out = {'some': (verts, tris, rng.random(40) < 0.3), 'none': (verts, tris, np.zeros(40, bool)), 'all': (verts, tris, np.ones(40, bool))}
    v = rng.uniform(-1, 1, (30, 3))
    t = rng.integers(0, 25, (24, 3)).astype(np.int32)
    t[3] = [7, 7, 2]; t[9] = [4, 11, 4]; t[10] = [5, 5, 5]                  # repeated vertices
    t[15] = t[1]; t[16] = t[1]; t[20] = t[3]                               # duplicated faces
    out['odd'] = (v, t, rng.random(30) < 0.25)
    out['empty'] = (rng.uniform(-1, 1, (10, 3)), np.zeros((0, 3), np.int64), rng.random(10) < 0.5)
    t = np.array([[0, 1, 2], [2, 3, 4], [8, 9, 10], [5, 6, 7], [4, 0, 2]], np.int64)
    m = np.zeros(12, bool); m[[2, 7]] = True
    out['corners'] = (rng.uniform(-1, 1, (12, 3)), t, m)
    return out


def main():
    rng = np.random.default_rng(20261017)
    ns = _defs_from('Fusion3DSeg/segUtils/meshUtils.py', NAMES, {'np': np})
    g = {}
    sc = scenes(rng)
    g['scenes'] = np.array(list(sc))
    for name, (verts, tris, mask) in sc.items():
        nv = len(verts)
        g[f'{name}_vertices'], g[f'{name}_triangles'], g[f'{name}_mask'] = verts, tris, mask
        tov, pov = ns['vertex_triangle_mapping'](tris, nv)
        g[f'{name}_offsets'] = np.concatenate([[0], np.cumsum([len(r) for r in tov])]).astype(np.int64)
        g[f'{name}_tov'] = np.array([x for r in tov for x in r], np.int64)
        g[f'{name}_pov'] = np.array([x for r in pov for x in r], np.int64)
        nr, rem, o2n = ns['remove_faces_by_vertices'](nv, tris, mask)
        assert rem.dtype == tris.dtype
        g[f'{name}_not_removed'], g[f'{name}_remaining'], g[f'{name}_old2new'] = nr, rem.reshape(-1, 3), o2n.astype(np.int64)
        kv, kt = ns['keep_faces_by_vertices'](verts, tris.copy(), mask)
        g[f'{name}_kept_vertices'] = np.array(kv, np.float64).reshape(-1, 3)
        g[f'{name}_kept_triangles'] = np.array(kt, tris.dtype).reshape(-1, 3)
    half = np.array([1.5, 0.4, 0.9])
    signs = np.array([[-1, -1, -1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1], [1, 1, 1], [-1, 1, 1], [1, -1, 1], [1, 1, -1]], np.float64)
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    g['box_corners'] = (signs * half) @ q.T + rng.uniform(-1, 1, 3)
    g['box_origin'], g['box_i'], g['box_j'], g['box_li'], g['box_lj'] = ns['bbox_axes'](g['box_corners'])
    g['ang_vec1'], g['ang_vec2'] = rng.standard_normal((4, 3)), rng.standard_normal((5, 3))
    v1, v2 = g['ang_vec1'].copy(), g['ang_vec2'].copy()
    g['ang_angles'] = ns['one_to_all_angles'](v1, v2)
    g['ang_vec1_after'], g['ang_vec2_after'] = v1, v2
    np.savez_compressed(OUT / 'mesh.npz', **g)
    print(f'wrote {OUT / "mesh.npz"}: {len(g)} arrays')


if __name__ == '__main__':
    main()
