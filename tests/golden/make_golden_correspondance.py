#!/usr/bin/env python3
"""Golden vectors of the reference's Fusion3DSeg/segUtils/correspondance.py (PointCorrespondance, Correspondance), run from the
reference.

Run in the build container (the reference is mounted at /root/reference): ``python tests/golden/make_golden_correspondance.py``.
Like make_golden.py, the class definitions are compiled from the reference's file by ``ast``; nothing of them is copied.  The
module's imports are not executed: the namespace holds NumPy, pickle, sklearn's KDTree and stand-in ``cv2`` / ``o3d`` /
``to_pcd`` / ``to_mesh`` names, which only the visualisation helpers would touch.

Contents (no pickles: every merge map is stored as CSR plus the ndim of the reference's object array):
* ``lk_*``: get_lookups(3, (4, 5));
* ``a_*``: 3 frames of 12x16 pixels (dropout pixels at the camera centres, coordinates on a 1/64 m lattice) against a cloud on the
  same lattice, r = 5/64 (many pairs exactly on r*r): merge maps and get_point on a query list with negative coordinates;
* ``b_*``: a scene whose rows all hold exactly one entry (the 2-D object array), r = 0;
* ``c_*``: a Correspondance scatter with overlapping lists and invalid points.
"""
import pickle
import sys
import types
from pathlib import Path

import numpy as np
from sklearn.neighbors import KDTree

OUT = Path(__file__).resolve().parent
sys.path.insert(0, str(OUT))
from make_golden import _defs_from  # noqa: E402


def _csr(maps):
    rows = [list(r) for r in (maps if maps.ndim == 1 else maps.tolist())]
    offs = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=offs[1:])
    idx = np.array([i for r in rows for i in r], np.int32)
    return offs, idx


def frames(rng, F, h, w):
    """F small depth frames on a 1/64 m lattice, cameras at (j/8, 0, 0); 10 % dropouts sit at their camera centre."""
    out = []
    for j in range(F):
        u, v = np.meshgrid(np.arange(w), np.arange(h))
        z = np.round((1.0 + 0.25 * np.sin(u / 5.0) + rng.uniform(0, 0.05, u.shape)) * 64) / 64
        x = np.round(((u - w / 2) / 16.0 * z + j / 8) * 64) / 64
        y = np.round(((v - h / 2) / 16.0 * z) * 64) / 64
        p = np.stack([x, y, z], -1).reshape(-1, 3)
        p[rng.random(len(p)) < 0.1] = [j / 8, 0.0, 0.0]
        out.append(p)
    return np.concatenate(out)


def main():
    rng = np.random.default_rng(20261016)
    ns = {'np': np, 'pickle': pickle, 'KDTree': KDTree, 'cv2': types.SimpleNamespace(), 'o3d': types.SimpleNamespace(),
          'to_pcd': None, 'to_mesh': None, 'tqdm': types.SimpleNamespace(), 'copy': None, 'os': None}
    _defs_from('Fusion3DSeg/segUtils/correspondance.py', ['Correspondance', 'PointCorrespondance'], ns)
    PC, CO = ns['PointCorrespondance'], ns['Correspondance']
    g = {}
    g['lk_pcd2xy'], g['lk_imgids'], g['lk_pcdimgs'] = PC.get_lookups(3, (4, 5))

    F, h, w = 3, 12, 16
    dense = frames(rng, F, h, w)
    sparse = dense[rng.choice(len(dense), 300, replace=False)] + rng.integers(-3, 4, (300, 3)) / 64
    sparse = np.concatenate([sparse, np.array([0.125, 0.0, 0.0]) + rng.integers(-1, 2, (40, 3)) / 64])   # a clump at camera 1
    r = 5 / 64
    pc = PC(sparse, dense, r, F, (h, w))
    a_offs, a_idx = _csr(pc.merge_maps)
    images = np.array([0, 1, 2, 2, -1, 0, 1])
    coords = np.array([[0, 0], [15, 11], [-1, -1], [7, 5], [3, -12], [-16, 4], [8, 6]])
    gi, gf = pc.get_point(images, coords)
    g.update(a_dense=dense, a_sparse=sparse, a_radius=np.float64(r), a_hw=np.array([F, h, w]), a_offsets=a_offs, a_indices=a_idx,
             a_ndim=np.int64(pc.merge_maps.ndim), a_images=images, a_coords=coords, a_point_indices=gi, a_point_frequency=gf)

    dense_b = np.unique(np.round(rng.uniform(-1, 1, (200, 3)) * 64) / 64, axis=0)[:192]
    sparse_b = dense_b[rng.permutation(len(dense_b))]
    mb = PC.get_merge_maps(sparse_b, dense_b, 0.0)
    b_offs, b_idx = _csr(mb)
    g.update(b_dense=dense_b, b_sparse=sparse_b, b_offsets=b_offs, b_indices=b_idx, b_ndim=np.int64(mb.ndim), b_shape=np.array(mb.shape))

    Fc, hc, wc = 2, 4, 5
    pcd2xy_c, imgids_c, _ = PC.get_lookups(Fc, (hc, wc))
    pcd2xy_c = np.vstack([PC.get_xys(hc, wc)] * Fc)                   # [N, 2], the layout Correspondance indexes with dense ids
    invalid_c = rng.random(Fc * hc * wc) < 0.3
    lists = [list(rng.choice(Fc * hc * wc, rng.integers(0, 12), replace=False)) for _ in range(9)]
    pcdimgs_c = np.full((Fc, hc, wc), -7, np.int32)
    co = CO(pcdimgs_c, invalid_c, imgids_c, pcd2xy_c, lists, (hc, wc))
    c_offs = np.zeros(len(lists) + 1, np.int64)
    np.cumsum([len(x) for x in lists], out=c_offs[1:])
    g.update(c_pcd2xy=pcd2xy_c, c_imgids=imgids_c, c_invalid=invalid_c, c_offsets=c_offs,
             c_indices=np.array([i for x in lists for i in x], np.int64), c_pcdimgs=co.pcdimgs)
    np.savez_compressed(OUT / 'correspondance.npz', **g)
    print('correspondance.npz', (OUT / 'correspondance.npz').stat().st_size, 'bytes;', 'a rows', len(a_offs) - 1, 'pairs', len(a_idx),
          'ndim', pc.merge_maps.ndim, '| b', mb.shape, '| c', co.pcdimgs.tolist())


if __name__ == '__main__':
    main()
