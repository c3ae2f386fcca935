#!/usr/bin/env python3
"""Golden vectors of the orientation step of RTAB2Cache.surface_normal_estimation (RTAB_utils/ios_rtab.py:236-248), run from
the reference.

Run in the build container (the reference is mounted at /root/reference): ``python tests/golden/make_golden_normals.py``.
Like make_golden.py, the class definition is compiled from the reference's file by ``ast``; nothing of it is copied.  Open3D
is not installed, so a stand-in ``o3d`` namespace is passed whose ``estimate_normals`` installs given raw unit normals: the
reference's own orientation lines (:241-246) then run on them.  Open3D's normals themselves cannot be pinned here.

Rows: random points and normals; rows with p == c (NaN direction: never flipped); rows whose dot product is exactly 0.
"""
import sys
import types
from pathlib import Path

import numpy as np

OUT = Path(__file__).resolve().parent
sys.path.insert(0, str(OUT))
from make_golden import _defs_from  # noqa: E402


def _o3d(raw):
    class PointCloud:
        def estimate_normals(self, search_param=None):
            assert search_param == (0.05, 30)
            self.normals = np.array(raw, copy=True)
    geometry = types.SimpleNamespace(PointCloud=PointCloud, KDTreeSearchParamHybrid=lambda radius, max_nn: (radius, max_nn))
    utility = types.SimpleNamespace(Vector3dVector=lambda a: np.asarray(a))
    return types.SimpleNamespace(geometry=geometry, utility=utility)


def main():
    rng = np.random.default_rng(20261015)
    cam = np.array([0.25, -1.5, 0.75])
    n = 2000
    pts = cam + rng.normal(size=(n, 3)) * rng.uniform(0.01, 3.0, (n, 1))
    raw = rng.normal(size=(n, 3))
    raw /= np.linalg.norm(raw, axis=1, keepdims=True)
    pts[:40] = cam                                                     # p == c: the zero-depth pixels
    # dot exactly 0: p - c along one axis, the normal in the orthogonal plane
    for k in range(40, 80):
        axis = k % 3
        d = np.zeros(3)
        d[axis] = rng.uniform(0.1, 2.0) * (1 if k % 2 else -1)
        pts[k] = cam + d
        v = rng.normal(size=3)
        v[axis] = 0.0
        raw[k] = v / np.linalg.norm(v)
    ns = {'np': np, 'o3d': _o3d(raw)}
    _defs_from('RTAB_utils/ios_rtab.py', ['RTAB2Cache'], ns)
    cache = object.__new__(ns['RTAB2Cache'])
    with np.errstate(invalid='ignore', divide='ignore'):
        oriented = cache.surface_normal_estimation(pts, cam)
    np.savez_compressed(OUT / 'normals_orient.npz', points=pts, cam_centre=cam, raw=raw, oriented=oriented)
    print('normals_orient.npz', (OUT / 'normals_orient.npz').stat().st_size, 'bytes')


if __name__ == '__main__':
    main()
