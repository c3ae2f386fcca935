"""CPU-side checks of the TSDF reconstruction: the bindings exist, the public surface is named, the NumPy restatement
(tests/tsdf_ref.py) produces a closed, consistently wound surface on an analytic sphere, and argument errors need no device."""
import ctypes as C

import numpy as np
import pytest

import f3d
import tsdf_ref as R
from Fusion3DSeg.segUtils import reconstruct

TSDF_SYMBOLS = ['f3d_tsdf_integrate', 'f3d_tsdf_integrate_dev', 'f3d_tsdf_extract_count', 'f3d_tsdf_extract_count_dev',
                'f3d_tsdf_extract_fill', 'f3d_tsdf_extract_fill_dev', 'f3d_ctx_reserve_tsdf', 'f3d_debug_tsdf_grid_cap']


def test_symbols_are_bound():
    lib = f3d.library()
    for name in TSDF_SYMBOLS:
        fn = getattr(lib, name)
        assert name in lib._f3d_symbols
        assert fn.restype is C.c_int and fn.argtypes and fn.argtypes[0] is C.c_void_p
    assert len(lib.f3d_tsdf_integrate_dev.argtypes) == len(lib.f3d_tsdf_integrate.argtypes) + 1
    assert len(lib.f3d_tsdf_extract_count_dev.argtypes) == len(lib.f3d_tsdf_extract_count.argtypes) + 1
    assert lib.f3d_tsdf_integrate.argtypes[9] is C.c_float and lib.f3d_tsdf_extract_count.argtypes[6] is C.c_float
    for name in ('reserve_tsdf', 'tsdf_integrate', 'tsdf_extract', 'tsdf_integrate_dev', 'tsdf_extract_count_dev', 'tsdf_extract_fill_dev'):
        assert callable(getattr(f3d.Context, name))


def test_scan_tile_constant_matches_the_header():
    import re
    from conftest import ROOT
    text = (ROOT / 'include' / 'f3d.h').read_text()
    assert int(re.search(r'#define F3D_TSDF_SCAN_TILE (\d+)', text).group(1)) == f3d.TSDF_SCAN_TILE
    assert f3d.TSDF_SCAN_TILE % 256 == 0                               # whole counts per thread of a 256-thread block


def test_public_surface():
    assert set(reconstruct.__all__) == {'TSDFVolume', 'reconstruct_mesh', 'depth_images'}
    for name in reconstruct.__all__:
        assert callable(getattr(reconstruct, name))
    from Fusion3DSeg.fusion import Fusion
    assert callable(Fusion.reconstruct_mesh)


def test_restatement_on_an_analytic_sphere():
    """tsdf = clamp((|c - centre| - r) / trunc), all weights 1, a sphere well inside a 24 x 20 x 18 volume: the surface is closed
    (every undirected edge in exactly two triangles), consistently wound (every directed edge once), a sphere topologically
    (V - E + F = 2), outward (positive signed volume), and within sqrt(3) voxels of the sphere: a vertex is a convex combination of
    points of a cell that holds a sign change, and a cell's diameter is sqrt(3) * vs."""
    dims, vs, lo = (24, 20, 18), 0.05, np.array([-0.6, -0.5, -0.45])
    centre, radius = np.array([0.013, -0.021, 0.007]), 0.31
    tsdf, weight = R.sphere_state(dims, lo, vs, centre, radius, 4 * vs)
    verts, tris = R.extract(tsdf, weight, lo, vs, 1.0)
    assert verts.dtype == np.float64 and tris.dtype == np.int32 and len(verts) > 100 and len(tris) > 200
    umax, umin, dmax, nedges = R.edge_stats(tris)
    assert (umax, umin) == (2, 2)
    assert dmax == 1
    assert len(verts) - nedges + len(tris) == 2
    assert R.signed_volume(verts, tris) > 0
    dist = np.abs(np.linalg.norm(verts - centre, axis=1) - radius)
    assert dist.max() <= np.sqrt(3.0) * vs
    assert tris.min() == 0 and tris.max() == len(verts) - 1


def test_restatement_integrates_the_scene():
    """The wall of the analytic scene, integrated from one camera: the voxels in front of it within trunc average towards
    (WALL_Z - z) / trunc, and nothing behind -trunc is touched."""
    K, q, t, depths = R.scene([(0.0, 0.0, 0.0)], [(0.0, 0.0, 1.0)], 40, 48)
    dims, vs, lo = (9, 7, 16), 0.05, np.array([0.4, -0.5, 1.1])         # the column x = 0.575, y = -0.425: its rays pass beside the sphere
    z0 = np.zeros(dims[::-1], np.float32)
    tsdf, weight = R.integrate(z0, z0, lo, vs, 0.2, 64, depths, K, q, t, 1.0, 10.0)
    zc = lo[2] + (np.arange(dims[2]) + 0.5) * vs
    seen = weight[:, 1, 3] > 0
    assert seen[zc < R.WALL_Z + 0.2 - vs].all() and not seen[zc > R.WALL_Z + 0.2 + vs].any()
    assert set(np.unique(weight)) <= {0.0, 1.0}
    want = np.clip((R.WALL_Z - zc) / 0.2, -1, 1)
    assert np.abs(tsdf[:, 1, 3][seen] - want[seen]).max() < 1e-6
    assert (z0 == 0).all()


def test_argument_errors_need_no_device():
    V = reconstruct.TSDFVolume
    for bad in [dict(dims=(0, 4, 4)), dict(dims=(4, 4)), dict(dims=(2048, 2048, 512)), dict(voxel=0.0), dict(voxel=float('nan')),
                dict(trunc=-1.0), dict(trunc=float('inf')), dict(max_weight=0.5), dict(max_weight=2.0 ** 24 + 2), dict(lo=(0.0, 1.0)),
                dict(lo=(0.0, float('nan'), 0.0))]:
        kw = dict(lo=(0.0, 0.0, 0.0), dims=(4, 4, 4), voxel=0.1)
        kw.update(bad)
        with pytest.raises(ValueError):
            V(**kw)
    vol = V((0.0, 0.0, 0.0), (4, 5, 6), 0.1)
    assert vol.trunc == pytest.approx(0.4) and vol.max_weight == 64.0
    assert vol.tsdf.shape == vol.weight.shape == (6, 5, 4) and vol.tsdf.dtype == np.float32 and not vol.tsdf.any() and not vol.weight.any()
    K, q, t = np.eye(3), np.array([[1.0, 0, 0, 0]]), np.zeros((1, 3))
    with pytest.raises(TypeError):
        vol.integrate(np.zeros((1, 4, 4), np.int32), K, q, t)
    with pytest.raises(ValueError):
        vol.integrate(np.zeros((4, 4)), K, q, t)
    with pytest.raises(ValueError):
        vol.integrate(np.zeros((1, 4, 4)), K, q, t, depth_scale=0.0)
    with pytest.raises(ValueError):
        vol.integrate(np.zeros((1, 4, 4)), K, q, t, max_depth=float('inf'))
    with pytest.raises(ValueError):
        vol.integrate(np.zeros((2, 4, 4)), K, q, t)                    # one pose for two frames
    with pytest.raises(ZeroDivisionError):
        vol.integrate(np.zeros((1, 4, 4)), K, np.zeros((1, 4)), t)
    with pytest.raises(ValueError):
        vol.extract_mesh(min_weight=0.5)
    with pytest.raises(ValueError):
        reconstruct.depth_images(np.zeros((2, 4, 4, 3)), q, t)
    assert vol.integrate(np.zeros((0, 4, 4)), K, np.zeros((0, 4)), np.zeros((0, 3))) is vol     # no frames: nothing to do, no device
