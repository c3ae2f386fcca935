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


# ------------------------------------------------------------------------------------------------ the scenes of test_tsdf_cull_gpu.py
# Each scene of the cull tests must reach the path it is meant for.  That is shown here on the restatement alone, from the per-voxel
# quantities of the contract (R.frame_terms): h0, h1, h2, px, py, d, sdf.  An x-run is the nx voxels of one (y, z) row.
def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def ring_states(F):
    """-> run(frames, max_weight): the state after integrating that selection of the ring's F frames into an empty volume."""
    g = R.RING
    K, q, t, depths = R.ring_scene(F)
    z = np.zeros(g['dims'][::-1], np.float32)
    return lambda sel, max_weight=64: R.integrate(z, z, g['lo'], g['vs'], g['trunc'], max_weight, depths[sel], K, q[sel], t[sel], 1.0, g['max_depth'])


@pytest.mark.parametrize('F', [128, 130])
def test_ring_scene_needs_every_frame_in_order(F):
    """More than 64 frames in one call: the default max_weight saturates, the order of the frames shows in at least 100 voxels, the
    frames beyond the first 64 change the state, and some voxel is seen by no frame."""
    run = ring_states(F)
    every = slice(0, F)
    tsdf, weight = run(every)
    assert weight.max() == 64 and run(every, 1e6)[1].max() > 64
    order = int((bits(tsdf) != bits(run(slice(None, None, -1))[0])).sum())
    first = run(slice(0, 64))
    beyond = int(((bits(tsdf) != bits(first[0])) | (bits(weight) != bits(first[1]))).sum())
    unseen = int((weight == 0).sum())
    print(f'ring F = {F}: order-sensitive voxels {order}, voxels the frames beyond 64 change {beyond}, unseen voxels {unseen} of {weight.size}')
    assert order >= 100 and beyond > 0 and 0 < unseen < weight.size


@pytest.mark.parametrize('F', [63, 64, 65])
def test_ring_scene_at_the_batch_edge(F):
    """Around one batch of 64 frames: the last frame changes the state, so a batch that drops it cannot pass."""
    run = ring_states(F)
    full, short = run(slice(0, F)), run(slice(0, F - 1))
    assert (bits(full[0]) != bits(short[0])).any() and (full[1] == 0).any()


def test_ring_scene_away_from_the_origin():
    """Shifted by (1000, -2000, 500) the 65 frames still reach the volume: the subtraction c - t brings every voxel back to the
    camera, up to the rounding of coordinates of that size."""
    g = R.RING
    K, q, t, depths = R.ring_scene(65)
    z = np.zeros(g['dims'][::-1], np.float32)
    here = R.integrate(z, z, g['lo'], g['vs'], g['trunc'], 64, depths, K, q, t, 1.0, g['max_depth'])
    there = R.integrate(z, z, g['lo'] + R.FAR_SHIFT, g['vs'], g['trunc'], 64, depths, K, q, t + R.FAR_SHIFT, 1.0, g['max_depth'])
    assert there[1].max() >= 10 and (there[1] == 0).any()
    assert (there[1] == here[1]).mean() > 0.9
    c = R.voxel_centres(g['lo'] + R.FAR_SHIFT, g['dims'], g['vs']) - (t[0] + R.FAR_SHIFT)[None, :]
    assert not np.array_equal(c, R.voxel_centres(g['lo'], g['dims'], g['vs']) - t[0][None, :])      # the coordinates did round


def bound_terms(rule):
    g = R.BOUNDS
    K, q, t, depth, max_depth = R.bound_scene(rule)
    terms = R.frame_terms(K, q, t, g['lo'], g['dims'], g['vs'], depth)
    z = np.zeros(g['dims'][::-1], np.float32)
    weight = R.integrate(z, z, g['lo'], g['vs'], g['trunc'], 64, depth[None], K, q[None], t[None], 1.0, max_depth)[1]
    live = R.applied(terms, max_depth, g['trunc'])
    assert np.array_equal(weight.reshape(live.shape) > 0, live)         # frame_terms says what integrate does
    return terms, R.failed_rules(terms, g['h'], g['w'], max_depth, g['trunc']), live, max_depth


@pytest.mark.parametrize('rule', list(R.BOUND_CAMERAS))
def test_each_bound_has_a_camera(rule):
    """At least 20 x-runs whose every voxel fails this rule and no other, at least 10 that hold voxels on both sides of it, and voxels
    the frame changes."""
    terms, fails, live, max_depth = bound_terms(rule)
    whole, straddling = R.run_counts(fails, rule)
    print(f'{rule}: {whole} runs fail it whole and nothing else, {straddling} straddle it, {int(live.sum())} voxels integrated')
    assert whole >= 20 and straddling >= 10 and live.sum() >= 500
    if rule == 'far':
        at_max = int((live & (terms['d'] == max_depth)).sum())
        print(f'far: {at_max} voxels integrated with d == max_depth, {int((live & (terms["d"] < max_depth)).sum())} with less')
        assert at_max >= 100 and (live & (terms['d'] < max_depth)).sum() >= 100
        assert (terms['d'] > max_depth).any()
    if rule == 'behind':
        g = R.BOUNDS
        eye = np.array(R.BOUND_CAMERAS[rule]['eye'])
        assert np.all((eye > g['lo']) & (eye < g['lo'] + np.array(g['dims']) * g['vs']))      # inside the volume
        front = terms['h2'] > 0
        crossing = front.any(axis=1) & ~front.all(axis=1)
        alive = int((crossing & (live & front).any(axis=1)).sum())
        print(f'behind: {int(crossing.sum())} of {len(front)} runs cross the camera plane, {alive} of them with integrated voxels in front')
        assert alive > len(front) // 2                                  # most runs cross the plane with live voxels in front


def tie_terms(volume):
    g, vol = R.TIES, R.TIE_VOLUMES[volume]
    depth = np.full((g['h'], g['w']), g['max_depth'])
    terms = R.frame_terms(g['K'], g['wxyz'], g['t'], vol['lo'], vol['dims'], g['vs'], depth)
    z = np.zeros(vol['dims'][::-1], np.float32)
    tsdf, weight = R.integrate(z, z, vol['lo'], g['vs'], g['trunc'], 64, depth[None], g['K'], g['wxyz'][None], g['t'][None], 1.0, g['max_depth'])
    return terms, tsdf.reshape(terms['h2'].shape), weight.reshape(terms['h2'].shape)


def test_tie_scene_sits_on_the_bounds():
    """Exact float equality on every bound: px == 0 and py == 0 (integrated), px == w (rejected), sdf == -trunc (integrated, with
    value -1), h2 == max_depth + trunc along whole runs, ends included (integrated)."""
    g = R.TIES
    c = R.voxel_centres(R.TIE_VOLUMES['wide']['lo'], R.TIE_VOLUMES['wide']['dims'], g['vs'])
    assert np.array_equal(R.O.rotate(R.O.quat_inverse(g['wxyz']), c), c)      # the identity pose moves no bit
    terms, tsdf, weight = tie_terms('wide')
    px, py, h2, sdf = terms['px'], terms['py'], terms['h2'], terms['sdf']
    with np.errstate(invalid='ignore'):
        in_y, in_x, near = (py >= 0) & (py < g['h']), (px >= 0) & (px < g['w']), h2 <= g['max_depth'] + g['trunc']
    left, top, right = (px == 0.0) & in_y & near, (py == 0.0) & in_x & near, (px == g['w']) & in_y & near
    on_trunc = sdf == -g['trunc']
    on_far = h2 == g['max_depth'] + g['trunc']
    print(f'ties: px == 0: {int(left.sum())}, py == 0: {int(top.sum())}, px == w: {int(right.sum())}, sdf == -trunc: {int(on_trunc.sum())}, '
          f'h2 == max_depth + trunc: {int(on_far.sum())} voxels in {int(on_far.all(axis=1).sum())} whole runs')
    assert left.sum() >= 5 and top.sum() >= 5 and right.sum() >= 5 and on_trunc.sum() >= 5 and on_far.sum() >= 5
    assert (weight[left] == 1).all() and (weight[top] == 1).all() and (weight[right] == 0).all()
    assert (weight[on_trunc] == 1).all() and (tsdf[on_trunc] == -1.0).all()
    runs = on_far.any(axis=1)
    assert np.array_equal(runs, on_far.all(axis=1))                     # h2 is constant along a run: its ends are on the bound too
    assert (weight[runs] == 1).any(axis=1).all()                        # and no such run may be skipped
    assert (weight[h2 > g['max_depth'] + g['trunc']] == 0).all() and (h2 > g['max_depth'] + g['trunc']).any()
    # py == 0 along whole runs: both ends of the run sit on the upper bound
    assert ((py == 0.0).all(axis=1) & (weight == 1).any(axis=1)).sum() >= 5
    # the narrow volume ends its first layer's runs on the left bound: px == 0 at the last voxel, everything before it outside
    terms, tsdf, weight = tie_terms('left-end')
    with np.errstate(invalid='ignore'):
        ends = (terms['px'][:, -1] == 0.0) & (terms['px'][:, :-1] < 0).all(axis=1) & (terms['py'][:, -1] >= 0)
    print(f'ties: {int(ends.sum())} runs end on px == 0')
    assert ends.sum() >= 5 and (weight[ends, -1] == 1).all() and (weight[ends, :-1] == 0).all()


def test_general_K_is_within_the_contract():
    """f3d_project_h reads all nine entries of K and views_build bounds each row by its 1-norm, so a K with skew and unequal focal
    lengths is admitted; the scene that uses one still has runs on both sides of the image."""
    g = R.RING
    K, q, t, depths = R.ring_scene(65)
    views = f3d.views_build(R.SKEW_K, g['w'], g['h'], q, t, g['max_depth'])
    fields = f3d.view_fields(views)
    assert np.array_equal(fields['K'][0], R.SKEW_K) and R.SKEW_K[0, 1] != 0 and R.SKEW_K[0, 0] != R.SKEW_K[1, 1]
    assert (fields['mnorm'][0] >= np.abs(R.SKEW_K).sum(axis=1)).all()
    z = np.zeros(g['dims'][::-1], np.float32)
    weight = R.integrate(z, z, g['lo'], g['vs'], g['trunc'], 64, depths, R.SKEW_K, q, t, 1.0, g['max_depth'])[1]
    assert weight.max() >= 10 and (weight == 0).any()
