"""CPU-side checks of registration (TSDF raycast, point-to-plane ICP, frame tracking): the bindings exist, the public surface is
named, the NumPy restatement (tests/icp_ref.py) behaves on analytic scenes, and argument errors need no device."""
import ctypes as C
import re

import numpy as np
import pytest

import f3d
import icp_ref as I
import tsdf_ref as R
from Fusion3DSeg.segUtils import reconstruct, registration

PAIRS = [('f3d_tsdf_raycast', 'f3d_tsdf_raycast_dev'), ('f3d_icp_sums', 'f3d_icp_sums_dev'), ('f3d_icp', 'f3d_icp_dev')]


def test_symbols_are_bound():
    lib = f3d.library()
    for name in [n for pair in PAIRS for n in pair] + ['f3d_ctx_reserve_icp']:
        fn = getattr(lib, name)
        assert name in lib._f3d_symbols
        assert fn.restype is C.c_int and fn.argtypes and fn.argtypes[0] is C.c_void_p
    for host, dev in PAIRS:
        assert len(getattr(lib, dev).argtypes) == len(getattr(lib, host).argtypes) + 1
    assert lib.f3d_tsdf_raycast.argtypes[8] is C.c_float                # min_weight, as in extract
    for name in ('reserve_icp', 'tsdf_raycast', 'icp_sums', 'icp', 'tsdf_raycast_dev', 'icp_sums_dev', 'icp_dev'):
        assert callable(getattr(f3d.Context, name))


def test_constants_match_the_header():
    from conftest import ROOT
    text = (ROOT / 'include' / 'f3d.h').read_text()
    define = lambda name: re.search(rf'#define {name} (\S+)', text).group(1)         # noqa: E731
    assert int(define('F3D_ICP_CHUNK')) == f3d.ICP_CHUNK == I.CHUNK
    assert int(define('F3D_ICP_NSUMS')) == f3d.ICP_NSUMS == I.NSUMS == 21 + 6 + 2
    assert float(define('F3D_ICP_PIVOT_EPS')) == f3d.ICP_PIVOT_EPS == I.PIVOT_EPS
    assert (int(define('F3D_ICP_OK')), int(define('F3D_ICP_LOST'))) == (f3d.ICP_OK, f3d.ICP_LOST) == (I.OK, I.LOST)
    assert f3d.ICP_CHUNK % 64 == 0                                      # whole pixels per lane


def test_public_surface():
    assert registration.__all__ == ['raycast', 'icp_sums', 'icp', 'track_frames']
    for name in registration.__all__:
        assert callable(getattr(registration, name))
    for topic in ('pyramid', 'photometric', 'robust', 'loop closure', 're-unprojecting'):
        assert topic in registration.__doc__                             # what is out of scope is said


# ------------------------------------------------------------------------------------------------ raycast on the analytic sphere
SPHERE = dict(dims=(24, 20, 18), vs=0.05, lo=np.array([-0.6, -0.5, -0.45]), centre=np.array([0.013, -0.021, 0.007]), radius=0.31)


@pytest.fixture(scope='module')
def sphere_maps():
    s = SPHERE
    tsdf, weight = R.sphere_state(s['dims'], s['lo'], s['vs'], s['centre'], s['radius'], 0.2)
    h, w = 40, 48
    q, t = R.look_at((0.1, -0.05, -1.2), s['centre'])                  # outside the volume, which ends at z = -0.45
    vertex, normal, depth = I.raycast(tsdf, weight, s['lo'], s['vs'], 1.0, R.intrinsics(h, w), q, t, h, w, 0.0, s['vs'], int(np.floor(3.0 / s['vs'])) + 1)
    return vertex, normal, depth, q, t, h, w


def test_restated_raycast_on_an_analytic_sphere(sphere_maps):
    """More than 100 pixels hit; a hit is the zero of the trilinear field on the ray, which lies in a cell with a sign change, so it
    is within a cell's diameter sqrt(3) * vs of the sphere (the bound of test_restatement_on_an_analytic_sphere); normals point
    outwards; a ray that misses the sphere is NaN with depth 0; depth is the camera z of the vertex."""
    vertex, normal, depth, q, t, h, w = sphere_maps
    s = SPHERE
    hit = depth > 0
    assert hit.sum() > 100 and (~hit).sum() > 100
    off = vertex[hit] - s['centre']
    assert np.abs(np.linalg.norm(off, axis=1) - s['radius']).max() <= np.sqrt(3.0) * s['vs']
    radial = off / np.linalg.norm(off, axis=1)[:, None]
    assert ((normal[hit] * radial).sum(axis=1) > 0).all()
    assert np.abs(np.linalg.norm(normal[hit], axis=1) - 1.0).max() < 1e-15
    assert np.isnan(vertex[~hit]).all() and np.isnan(normal[~hit]).all() and (depth[~hit] == 0).all()
    cam = I.O.rotate(I.O.quat_inverse(q), vertex[hit] - t[None, :])
    assert np.abs(cam[:, 2] - depth[hit]).max() < 1e-12
    # the rays that miss are those whose pixel-centre ray passes the sphere at more than its radius
    K = R.intrinsics(h, w)
    vv, uu = np.meshgrid(np.arange(h) + 0.5, np.arange(w) + 0.5, indexing='ij')
    d = I.O.rotate(I.normalise(q), np.stack([(uu.reshape(-1) - K[0, 2]) / K[0, 0], (vv.reshape(-1) - K[1, 2]) / K[1, 1], np.ones(h * w)], axis=1))
    d /= np.linalg.norm(d, axis=1)[:, None]
    oc = s['centre'] - t
    closest = np.linalg.norm(oc[None, :] - (d @ oc)[:, None] * d, axis=1)
    assert not hit[closest > s['radius'] + np.sqrt(3.0) * s['vs']].any() and hit[closest < s['radius'] - np.sqrt(3.0) * s['vs']].all()


def test_restated_normals_on_the_sphere(sphere_maps):
    """The largest angle between a restated normal (central differences of the trilinear field over +-1 voxel) and the radial
    direction on this scene, measured here: 0.0054839 rad (0.314 degrees).  Twice that is asserted: the factor only guards against
    another host's libm; the arithmetic is exact-order."""
    vertex, normal, depth, *_ = sphere_maps
    hit = depth > 0
    off = vertex[hit] - SPHERE['centre']
    radial = off / np.linalg.norm(off, axis=1)[:, None]
    angle = np.arccos(np.clip((normal[hit] * radial).sum(axis=1), -1.0, 1.0)).max()
    print('largest normal angle', angle)
    assert angle <= 2 * 0.0054839


# ------------------------------------------------------------------------------------------------ ICP on the sphere-and-wall scene
@pytest.fixture(scope='module')
def scene():
    return I.icp_scene()


def run_icp(s, iterations=10, min_pairs=100, start=None):
    q0, t0 = start or (s['q0'], s['t0'])
    return I.icp(s['depths'][0], s['K'], q0, t0, 1.0, I.MAX_DEPTH, s['vertex'], s['normal'], I.H, I.W, s['K'], s['q'][0], s['t'][0], 0.1, iterations,
                 min_pairs)


def test_restated_icp_on_the_scene(scene):
    """Frame 0 against the maps ray-cast at its true pose, from a start 2 cm and 1 degree (oblique axis) off, 10 rounds.  Measured here:
        translation error          0.020000 m   -> 0.0048369 m    (shrinks 4.13 x)
        rotation error             0.017453 rad -> 0.064984 rad   (GROWS: 0.269 x)
        sphere centre as seen      0.023199 m   -> 0.0025202 m    (shrinks 9.21 x)
        wall normal as seen        0.015826 rad -> 0.00081422 rad (shrinks 19.4 x)
    The rotation error grows because the scene cannot hold it: a sphere in front of a wall maps onto itself under every rotation about the
    line through the sphere's centre along the wall's normal (nearly frame 0's optical axis), so depth alone does not see that angle.
    The eigenvalue of A along it (0.19 against 58 .. 1400 for the other five, at the true pose) is small but far above what
    F3D_ICP_PIVOT_EPS guards against, because the voxel grid breaks the symmetry slightly, and the rounds wander along it.  The five
    observable degrees of freedom (I.scene_error) converge.  Each error is held to half its measured factor: a factor above 1 for
    what the scene can hold, a bound on the wandering for the rotation."""
    s = scene
    pose, stats, status = run_icp(s)
    assert status == I.OK and (stats[:, 2] == I.OK).all()
    assert (stats[:, 0] > 100).all() and stats[-1, 1] <= stats[0, 1]
    qt, tt = s['q'][0], s['t'][0]
    before = (np.linalg.norm(s['t0'] - tt), I.rotation_angle(s['q0'], qt)) + I.scene_error(s['q0'], s['t0'], qt, tt)
    after = (np.linalg.norm(pose[4:] - tt), I.rotation_angle(pose[:4], qt)) + I.scene_error(pose[:4], pose[4:], qt, tt)
    print('before', before, 'after', after, 'counts', stats[:, 0], 'sum r2', stats[:, 1])
    assert before[0] == pytest.approx(0.02) and before[1] == pytest.approx(np.radians(1.0))
    for b, a, factor in zip(before, after, (4.13, 0.269, 9.21, 19.4)):
        assert b / a >= factor / 2
    assert after[2] < before[2] and after[3] < before[3]
    assert np.abs(np.linalg.norm(pose[:4]) - 1.0) < 1e-15


def plane_case(h=12, w=16):
    """Hand-made maps of the plane z = 1.5 with normals exactly (0, 0, -1), seen from the origin, and a flat depth frame at 1.5."""
    K = R.intrinsics(h, w)
    vv, uu = np.meshgrid(np.arange(h) + 0.5, np.arange(w) + 0.5, indexing='ij')
    vertex = np.stack([(uu - K[0, 2]) * (1.5 / K[0, 0]), (vv - K[1, 2]) * (1.5 / K[1, 1]), np.full((h, w), 1.5)], axis=-1)
    normal = np.broadcast_to(np.array([0.0, 0.0, -1.0]), (h, w, 3)).copy()
    return K, np.full((h, w), 1.5), vertex, normal


def test_restated_icp_is_lost_on_a_degenerate_model():
    """A plane with normals exactly (0, 0, -1): the v_x and v_y columns of J are exactly zero (and so is the omega_z one, pr x N having
    no z component), a pivot is 0 and round 0 reports LOST; the start pose comes back unchanged, un-normalised as it was given."""
    K, depth, vertex, normal = plane_case()
    q0, t0 = np.array([2.0, 0.0, 0.0, 0.0]), np.array([0.001, -0.002, 0.003])
    ident, zero = np.array([1.0, 0.0, 0.0, 0.0]), np.zeros(3)
    tot = I.icp_sums(depth, K, q0, t0, 1.0, 10.0, vertex, normal, 12, 16, K, ident, zero, 0.1)
    assert tot[28] > 100 and tot[15] == 0 and tot[18] == 0 and tot[11] == 0     # J3 J3, J4 J4, J2 J2
    pose, stats, status = I.icp(depth, K, q0, t0, 1.0, 10.0, vertex, normal, 12, 16, K, ident, zero, 0.1, 3, 100)
    assert status == I.LOST
    assert np.array_equal(pose, np.concatenate([q0, t0]))
    assert stats[0, 0] == tot[28] and stats[0, 1] == tot[27] and stats[0, 2] == I.LOST
    assert np.array_equal(stats[1:], [[0.0, 0.0, 1.0]] * 2)


def test_restated_icp_is_lost_with_too_few_pairs(scene):
    s = scene
    pose, stats, status = run_icp(s, iterations=2, min_pairs=I.H * I.W + 1)
    assert status == I.LOST and np.array_equal(pose, np.concatenate([s['q0'], s['t0']]))
    assert 100 < stats[0, 0] <= I.H * I.W and stats[0, 2] == I.LOST and np.array_equal(stats[1], [0.0, 0.0, 1.0])


def test_restated_tracking_beats_the_priors(scene):
    """Six frames whose poses are each 1 - 2 cm and 0.3 - 0.9 degrees off, tracked into an empty volume.  Mean error of frames 1 .. 5
    against the true poses, as the scene can hold it (I.scene_error, in the frame that frame 0's prior gives the model), measured here:
        sphere centre as seen   0.015811 m   -> 0.010842 m
        wall normal as seen     0.010769 rad -> 0.00087455 rad
    The plain camera-centre distance to the true poses goes from 0.013149 m to 0.042739 m: that is the unobservable rotation about the
    scene's symmetry axis moving the cameras along their circles around it, plus frame 0's own 1 cm, which no later frame can undo."""
    s = scene
    pq, pt = I.tracking_priors(s['q'], s['t'])
    shifts = np.linalg.norm(pt - s['t'], axis=1)
    assert (shifts >= 0.01).all() and (shifts <= 0.02).all()
    assert all(0 < I.rotation_angle(pq[f], s['q'][f]) < np.radians(1.0) for f in range(6))
    z = np.zeros(I.DIMS[::-1], np.float32)
    q, t, status, tsdf, weight = I.track_frames(z, z, I.LO, I.VS, I.TRUNC, 64, s['depths'], s['K'], pq, pt, 1.0, I.MAX_DEPTH)
    assert (status == I.OK).all() and np.array_equal(q[0], pq[0]) and np.array_equal(t[0], pt[0])
    prior, refined = I.tracking_errors(pq, pt, pq, pt, s['q'], s['t']), I.tracking_errors(pq, pt, q, t, s['q'], s['t'])
    print('prior', prior, 'refined', refined, 'plain', shifts.mean(), np.linalg.norm(t - s['t'], axis=1).mean())
    assert refined[0] < prior[0] and refined[1] < prior[1]
    assert weight.max() >= 3 and not z.any()


# ------------------------------------------------------------------------------------------------ argument errors
def test_argument_errors_need_no_device():
    vol = reconstruct.TSDFVolume((0.0, 0.0, 0.0), (4, 5, 6), 0.1)
    K, q, t = np.eye(3), np.array([1.0, 0, 0, 0]), np.zeros(3)
    ray = lambda **kw: registration.raycast(vol, **{**dict(K=K, wxyz=q, t=t, hw=(4, 4)), **kw})            # noqa: E731
    for bad in [dict(hw=(0, 4)), dict(hw=(1 << 16, 1 << 16)), dict(min_weight=0.5), dict(near=-1.0), dict(far=float('inf')), dict(near=2.0, far=1.0),
                dict(step=0.0), dict(step=float('nan')), dict(K=np.eye(4)), dict(K=np.full((3, 3), np.nan)), dict(t=[0.0, float('inf'), 0.0]),
                dict(wxyz=[1.0, 0, 0]), dict(wxyz=[float('nan'), 0, 0, 0])]:
        with pytest.raises(ValueError):
            ray(**bad)
    with pytest.raises(ZeroDivisionError):
        ray(wxyz=np.zeros(4))
    maps = np.zeros((4, 4, 3))
    base = dict(depth=np.zeros((4, 4)), K=K, wxyz=q, t=t, model_vertex=maps, model_normal=maps, model_K=K, model_wxyz=q, model_t=t)
    for fn in (registration.icp_sums, registration.icp):
        for bad in [dict(depth=np.zeros((1, 4, 4))), dict(depth=np.zeros((0, 4))), dict(model_vertex=np.zeros((4, 4))), dict(model_normal=np.zeros((4, 5, 3))),
                    dict(max_dist=0.0), dict(max_dist=float('nan')), dict(depth_scale=-1.0), dict(max_depth=float('inf')), dict(model_K=np.eye(2)),
                    dict(t=[0.0, 0.0])]:
            with pytest.raises(ValueError):
                fn(**{**base, **bad})
        with pytest.raises(TypeError):
            fn(**{**base, 'depth': np.zeros((4, 4), np.int32)})
        with pytest.raises(ZeroDivisionError):
            fn(**{**base, 'model_wxyz': np.zeros(4)})
    for bad in [dict(iterations=0), dict(min_pairs=5)]:
        with pytest.raises(ValueError):
            registration.icp(**{**base, **bad})
    track = lambda **kw: registration.track_frames(vol, **{**dict(depths=np.zeros((2, 4, 4)), K=K, wxyzs=[q, q], translations=[t, t]), **kw})   # noqa: E731
    for bad in [dict(depths=np.zeros((4, 4))), dict(wxyzs=[q]), dict(translations=[t]), dict(max_dist=0.0), dict(iterations=0), dict(min_pairs=2),
                dict(min_weight=0.0), dict(depth_scale=0.0), dict(max_depth=float('nan'))]:
        with pytest.raises(ValueError):
            track(**bad)
    with pytest.raises(TypeError):
        track(depths=np.zeros((2, 4, 4), np.int64))
    q_out, t_out, status = track(depths=np.zeros((0, 4, 4)), wxyzs=np.zeros((0, 4)), translations=np.zeros((0, 3)))     # no frames: no device
    assert q_out.shape == (0, 4) and t_out.shape == (0, 3) and status.shape == (0,) and status.dtype == np.int32


# ------------------------------------------------------------------------------------------------ the scenes of test_raycast_range_gpu.py
# Each case of the sample-range tests must reach the path it is meant for.  That is shown here on the restatement alone: the rays of
# the header (I.ray_rays), the validity of every sample (I.first_valid, from I.sample) and the restated maps.
@pytest.fixture(scope='module')
def ray_scene():
    """(cases, name -> (first valid sample, hit mask, index of the sample before each hit))."""
    cases, states, seen = I.ray_cases(), {}, {}

    def look(name):
        if name not in seen:
            case = cases[name]
            state = states.setdefault(case['vs'], I.ray_volume(case['vs'])[:2])
            depth = I.ray_case_maps(case, state)[2]
            hit = depth > 0
            before = np.where(hit, np.floor((depth - case['near']) / case['step']), -1).astype(np.int64)
            seen[name] = (I.first_valid(case, state), hit, before, state)
        return seen[name]
    return cases, look


def near_first(fv, hit, before):
    """hits whose last sample in front of the surface is the ray's first valid sample or the one after it"""
    return int((hit & (before - fv <= 1)).sum())


@pytest.mark.parametrize('name', ['axis' + a for a in I.AXIS_CAMERAS] + ['fine-voxels'])
def test_axis_cameras_have_rays_along_the_faces(ray_scene, name):
    cases, look = ray_scene
    fv, hit, before, _ = look(name)
    zeros = int((I.ray_rays(cases[name]) == 0).sum())
    print(f'{name}: {zeros} direction components exactly 0, {int(hit.sum())} hits, {int((fv < 0).sum())} rays without a valid sample, '
          f'{near_first(fv, hit, before)} hits within one step of the first valid sample')
    assert zeros >= I.RAY_H + I.RAY_W
    assert hit.sum() >= 5 and (fv < 0).sum() >= 5 and near_first(fv, hit, before) >= 5


@pytest.mark.parametrize('c', range(8))
def test_corner_cameras_enter_through_edges_and_corners(ray_scene, c):
    """Among the first valid samples of the rays there are cells on an edge of the volume (two indices at an end of their range)."""
    cases, look = ray_scene
    case = cases[f'corner{c}']
    fv, hit, before, _ = look(f'corner{c}')
    P = case['t'][None, :] + (case['near'] + fv[fv >= 0].astype(np.float64) * case['step'])[:, None] * I.ray_rays(case)[fv >= 0]
    cell = np.floor((P - case['lo'][None, :]) / case['vs'] - 0.5)
    at_end = (cell == 0) | (cell == np.array(I.RAY_DIMS)[None, :] - 2)
    print(f'corner{c}: {int(hit.sum())} hits, {int((fv < 0).sum())} rays without a valid sample, {near_first(fv, hit, before)} hits within one step '
          f'of the first valid sample, {int((at_end.sum(axis=1) >= 2).sum())} rays enter through an edge cell')
    assert hit.sum() >= 5 and (fv < 0).sum() >= 5 and (at_end.sum(axis=1) >= 2).sum() >= 3


def test_rays_beside_the_volume(ray_scene):
    """`beside`: the centre column has dw_x == 0 and starts three voxels outside the volume; it is NaN, columns right of it hit.
    `just-outside`: the centre row has dw_y == 0 and starts inside the volume, a quarter voxel past the last valid position: only the
    index rule of F(P) rejects its samples.  `beside-high` and `just-outside-low` are the same on the opposite faces."""
    cases, look = ray_scene
    shape = (I.RAY_H, I.RAY_W)
    case = cases['beside']
    fv, hit, _, _ = look('beside')
    beside_hits = int(hit.sum())
    dw = I.ray_rays(case).reshape(shape + (3,))
    assert (dw[:, I.RAY_W // 2, 0] == 0).all() and case['t'][0] < I.RAY_LO[0] - 2.5 * case['vs']
    assert (fv.reshape(shape)[:, :I.RAY_W // 2 + 1] < 0).all() and not hit.reshape(shape)[:, :I.RAY_W // 2 + 1].any()
    assert hit.reshape(shape)[:, I.RAY_W // 2 + 1:].sum() >= 5
    case = cases['just-outside']
    fv, hit, _, _ = look('just-outside')
    dw = I.ray_rays(case).reshape(shape + (3,))
    top = I.RAY_LO[1] + (I.RAY_DIMS[1] - 0.5) * case['vs']
    assert (dw[I.RAY_H // 2, :, 1] == 0).all() and top < case['t'][1] < top + 0.5 * case['vs']
    assert (fv.reshape(shape)[I.RAY_H // 2:] < 0).all() and (fv.reshape(shape)[:I.RAY_H // 2] >= 0).any()
    print(f'beside: {beside_hits} hits; just-outside: {int(hit.sum())} hits, {int((fv >= 0).sum())} rays with a valid sample')
    assert hit.reshape(shape)[:I.RAY_H // 2].sum() >= 5
    # the mirrored pair: beyond the +x face, and below the first valid position on y
    case, mid = cases['beside-high'], I.RAY_W // 2
    fv, hit, _, _ = look('beside-high')
    high_hits = int(hit.sum())
    assert (I.ray_rays(case).reshape(shape + (3,))[:, mid, 0] == 0).all()
    assert case['t'][0] > I.RAY_LO[0] + (I.RAY_DIMS[0] + 2.5) * case['vs']
    assert (fv.reshape(shape)[:, mid:] < 0).all() and not hit.reshape(shape)[:, mid:].any() and hit.reshape(shape)[:, :mid].sum() >= 5
    case, mid = cases['just-outside-low'], I.RAY_H // 2
    fv, hit, _, _ = look('just-outside-low')
    bottom = I.RAY_LO[1] + 0.5 * case['vs']
    assert (I.ray_rays(case).reshape(shape + (3,))[mid, :, 1] == 0).all() and bottom - 0.5 * case['vs'] < case['t'][1] < bottom
    assert (fv.reshape(shape)[:mid + 1] < 0).all() and hit.reshape(shape)[mid + 1:].sum() >= 5
    print(f'beside-high: {high_hits} hits; just-outside-low: {int(hit.sum())} hits, {int((fv >= 0).sum())} rays with a valid sample')


def test_range_clips(ray_scene):
    cases, look = ray_scene
    for name in ('coarse-steps', 'fine-steps', 'near-inside', 'distant', 'distant-shifted', 'shifted'):
        fv, hit, before, _ = look(name)
        print(f'{name}: {int(hit.sum())} hits, {near_first(fv, hit, before)} within one step of the first valid sample')
        assert hit.sum() >= 5
    case = cases['near-inside']
    start = case['t'] + case['near'] * I.ray_rays(case)[(I.RAY_H // 2) * I.RAY_W + I.RAY_W // 2]
    assert np.all((start > I.RAY_LO) & (start < I.RAY_LO + np.array(I.RAY_DIMS) * case['vs']))
    assert (look('near-inside')[0] == 0).sum() >= 5                     # first samples that are valid
    for name in ('near-beyond', 'ends-before'):
        fv, hit, _, _ = look(name)
        assert (fv < 0).all() and not hit.any()
    fv, hit, _, state = look('ends-inside')
    later = I.ray_case_maps(cases['ends-inside'], state, nsteps=81)[2] > 0
    print(f'ends-inside: {int(hit.sum())} hits, {int((later & ~hit).sum())} more on later samples')
    assert hit.sum() >= 5 and (later & ~hit).sum() >= 5 and not (hit & ~later).any()
    assert abs(np.linalg.norm(cases['distant']['t'] - I.ray_volume()[4]) - 60.0) < 1e-9 and cases['distant']['near'] == 58.0
