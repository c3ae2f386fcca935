"""CPU-side checks of colour in registration (colour raycast, the photometric ICP term, colour tracking): the bindings exist, argument
errors need no device, and the NumPy restatement (tests/icp_color_ref.py) does what the feature is for on the textured sphere-and-wall
scene."""
import ctypes as C
import re

import numpy as np
import pytest

import f3d
import icp_color_ref as CR
import icp_ref as I
import tsdf_ref as R
from Fusion3DSeg.segUtils import reconstruct, registration

PAIRS = [('f3d_tsdf_raycast_color', 'f3d_tsdf_raycast_color_dev'), ('f3d_icp_color_sums', 'f3d_icp_color_sums_dev'),
         ('f3d_icp_color', 'f3d_icp_color_dev')]
COLOR_WEIGHT = 0.1                                                       # chosen in test_colour_holds_the_rotation_depth_cannot_see


# ------------------------------------------------------------------------------------------------ bindings
def test_symbols_are_bound():
    lib = f3d.library()
    for name in [n for pair in PAIRS for n in pair] + ['f3d_ctx_reserve_icp_color']:
        fn = getattr(lib, name)
        assert name in lib._f3d_symbols
        assert fn.restype is C.c_int and fn.argtypes and fn.argtypes[0] is C.c_void_p
    for host, dev in PAIRS:
        assert len(getattr(lib, dev).argtypes) == len(getattr(lib, host).argtypes) + 1
    # the plain entry's arguments with the colour state after the weights / the three colour arguments after max_dist
    plain, color = list(lib.f3d_tsdf_raycast.argtypes), list(lib.f3d_tsdf_raycast_color.argtypes)
    assert color == plain[:3] + [C.c_void_p] + plain[3:] + [C.c_void_p, C.c_void_p]
    for a, b in (('f3d_icp_sums', 'f3d_icp_color_sums'), ('f3d_icp', 'f3d_icp_color')):
        plain, color = list(getattr(lib, a).argtypes), list(getattr(lib, b).argtypes)
        assert color == plain[:16] + [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double] + plain[16:]
    for name in ('reserve_icp_color', 'tsdf_raycast_color', 'icp_color_sums', 'icp_color', 'tsdf_raycast_color_dev', 'icp_color_sums_dev',
                 'icp_color_dev'):
        assert callable(getattr(f3d.Context, name))


def test_constants_match_the_header():
    from conftest import ROOT
    text = (ROOT / 'include' / 'f3d.h').read_text()
    define = lambda name: re.search(rf'#define {name} (\S+)', text).group(1)         # noqa: E731
    assert int(define('F3D_ICP_NSUMS_COLOR')) == f3d.ICP_NSUMS_COLOR == CR.NSUMS == 2 * f3d.ICP_NSUMS
    for name in [n for pair in PAIRS for n in pair] + ['f3d_ctx_reserve_icp_color']:
        assert re.search(rf'\bint {name}\(f3d_ctx\* ctx', text)


def test_public_surface():
    import inspect
    assert registration.__all__ == ['raycast', 'icp_sums', 'icp', 'track_frames']
    assert inspect.signature(registration.raycast).parameters['colors'].default is False
    for fn in (registration.icp_sums, registration.icp):
        p = inspect.signature(fn).parameters
        assert all(p[k].default is None and p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ('color', 'model_intensity', 'color_weight'))
    assert inspect.signature(registration.track_frames).parameters['color_weight'].default is None
    for topic in ('robust weights', 'intensity-difference gate', 'pyramids', 'exposure compensation', 'anything but the volume'):
        assert topic in registration.__doc__                             # what is out of scope is said


def test_argument_errors_need_no_device():
    """A Context that was never opened has no library handle and no device: a call that got past the array checks would fail with
    AttributeError.  Every bad array is refused with TypeError / ValueError before that; so are the module's colour arguments."""
    ctx = object.__new__(f3d.Context)
    K, q, t = np.eye(3), np.array([1.0, 0, 0, 0]), np.zeros(3)
    maps, view = np.zeros((12, 3)), np.zeros(f3d.VIEW_DOUBLES)
    good = dict(depth=np.ones((4, 4)), model_intensity=np.zeros(12), rgb=np.zeros((5, 7, 3), np.uint8), color_weight=0.5)

    def call(fn, **kw):
        a = {**good, **kw}
        return fn(a['depth'], K, q, t, maps, maps, 3, 4, view, 0.1, a['model_intensity'], a['rgb'], a['color_weight'])

    for fn in (ctx.icp_color_sums, ctx.icp_color):
        for bad in [dict(model_intensity=np.zeros(11)), dict(model_intensity=np.zeros((3, 5))), dict(rgb=np.zeros((5, 7), np.uint8)),
                    dict(rgb=np.zeros((5, 7, 4), np.uint8)), dict(rgb=np.zeros((0, 7, 3), np.uint8)), dict(rgb=np.zeros((2, 5, 7, 3), np.uint8)),
                    dict(color_weight=-1.0), dict(color_weight=float('nan')), dict(color_weight=float('inf')), dict(depth=np.ones((1, 4, 4)))]:
            with pytest.raises(ValueError):
                call(fn, **bad)
        for bad in [dict(model_intensity=np.zeros(12, np.float32)), dict(rgb=np.zeros((5, 7, 3), np.float32)), dict(depth=np.ones((4, 4), np.int32))]:
            with pytest.raises(TypeError):
                call(fn, **bad)
        with pytest.raises(AttributeError):                              # the good arguments get as far as the library
            call(fn)
    shape = (6, 5, 4)
    tsdf, weight, color = np.zeros(shape, np.float32), np.zeros(shape, np.float32), np.zeros(shape + (4,), np.float32)
    ray = lambda **kw: ctx.tsdf_raycast_color(*[kw.get(k, v) for k, v in (('tsdf', tsdf), ('weight', weight), ('color', color))], np.zeros(3), 0.1, 1.0, K,  # noqa: E731
                                              q, t, kw.get('h', 4), 4, 0.0, 0.1, 10)
    for bad in [dict(color=np.zeros(shape + (3,), np.float32)), dict(color=np.zeros((6, 5, 5, 4), np.float32)), dict(h=0),
                dict(color=np.zeros(shape[::-1] + (4,), np.float32).transpose(2, 1, 0, 3))]:
        with pytest.raises(ValueError):
            ray(**bad)
    with pytest.raises(TypeError):
        ray(color=np.zeros(shape + (4,)))
    with pytest.raises(AttributeError):
        ray()
    # the module: a volume without colour, some of the three colour arguments, a weight without images
    vol = reconstruct.TSDFVolume((0.0, 0.0, 0.0), (4, 5, 6), 0.1)
    with pytest.raises(ValueError):
        registration.raycast(vol, K, q, t, (4, 4), colors=True)
    m3 = np.zeros((4, 4, 3))
    base = dict(depth=np.zeros((4, 4)), K=K, wxyz=q, t=t, model_vertex=m3, model_normal=m3, model_K=K, model_wxyz=q, model_t=t)
    three = dict(color=np.zeros((4, 4, 3), np.uint8), model_intensity=np.zeros((4, 4)), color_weight=1.0)
    for fn in (registration.icp_sums, registration.icp):
        for drop in three:
            with pytest.raises(ValueError):
                fn(**base, **{k: v for k, v in three.items() if k != drop})
        for bad in [dict(model_intensity=np.zeros((4, 5))), dict(model_intensity=np.zeros(16)), dict(color=np.zeros((4, 4), np.uint8)),
                    dict(color_weight=-0.5), dict(color_weight=float('nan'))]:
            with pytest.raises(ValueError):
                fn(**base, **{**three, **bad})
        with pytest.raises(TypeError):
            fn(**base, **{**three, 'color': np.zeros((4, 4, 3))})
        with pytest.raises(TypeError):
            fn(**base, **{**three, 'model_intensity': np.zeros((4, 4), np.float32)})
    cvol = reconstruct.TSDFVolume((0.0, 0.0, 0.0), (4, 5, 6), 0.1, color=True)
    track = lambda v, **kw: registration.track_frames(v, np.zeros((2, 4, 4)), K, [q, q], [t, t], **kw)          # noqa: E731
    rgbs = np.zeros((2, 4, 4, 3), np.uint8)
    for v, kw in [(cvol, dict(color_weight=1.0)), (vol, dict(colors=rgbs, color_weight=1.0)), (cvol, dict(colors=rgbs, color_weight=-1.0)),
                  (cvol, dict(colors=rgbs, color_weight=float('inf'))), (cvol, dict(colors=rgbs[:1], color_weight=1.0))]:
        with pytest.raises(ValueError):
            track(v, **kw)


# ------------------------------------------------------------------------------------------------ the restated raycast
@pytest.fixture(scope='module')
def scene():
    s = CR.color_scene()
    for a in s.values():
        a.setflags(write=False)
    return s


def nsteps():
    return int(np.floor(I.MAX_DEPTH / I.VS)) + 1


def test_a_constant_colour_ray_casts_to_itself(scene):
    s = scene
    color = np.zeros(I.DIMS[::-1] + (4,), np.float32)
    color[...] = (200.0, 30.0, 90.0, 1.0)
    vertex, normal, depth, rgb, inten = CR.raycast_color(s['tsdf'], s['weight'], color, I.LO, I.VS, 1.0, s['K'], s['q'][0], s['t'][0], I.H, I.W, 0.0, I.VS,
                                                         nsteps())
    hit = depth > 0
    assert hit.sum() > 1000 and (~hit).any()
    assert (rgb[hit] == [200.0, 30.0, 90.0]).all() and np.isnan(rgb[~hit]).all()       # c0 + f * (c1 - c0) with c1 == c0 is c0 exactly
    assert (inten[hit] == ((0.299 * 200.0 + 0.587 * 30.0) + 0.114 * 90.0) / 255.0).all() and np.isnan(inten[~hit]).all()
    for got, want in zip((vertex, normal, depth), I.raycast(s['tsdf'], s['weight'], I.LO, I.VS, 1.0, s['K'], s['q'][0], s['t'][0], I.H, I.W, 0.0, I.VS,
                                                            nsteps())):
        assert np.array_equal(got.view(np.int64), want.view(np.int64))


def test_a_hit_beside_a_voxel_without_colour_is_nan_in_colour_only(scene):
    s = scene
    color = np.array(s['color'])
    px = (I.H // 2) * I.W + I.W // 2                                    # the centre pixel sees the sphere
    V = s['vertex'][px]
    cell = np.floor((V - I.LO) / I.VS - 0.5).astype(int)
    assert color[cell[2], cell[1], cell[0], 3] > 0
    color[cell[2] + 1, cell[1], cell[0] + 1, 3] = 0.0                   # one corner of the hit's cell loses its colour
    vertex, normal, depth, rgb, inten = CR.raycast_color(s['tsdf'], s['weight'], color, I.LO, I.VS, 1.0, s['K'], s['q'][0], s['t'][0], I.H, I.W, 0.0, I.VS,
                                                         nsteps())
    assert np.array_equal(vertex, s['vertex'], equal_nan=True) and np.array_equal(depth, s['depth'])
    lost = np.isnan(inten) & np.isfinite(s['intensity'])
    assert lost[px] and np.isnan(rgb[lost]).all() and depth[lost].all() and np.isfinite(vertex[lost]).all()
    # exactly the coloured hits whose cell has that voxel as one of its 8 corners
    with np.errstate(invalid='ignore'):
        off = np.array([cell[0] + 1, cell[1], cell[2] + 1]) - np.floor((s['vertex'] - I.LO) / I.VS - 0.5)
        corner = ((off == 0) | (off == 1)).all(axis=1)
    assert np.array_equal(lost, corner & np.isfinite(s['intensity'])) and 1 <= lost.sum() < 100
    keep = ~lost
    assert np.array_equal(rgb[keep], s['rgb'][keep], equal_nan=True)
    # the scene's own maps: some hits have no colour (their cell reaches into voxels that were never in band), most do
    hit = s['depth'] > 0
    assert 0 < (hit & np.isnan(s['intensity'])).sum() < 0.05 * hit.sum()
    seen = np.isfinite(s['intensity'])
    assert s['rgb'][seen].min() >= 0 and s['rgb'][seen].max() <= 255 and np.ptp(s['intensity'][seen]) > 0.5


# ------------------------------------------------------------------------------------------------ the restated ICP
def model_of(s):
    return (s['vertex'], s['normal'], s['intensity'], I.H, I.W, s['K'], s['q'][0], s['t'][0], 0.1)


def run_color(s, color_weight, iterations=10, start=None):
    q0, t0 = start or (s['q0'], s['t0'])
    return CR.icp_color(s['depths'][0], s['rgbs'][0], s['K'], q0, t0, 1.0, I.MAX_DEPTH, *model_of(s), color_weight, iterations, 100)


def run_plain(s, iterations=10):
    return I.icp(s['depths'][0], s['K'], s['q0'], s['t0'], 1.0, I.MAX_DEPTH, s['vertex'], s['normal'], I.H, I.W, s['K'], s['q'][0], s['t'][0], 0.1, iterations,
                 100)


def test_zero_weight_is_the_depth_only_icp(scene):
    """A + 0.0 * A_c: the values of the depth-only system (a zero may change its sign, which np.array_equal does not see), so the same
    pose and the same first three stats columns."""
    pose, stats, status = run_color(scene, 0.0)
    want = run_plain(scene)
    assert status == want[2] == I.OK
    assert np.array_equal(pose, want[0]) and np.array_equal(stats[:, :3], want[1])
    assert (stats[:, 3] > 1000).all() and (stats[:, 4] > 0).all()        # the photometric pairs are counted all the same
    sums = CR.icp_color_sums(scene['depths'][0], scene['rgbs'][0], scene['K'], scene['q0'], scene['t0'], 1.0, I.MAX_DEPTH, *model_of(scene))
    assert sums.shape == (58,) and sums[57] == stats[0, 3] and sums[56] == stats[0, 4] and 0 < sums[57] <= sums[28]


def test_jc_is_the_derivative_of_rc(scene):
    """Jc against central differences of rc under the six pose increments of the header's update (dq = (1, e/2 axis), t' = t + e axis),
    for the pixels that have a pair at -e, 0 and +e in one bilinear cell and away from its border.

    The tolerance, from the step e = 1e-6 alone: |(rc(+e) - rc(-e)) / 2e - Jc| <= e^2 / 6 * max|rc'''| + rounding / e.
    rc = Im(x, y) - Is with Im bilinear in one cell, so rc''' = gx x''' + gy y''' + 3 gxy (x'' y' + x' y''); intensities lie in [0, 1],
    so |gx|, |gy| <= 1 and |gxy| <= 2.  x = fx X/Z + cx with fx = 43.2; an increment of size 1 moves the point by at most
    s = 1 + |pr| <= 2.6 (no point of the scene is farther than 1.6 m), Z >= 0.7 and |X/Z| <= 0.6, so the k-th derivative of x is at
    most fx k! (s/Z)^k (1 + |X/Z|): 255, 1.9e3, 2.1e4 for k = 1, 2, 3.  max|rc'''| <= 2 * 2.1e4 + 3 * 2 * 2 * 1.9e3 * 255 < 6e6: the
    truncation is below 1e6 e^2 = 1e-6.  The update rotates by 2 atan(e/2) = e - e^3/12, odd in e: e^2/12 * |Jc| more, far below
    that.  Rounding: rc is good to about 1e-13 (x to 10 ulp of 50 pixels, times a gradient of 1), so 1e-13 / e = 1e-7."""
    s, e = scene, 1e-6
    tol = 1e6 * e * e + 1e-13 / e
    q0, t0 = I.normalise(s['q0']), s['t0']
    args = (1.0, I.MAX_DEPTH) + model_of(s)
    mid = CR.pair_parts(s['depths'][0], s['rgbs'][0], s['K'], q0, t0, *args)
    worst, used = 0.0, 0
    for a in range(6):
        x = np.zeros(6)
        x[a] = e
        plus = CR.pair_parts(s['depths'][0], s['rgbs'][0], s['K'], *I.update(q0, t0, x), *args)
        minus = CR.pair_parts(s['depths'][0], s['rgbs'][0], s['K'], *I.update(q0, t0, -x), *args)
        sel = mid['ok'] & plus['ok'] & minus['ok']
        for P in (plus, minus):
            sel &= (P['i0'] == mid['i0']) & (P['j0'] == mid['j0'])
        for P in (plus, mid, minus):
            sel &= (P['fa'] > 1e-3) & (P['fa'] < 1 - 1e-3) & (P['fb'] > 1e-3) & (P['fb'] < 1 - 1e-3)
        assert sel.sum() > 1000
        diff = (plus['rc'][sel] - minus['rc'][sel]) / (2 * e)
        err = np.abs(diff - mid['Jc'][sel, a]).max()
        print(f'increment {a}: {int(sel.sum())} pixels, largest |Jc| {np.abs(mid["Jc"][sel, a]).max():.3f}, largest difference {err:.3e} (bound {tol:.3e})')
        assert np.abs(mid['Jc'][sel, a]).max() > 0.1                     # the comparison is not between zeros
        worst, used = max(worst, err), used + int(sel.sum())
    assert worst <= tol


def rotation_error(pose, s):
    return I.rotation_angle(pose[:4], s['q'][0])


def test_colour_holds_the_rotation_depth_cannot_see(scene):
    """The reason for the feature.  Frame 0 of the textured scene (sinusoids of wavelength 0.5 m and amplitude 100 per channel: the
    first texture tried) against the five maps ray-cast at its true pose, from icp_scene()'s start pose, 10 rounds.  Measured here, as
    (translation error m, plain rotation error rad, sphere centre as seen m, wall normal as seen rad):
        start               0.020000  0.017453  0.023199  0.015826
        depth-only          0.004837  0.064984  0.002520  0.000814
        color_weight 1e-4   0.002732  0.005042  0.002363  0.000869
        color_weight 1e-3   0.002642  0.000974  0.002331  0.000869
        color_weight 1e-2   0.002462  0.000926  0.002201  0.000848
        color_weight 1e-1   0.002289  0.000784  0.002041  0.000783     <- chosen
        color_weight 1      0.002051  0.001574  0.001442  0.001442
        color_weight 10     0.001562  0.001678  0.000512  0.001456
        color_weight 100    0.001509  0.001620  0.000544  0.001372
    Depth-only lets the rotation about the scene's symmetry axis wander to 0.065 rad; every weight tried holds it, and 0.1 has the
    smallest rotation error with both observable errors below depth-only's.  The margin on scene_error: none is needed at 0.1, where
    both components are smaller than depth-only's; the assertion allows the voxel size's share of a pixel nonetheless, 10 %."""
    s = scene
    start = rotation_error(np.concatenate([s['q0'], s['t0']]), s)
    plain = run_plain(s)[0]
    pose, stats, status = run_color(s, COLOR_WEIGHT)
    qt, tt = s['q'][0], s['t'][0]
    e_plain, e_color = I.scene_error(plain[:4], plain[4:], qt, tt), I.scene_error(pose[:4], pose[4:], qt, tt)
    print('rotation error: start', start, 'depth-only', rotation_error(plain, s), 'colour', rotation_error(pose, s))
    print('scene error: depth-only', e_plain, 'colour', e_color, 'translation', np.linalg.norm(plain[4:] - tt), np.linalg.norm(pose[4:] - tt))
    print('colour counts', stats[:, 3], 'sum rc^2', stats[:, 4])
    assert status == I.OK and (stats[:, 2] == I.OK).all()
    assert rotation_error(pose, s) < start
    assert rotation_error(pose, s) < rotation_error(plain, s)
    assert rotation_error(plain, s) > start                               # the pinned weakness is still what depth-only does
    assert e_color[0] <= 1.1 * e_plain[0] and e_color[1] <= 1.1 * e_plain[1]
    assert stats[-1, 4] < stats[0, 4]                                     # the photometric error went down, too


def test_restated_colour_tracking_beats_depth_only_tracking(scene):
    """The six frames with icp_ref.tracking_priors, into an empty volume.  Mean plain rotation error of frames 1 .. 5 against the true
    poses, measured here: priors 0.009080 rad, depth-only tracking 0.101297 rad (the model's symmetry lets every frame slide),
    colour tracking at color_weight 0.1: 0.009749 rad (0.01: 0.008976, 1: 0.010901), of which 0.008229 rad is frame 0's own prior, which
    the model inherits and no later frame can undo."""
    s = scene
    pq, pt = I.tracking_priors(s['q'], s['t'])
    z, zc = np.zeros(I.DIMS[::-1], np.float32), np.zeros(I.DIMS[::-1] + (4,), np.float32)
    q, t, status, *_ = I.track_frames(z, z, I.LO, I.VS, I.TRUNC, 64, s['depths'], s['K'], pq, pt, 1.0, I.MAX_DEPTH)
    qc, tc, cstatus, tsdf, weight, color = CR.track_frames_color(z, z, zc, I.LO, I.VS, I.TRUNC, 64, s['depths'], s['rgbs'], s['K'], pq, pt, COLOR_WEIGHT,
                                                                 1.0, I.MAX_DEPTH)
    mean = lambda qs: np.mean([I.rotation_angle(qs[f], s['q'][f]) for f in range(1, 6)])     # noqa: E731
    print('mean rotation error: priors', mean(pq), 'depth-only', mean(q), 'colour', mean(qc))
    assert (status == I.OK).all() and (cstatus == I.OK).all()
    assert np.array_equal(qc[0], pq[0]) and np.array_equal(tc[0], pt[0])
    assert mean(qc) < mean(q)
    assert (color[..., 3] > 0).sum() > 1000 and not z.any() and not zc.any()
