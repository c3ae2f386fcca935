"""CPU-side checks of coarse-to-fine registration (depth and model pyramids, levelled ICP): the bindings exist and match the header,
argument errors need no device, the K rule of a half-sampled image, the edge cases of the two restated half-samplings
(tests/levels_ref.py), and the reason for the feature: on the corrugated scene the restated single-level ICP ends a period away with
status OK, the three-level one at the truth."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

import f3d
import icp_ref as I
import levels_ref as L
from f3d import levels as LV
from Fusion3DSeg.segUtils import reconstruct, registration

PAIRS = [('f3d_depth_half', 'f3d_depth_half_dev'), ('f3d_maps_half', 'f3d_maps_half_dev'), ('f3d_icp_levels', 'f3d_icp_levels_dev')]
IDENT = np.array([1.0, 0.0, 0.0, 0.0])


# ------------------------------------------------------------------------------------------------ bindings
def test_symbols_are_bound():
    lib = f3d.library()
    for name in [n for pair in PAIRS for n in pair]:
        fn = getattr(lib, name)
        assert name in lib._f3d_symbols
        assert fn.restype is C.c_int and fn.argtypes and fn.argtypes[0] is C.c_void_p
    for host, dev in PAIRS:
        assert list(getattr(lib, dev).argtypes) == list(getattr(lib, host).argtypes) + [C.c_void_p]
    for name in ('depth_half', 'maps_half', 'icp_levels'):
        assert callable(getattr(f3d.Context, name))
        assert not hasattr(f3d.Context, name + '_dev')                  # the device twins live in f3d.levels (its docstring says why)
    assert LV.__all__ == ['depth_half_dev', 'maps_half_dev', 'icp_levels_dev']
    for name in LV.__all__:
        assert list(inspect.signature(getattr(LV, name)).parameters)[0] == 'ctx'
    assert 'route_cases' in LV.__doc__ and 'follow-up' in LV.__doc__


def test_constants_and_the_level_record_match_the_header():
    from conftest import ROOT
    text = (ROOT / 'include' / 'f3d.h').read_text()
    assert int(re.search(r'#define F3D_ICP_MAX_LEVELS (\S+)', text).group(1)) == f3d.ICP_MAX_LEVELS == L.MAX_LEVELS == 6
    for name in [n for pair in PAIRS for n in pair]:
        assert re.search(rf'\bint {name}\(f3d_ctx\* ctx', text)
    body = re.search(r'typedef struct f3d_icp_level \{(.*?)\} f3d_icp_level;', text, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body)
    names = []
    for decl in body.split(';'):
        decl = decl.strip()
        if decl:
            names += [re.sub(r'[\*\s]|\[\d+\]', '', part.split()[-1]) for part in decl.split(',')]
    assert names == [n for n, _ in f3d.IcpLevel._fields_]
    # 8-byte pointers and doubles, 4-byte ints: the C layout of the header's field order
    assert C.sizeof(f3d.IcpLevel) == 8 + 3 * 4 + 4 + 9 * 8 + 8 + 3 * 8 + 2 * 4 + 8 + 8 + 2 * 4
    assert f3d.IcpLevel.K.offset == 24 and f3d.IcpLevel.model_view.offset == 24 + 72 + 8 + 24 + 8


def test_public_surface():
    assert registration.__all__ == ['raycast', 'icp_sums', 'icp', 'track_frames']          # no new public function
    p = inspect.signature(registration.icp).parameters
    assert p['levels'].default == 1 and p['level_iterations'].default is None and p['gate'].default is None
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ('levels', 'level_iterations', 'gate'))
    p = inspect.signature(registration.track_frames).parameters
    assert p['levels'].default == 1 and p['level_iterations'].default is None and p['gate'].default is None
    assert 'levels=3' in registration.__doc__ and 'pyramids of the colour image' in registration.__doc__


# ------------------------------------------------------------------------------------------------ argument errors
def level(**kw):
    base = dict(depth=np.ones((4, 4)), K=np.eye(3), model_vertex=np.zeros((12, 3)), model_normal=np.zeros((12, 3)), hm=3, wm=4,
                model_view=np.zeros(f3d.VIEW_DOUBLES), max_dist=0.1, iterations=2, min_pairs=6)
    base.update(kw)
    return {k: v for k, v in base.items() if v is not ...}


def test_argument_errors_need_no_device():
    """A Context that was never opened has no library handle: a call that got past the checks fails with AttributeError."""
    ctx = object.__new__(f3d.Context)
    t = np.zeros(3)
    for bad in [dict(depth=np.ones((1, 4))), dict(depth=np.ones((4, 1))), dict(depth=np.ones((2, 4, 4))), dict(gate=0.0), dict(gate=-1.0),
                dict(gate=float('nan')), dict(gate=float('inf'))]:
        a = {**dict(depth=np.ones((4, 4)), gate=0.1), **bad}
        with pytest.raises(ValueError):
            ctx.depth_half(a['depth'], 1.0, 10.0, a['gate'])
    with pytest.raises(TypeError):
        ctx.depth_half(np.ones((4, 4), np.int32))
    with pytest.raises(AttributeError):
        ctx.depth_half(np.ones((4, 4)))
    maps, view = np.zeros((12, 3)), np.zeros(f3d.VIEW_DOUBLES)
    for bad in [dict(hm=1, wm=12), dict(hm=12, wm=1), dict(maps=np.zeros((11, 3))), dict(gate=0.0), dict(gate=float('inf')),
                dict(intensity=np.zeros(11)), dict(view=np.zeros(87))]:
        a = {**dict(hm=3, wm=4, maps=maps, gate=0.1, intensity=None, view=view), **bad}
        with pytest.raises(ValueError):
            ctx.maps_half(a['maps'], a['maps'], a['hm'], a['wm'], a['view'], a['gate'], a['intensity'])
    with pytest.raises(TypeError):
        ctx.maps_half(maps, maps, 3, 4, view, 0.1, np.zeros(12, np.float32))
    with pytest.raises(AttributeError):
        ctx.maps_half(maps, maps, 3, 4, view, 0.1, np.zeros(12))
    rgb = np.zeros((5, 7, 3), np.uint8)
    for levels, kw in [([], {}), ([level()] * 7, {}), ([level(iterations=0)], {}), ([level(min_pairs=5)], {}), ([level(max_dist=...)], {}),
                       ([level(model_intensity=np.zeros(12))], {}), ([level()], dict(rgb=rgb, color_weight=1.0)),
                       ([level(model_intensity=np.zeros(12)), level()], dict(rgb=rgb, color_weight=1.0)),
                       ([level(model_intensity=np.zeros(12))], dict(rgb=rgb)), ([level()], dict(color_weight=1.0)),
                       ([level(model_intensity=np.zeros(12))], dict(rgb=rgb, color_weight=-1.0)),
                       ([level(model_intensity=np.zeros(11))], dict(rgb=rgb, color_weight=1.0)),
                       ([level(model_vertex=np.zeros((11, 3)))], {}), ([level(depth=np.ones((1, 4, 4)))], {})]:
        with pytest.raises(ValueError):
            ctx.icp_levels(levels, IDENT, t, 10.0, **kw)
    with pytest.raises(AttributeError):
        ctx.icp_levels([level(), level()], IDENT, t, 10.0)
    with pytest.raises(AttributeError):
        ctx.icp_levels([level(model_intensity=np.zeros(12))], IDENT, t, 10.0, rgb=rgb, color_weight=0.5)
    # the device-pointer functions: the same checks, pointers are plain integers here
    with pytest.raises(ValueError):
        LV.depth_half_dev(ctx, 256, 0, 1, 4, 1.0, 10.0, 0.1, 512)
    with pytest.raises(ValueError):
        LV.depth_half_dev(ctx, 256, 0, 4, 4, 1.0, 10.0, 0.0, 512)
    with pytest.raises(ValueError):
        LV.maps_half_dev(ctx, 256, 512, None, 4, 1, 768, 0.1, 1024, 1280)
    with pytest.raises(ValueError):
        LV.maps_half_dev(ctx, 256, 512, 768, 4, 4, 768, 0.1, 1024, 1280, None)
    dev_level = dict(depth=256, depth_type=0, h=4, w=4, K=np.eye(3), model_vertex=512, model_normal=768, hm=3, wm=4, model_view=1024, max_dist=0.1,
                     iterations=2, min_pairs=6)
    for levels, kw in [([], {}), ([dev_level] * 7, {}), ([{**dev_level, 'iterations': 0}], {}), ([dev_level], dict(rgb_ptr=2048, color_weight=1.0)),
                       ([{k: v for k, v in dev_level.items() if k != 'h'}], {}),
                       ([{**dev_level, 'model_intensity': 4096}], dict(rgb_ptr=2048, hc=2, wc=2, color_weight=float('nan')))]:
        with pytest.raises(ValueError):
            LV.icp_levels_dev(ctx, levels, IDENT, t, 10.0, 8192, 16384, **kw)
    with pytest.raises(AttributeError):
        LV.icp_levels_dev(ctx, [dev_level], IDENT, t, 10.0, 8192, 16384)


def test_keyword_errors_come_before_any_device_call():
    """levels, level_iterations and gate are checked where the other arguments are: nothing below reaches a context."""
    K, t = np.array([[10.0, 0, 4], [0, 10.0, 4], [0, 0, 1]]), np.zeros(3)
    m3 = np.zeros((8, 8, 3))
    base = dict(depth=np.zeros((8, 8)), K=K, wxyz=IDENT, t=t, model_vertex=m3, model_normal=m3, model_K=K, model_wxyz=IDENT, model_t=t)
    for bad in [dict(levels=0), dict(levels=7), dict(levels=5), dict(levels=2, level_iterations=(3,)), dict(levels=2, level_iterations=(3, 0)),
                dict(levels=1, level_iterations=(3, 3)), dict(levels=2, gate=0.0), dict(levels=1, gate=float('nan')),
                dict(levels=4, model_vertex=np.zeros((8, 4, 3)), model_normal=np.zeros((8, 4, 3)))]:
        with pytest.raises(ValueError):
            registration.icp(**{**base, **bad})
    vol = reconstruct.TSDFVolume((0.0, 0.0, 0.0), (4, 5, 6), 0.1)
    for bad in [dict(levels=0), dict(levels=4), dict(levels=2, level_iterations=(3, 3, 3)), dict(levels=2, level_iterations=(0, 3)), dict(gate=-0.1)]:
        with pytest.raises(ValueError):
            registration.track_frames(vol, np.zeros((2, 4, 4)), K, [IDENT, IDENT], [t, t], **bad)
    assert registration._levels_plan(1, None, None, 10, 100, 0.1, ((8, 8),)) is None
    assert registration._levels_plan(3, None, None, 10, 100, 0.1, ((8, 8), (4, 4))) == (3, (10, 5, 5), 0.1, (100, 25, 6))
    assert registration._levels_plan(2, None, 0.05, 1, 6, 0.1, ((2, 2),)) == (2, (1, 1), 0.05, (6, 6))
    assert registration._levels_plan(1, (7,), None, 10, 100, 0.2, ((1, 1),)) == (1, (7,), 0.2, (100,))


# ------------------------------------------------------------------------------------------------ the K rule
def test_a_coarse_pixels_ray_is_the_mean_of_its_four_fine_rays():
    """(x / z, y / z) of the ray through a level-1 pixel centre under K' = rows 0 and 1 of K halved, against the mean over its four
    level-0 pixels under K.  Both are exact up to a few roundings of numbers below 2: 8 ulp of 2 is allowed."""
    K = np.array([[110.3, 0.0, 63.7], [0.0, 109.1, 47.9], [0.0, 0.0, 1.0]])
    K2 = registration._half_K(K)
    assert np.array_equal(K2, L.half_K(K)) and np.array_equal(K2[:2], K[:2] / 2) and np.array_equal(K2[2], K[2])
    ray = lambda K, u, v: np.array([((u + 0.5) - K[0, 2]) / K[0, 0], ((v + 0.5) - K[1, 2]) / K[1, 1]])     # noqa: E731
    for u, v in [(0, 0), (5, 3), (63, 47), (31, 0)]:
        fine = np.mean([ray(K, 2 * u + a, 2 * v + b) for b in (0, 1) for a in (0, 1)], axis=0)
        assert np.abs(ray(K2, u, v) - fine).max() <= 8 * np.spacing(2.0)


# ------------------------------------------------------------------------------------------------ depth_half edge cases
def test_depth_half_edge_cases():
    two = np.array([[1.0, 1.5], [2.0, 2.5]])
    assert np.array_equal(L.depth_half(two, 1.0, 10.0, 5.0), [[((1.0 + 1.5) + 2.0) + 2.5]] / np.float64(4))
    odd = np.arange(1.0, 16.0).reshape(3, 5)                            # the last row and the last column are dropped
    out = L.depth_half(odd, 1.0, 100.0, 100.0)
    assert out.shape == (1, 2) and np.array_equal(out, [[(((1.0 + 2.0) + 6.0) + 7.0) / 4.0, (((3.0 + 4.0) + 8.0) + 9.0) / 4.0]])
    # blocks with 0, 1 and 4 valid samples (0, NaN, inf, negative and beyond max_depth are invalid)
    d = np.array([[0.0, np.nan, 0.0, 50.0, 1.0, 1.0], [np.inf, -1.0, 2.0, 0.0, 1.0, 1.0]])
    assert np.array_equal(L.depth_half(d, 1.0, 10.0, 0.1), [[0.0, 2.0, 1.0]])
    # a block straddling a 0.5 m step: the foreground mean only
    step = np.array([[1.0, 1.5], [1.02, 1.52]])
    assert np.array_equal(L.depth_half(step, 1.0, 10.0, 0.1), [[(1.0 + 1.02) / 2.0]])
    # d - dmin == gate exactly is used: 0.5 and 0.25 are exact, so is their difference
    exact = np.array([[0.25, 0.5], [0.5000000001, 0.0]])
    assert np.array_equal(L.depth_half(exact, 1.0, 10.0, 0.25), [[(0.25 + 0.5) / 2.0]])
    # uint16 millimetres: 4000 is max_depth itself (valid), 4001 just above it
    mm = np.array([[3990, 4000], [4001, 0]], np.uint16)
    assert np.array_equal(L.depth_half(mm, 1000.0, 4.0, 0.1), [[(3990 / np.float64(1000) + 4000 / np.float64(1000)) / 2.0]])
    assert np.array_equal(L.depth_half(np.array([[4001, 4001], [4001, 65535]], np.uint16), 1000.0, 4.0, 0.1), [[0.0]])
    # the nearest valid sample decides, not the first: the far one comes first here
    assert np.array_equal(L.depth_half(np.array([[2.0, 1.0], [0.0, 0.0]]), 1.0, 10.0, 0.1), [[1.0]])


# ------------------------------------------------------------------------------------------------ maps_half edge cases
def plane_maps(hm, wm, z=2.0):
    """A fronto-parallel plane seen by the identity camera with fx = fy = 10: vertex and normal maps [hm*wm, 3]."""
    K = np.array([[10.0, 0.0, wm / 2.0], [0.0, 10.0, hm / 2.0], [0.0, 0.0, 1.0]])
    vv, uu = np.meshgrid(np.arange(hm) + 0.5, np.arange(wm) + 0.5, indexing='ij')
    vertex = np.stack([(uu - K[0, 2]) * (z / 10.0), (vv - K[1, 2]) * (z / 10.0), np.full((hm, wm), z)], axis=-1).reshape(-1, 3)
    return K, vertex, np.tile([0.0, 0.0, -1.0], (hm * wm, 1))


def test_maps_half_edge_cases():
    hm, wm = 2, 8                                                        # four blocks side by side
    K, vertex, normal = plane_maps(hm, wm)
    inten = np.arange(16.0) / 16.0
    half = lambda v, n, i=None, gate=0.1: L.maps_half(v, n, i, hm, wm, K, IDENT, np.zeros(3), gate)     # noqa: E731
    v2, n2, i2 = half(vertex, normal, inten)
    assert v2.shape == (4, 3) and n2.shape == (4, 3) and i2.shape == (4,)
    assert np.array_equal(n2, np.tile([0.0, 0.0, -1.0], (4, 1))) and np.array_equal(v2[:, 2], np.full(4, 2.0))
    assert np.array_equal(v2[0], (((vertex[0] + vertex[1]) + vertex[8]) + vertex[9]) / 4.0)
    assert np.array_equal(i2, [(((inten[2 * u] + inten[2 * u + 1]) + inten[8 + 2 * u]) + inten[9 + 2 * u]) / 4.0 for u in range(4)])
    assert half(vertex, normal)[2] is None
    # block 0: one NaN row leaves three; block 1: all four rows NaN; block 2: a non-finite normal counts as a NaN row
    v, n = vertex.copy(), normal.copy()
    v[1, 0] = np.nan
    v[[2, 3, 10, 11]] = np.nan
    n[4, 2] = np.inf
    v2, n2, i2 = half(v, n, inten)
    assert np.array_equal(v2[0], ((vertex[0] + vertex[8]) + vertex[9]) / 3.0) and i2[0] == ((inten[0] + inten[8]) + inten[9]) / 3.0
    assert np.isnan(v2[1]).all() and np.isnan(n2[1]).all() and np.isnan(i2[1])
    assert np.array_equal(v2[2], ((vertex[5] + vertex[12]) + vertex[13]) / 3.0) and np.array_equal(n2[2], [0.0, 0.0, -1.0])
    # opposite normals: len == 0 gives NaN rows; the intensity of the used rows stays
    n = normal.copy()
    n[[0, 8]] = [0.0, 0.0, 1.0]
    v2, n2, i2 = half(vertex, n, inten)
    assert np.isnan(v2[0]).all() and np.isnan(n2[0]).all() and i2[0] == (((inten[0] + inten[1]) + inten[8]) + inten[9]) / 4.0
    assert np.isfinite(v2[1:]).all()
    # a row behind the model camera is not usable (z <= 0), one further away than the gate is not used
    v = vertex.copy()
    v[0, 2] = -2.0
    v[3, 2] = 2.5
    v2, n2, _ = half(v, normal)
    assert np.array_equal(v2[0], ((vertex[1] + vertex[8]) + vertex[9]) / 3.0)
    assert np.array_equal(v2[1], ((vertex[2] + vertex[10]) + vertex[11]) / 3.0)
    assert np.array_equal(half(v, normal, gate=0.5)[0][1], (((v[2] + v[3]) + v[10]) + v[11]) / 4.0)       # z - zmin == gate exactly is used
    # intensity missing on a used row: the mean of the others; missing on all four: NaN, the geometry stays
    i = inten.copy()
    i[1] = np.nan
    i[[2, 3, 10, 11]] = np.nan
    v2, n2, i2 = half(vertex, normal, i)
    assert i2[0] == ((inten[0] + inten[8]) + inten[9]) / 3.0 and np.isnan(i2[1]) and np.isfinite(v2).all() and np.isfinite(n2).all()
    # normals are renormalised: two unit normals 90 degrees apart average to their bisector
    n = normal.copy()
    n[[0, 1]] = [1.0, 0.0, 0.0]
    g = np.array([2.0, 0.0, -2.0])
    assert np.array_equal(half(vertex, n)[1][0], g / np.sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]))
    odd = plane_maps(3, 5)
    assert L.maps_half(odd[1], odd[2], None, 3, 5, odd[0], IDENT, np.zeros(3), 0.1)[0].shape == (2, 3)


def test_restated_levels_chain_and_the_once_lost_rule():
    """One level is icp_ref.icp; two levels are two chained calls; a level lost in the middle freezes the pose and fills the rest."""
    s = I.icp_scene()
    model = (s['vertex'], s['normal'], None, I.H, I.W, s['K'], s['q'][0], s['t'][0], 0.1, 0.1)
    one = L.pyramid(s['depths'][0], s['K'], 1.0, I.MAX_DEPTH, *model, (3,), 100)
    want = I.icp(s['depths'][0], s['K'], s['q0'], s['t0'], 1.0, I.MAX_DEPTH, s['vertex'], s['normal'], I.H, I.W, s['K'], s['q'][0], s['t'][0], 0.1, 3, 100)
    got = L.icp_levels(one, s['q0'], s['t0'], I.MAX_DEPTH)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2] == I.OK
    three = L.pyramid(s['depths'][0], s['K'], 1.0, I.MAX_DEPTH, *model, (2, 2, 2), 100)
    assert [(lv['hm'], lv['wm'], lv['min_pairs']) for lv in three] == [(10, 12, 6), (20, 24, 25), (40, 48, 100)]
    assert three[0]['depth'].shape == (10, 12) and three[0]['K'][0, 0] == s['K'][0, 0] / 4 and three[0]['depth_scale'] == 1.0
    pose, stats, status = L.icp_levels(three, s['q0'], s['t0'], I.MAX_DEPTH)
    assert status == I.OK and stats.shape == (6, 3) and (stats[:, 2] == I.OK).all()
    assert stats[0, 0] <= 120 and stats[2, 0] <= 480 and stats[4, 0] > 480        # the rows are in running order, coarsest first
    first = L.icp_levels(three[:1], s['q0'], s['t0'], I.MAX_DEPTH)
    three[1]['min_pairs'] = 20 * 24 + 1
    pose, stats, status = L.icp_levels(three, s['q0'], s['t0'], I.MAX_DEPTH)
    assert status == I.LOST and np.array_equal(pose, first[0]) and np.array_equal(stats[:2], first[1])
    assert stats[2, 0] > 100 and stats[2, 2] == I.LOST and np.array_equal(stats[3:], [[0.0, 0.0, 1.0]] * 3)


# ------------------------------------------------------------------------------------------------ why the feature exists
STARTS = [(0.05, 2.0), (0.08, 3.0), (0.12, 4.0)]
# final (metres, radians) of the restated single-level runs, measured here: {start: (10 rounds, 23 rounds)}
SINGLE = {(0.05, 2.0): ((0.093101, 0.016428), (0.093072, 0.016423)), (0.08, 3.0): ((0.085575, 0.014989), (0.093072, 0.016423)),
          (0.12, 4.0): ((0.163846, 0.033157), (0.093080, 0.016418))}


@pytest.fixture(scope='module')
def corrugated():
    s = L.corrugated_scene()
    for a in s.values():
        a.setflags(write=False)
    return s


@pytest.mark.parametrize('start', STARTS)
def test_three_levels_converge_where_one_level_slides_a_period(corrugated, start):
    """The corrugated scene (96 x 128, period 0.08 m = 5.9 pixels at 1.5 m), the source frame the model's own depth, so the true pose
    is the identity; max_dist 0.1, min_pairs 50.  Final translation error in metres / rotation error in radians, measured with the
    restatement:
        start          1 level, 10 rounds     1 level, 23 rounds     3 levels, 5 + 5 + 10 rounds
        0.05 m, 2 deg  0.093101 / 0.016428    0.093072 / 0.016423    9.95e-17 / 0
        0.08 m, 3 deg  0.085575 / 0.014989    0.093072 / 0.016423    9.09e-17 / 0
        0.12 m, 4 deg  0.163846 / 0.033157    0.093080 / 0.016418    7.62e-17 / 0
    Every run reports OK in every round.  The single-level runs end one corrugation period (0.0931 m along the start's shift) away; the
    assertion asks for at least half the measured distance.  Three levels end at the truth to the last bits (the source frame is the
    model's own depth); they must end within 1e-3 m and 1e-3 rad, a hundredth of a period, whatever the order of the block sums."""
    s = corrugated
    q0, t0 = L.corrugated_start(*start)
    for rounds, measured in zip(((10,), (23,)), SINGLE[start]):
        pose, stats, status = L.corrugated_run(s, (q0, t0), rounds)
        err = L.pose_error(pose)
        print(f'start {start}, 1 level, {rounds[0]} rounds: {err[0]:.6f} m, {err[1]:.6f} rad, status {status}')
        assert status == I.OK and (stats[:, 2] == I.OK).all() and (stats[:, 0] > 1000).all()
        assert err[0] >= 0.5 * measured[0]
    pose, stats, status = L.corrugated_run(s, (q0, t0), (10, 5, 5))
    err = L.pose_error(pose)
    print(f'start {start}, 3 levels: {err[0]:.3e} m, {err[1]:.3e} rad, status {status}, pairs per round {stats[:, 0]}')
    assert status == I.OK and stats.shape == (20, 3) and (stats[:, 2] == I.OK).all()
    assert err[0] <= 1e-3 and err[1] <= 1e-3
