"""Coarse-to-fine registration on the GPU against its NumPy restatement (tests/levels_ref.py): the half-sampled frames and maps, the
poses, stats and status of the levelled rounds bit for bit (compared as integer views); launch shapes, uninitialised memory, a strict
context; the public surface on both routes; and the hand-off from torch of the three f3d.levels functions behind a stalled stream and
from strided inputs (the cases tests/route_cases.py will carry once they move onto Context)."""
import numpy as np
import pytest

import f3d
import icp_color_ref as CR
import icp_ref as I
import levels_ref as L
import stalled_streams as S
from f3d import levels as LV
from poison import poisoned_empty
from Fusion3DSeg.segUtils import reconstruct, registration

pytestmark = pytest.mark.gpu

H, W, MAX_DEPTH = I.H, I.W, I.MAX_DEPTH
COLOR_WEIGHT, GATE = 0.1, 0.1
IDENT = np.array([1.0, 0.0, 0.0, 0.0])


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def same_bits(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and got.dtype == want.dtype == np.float64 and np.array_equal(bits(got), bits(want))


@pytest.fixture(scope='module')
def ctx():
    return f3d.default_context()


@pytest.fixture(scope='module')
def scene():
    """icp_color_ref.color_scene() with holes in the three model maps."""
    s = CR.color_scene()
    s['vertex'][3 * W + 5:3 * W + 9] = np.nan
    s['normal'][17 * W + 20, 1] = np.nan
    s['vertex'][25 * W + 30, 2] = np.inf
    s['intensity'][12 * W + 10:12 * W + 30:3] = np.nan
    s['intensity'][30 * W + 7] = np.inf
    for a in s.values():
        a.setflags(write=False)
    return s


# ------------------------------------------------------------------------------------------------ depth_half
def random_depth(h, w, dtype, seed):
    """Two surfaces 0.3 m apart in patches, 2 cm of noise, and invalid pixels of every kind -> (raw frame, depth_scale)."""
    rng = np.random.default_rng(seed)
    d = np.where(rng.random((h, w)) < 0.5, 1.2, 1.5) + rng.uniform(-0.02, 0.02, (h, w))
    d[rng.random((h, w)) < 0.15] = 0.0
    d[rng.random((h, w)) < 0.05] = 5.5                                  # beyond max_depth
    if dtype == np.uint16:
        return np.round(d * 1000.0).astype(np.uint16), 1000.0
    d[rng.random((h, w)) < 0.05] = np.nan
    d[rng.random((h, w)) < 0.03] = np.inf
    d[rng.random((h, w)) < 0.03] = -1.0
    return d.astype(dtype), 1.0


def scene_depth(s, dtype):
    d = np.array(s['depths'][0])
    d.reshape(-1)[3::41] = 0.0
    return (np.round(d * 1000.0).astype(np.uint16), 1000.0) if dtype == np.uint16 else (d.astype(dtype), 1.0)


@pytest.mark.parametrize('dtype', [np.float64, np.float32, np.uint16])
def test_depth_half_equals_the_restatement(ctx, scene, dtype):
    """2 x 2 (one output pixel), 3 x 5 (an odd row and column dropped), the scene's 40 x 48 frame, 65 x 129 (32 x 64 outputs: 8 blocks,
    and a dropped row and column)."""
    frames = [random_depth(2, 2, dtype, 1), random_depth(3, 5, dtype, 2), scene_depth(scene, dtype), random_depth(65, 129, dtype, 3)]
    for raw, scale in frames:
        for gate in (0.05, 10.0):
            want = L.depth_half(raw, scale, MAX_DEPTH, gate)
            got = ctx.depth_half(raw, scale, MAX_DEPTH, gate)
            assert got.shape == (raw.shape[0] // 2, raw.shape[1] // 2) and same_bits(got, want)
    big, scale = frames[3]
    tight, loose = L.depth_half(big, scale, MAX_DEPTH, 0.05), L.depth_half(big, scale, MAX_DEPTH, 10.0)
    assert (tight == 0).any() and (tight != loose).sum() > 100 and (tight[tight > 0] < 1.6).all()     # the gate decided many blocks
    with pytest.raises(ValueError):
        ctx._check(ctx._lib.f3d_depth_half(ctx._h, f3d._ptr(np.ones((1, 4))), 0, 1, 4, 1.0, MAX_DEPTH, 0.1, f3d._ptr(np.ones(4))))


# ------------------------------------------------------------------------------------------------ maps_half
def random_maps(hm, wm, seed):
    """Maps seen by the identity camera: two depths in patches, random unit normals, NaN and inf rows, points behind the camera, and an
    intensity map with holes -> (K, vertex, normal, intensity)."""
    rng = np.random.default_rng(seed)
    K = np.array([[60.0, 0.0, wm / 2.0], [0.0, 60.0, hm / 2.0], [0.0, 0.0, 1.0]])
    z = np.where(rng.random((hm, wm)) < 0.5, 1.2, 1.5) + rng.uniform(-0.02, 0.02, (hm, wm))
    z[rng.random((hm, wm)) < 0.05] = -0.5
    vv, uu = np.meshgrid(np.arange(hm) + 0.5, np.arange(wm) + 0.5, indexing='ij')
    vertex = np.stack([(uu - K[0, 2]) * (z / 60.0), (vv - K[1, 2]) * (z / 60.0), z], axis=-1).reshape(-1, 3)
    normal = rng.normal(size=(hm * wm, 3))
    normal /= np.linalg.norm(normal, axis=1, keepdims=True)
    vertex[rng.random(hm * wm) < 0.15] = np.nan
    normal[rng.random(hm * wm) < 0.05, 1] = np.inf
    inten = rng.random(hm * wm)
    inten[rng.random(hm * wm) < 0.2] = np.nan
    return K, vertex, normal, inten


def check_maps(ctx, vertex, normal, inten, hm, wm, K, q, t, gate=GATE):
    view = f3d.views_build(K, wm, hm, np.asarray(q)[None], np.asarray(t)[None], MAX_DEPTH)
    want = L.maps_half(vertex, normal, inten, hm, wm, K, q, t, gate)
    got = ctx.maps_half(vertex, normal, hm, wm, view, gate, inten)
    assert len(got) == (2 if inten is None else 3)
    for g, x in zip(got, want):
        assert same_bits(g, x)
    return want


@pytest.mark.parametrize('with_intensity', [False, True])
def test_maps_half_equals_the_restatement(ctx, scene, with_intensity):
    s = scene
    inten = s['intensity'] if with_intensity else None
    v2, n2, i2 = check_maps(ctx, s['vertex'], s['normal'], inten, H, W, s['K'], s['q'][0], s['t'][0])
    hit = np.isfinite(v2).all(axis=1)
    assert hit.sum() > 300 and (~hit).any() and np.allclose(np.linalg.norm(n2[hit], axis=1), 1.0)
    if with_intensity:
        assert np.isfinite(i2).sum() > 300
    for hm, wm, seed in [(2, 2, 4), (3, 5, 5), (37, 43, 6), (65, 129, 7)]:                  # odd widths: the lower row pairs are not 16-byte aligned
        K, vertex, normal, ri = random_maps(hm, wm, seed)
        for gate in (0.05, 10.0):
            out = check_maps(ctx, vertex, normal, ri if with_intensity else None, hm, wm, K, IDENT, np.zeros(3), gate)
    assert np.isnan(out[0]).any() and np.isfinite(out[0]).any()


def test_maps_half_from_unaligned_device_pointers(ctx):
    """Maps that start 8 bytes into their allocation take the scalar loads: the same bits as the 16-byte aligned copies."""
    import torch
    hm, wm = 20, 24
    K, vertex, normal, inten = random_maps(hm, wm, 8)
    want = L.maps_half(vertex, normal, inten, hm, wm, K, IDENT, np.zeros(3), GATE)
    view = torch.from_numpy(f3d.views_build(K, wm, hm, IDENT[None], np.zeros((1, 3)), MAX_DEPTH)).cuda()
    shifted = lambda a: torch.cat([torch.zeros(1, dtype=torch.float64), torch.from_numpy(a.reshape(-1))]).cuda()[1:]     # noqa: E731
    dv, dn, di = shifted(vertex), shifted(normal), shifted(inten)
    assert dv.data_ptr() % 16 == 8 and dn.data_ptr() % 16 == 8
    n2 = (hm // 2) * (wm // 2)
    outs = [torch.zeros(n2 * 3 + 1, dtype=torch.float64, device='cuda')[1:] for _ in range(2)] + [torch.zeros(n2 + 1, dtype=torch.float64, device='cuda')[1:]]
    torch.cuda.synchronize()                                            # the context's own stream is not ordered with torch's
    LV.maps_half_dev(ctx, dv.data_ptr(), dn.data_ptr(), di.data_ptr(), hm, wm, view.data_ptr(), GATE, *(o.data_ptr() for o in outs))
    ctx.synchronize()
    for o, x in zip(outs, want):
        assert same_bits(o.cpu().numpy().reshape(x.shape), x)


# ------------------------------------------------------------------------------------------------ launch shapes, poison
@pytest.fixture(scope='module')
def big():
    """A 65 x 129 frame and maps (32 x 64 outputs: 8 blocks of either kernel) and what the restatement gives for them."""
    raw, scale = random_depth(65, 129, np.float32, 9)
    K, vertex, normal, inten = random_maps(65, 129, 10)
    return dict(raw=raw, scale=scale, K=K, vertex=vertex, normal=normal, inten=inten, depth2=L.depth_half(raw, scale, MAX_DEPTH, GATE),
                maps2=L.maps_half(vertex, normal, inten, 65, 129, K, IDENT, np.zeros(3), GATE),
                plain2=L.maps_half(vertex, normal, None, 65, 129, K, IDENT, np.zeros(3), GATE),
                view=f3d.views_build(K, 129, 65, IDENT[None], np.zeros((1, 3)), MAX_DEPTH))


def check_big(own, b):
    assert same_bits(own.depth_half(b['raw'], b['scale'], MAX_DEPTH, GATE), b['depth2'])
    for g, x in zip(own.maps_half(b['vertex'], b['normal'], 65, 129, b['view'], GATE, b['inten']), b['maps2']):
        assert same_bits(g, x)
    for g, x in zip(own.maps_half(b['vertex'], b['normal'], 65, 129, b['view'], GATE), b['plain2']):
        assert same_bits(g, x)


@pytest.mark.parametrize('cap', [1, 3])
def test_half_samplings_do_not_depend_on_the_launch_shape(big, cap):
    own = f3d.Context(0)
    try:
        own.debug_grid_cap(0)
        own.debug_grid_cap_stats()
        own.debug_grid_cap(cap)
        try:
            check_big(own, big)
        finally:
            own.debug_grid_cap(0)
        calls, lowered = own.debug_grid_cap_stats()
        print(f'cap {cap}: {calls} grids sized under the cap, {lowered} lowered')
        assert calls >= lowered >= 3                                    # one depth_half and two maps_half launches of 8 blocks each
    finally:
        own.debug_grid_cap(0)
        own.close()


@pytest.mark.parametrize('byte', [0x00, 0xFF, 0x5A])
def test_half_samplings_do_not_depend_on_uninitialised_memory(big, byte):
    own = f3d.Context(0)
    try:
        check_big(own, big)                                             # the staging buffers exist and hold other values
        own.debug_poison(byte)
        with poisoned_empty(byte):                                      # the outputs the bindings allocate are pre-filled
            check_big(own, big)
    finally:
        own.close()


# ------------------------------------------------------------------------------------------------ icp_levels
def source(s, color):
    return (s['depths'][0], s['K'], 1.0, MAX_DEPTH, s['vertex'], s['normal'], s['intensity'] if color else None, H, W, s['K'], s['q'][0], s['t'][0], 0.1,
            GATE)


def with_views(levels):
    """The restatement's levels as Context.icp_levels takes them: the model camera as a views_build record."""
    out = []
    for lv in levels:
        view = f3d.views_build(lv['model_K'], lv['wm'], lv['hm'], np.asarray(lv['model_q'])[None], np.asarray(lv['model_t'])[None], MAX_DEPTH)
        out.append({**{k: v for k, v in lv.items() if k not in ('model_K', 'model_q', 'model_t')}, 'model_view': view})
    return out


def colour_of(s, color):
    return dict(rgb=s['rgbs'][0], color_weight=COLOR_WEIGHT) if color else {}


@pytest.mark.parametrize('color', [False, True])
def test_one_level_is_icp(ctx, scene, color):
    s = scene
    levels = with_views(L.pyramid(*source(s, color), (4,), 100))
    pose, stats, status = ctx.icp_levels(levels, s['q0'], s['t0'], MAX_DEPTH, **colour_of(s, color))
    view = levels[0]['model_view']
    if color:
        want = ctx.icp_color(s['depths'][0], s['K'], s['q0'], s['t0'], s['vertex'], s['normal'], H, W, view, 0.1, s['intensity'], s['rgbs'][0],
                             COLOR_WEIGHT, 1.0, MAX_DEPTH, 4, 100)
    else:
        want = ctx.icp(s['depths'][0], s['K'], s['q0'], s['t0'], s['vertex'], s['normal'], H, W, view, 0.1, 1.0, MAX_DEPTH, 4, 100)
    assert status == want[2] == I.OK and same_bits(pose, want[0]) and same_bits(stats, want[1])


@pytest.fixture(scope='module')
def three(scene):
    """{color: (the restatement's three levels with 2 + 2 + 3 rounds, what it gives from the scene's start pose)}"""
    out = {}
    for color in (False, True):
        levels = L.pyramid(*source(scene, color), (3, 2, 2), 100)
        out[color] = (levels, L.icp_levels(levels, scene['q0'], scene['t0'], MAX_DEPTH, *colour_of(scene, color).values()))
    return out


@pytest.mark.parametrize('color', [False, True])
def test_three_levels_equal_the_chained_restatement(ctx, scene, three, color):
    s = scene
    levels, want = three[color]
    assert [(lv['hm'], lv['wm'], lv['iterations'], lv['min_pairs']) for lv in levels] == [(10, 12, 2, 6), (20, 24, 2, 25), (40, 48, 3, 100)]
    pose, stats, status = ctx.icp_levels(with_views(levels), s['q0'], s['t0'], MAX_DEPTH, **colour_of(s, color))
    assert status == want[2] == I.OK and stats.shape == (7, 5 if color else 3)
    assert same_bits(stats, want[1]) and same_bits(pose, want[0])
    assert stats[0, 0] <= 120 < stats[2, 0] <= 480 < stats[4, 0]        # running order: coarsest first
    if color:
        assert (stats[:, 3] > 0).all() and not same_bits(pose, three[False][1][0])


def test_a_call_lost_at_the_middle_level(ctx, scene, three):
    """min_pairs above the middle level's pixel count: the pose the first level produced, {0, 0, 1} rows after the lost round, LOST."""
    s = scene
    levels = [dict(lv) for lv in three[False][0]]
    levels[1]['min_pairs'] = 20 * 24 + 1
    want = L.icp_levels(levels, s['q0'], s['t0'], MAX_DEPTH)
    first = L.icp_levels(levels[:1], s['q0'], s['t0'], MAX_DEPTH)
    pose, stats, status = ctx.icp_levels(with_views(levels), s['q0'], s['t0'], MAX_DEPTH)
    assert status == want[2] == I.LOST and same_bits(pose, want[0]) and same_bits(stats, want[1])
    assert same_bits(pose, first[0]) and same_bits(stats[:2], first[1]) and stats[2, 0] > 100 and stats[2, 2] == I.LOST
    assert np.array_equal(stats[3:], [[0.0, 0.0, 1.0]] * 4)
    with pytest.raises(ValueError):                                     # the C entry refuses no levels, too
        recs = (f3d.IcpLevel * 1)()
        ctx._check(ctx._lib.f3d_icp_levels(ctx._h, recs, 0, MAX_DEPTH, f3d._ptr(IDENT), f3d._ptr(np.zeros(3)), None, 0, 0, 0.0,
                                           f3d._ptr(np.zeros(7)), f3d._ptr(np.zeros(3)), f3d._ptr(np.zeros(1, np.int32))))


def device_levels(torch, levels, views):
    """The restatement's levels with every array on the device -> (level dicts of pointers, the tensors)."""
    keep, out = [], []
    for l, lv in enumerate(levels):
        t = {k: torch.from_numpy(np.array(lv[k])).cuda() for k in ('depth', 'model_vertex', 'model_normal', 'model_intensity')
             if lv[k] is not None}
        keep.append(t)
        out.append(dict(depth=t['depth'].data_ptr(), depth_type=0, h=lv['depth'].shape[0], w=lv['depth'].shape[1], K=lv['K'],
                        depth_scale=lv['depth_scale'], model_vertex=t['model_vertex'].data_ptr(), model_normal=t['model_normal'].data_ptr(),
                        model_intensity=t['model_intensity'].data_ptr() if 'model_intensity' in t else None, hm=lv['hm'], wm=lv['wm'],
                        model_view=views[l].data_ptr(), max_dist=lv['max_dist'], iterations=lv['iterations'], min_pairs=lv['min_pairs']))
    return out, keep


@pytest.mark.parametrize('color', [False, True])
def test_strict_reserved_context_allocates_nothing(scene, three, color):
    """The scratch of the largest level, reserved: the two half-samplings and the levelled rounds allocate nothing."""
    import torch
    s = scene
    levels, want = three[color]
    own = f3d.Context(0)
    try:
        (own.reserve_icp_color if color else own.reserve_icp)(H * W)
        views = torch.from_numpy(np.concatenate([lv['model_view'] for lv in with_views(levels)])).cuda()
        recs, keep = device_levels(torch, levels, views)
        empty = lambda *shape: torch.empty(shape, dtype=torch.float64, device='cuda')     # noqa: E731
        pose, stats, status = empty(7), empty(7, 5 if color else 3), torch.empty(1, dtype=torch.int32, device='cuda')
        rgb = torch.from_numpy(np.array(s['rgbs'][0])).cuda()
        d2, v2, n2, i2 = empty(20 * 24), empty(20 * 24, 3), empty(20 * 24, 3), empty(20 * 24)
        fine = keep[2]
        torch.cuda.synchronize()
        own.set_strict(True)
        before = own.alloc_count
        LV.depth_half_dev(own, fine['depth'].data_ptr(), 0, H, W, 1.0, MAX_DEPTH, GATE, d2.data_ptr())
        LV.maps_half_dev(own, fine['model_vertex'].data_ptr(), fine['model_normal'].data_ptr(), fine['model_intensity'].data_ptr() if color else None, H, W,
                         views[2].data_ptr(), GATE, v2.data_ptr(), n2.data_ptr(), i2.data_ptr() if color else None)
        col = dict(rgb_ptr=rgb.data_ptr(), hc=H, wc=W, color_weight=COLOR_WEIGHT) if color else {}
        LV.icp_levels_dev(own, recs, s['q0'], s['t0'], MAX_DEPTH, pose.data_ptr(), stats.data_ptr(), status.data_ptr(), **col)
        own.synchronize()
        assert own.alloc_count == before
        assert same_bits(pose.cpu().numpy(), want[0]) and same_bits(stats.cpu().numpy(), want[1]) and int(status[0]) == want[2]
        assert same_bits(d2.cpu().numpy().reshape(20, 24), levels[1]['depth']) and same_bits(v2.cpu().numpy(), levels[1]['model_vertex'])
        assert same_bits(n2.cpu().numpy(), levels[1]['model_normal'])
        if color:
            assert same_bits(i2.cpu().numpy(), levels[1]['model_intensity'])
    finally:
        own.close()


# ------------------------------------------------------------------------------------------------ the public surface
def module_args(s, color, device=False):
    import torch
    up = (lambda a: torch.from_numpy(np.array(a)).cuda()) if device else (lambda a: a)     # noqa: E731
    args = (up(s['depths'][0]), s['K'], s['q0'], s['t0'], up(s['vertex'].reshape(H, W, 3)), up(s['normal'].reshape(H, W, 3)), s['K'], s['q'][0], s['t'][0])
    kw = dict(max_depth=MAX_DEPTH, iterations=3)
    if color:
        kw.update(color=up(s['rgbs'][0]), model_intensity=up(s['intensity'].reshape(H, W)), color_weight=COLOR_WEIGHT)
    return args, kw


@pytest.mark.parametrize('color', [False, True])
def test_icp_with_levels_on_both_routes(ctx, scene, color):
    """levels=3 with the defaults: 3 rounds at full resolution and 1 on each coarser level, gate = max_dist, min_pairs 100, 25, 6."""
    s = scene
    levels = L.pyramid(*source(s, color), (3, 1, 1), 100)
    want = L.icp_levels(levels, s['q0'], s['t0'], MAX_DEPTH, *colour_of(s, color).values())
    args, kw = module_args(s, color)
    q, t, info = registration.icp(*args, **kw, levels=3)
    assert same_bits(np.concatenate([q, t]), want[0]) and info['status'] == want[2] == 0 and info['level_rounds'] == (1, 1, 3)
    assert same_bits(info['counts'], want[1][:, 0]) and info['rms'].shape == (5,)
    dargs, dkw = module_args(s, color, device=True)
    dq, dt, dinfo = registration.icp(*dargs, **dkw, levels=3)
    assert dq.is_cuda and dt.is_cuda and dinfo['counts'].is_cuda and dinfo['level_rounds'] == (1, 1, 3) and dinfo['status'] == 0
    assert same_bits(dq.cpu().numpy(), q) and same_bits(dt.cpu().numpy(), t) and same_bits(dinfo['counts'].cpu().numpy(), info['counts'])
    if color:
        assert same_bits(dinfo['color_counts'].cpu().numpy(), want[1][:, 3]) and same_bits(info['color_counts'], want[1][:, 3])
    # levels=1 is the call without the keyword; level_iterations alone goes through the levelled entry and gives the same bits
    plain = registration.icp(*args, **kw)
    one = registration.icp(*args, **kw, levels=1)
    assert same_bits(one[0], plain[0]) and same_bits(one[1], plain[1]) and 'level_rounds' not in one[2] and same_bits(one[2]['counts'], plain[2]['counts'])
    single = registration.icp(*args, **kw, level_iterations=(3,))
    assert same_bits(single[0], plain[0]) and same_bits(single[1], plain[1]) and single[2]['level_rounds'] == (3,)
    assert not same_bits(q, plain[0])


def test_track_frames_with_levels_on_both_routes(ctx, scene):
    import torch
    s = scene
    pq, pt = I.tracking_priors(s['q'], s['t'])
    runs = {}
    for color in (False, True):
        kw = dict(max_depth=MAX_DEPTH, iterations=4, levels=3, level_iterations=(4, 2, 2))
        if color:
            kw.update(colors=s['rgbs'][:4], color_weight=COLOR_WEIGHT)
        vol = reconstruct.TSDFVolume(I.LO, I.DIMS, I.VS, I.TRUNC, color=color)
        q, t, status = registration.track_frames(vol, s['depths'][:4], s['K'], pq[:4], pt[:4], **kw)
        dvol = reconstruct.TSDFVolume(I.LO, I.DIMS, I.VS, I.TRUNC, color=color)
        if color:
            kw['colors'] = torch.from_numpy(np.array(s['rgbs'][:4])).cuda()
        dq, dt, dstatus = registration.track_frames(dvol, torch.from_numpy(np.array(s['depths'][:4])).cuda(), s['K'], pq[:4], pt[:4], **kw)
        assert (status == 0).all() and np.array_equal(dstatus.cpu().numpy(), status)
        assert same_bits(dq.cpu().numpy(), q) and same_bits(dt.cpu().numpy(), t)
        assert np.array_equal(dvol.tsdf.cpu().numpy().view(np.int32), vol.tsdf.view(np.int32))
        assert np.array_equal(q[0], pq[0]) and not np.array_equal(q[1], pq[1])
        runs[color] = q
    vol = reconstruct.TSDFVolume(I.LO, I.DIMS, I.VS, I.TRUNC)
    plain = registration.track_frames(vol, s['depths'][:4], s['K'], pq[:4], pt[:4], max_depth=MAX_DEPTH, iterations=4)
    vol1 = reconstruct.TSDFVolume(I.LO, I.DIMS, I.VS, I.TRUNC)
    one = registration.track_frames(vol1, s['depths'][:4], s['K'], pq[:4], pt[:4], max_depth=MAX_DEPTH, iterations=4, levels=1)
    assert same_bits(one[0], plain[0]) and same_bits(one[1], plain[1]) and not same_bits(runs[False], plain[0])


def test_the_corrugated_scene_through_the_module(ctx):
    """The (0.08 m, 3 degrees) start of tests/test_registration_levels_cpu.py, with its bounds: the single-level call reports status 0
    and ends at least half its measured 0.085575 m from the truth; levels=3 with (10, 5, 5) rounds ends within 1e-3 m and 1e-3 rad."""
    s = L.corrugated_scene()
    q0, t0 = L.corrugated_start(0.08, 3.0)
    args = (s['depth'], s['K'], q0, t0, s['vertex'].reshape(L.CH, L.CW, 3), s['normal'].reshape(L.CH, L.CW, 3), s['K'], s['q'], s['t'])
    kw = dict(max_dist=0.1, max_depth=L.CMAX_DEPTH, iterations=10, min_pairs=50)
    q, t, info = registration.icp(*args, **kw)
    err = L.pose_error(np.concatenate([q, t]))
    print(f'1 level: {err[0]:.6f} m, {err[1]:.6f} rad, status {info["status"]}')
    assert info['status'] == 0 and err[0] >= 0.5 * 0.085575
    q, t, info = registration.icp(*args, **kw, levels=3, level_iterations=(10, 5, 5))
    err = L.pose_error(np.concatenate([q, t]))
    print(f'3 levels: {err[0]:.3e} m, {err[1]:.3e} rad, status {info["status"]}, pairs {info["counts"]}')
    assert info['status'] == 0 and info['level_rounds'] == (5, 5, 10) and err[0] <= 1e-3 and err[1] <= 1e-3
    want = L.corrugated_run(s, (q0, t0), (10, 5, 5))
    assert same_bits(np.concatenate([q, t]), want[0]) and same_bits(info['counts'], want[1][:, 0])


# ------------------------------------------------------------------------------------------------ the hand-off from torch
def handoff_run(torch, ctx, t, views, q0, t0, stream):
    """depth_half_dev, maps_half_dev and a two-level icp_levels_dev with colour over their outputs, all enqueued on `stream`."""
    f64 = lambda *shape: torch.zeros(shape, dtype=torch.float64, device='cuda')     # noqa: E731
    h2, w2 = H // 2, W // 2
    d2, v2, n2, i2, pose, stats = f64(h2 * w2), f64(h2 * w2, 3), f64(h2 * w2, 3), f64(h2 * w2), f64(7), f64(4, 5)
    status = torch.zeros(1, dtype=torch.int32, device='cuda')
    LV.depth_half_dev(ctx, t['depth'].data_ptr(), 0, H, W, 1.0, MAX_DEPTH, GATE, d2.data_ptr(), stream)
    LV.maps_half_dev(ctx, t['vertex'].data_ptr(), t['normal'].data_ptr(), t['intensity'].data_ptr(), H, W, views[0].data_ptr(), GATE, v2.data_ptr(),
                     n2.data_ptr(), i2.data_ptr(), stream)
    K = np.array(t['K'])
    fine = dict(depth=t['depth'].data_ptr(), depth_type=0, h=H, w=W, K=K, model_vertex=t['vertex'].data_ptr(), model_normal=t['normal'].data_ptr(),
                model_intensity=t['intensity'].data_ptr(), hm=H, wm=W, model_view=views[0].data_ptr(), max_dist=0.1, iterations=2, min_pairs=100)
    coarse = dict(depth=d2.data_ptr(), depth_type=0, h=h2, w=w2, K=L.half_K(K), model_vertex=v2.data_ptr(), model_normal=n2.data_ptr(),
                  model_intensity=i2.data_ptr(), hm=h2, wm=w2, model_view=views[1].data_ptr(), max_dist=0.1, iterations=2, min_pairs=25)
    LV.icp_levels_dev(ctx, [coarse, fine], q0, t0, MAX_DEPTH, pose.data_ptr(), stats.data_ptr(), status.data_ptr(), t['rgb'].data_ptr(), H, W, COLOR_WEIGHT,
                      stream)
    return dict(d2=d2, v2=v2, n2=n2, i2=i2, pose=pose, stats=stats, status=status)


def test_the_three_device_functions_behind_a_stalled_stream(ctx, scene):
    """The caller's stream sleeps; behind the sleep the inputs, which hold a decoy, are overwritten with the scene; the three functions
    are enqueued at once, their outputs cloned on the stream, and the inputs overwritten with the decoy again.  Work that ran on
    another stream, or before the caller's stream got there, read the decoy."""
    import torch
    s = scene
    levels = L.pyramid(*source(s, True), (2, 2), 100)
    want = L.icp_levels(levels, s['q0'], s['t0'], MAX_DEPTH, s['rgbs'][0], COLOR_WEIGHT)
    a = dict(depth=s['depths'][0], vertex=s['vertex'], normal=s['normal'], intensity=s['intensity'], rgb=s['rgbs'][0])
    b = dict(depth=np.array(s['depths'][1]), vertex=np.roll(s['vertex'], 7, axis=0), normal=np.roll(s['normal'], 5, axis=0),
             intensity=np.roll(s['intensity'], 11), rgb=255 - s['rgbs'][0])
    up = lambda d: {k: torch.from_numpy(np.array(v)).cuda() for k, v in d.items()}     # noqa: E731
    views = torch.from_numpy(np.concatenate([lv['model_view'] for lv in with_views(levels[::-1])])).cuda()
    caller = torch.cuda.Stream()
    src_a, src_b, t = up(a), up(b), up(b)
    t['K'] = s['K']

    def check(got):
        assert same_bits(got['d2'].cpu().numpy().reshape(H // 2, W // 2), levels[0]['depth'])
        for k, x in (('v2', 'model_vertex'), ('n2', 'model_normal'), ('i2', 'model_intensity')):
            assert same_bits(got[k].cpu().numpy(), levels[0][x])
        assert same_bits(got['pose'].cpu().numpy(), want[0]) and same_bits(got['stats'].cpu().numpy(), want[1]) and int(got['status'][0]) == want[2]

    with torch.cuda.stream(caller):
        for k in src_a:                                                 # the unstalled warm-up: the scratch has grown, the scene passes
            t[k].copy_(src_a[k])
        warm = handoff_run(torch, ctx, t, views, s['q0'], s['t0'], caller.cuda_stream)
        caller.synchronize()
        check(warm)
        for k in src_b:
            t[k].copy_(src_b[k])
        torch.cuda.synchronize()
        e = S.stall(caller)
        for k in src_a:
            t[k].copy_(src_a[k])
        got = handoff_run(torch, ctx, t, views, s['q0'], s['t0'], caller.cuda_stream)
        still_stalled = not e.query()
        snapshot = {k: v.clone() for k, v in got.items()}
        for k in src_b:
            t[k].copy_(src_b[k])
    assert still_stalled, f'the {S.STALL_MS} ms stall had ended when the three calls returned: one of them waited for the device'
    caller.synchronize()
    check(snapshot)


@pytest.mark.parametrize('color', [False, True])
def test_strided_sliced_and_offset_inputs(ctx, scene, color):
    """registration.icp(levels=3) from views into larger tensors (a column slice, every other row, a channel slice, an offset into a flat
    buffer) against the same call from contiguous tensors."""
    import torch
    s = scene
    args, kw = module_args(s, color, device=True)
    want = registration.icp(*args, **kw, levels=3)
    depth = torch.zeros((H, W + 6), dtype=torch.float64, device='cuda')
    depth[:, 3:3 + W] = args[0]
    vertex = torch.zeros((2 * H, W, 3), dtype=torch.float64, device='cuda')
    vertex[::2] = args[4]
    normal = torch.zeros((H, W, 5), dtype=torch.float64, device='cuda')
    normal[..., 1:4] = args[5]
    sargs = (depth[:, 3:3 + W], *args[1:4], vertex[::2], normal[..., 1:4], *args[6:])
    assert not sargs[0].is_contiguous() and not sargs[4].is_contiguous() and not sargs[5].is_contiguous()
    if color:
        flat = torch.zeros(H * W + 3, dtype=torch.float64, device='cuda')
        flat[3:] = kw['model_intensity'].reshape(-1)
        rgb = torch.zeros((H, W, 4), dtype=torch.uint8, device='cuda')
        rgb[..., :3] = kw['color']
        kw = {**kw, 'model_intensity': flat[3:].reshape(H, W), 'color': rgb[..., :3]}
    got = registration.icp(*sargs, **kw, levels=3)
    assert same_bits(got[0].cpu().numpy(), want[0].cpu().numpy()) and same_bits(got[1].cpu().numpy(), want[1].cpu().numpy())
    assert same_bits(got[2]['counts'].cpu().numpy(), want[2]['counts'].cpu().numpy()) and got[2]['status'] == want[2]['status'] == 0
