"""Colour in registration on the GPU against its NumPy restatement (tests/icp_color_ref.py): the five maps, the 58 sums, poses, stats and
volume states bit for bit (compared as integer views)."""
import numpy as np
import pytest

import f3d
import icp_color_ref as CR
import icp_ref as I
import tsdf_color_ref as C
import tsdf_ref as R
from poison import poisoned_empty
from Fusion3DSeg.segUtils import reconstruct, registration

pytestmark = pytest.mark.gpu

H, W, MAX_DEPTH = I.H, I.W, I.MAX_DEPTH
COLOR_WEIGHT = 0.1                                                       # chosen in test_registration_color_cpu.py
NSTEPS = int(np.floor(MAX_DEPTH / I.VS)) + 1


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


def same_bits(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(bits(got), bits(want))


@pytest.fixture(scope='module')
def ctx():
    return f3d.default_context()


# ------------------------------------------------------------------------------------------------ raycast
@pytest.fixture(scope='module')
def base():
    """The base volume of the TSDF tests (37 x 29 x 21, five cameras, holes in the depths) integrated with random colour bytes."""
    K, q, t, depths = C.base_frames()
    rgb = np.random.default_rng(3).integers(0, 256, (5, C.H, C.W, 3), dtype=np.uint8)
    z = np.zeros(C.DIMS[::-1], np.float32)
    tsdf, weight, color = C.integrate_color(z, z, np.zeros(C.DIMS[::-1] + (4,), np.float32), C.LO, C.VS, C.TRUNC, 64, depths, rgb, K, q, t, 1.0, MAX_DEPTH)
    for a in (tsdf, weight, color, q, t):
        a.setflags(write=False)
    return K, q, t, tsdf, weight, color


def check_raycast(ctx, state, K, q, t, min_weight=1.0, h=H, w=W):
    """The five outputs against the restatement, and the three geometry maps against the depth-only entry."""
    tsdf, weight, color = (np.array(a) for a in state)
    want = CR.raycast_color(tsdf, weight, color, C.LO, C.VS, min_weight, K, q, t, h, w, 0.0, C.VS, NSTEPS)
    got = ctx.tsdf_raycast_color(tsdf, weight, color, C.LO, C.VS, min_weight, K, q, t, h, w, 0.0, C.VS, NSTEPS)
    assert len(got) == 5
    for g, x in zip(got, want):
        assert same_bits(g, x)
    for g, x in zip(got, ctx.tsdf_raycast(tsdf, weight, C.LO, C.VS, min_weight, K, q, t, h, w, 0.0, C.VS, NSTEPS)):
        assert same_bits(g, x)
    return want


@pytest.mark.parametrize('cam,expect', [(0, 'hits'), (1, 'hits'), (3, 'none'), (4, 'hits')])
def test_raycast_color_equals_the_restatement(ctx, base, cam, expect):
    """In front of the volume, inside it, looking away from it (every pixel NaN) and from the side with an un-normalised quaternion."""
    K, q, t, tsdf, weight, color = base
    vertex, normal, depth, rgb, inten = check_raycast(ctx, (tsdf, weight, color), K, q[cam], t[cam])
    hit, seen = depth > 0, np.isfinite(inten)
    assert not (seen & ~hit).any() and np.array_equal(seen, np.isfinite(rgb).all(axis=1))
    if expect == 'none':
        assert not hit.any() and np.isnan(rgb).all() and np.isnan(inten).all()
    else:
        assert seen.sum() > 100 and (~hit).any()
        assert rgb[seen].min() > -1e-9 and rgb[seen].max() < 255.0 + 1e-9 and np.ptp(inten[seen]) > 0.1


def test_raycast_color_with_holes_and_a_random_colour_state(ctx, base):
    """min_weight 3 leaves holes in the geometry; a random colour state with a quarter of its weights 0 leaves hits without colour."""
    K, q, t, tsdf, weight, color = base
    plain = check_raycast(ctx, (tsdf, weight, color), K, q[0], t[0])
    holes = check_raycast(ctx, (tsdf, weight, color), K, q[0], t[0], min_weight=3.0)
    assert (holes[2] > 0).any() and not same_bits(holes[2], plain[2])
    state = C.random_color_state(np.random.default_rng(11), C.DIMS[::-1], 64)
    assert (state[..., 3] == 0).mean() > 0.2
    vertex, normal, depth, rgb, inten = check_raycast(ctx, (tsdf, weight, state), K, q[0], t[0])
    hit = depth > 0
    assert (hit & np.isnan(inten)).sum() > 100 and (hit & np.isfinite(inten)).sum() > 10
    K2 = R.intrinsics(37, 43)                                           # sizes that are no multiple of the 8 x 8 tile
    check_raycast(ctx, (tsdf, weight, state), K2, q[1], t[1], h=37, w=43)


def test_raycast_color_optional_outputs(ctx, base):
    """Each of the five outputs left NULL in turn: the other four are written, with the same bits; all five NULL is a no-op."""
    K, q, t, tsdf, weight, color = base
    want = CR.raycast_color(tsdf, weight, color, C.LO, C.VS, 1.0, K, q[0], t[0], H, W, 0.0, C.VS, NSTEPS)
    T_, W_, C_, Kc, qc, tc = np.array(tsdf), np.array(weight), np.array(color), np.ascontiguousarray(K), np.array(q[0]), np.array(t[0])

    def call(ptrs):
        return ctx._lib.f3d_tsdf_raycast_color(ctx._h, f3d._ptr(T_), f3d._ptr(W_), f3d._ptr(C_), *C.DIMS, f3d._ptr(C.LO), C.VS, 1.0, f3d._ptr(Kc),
                                               f3d._ptr(qc), f3d._ptr(tc), H, W, 0.0, C.VS, NSTEPS, *ptrs)
    for skip in range(5):
        outs = [np.full(x.shape, 7.0) for x in want]
        assert call([None if k == skip else f3d._ptr(o) for k, o in enumerate(outs)]) == 0
        for k in range(5):
            assert (outs[k] == 7.0).all() if k == skip else same_bits(outs[k], want[k])
    assert call([None] * 5) == 0
    assert ctx._lib.f3d_tsdf_raycast_color(ctx._h, f3d._ptr(T_), f3d._ptr(W_), None, *C.DIMS, f3d._ptr(C.LO), C.VS, 1.0, f3d._ptr(Kc), f3d._ptr(qc),
                                           f3d._ptr(tc), H, W, 0.0, C.VS, NSTEPS, *[None] * 5) == f3d.ERR_INVALID


# ------------------------------------------------------------------------------------------------ the 58 sums
@pytest.fixture(scope='module')
def scene():
    s = CR.color_scene()
    s['vertex'][3 * W + 5:3 * W + 9] = np.nan                           # holes in the model maps, in any of the three
    s['normal'][17 * W + 20, 1] = np.nan
    s['vertex'][25 * W + 30, 2] = np.inf
    s['intensity'][12 * W + 10:12 * W + 30:3] = np.nan
    s['intensity'][30 * W + 7] = np.inf
    s['view'] = f3d.views_build(s['K'], W, H, s['q'][0][None], s['t'][0][None], MAX_DEPTH)
    return s


def source_frame(s, h, w, dtype=np.float64, scale=1.0, hc=H, wc=W):
    """Frame 1 of the scene at another image size, with depths that are 0, NaN, inf and beyond max_depth, its pose a little off, and
    its colour image at a third size.  The model is frame 0's 40 x 48 maps, so part of the frame projects outside the model image."""
    K = R.intrinsics(h, w)
    depth = R.cast_depth(K, s['q'][1], s['t'][1], h, w)
    flat = depth.reshape(-1)
    flat[3::41] = 0.0
    flat[7::53] = 50.0
    if dtype != np.uint16:
        flat[11::67] = np.nan
        flat[13::71] = np.inf
    with np.errstate(invalid='ignore'):
        raw = depth * scale
        if dtype == np.uint16:
            raw = np.clip(np.round(raw), 0, 65535)
    Kc = R.intrinsics(hc, wc)
    rgb = CR.textured_images(Kc, s['q'][1][None], s['t'][1][None], R.cast_depth(Kc, s['q'][1], s['t'][1], hc, wc)[None])[0]
    q, t = I.moved(s['q'][1], s['t'][1], (0.2, 0.9, -0.3), 0.7, np.array([0.01, -0.006, 0.008]))
    return K, raw.astype(dtype), rgb, q, t


def check_sums(ctx, s, K, depth, rgb, q, t, scale=1.0, max_dist=0.1, intensity=None):
    mi = s['intensity'] if intensity is None else intensity
    want = CR.icp_color_sums(depth, rgb, K, q, t, scale, MAX_DEPTH, s['vertex'], s['normal'], mi, H, W, s['K'], s['q'][0], s['t'][0], max_dist)
    got = ctx.icp_color_sums(depth, K, q, t, s['vertex'], s['normal'], H, W, s['view'], max_dist, mi, rgb, COLOR_WEIGHT, scale, MAX_DEPTH)
    assert got.shape == (f3d.ICP_NSUMS_COLOR,) and same_bits(got, want)
    assert same_bits(got[:29], ctx.icp_sums(depth, K, q, t, s['vertex'], s['normal'], H, W, s['view'], max_dist, scale, MAX_DEPTH))
    return want


@pytest.mark.parametrize('h,w', [(15, 17), (16, 16), (1, 257), (127, 129), (128, 128), (113, 145)])
def test_color_sums_at_chunk_edges(ctx, scene, h, w):
    """h * w = one chunk of 256 pixels and one pixel either side; 64 chunks and one pixel either side, where lane 0 of the second
    level takes its second item."""
    assert h * w in (255, 256, 257, 16383, 16384, 16385)
    K, depth, rgb, q, t = source_frame(scene, h, w)
    tot = check_sums(ctx, scene, K, depth, rgb, q, t)
    assert 0.1 * h * w < tot[29 + 28] < tot[28] < 0.9 * h * w            # pairs; geometric pairs without a photometric one; pixels without either


@pytest.mark.parametrize('hc,wc', [(40, 48), (80, 96), (7, 5)])
def test_color_sums_colour_image_sizes(ctx, scene, hc, wc):
    K, depth, rgb, q, t = source_frame(scene, 31, 37, hc=hc, wc=wc)
    assert rgb.shape == (hc, wc, 3)
    assert check_sums(ctx, scene, K, depth, rgb, q, t)[29 + 28] > 100


@pytest.mark.parametrize('dtype,scale', [(np.float64, 1.0), (np.float32, 1.0), (np.uint16, 1000.0)])
def test_color_sums_depth_types(ctx, scene, dtype, scale):
    K, depth, rgb, q, t = source_frame(scene, 31, 37, dtype, scale)
    assert check_sums(ctx, scene, K, depth, rgb, q, t, scale)[29 + 28] > 100


def test_color_sums_without_a_pair(ctx, scene):
    """A model without intensity: 29 geometric sums and 29 zeros.  A frame of zeros, one behind the model camera, one of NaN: 58 zeros."""
    s = scene
    K, depth, rgb, q, t = source_frame(s, 31, 37)
    tot = check_sums(ctx, s, K, depth, rgb, q, t, intensity=np.full(H * W, np.nan))
    assert tot[28] > 100 and same_bits(tot[29:], np.zeros(29))
    K = R.intrinsics(20, 24)
    zeros, rgb = np.zeros(f3d.ICP_NSUMS_COLOR), np.full((20, 24, 3), 90, np.uint8)
    assert same_bits(check_sums(ctx, s, K, np.zeros((20, 24)), rgb, s['q'][0], s['t'][0]), zeros)
    behind = R.look_at((0.0, 0.0, -0.2), (0.0, 0.0, -3.0))
    assert same_bits(check_sums(ctx, s, K, np.full((20, 24), 1.0), rgb, *behind), zeros)
    assert same_bits(check_sums(ctx, s, K, np.full((20, 24), np.nan), rgb, s['q'][0], s['t'][0]), zeros)


# ------------------------------------------------------------------------------------------------ icp_color
def run_icp(ctx, s, iterations, color_weight, min_pairs=100):
    return ctx.icp_color(s['depths'][0], s['K'], s['q0'], s['t0'], s['vertex'], s['normal'], H, W, s['view'], 0.1, s['intensity'], s['rgbs'][0],
                         color_weight, 1.0, MAX_DEPTH, iterations, min_pairs)


def want_icp(s, iterations, color_weight, min_pairs=100):
    return CR.icp_color(s['depths'][0], s['rgbs'][0], s['K'], s['q0'], s['t0'], 1.0, MAX_DEPTH, s['vertex'], s['normal'], s['intensity'], H, W, s['K'],
                        s['q'][0], s['t'][0], 0.1, color_weight, iterations, min_pairs)


@pytest.fixture(scope='module')
def wanted(scene):
    return {(n, cw): want_icp(scene, n, cw) for n in (1, 10) for cw in (0.0, COLOR_WEIGHT)}


@pytest.mark.parametrize('color_weight', [0.0, COLOR_WEIGHT])
@pytest.mark.parametrize('iterations', [1, 10])
def test_icp_color_equals_the_restatement(ctx, scene, wanted, iterations, color_weight):
    pose, stats, status = run_icp(ctx, scene, iterations, color_weight)
    want = wanted[iterations, color_weight]
    assert status == want[2] == I.OK and stats.shape == (iterations, 5)
    assert same_bits(stats, want[1])
    assert same_bits(pose, want[0])
    again = run_icp(ctx, scene, iterations, color_weight)               # two calls give identical bits
    assert same_bits(again[0], pose) and same_bits(again[1], stats) and again[2] == status
    if color_weight == 0.0:                                             # the depth-only entry's pose and stats, up to the sign of a zero
        s = scene
        plain = ctx.icp(s['depths'][0], s['K'], s['q0'], s['t0'], s['vertex'], s['normal'], H, W, s['view'], 0.1, 1.0, MAX_DEPTH, iterations, 100)
        assert np.array_equal(plain[0], pose) and np.array_equal(plain[1], stats[:, :3]) and plain[2] == status
    else:
        assert not same_bits(pose, wanted[iterations, 0.0][0])


def test_icp_color_lost(ctx, scene):
    """Too few geometric pairs, and a degenerate model (a plane with exact normals and one intensity everywhere: Jc is zero, so the
    weighted system has the depth-only one's zero pivot): LOST in round 0, the start pose back unchanged, the later rows {0, 0, 1, 0, 0}."""
    pose, stats, status = run_icp(ctx, scene, 3, COLOR_WEIGHT, min_pairs=H * W + 1)
    want = want_icp(scene, 3, COLOR_WEIGHT, min_pairs=H * W + 1)
    assert status == want[2] == I.LOST and same_bits(pose, want[0]) and same_bits(stats, want[1])
    assert same_bits(pose, np.concatenate([scene['q0'], scene['t0']])) and stats[0, 3] > 100
    assert np.array_equal(stats[1:], [[0.0, 0.0, 1.0, 0.0, 0.0]] * 2)
    h, w = 12, 16
    K = R.intrinsics(h, w)
    vv, uu = np.meshgrid(np.arange(h) + 0.5, np.arange(w) + 0.5, indexing='ij')
    vertex = np.stack([(uu - K[0, 2]) * (1.5 / K[0, 0]), (vv - K[1, 2]) * (1.5 / K[1, 1]), np.full((h, w), 1.5)], axis=-1)
    normal = np.broadcast_to(np.array([0.0, 0.0, -1.0]), (h, w, 3)).copy()
    inten, rgb = np.full(h * w, 0.5), np.full((h, w, 3), 128, np.uint8)
    q0, t0, ident = np.array([2.0, 0.0, 0.0, 0.0]), np.array([0.001, -0.002, 0.003]), np.array([1.0, 0.0, 0.0, 0.0])
    depth = np.full((h, w), 1.5)
    want = CR.icp_color(depth, rgb, K, q0, t0, 1.0, 10.0, vertex, normal, inten, h, w, K, ident, np.zeros(3), 0.1, COLOR_WEIGHT, 3, 100)
    view = f3d.views_build(K, w, h, ident[None], np.zeros((1, 3)), 10.0)
    pose, stats, status = ctx.icp_color(depth, K, q0, t0, vertex, normal, h, w, view, 0.1, inten, rgb, COLOR_WEIGHT, 1.0, 10.0, 3, 100)
    assert status == want[2] == I.LOST and stats[0, 0] > 100 and stats[0, 3] > 50
    assert same_bits(pose, want[0]) and same_bits(stats, want[1]) and same_bits(pose, np.concatenate([q0, t0]))
    for bad in [dict(color_weight=-1.0), dict(color_weight=float('nan')), dict(iterations=0), dict(min_pairs=5)]:
        a = {**dict(color_weight=COLOR_WEIGHT, iterations=3, min_pairs=100), **bad}
        with pytest.raises(ValueError):
            ctx.icp_color(depth, K, q0, t0, vertex, normal, h, w, view, 0.1, inten, rgb, a['color_weight'], 1.0, 10.0, a['iterations'], a['min_pairs'])
    with pytest.raises(ValueError):
        ctx.icp_color_sums(depth, K, q0, t0, vertex, normal, h, w, view, 0.0, inten, rgb, COLOR_WEIGHT)


def test_device_route_equals_the_host_route(ctx, scene, wanted):
    import torch
    s = scene
    args = (s['K'], s['q0'], s['t0'])
    model = (s['K'], s['q'][0], s['t'][0])
    mv, mn, mi = s['vertex'].reshape(H, W, 3), s['normal'].reshape(H, W, 3), s['intensity'].reshape(H, W)
    col = dict(color=s['rgbs'][0], model_intensity=mi, color_weight=COLOR_WEIGHT)
    host_sums = registration.icp_sums(s['depths'][0], *args, mv, mn, *model, max_depth=MAX_DEPTH, **col)
    host = registration.icp(s['depths'][0], *args, mv, mn, *model, max_depth=MAX_DEPTH, iterations=10, **col)
    want = wanted[10, COLOR_WEIGHT]
    assert host_sums.shape == (58,) and same_bits(np.concatenate(host[:2]), want[0]) and host[2]['status'] == 0
    assert same_bits(host[2]['counts'], want[1][:, 0]) and same_bits(host[2]['color_counts'], want[1][:, 3])
    assert same_bits(host[2]['color_rms'], np.sqrt(want[1][:, 4] / want[1][:, 3]))
    dd, dv, dn, di, drgb = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (s['depths'][0], mv, mn, mi, s['rgbs'][0]))
    dcol = dict(color=drgb, model_intensity=di, color_weight=COLOR_WEIGHT)
    dev_sums = registration.icp_sums(dd, *args, dv, dn, *model, max_depth=MAX_DEPTH, **dcol)
    dev = registration.icp(dd, *args, dv, dn, *model, max_depth=MAX_DEPTH, iterations=10, **dcol)
    assert dev_sums.is_cuda and dev[0].is_cuda and dev[1].is_cuda and dev[2]['color_counts'].is_cuda
    assert same_bits(dev_sums.cpu().numpy(), host_sums)
    assert same_bits(dev[0].cpu().numpy(), host[0]) and same_bits(dev[1].cpu().numpy(), host[1])
    assert same_bits(dev[2]['color_counts'].cpu().numpy(), host[2]['color_counts']) and dev[2]['status'] == 0
    mixed = registration.icp(s['depths'][0], *args, mv, mn, *model, max_depth=MAX_DEPTH, iterations=10, **{**col, 'color': drgb})   # one device array
    assert mixed[0].is_cuda and same_bits(mixed[0].cpu().numpy(), host[0])
    # none of the three: today's path
    plain = registration.icp(s['depths'][0], *args, mv, mn, *model, max_depth=MAX_DEPTH, iterations=4)
    assert 'color_counts' not in plain[2] and registration.icp_sums(s['depths'][0], *args, mv, mn, *model, max_depth=MAX_DEPTH).shape == (29,)


# ------------------------------------------------------------------------------------------------ launch shapes, poison, strict
@pytest.fixture(scope='module')
def frame64(scene):
    """A 64 x 72 source frame (18 chunks, 5 blocks of the terms kernel) and what the restatement gives for it."""
    s = scene
    K, depth, rgb, q, t = source_frame(s, 64, 72)
    model = (s['vertex'], s['normal'], s['intensity'], H, W, s['K'], s['q'][0], s['t'][0], 0.1)
    sums = CR.icp_color_sums(depth, rgb, K, q, t, 1.0, MAX_DEPTH, *model)
    icp = CR.icp_color(depth, rgb, K, q, t, 1.0, MAX_DEPTH, *model, COLOR_WEIGHT, 4, 100)
    return K, depth, rgb, q, t, sums, icp


def check_frame64(own, s, frame64):
    K, depth, rgb, q, t, sums, icp = frame64
    args = (depth, K, q, t, s['vertex'], s['normal'], H, W, s['view'], 0.1, s['intensity'], rgb, COLOR_WEIGHT, 1.0, MAX_DEPTH)
    assert same_bits(own.icp_color_sums(*args), sums)
    pose, stats, status = own.icp_color(*args, 4, 100)
    assert status == icp[2] == I.OK and same_bits(pose, icp[0]) and same_bits(stats, icp[1])


@pytest.mark.parametrize('cap', [1, 3])
def test_results_do_not_depend_on_the_launch_shape(scene, frame64, base, cap):
    """One and three blocks per launch: the terms kernel walks its 18 chunks in several passes, the raycast its 30 tiles."""
    K, q, t, tsdf, weight, color = base
    own = f3d.Context(0)
    try:
        own.debug_grid_cap(0)
        own.debug_grid_cap_stats()
        own.debug_grid_cap(cap)
        try:
            check_frame64(own, scene, frame64)
            check_raycast(own, (tsdf, weight, color), K, q[0], t[0])
        finally:
            own.debug_grid_cap(0)
        calls, lowered = own.debug_grid_cap_stats()
        print(f'cap {cap}: {calls} grids sized under the process-wide cap, {lowered} lowered')
        assert calls >= lowered >= 7                                    # 1 + 4 terms launches and two raycasts
        own.debug_tsdf_grid_cap(cap)                                    # the TSDF hook caps the raycast, too
        check_raycast(own, (tsdf, weight, color), K, q[1], t[1])
    finally:
        own.debug_grid_cap(0)
        own.close()


@pytest.mark.parametrize('byte', [0x00, 0xFF, 0x5A])
def test_nothing_depends_on_uninitialised_memory(scene, frame64, base, byte):
    K, q, t, tsdf, weight, color = base
    own = f3d.Context(0)
    try:
        check_frame64(own, scene, frame64)                              # the scratch and staging buffers exist and hold other values
        own.debug_poison(byte)
        with poisoned_empty(byte):
            check_frame64(own, scene, frame64)
        own.debug_poison(byte)
        with poisoned_empty(byte):
            check_raycast(own, (tsdf, weight, color), K, q[0], t[0])
    finally:
        own.close()


def test_strict_reserved_context_allocates_nothing(scene, wanted):
    import torch
    s = scene
    own = f3d.Context(0)
    try:
        own.reserve_icp_color(H * W)
        cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()     # noqa: E731
        dd, dv, dn, di, drgb = (cuda(a) for a in (s['depths'][0], s['vertex'], s['normal'], s['intensity'], s['rgbs'][0]))
        dview = cuda(s['view'])
        dt, dw, dc = cuda(s['tsdf']), cuda(s['weight']), cuda(s['color'])
        empty = lambda *shape: torch.empty(shape, dtype=torch.float64, device='cuda')     # noqa: E731
        pose, stats, sums, plain = empty(7), empty(10, 5), empty(58), empty(29)
        status = torch.empty(1, dtype=torch.int32, device='cuda')
        maps = [empty(H * W, 3), empty(H * W, 3), empty(H * W), empty(H * W, 3), empty(H * W)]
        torch.cuda.synchronize()
        own.set_strict(True)
        before = own.alloc_count
        ray = (I.DIMS, I.LO, I.VS, 1.0, s['K'], s['q'][0], s['t'][0], H, W, 0.0, I.VS, NSTEPS)
        own.tsdf_raycast_color_dev(dt.data_ptr(), dw.data_ptr(), dc.data_ptr(), *ray, *(m.data_ptr() for m in maps))
        icp = (dd.data_ptr(), 0, H, W, s['K'], s['q0'], s['t0'], dv.data_ptr(), dn.data_ptr(), H, W, dview.data_ptr(), 0.1)
        col = (di.data_ptr(), drgb.data_ptr(), H, W, COLOR_WEIGHT, 1.0, MAX_DEPTH)
        own.icp_color_sums_dev(*icp, *col, sums.data_ptr())
        own.icp_color_dev(*icp, *col, 10, 100, pose.data_ptr(), stats.data_ptr(), status.data_ptr())
        own.icp_sums_dev(*icp, 1.0, MAX_DEPTH, plain.data_ptr())         # the reserve covers the 29-sum entries
        own.synchronize()
        assert own.alloc_count == before
        want = wanted[10, COLOR_WEIGHT]
        assert same_bits(pose.cpu().numpy(), want[0]) and same_bits(stats.cpu().numpy(), want[1]) and int(status[0]) == want[2]
        assert same_bits(sums.cpu().numpy()[:29], plain.cpu().numpy()) and same_bits(sums.cpu().numpy()[56:], want[1][0, [4, 3]])
        clean = CR.color_scene()                                        # the maps before the fixture's holes
        for m, x in zip(maps, (clean['vertex'], clean['normal'], clean['depth'], clean['rgb'], clean['intensity'])):
            assert same_bits(m.cpu().numpy(), x)
        with pytest.raises(ValueError):                                 # a colour state that is not 16-byte aligned
            own.tsdf_raycast_color_dev(dt.data_ptr(), dw.data_ptr(), dc.data_ptr() + 8, *ray, *(m.data_ptr() for m in maps))
        big = torch.zeros((2 * H, 2 * W), dtype=torch.float64, device='cuda')
        with pytest.raises(MemoryError):                                # a larger frame would have to grow the scratch
            own.icp_color_sums_dev(big.data_ptr(), 0, 2 * H, 2 * W, *icp[4:], *col, sums.data_ptr())
    finally:
        own.close()


# ------------------------------------------------------------------------------------------------ raycast through the module, track_frames
def colour_volume(s, device=False):
    vol = reconstruct.TSDFVolume(I.LO, I.DIMS, I.VS, I.TRUNC, color=True)
    vol.tsdf[...], vol.weight[...], vol.color[...] = s['tsdf'], s['weight'], s['color']
    if device:
        vol._to_device()
    return vol


def test_module_raycast_with_colours(ctx, scene):
    s = scene
    want = CR.raycast_color(s['tsdf'], s['weight'], s['color'], I.LO, I.VS, 1.0, s['K'], s['q'][0], s['t'][0], H, W, 0.0, I.VS, NSTEPS)
    got = registration.raycast(colour_volume(s), s['K'], s['q'][0], s['t'][0], (H, W), far=MAX_DEPTH, colors=True)
    assert len(got) == 5 and got[3].shape == (H, W, 3) and got[4].shape == (H, W)
    for g, x in zip(got, want):
        assert same_bits(g.reshape(x.shape), x)
    dev = registration.raycast(colour_volume(s, device=True), s['K'], s['q'][0], s['t'][0], (H, W), far=MAX_DEPTH, colors=True)
    for g, x in zip(dev, want):
        assert g.is_cuda and same_bits(g.cpu().numpy().reshape(x.shape), x)
    assert len(registration.raycast(colour_volume(s), s['K'], s['q'][0], s['t'][0], (H, W), far=MAX_DEPTH)) == 3
    with pytest.raises(ValueError):
        registration.raycast(reconstruct.TSDFVolume(I.LO, I.DIMS, I.VS, I.TRUNC), s['K'], s['q'][0], s['t'][0], (H, W), colors=True)


@pytest.fixture(scope='module')
def tracked(scene):
    s = scene
    pq, pt = I.tracking_priors(s['q'], s['t'])
    z, zc = np.zeros(I.DIMS[::-1], np.float32), np.zeros(I.DIMS[::-1] + (4,), np.float32)
    return (pq, pt) + CR.track_frames_color(z, z, zc, I.LO, I.VS, I.TRUNC, 64, s['depths'], s['rgbs'], s['K'], pq, pt, COLOR_WEIGHT, 1.0, MAX_DEPTH)


def test_track_frames_with_colour_equals_the_restated_loop(ctx, scene, tracked):
    """Six frames 1 - 2 cm and under 1 degree off into an empty colour volume: poses, status and the final state as the restated loop
    gives them (what the colour term buys is measured in test_registration_color_cpu.py)."""
    s = scene
    pq, pt, wq, wt, wstatus, wtsdf, wweight, wcolor = tracked
    vol = reconstruct.TSDFVolume(I.LO, I.DIMS, I.VS, I.TRUNC, color=True)
    q, t, status = registration.track_frames(vol, s['depths'], s['K'], pq, pt, max_depth=MAX_DEPTH, colors=s['rgbs'], color_weight=COLOR_WEIGHT)
    assert status.dtype == np.int32 and np.array_equal(status, wstatus) and (status == 0).all()
    assert same_bits(q, wq) and same_bits(t, wt)
    assert same_bits(vol.tsdf, wtsdf) and same_bits(vol.weight, wweight) and same_bits(vol.color, wcolor)


def test_track_frames_with_colour_on_the_device(ctx, scene, tracked):
    import torch
    s = scene
    pq, pt, wq, wt, wstatus, wtsdf, wweight, wcolor = tracked
    vol = reconstruct.TSDFVolume(I.LO, I.DIMS, I.VS, I.TRUNC, color=True)
    q, t, status = registration.track_frames(vol, torch.from_numpy(s['depths']).cuda(), s['K'], pq, pt, max_depth=MAX_DEPTH,
                                             colors=torch.from_numpy(s['rgbs']).cuda(), color_weight=COLOR_WEIGHT)
    assert q.is_cuda and t.is_cuda and status.is_cuda and vol.on_device
    assert same_bits(q.cpu().numpy(), wq) and same_bits(t.cpu().numpy(), wt) and np.array_equal(status.cpu().numpy(), wstatus)
    assert same_bits(vol.tsdf.cpu().numpy(), wtsdf) and same_bits(vol.weight.cpu().numpy(), wweight) and same_bits(vol.color.cpu().numpy(), wcolor)


def test_track_frames_without_a_weight_is_todays(ctx, scene, tracked):
    """color_weight=None: the depth-only alignment, the images only integrated: the poses of icp_ref.track_frames, the state of
    integrating at them; and not the colour loop's poses."""
    s = scene
    pq, pt = tracked[:2]
    z = np.zeros(I.DIMS[::-1], np.float32)
    wq, wt, wstatus, wtsdf, wweight = I.track_frames(z, z, I.LO, I.VS, I.TRUNC, 64, s['depths'], s['K'], pq, pt, 1.0, MAX_DEPTH)
    vol = reconstruct.TSDFVolume(I.LO, I.DIMS, I.VS, I.TRUNC, color=True)
    q, t, status = registration.track_frames(vol, s['depths'], s['K'], pq, pt, max_depth=MAX_DEPTH, colors=s['rgbs'])
    assert same_bits(q, wq) and same_bits(t, wt) and np.array_equal(status, wstatus)
    assert same_bits(vol.tsdf, wtsdf) and same_bits(vol.weight, wweight) and not same_bits(q, tracked[2])
    wcolor = C.integrate_color(z, z, np.zeros(I.DIMS[::-1] + (4,), np.float32), I.LO, I.VS, I.TRUNC, 64, s['depths'], s['rgbs'], s['K'], wq, wt, 1.0,
                               MAX_DEPTH)[2]
    assert same_bits(vol.color, wcolor)
    bare = reconstruct.TSDFVolume(I.LO, I.DIMS, I.VS, I.TRUNC)
    q2, t2, _ = registration.track_frames(bare, s['depths'], s['K'], pq, pt, max_depth=MAX_DEPTH)
    assert same_bits(q2, wq) and same_bits(t2, wt)
