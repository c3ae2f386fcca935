"""Registration on the GPU against its NumPy restatement (tests/icp_ref.py): maps, sums, poses, stats and volume states bit for bit
(compared as integer views)."""
import numpy as np
import pytest

import f3d
import icp_ref as I
import tsdf_ref as R
from Fusion3DSeg.segUtils import reconstruct, registration

pytestmark = pytest.mark.gpu

# the base scene of the TSDF tests: five cameras, holes in the depths, a volume no dim of which is a multiple of anything
DIMS, VS, LO, TRUNC = (37, 29, 21), 0.05, np.array([-0.9, -0.7, 0.55]), 0.2
H, W, MAX_DEPTH = 40, 48, 4.0
EYES = [(0.0, 0.0, 0.0), (-0.5, 0.3, 0.8), (1.5, 1.2, 0.9), (0.0, 0.0, -1.0), (0.6, -0.4, 0.3)]
TARGETS = [(0.0, 0.0, 1.0), (0.05, 0.0, 1.2), (1.0, 0.8, 1.7), (0.0, 0.0, -3.0), (0.0, 0.0, 1.1)]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


def same_bits(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(bits(got), bits(want))


@pytest.fixture(scope='module')
def ctx():
    return f3d.default_context()


@pytest.fixture(scope='module')
def base():
    K, q, t, depths = R.scene(EYES, TARGETS, H, W)
    q[4] = 1.3 * q[4]
    depths[0, 5:9, 7:12] = 0.0
    depths[0, 20, 3:30] = np.nan
    depths[1, 11:14, 20:26] = np.inf
    z = np.zeros(DIMS[::-1], np.float32)
    tsdf, weight = R.integrate(z, z, LO, VS, TRUNC, 64, depths, K, q, t, 1.0, MAX_DEPTH)
    for a in (tsdf, weight, q, t):
        a.setflags(write=False)
    return K, q, t, tsdf, weight


def nsteps_for(near, far, step):
    return int(np.floor((far - near) / step)) + 1


def check_raycast(ctx, state, lo, K, q, t, min_weight=1.0, near=0.0, step=VS, h=H, w=W):
    tsdf, weight = state
    n = nsteps_for(near, MAX_DEPTH, step)
    want = I.raycast(tsdf, weight, lo, VS, min_weight, K, q, t, h, w, near, step, n)
    got = ctx.tsdf_raycast(np.array(tsdf), np.array(weight), lo, VS, min_weight, K, q, t, h, w, near, step, n)
    for g, x in zip(got, want):
        assert same_bits(g, x)
    return want


# ------------------------------------------------------------------------------------------------ raycast
@pytest.mark.parametrize('cam,expect', [(0, 'hits'), (1, 'hits'), (3, 'none'), (4, 'hits')])
def test_raycast_equals_the_restatement(ctx, base, cam, expect):
    """In front of the volume, inside it, looking away from it (every pixel NaN) and from the side with an un-normalised quaternion."""
    K, q, t, tsdf, weight = base
    vertex, normal, depth = check_raycast(ctx, (tsdf, weight), LO, K, q[cam], t[cam])
    hit = depth > 0
    if expect == 'none':
        assert not hit.any() and np.isnan(vertex).all() and np.isnan(normal).all()
    else:
        assert hit.sum() > 100 and (~hit).any()
    if cam == 1:
        assert np.all((t[1] > LO) & (t[1] < LO + np.array(DIMS) * VS))


@pytest.mark.parametrize('kw', [dict(min_weight=3.0), dict(step=VS / 2), dict(near=0.93), dict(near=1.2, step=VS / 2, min_weight=2.0)],
                         ids=['holes', 'half-step', 'near-inside', 'all-three'])
def test_raycast_variants(ctx, base, kw):
    """min_weight 3 leaves holes (rays that enter the surface from unobserved space are no hits); steps of half a voxel; a march
    that starts inside the volume, for some rays behind the surface."""
    K, q, t, tsdf, weight = base
    plain = I.raycast(tsdf, weight, LO, VS, 1.0, K, q[0], t[0], H, W, 0.0, VS, nsteps_for(0.0, MAX_DEPTH, VS))
    vertex, normal, depth = check_raycast(ctx, (tsdf, weight), LO, K, q[0], t[0], **kw)
    assert (depth > 0).any() and not same_bits(depth, plain[2])
    if kw.get('near'):
        assert LO[2] < kw['near'] < LO[2] + DIMS[2] * VS


def test_raycast_optional_outputs_and_thin_volume(ctx, base):
    """Each output may be left out; a volume with a dimension of 1 has no cell, so every pixel is NaN."""
    import ctypes as C
    K, q, t, tsdf, weight = base
    n = nsteps_for(0.0, MAX_DEPTH, VS)
    want = I.raycast(tsdf, weight, LO, VS, 1.0, K, q[0], t[0], H, W, 0.0, VS, n)
    T_, W_, Kc, qc, tc = np.array(tsdf), np.array(weight), np.ascontiguousarray(K), np.array(q[0]), np.array(t[0])
    for keep in range(3):
        outs = [np.empty((H * W, 3)), np.empty((H * W, 3)), np.empty(H * W)]
        ptrs = [f3d._ptr(o) if k == keep else None for k, o in enumerate(outs)]
        assert ctx._lib.f3d_tsdf_raycast(ctx._h, f3d._ptr(T_), f3d._ptr(W_), *DIMS, f3d._ptr(LO), VS, 1.0, f3d._ptr(Kc), f3d._ptr(qc), f3d._ptr(tc), H, W,
                                         0.0, VS, n, *ptrs) == 0
        assert same_bits(outs[keep], want[keep])
    for dims in [(37, 29, 1), (1, 29, 21)]:
        state = (np.full(dims[::-1], -0.5, np.float32), np.ones(dims[::-1], np.float32))
        vertex, normal, depth = check_raycast(ctx, state, LO, K, q[0], t[0])
        assert np.isnan(vertex).all() and np.isnan(normal).all() and not depth.any()
    for bad in [dict(vs=0.0), dict(min_weight=0.5), dict(near=-0.1), dict(step=0.0), dict(nsteps=0), dict(q=np.zeros(4)), dict(q=np.array([np.nan, 0, 0, 1]))]:
        a = dict(vs=VS, min_weight=1.0, near=0.0, step=VS, nsteps=n, q=q[0])
        a.update(bad)
        with pytest.raises(ValueError):
            ctx.tsdf_raycast(T_, W_, LO, a['vs'], a['min_weight'], K, a['q'], t[0], H, W, a['near'], a['step'], a['nsteps'])


def test_raycast_with_capped_grids(base):
    """Three blocks per launch: every block marches dozens of tiles, and the maps are the same bits.  An image whose sizes are no
    multiple of the 8 x 8 tile, too."""
    K, q, t, tsdf, weight = base
    own = f3d.Context(0)
    try:
        own.debug_tsdf_grid_cap(3)
        check_raycast(own, (tsdf, weight), LO, K, q[0], t[0])
        K2 = R.intrinsics(37, 43)
        check_raycast(own, (tsdf, weight), LO, K2, q[1], t[1], h=37, w=43)
    finally:
        own.close()


# ------------------------------------------------------------------------------------------------ icp_sums
@pytest.fixture(scope='module')
def scene():
    s = I.icp_scene()
    s['vertex'][3 * W + 5:3 * W + 9] = np.nan                           # holes in the model maps, in either map
    s['normal'][17 * W + 20, 1] = np.nan
    s['vertex'][25 * W + 30, 2] = np.inf
    return s


def source_frame(s, h, w, dtype=np.float64, scale=1.0):
    """Frame 1 of the scene at another image size, with depths that are 0, NaN, inf and beyond max_depth; its pose a little off.  The
    model is frame 0's 40 x 48 maps, so part of the frame projects outside the model image."""
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
    q, t = I.moved(s['q'][1], s['t'][1], (0.2, 0.9, -0.3), 0.7, np.array([0.01, -0.006, 0.008]))
    return K, raw.astype(dtype), q, t


def check_sums(ctx, s, K, depth, q, t, scale=1.0, max_dist=0.1):
    want = I.icp_sums(depth, K, q, t, scale, MAX_DEPTH, s['vertex'], s['normal'], H, W, s['K'], s['q'][0], s['t'][0], max_dist)
    view = f3d.views_build(s['K'], W, H, s['q'][0][None], s['t'][0][None], MAX_DEPTH)
    got = ctx.icp_sums(depth, K, q, t, s['vertex'], s['normal'], H, W, view, max_dist, scale, MAX_DEPTH)
    assert same_bits(got, want)
    return want


@pytest.mark.parametrize('h,w', [(15, 17), (16, 16), (1, 257), (127, 129), (128, 128), (113, 145)])
def test_icp_sums_at_chunk_edges(ctx, scene, h, w):
    """h * w = one chunk of 256 pixels and one pixel either side; 64 chunks and one pixel either side, where lane 0 of the second
    level takes its second item."""
    assert h * w in (255, 256, 257, 16383, 16384, 16385)
    K, depth, q, t = source_frame(scene, h, w)
    tot = check_sums(ctx, scene, K, depth, q, t)
    assert 0.1 * h * w < tot[28] < 0.9 * h * w                          # pairs, and pixels without one: outside the model image, holes, bad depths


@pytest.mark.parametrize('scale', [1.0, 1000.0])
@pytest.mark.parametrize('dtype', [np.float64, np.float32, np.uint16])
def test_icp_sums_depth_types(ctx, scene, dtype, scale):
    if dtype == np.uint16 and scale == 1.0:
        K, depth, q, t = source_frame(scene, 31, 37, dtype, scale)       # whole metres: few pixels survive, the sums still agree
        check_sums(ctx, scene, K, depth, q, t, scale, max_dist=0.6)
        return
    K, depth, q, t = source_frame(scene, 31, 37, dtype, scale)
    assert check_sums(ctx, scene, K, depth, q, t, scale)[28] > 100


def test_icp_sums_without_a_pair(ctx, scene):
    """A frame of zeros, a frame behind the model camera, a frame that looks past the model image: 29 zeros each."""
    s = scene
    K = R.intrinsics(20, 24)
    zeros = np.zeros(f3d.ICP_NSUMS)
    assert same_bits(check_sums(ctx, s, K, np.zeros((20, 24)), s['q'][0], s['t'][0]), zeros)
    behind = R.look_at((0.0, 0.0, -0.2), (0.0, 0.0, -3.0))
    assert same_bits(check_sums(ctx, s, K, np.full((20, 24), 1.0), *behind), zeros)
    aside = R.look_at((0.0, 0.0, 0.0), (3.0, 0.0, 0.3))
    assert same_bits(check_sums(ctx, s, K, np.full((20, 24), 1.0), *aside), zeros)
    assert same_bits(check_sums(ctx, s, K, np.full((20, 24), np.nan), s['q'][0], s['t'][0]), zeros)


# ------------------------------------------------------------------------------------------------ icp
def run_icp(ctx, s, iterations, min_pairs=100):
    view = f3d.views_build(s['K'], W, H, s['q'][0][None], s['t'][0][None], MAX_DEPTH)
    return ctx.icp(s['depths'][0], s['K'], s['q0'], s['t0'], s['vertex'], s['normal'], H, W, view, 0.1, 1.0, MAX_DEPTH, iterations, min_pairs)


def want_icp(s, iterations, min_pairs=100):
    return I.icp(s['depths'][0], s['K'], s['q0'], s['t0'], 1.0, MAX_DEPTH, s['vertex'], s['normal'], H, W, s['K'], s['q'][0], s['t'][0], 0.1, iterations,
                 min_pairs)


@pytest.mark.parametrize('iterations', [1, 10])
def test_icp_equals_the_restatement(ctx, scene, iterations):
    pose, stats, status = run_icp(ctx, scene, iterations)
    want = want_icp(scene, iterations)
    assert status == want[2] == I.OK
    assert same_bits(stats, want[1])
    assert same_bits(pose, want[0])
    again = run_icp(ctx, scene, iterations)                             # two calls give identical bits
    assert same_bits(again[0], pose) and same_bits(again[1], stats) and again[2] == status


def test_icp_lost(ctx, scene):
    """Too few pairs, and a degenerate model (a plane with exact normals: a zero pivot): LOST in round 0, the start pose back unchanged,
    the later rows {0, 0, 1}."""
    pose, stats, status = run_icp(ctx, scene, 3, min_pairs=H * W + 1)
    want = want_icp(scene, 3, min_pairs=H * W + 1)
    assert status == want[2] == I.LOST and same_bits(pose, want[0]) and same_bits(stats, want[1])
    assert same_bits(pose, np.concatenate([scene['q0'], scene['t0']]))
    h, w = 12, 16
    K = R.intrinsics(h, w)
    vv, uu = np.meshgrid(np.arange(h) + 0.5, np.arange(w) + 0.5, indexing='ij')
    vertex = np.stack([(uu - K[0, 2]) * (1.5 / K[0, 0]), (vv - K[1, 2]) * (1.5 / K[1, 1]), np.full((h, w), 1.5)], axis=-1)
    normal = np.broadcast_to(np.array([0.0, 0.0, -1.0]), (h, w, 3)).copy()
    q0, t0, ident = np.array([2.0, 0.0, 0.0, 0.0]), np.array([0.001, -0.002, 0.003]), np.array([1.0, 0.0, 0.0, 0.0])
    depth = np.full((h, w), 1.5)
    want = I.icp(depth, K, q0, t0, 1.0, 10.0, vertex, normal, h, w, K, ident, np.zeros(3), 0.1, 3, 100)
    view = f3d.views_build(K, w, h, ident[None], np.zeros((1, 3)), 10.0)
    pose, stats, status = ctx.icp(depth, K, q0, t0, vertex, normal, h, w, view, 0.1, 1.0, 10.0, 3, 100)
    assert status == want[2] == I.LOST and stats[0, 0] > 100
    assert same_bits(pose, want[0]) and same_bits(stats, want[1]) and same_bits(pose, np.concatenate([q0, t0]))
    for bad in [dict(iterations=0), dict(min_pairs=5)]:
        with pytest.raises(ValueError):
            ctx.icp(depth, K, q0, t0, vertex, normal, h, w, view, 0.1, 1.0, 10.0, **{**dict(iterations=3, min_pairs=100), **bad})
    for bad in [dict(max_dist=0.0), dict(depth_scale=float('inf')), dict(max_depth=-1.0)]:
        with pytest.raises(ValueError):
            ctx.icp_sums(depth, K, q0, t0, vertex, normal, h, w, view, **{**dict(max_dist=0.1, depth_scale=1.0, max_depth=10.0), **bad})
    with pytest.raises(ValueError):
        ctx.icp_sums(depth, K, np.zeros(4), t0, vertex, normal, h, w, view, 0.1)


def test_device_route_equals_the_host_route(ctx, scene):
    import torch
    s = scene
    args = (s['K'], s['q0'], s['t0'])
    model = (s['K'], s['q'][0], s['t'][0])
    mv, mn = s['vertex'].reshape(H, W, 3), s['normal'].reshape(H, W, 3)
    host_sums = registration.icp_sums(s['depths'][0], *args, mv, mn, *model, max_depth=MAX_DEPTH)
    host = registration.icp(s['depths'][0], *args, mv, mn, *model, max_depth=MAX_DEPTH, iterations=4)
    want = want_icp(s, 4)
    assert same_bits(np.concatenate(host[:2]), want[0]) and host[2]['status'] == 0
    assert same_bits(host[2]['counts'], want[1][:, 0]) and same_bits(host[2]['rms'], np.sqrt(want[1][:, 1] / want[1][:, 0]))
    dd, dv, dn = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (s['depths'][0], mv, mn))
    dev_sums = registration.icp_sums(dd, *args, dv, dn, *model, max_depth=MAX_DEPTH)
    dev = registration.icp(dd, *args, dv, dn, *model, max_depth=MAX_DEPTH, iterations=4)
    assert dev_sums.is_cuda and dev[0].is_cuda and dev[1].is_cuda and dev[2]['counts'].is_cuda
    assert same_bits(dev_sums.cpu().numpy(), host_sums)
    assert same_bits(dev[0].cpu().numpy(), host[0]) and same_bits(dev[1].cpu().numpy(), host[1])
    assert same_bits(dev[2]['counts'].cpu().numpy(), host[2]['counts']) and dev[2]['status'] == 0


def test_strict_reserved_context_allocates_nothing(scene):
    import torch
    s = scene
    own = f3d.Context(0)
    try:
        own.reserve_icp(H * W)
        dd, dv, dn = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (s['depths'][0], s['vertex'], s['normal']))
        dview = torch.from_numpy(f3d.views_build(s['K'], W, H, s['q'][0][None], s['t'][0][None], MAX_DEPTH)).cuda()
        pose, stats = torch.empty(7, dtype=torch.float64, device='cuda'), torch.empty((10, 3), dtype=torch.float64, device='cuda')
        sums, status = torch.empty(29, dtype=torch.float64, device='cuda'), torch.empty(1, dtype=torch.int32, device='cuda')
        torch.cuda.synchronize()
        own.set_strict(True)
        before = own.alloc_count
        own.icp_sums_dev(dd.data_ptr(), 0, H, W, s['K'], s['q0'], s['t0'], dv.data_ptr(), dn.data_ptr(), H, W, dview.data_ptr(), 0.1, 1.0, MAX_DEPTH,
                         sums.data_ptr())
        own.icp_dev(dd.data_ptr(), 0, H, W, s['K'], s['q0'], s['t0'], dv.data_ptr(), dn.data_ptr(), H, W, dview.data_ptr(), 0.1, 1.0, MAX_DEPTH, 10, 100,
                    pose.data_ptr(), stats.data_ptr(), status.data_ptr())
        own.synchronize()
        assert own.alloc_count == before
        want = want_icp(s, 10)
        assert same_bits(pose.cpu().numpy(), want[0]) and same_bits(stats.cpu().numpy(), want[1]) and int(status[0]) == want[2]
        assert same_bits(sums.cpu().numpy(), I.icp_sums(s['depths'][0], s['K'], s['q0'], s['t0'], 1.0, MAX_DEPTH, s['vertex'], s['normal'], H, W, s['K'],
                                                        s['q'][0], s['t'][0], 0.1))
        big = torch.zeros((2 * H, 2 * W), dtype=torch.float64, device='cuda')
        with pytest.raises(MemoryError):                               # a larger frame would have to grow the scratch
            own.icp_sums_dev(big.data_ptr(), 0, 2 * H, 2 * W, s['K'], s['q0'], s['t0'], dv.data_ptr(), dn.data_ptr(), H, W, dview.data_ptr(), 0.1, 1.0,
                             MAX_DEPTH, sums.data_ptr())
    finally:
        own.close()


# ------------------------------------------------------------------------------------------------ raycast through the module, track_frames
def test_module_raycast(ctx, scene):
    s = scene
    vol = reconstruct.TSDFVolume(I.LO, I.DIMS, I.VS, I.TRUNC)
    vol.tsdf[...], vol.weight[...] = s['tsdf'], s['weight']
    want = I.raycast(s['tsdf'], s['weight'], I.LO, I.VS, 1.0, s['K'], s['q'][0], s['t'][0], H, W, 0.0, I.VS, nsteps_for(0.0, MAX_DEPTH, I.VS))
    got = registration.raycast(vol, s['K'], s['q'][0], s['t'][0], (H, W), far=MAX_DEPTH)
    assert got[0].shape == (H, W, 3) and got[2].shape == (H, W)
    for g, x in zip(got, want):
        assert same_bits(g.reshape(x.shape), x)
    fed = reconstruct.TSDFVolume(I.LO, I.DIMS, I.VS, I.TRUNC)
    fed.tsdf[...], fed.weight[...] = s['tsdf'], s['weight']
    fed._to_device()
    dev = registration.raycast(fed, s['K'], s['q'][0], s['t'][0], (H, W), far=MAX_DEPTH)
    for g, x in zip(dev, want):
        assert g.is_cuda and same_bits(g.cpu().numpy().reshape(x.shape), x)


@pytest.fixture(scope='module')
def tracked(scene):
    s = scene
    pq, pt = I.tracking_priors(s['q'], s['t'])
    z = np.zeros(I.DIMS[::-1], np.float32)
    return (pq, pt) + I.track_frames(z, z, I.LO, I.VS, I.TRUNC, 64, s['depths'], s['K'], pq, pt, 1.0, MAX_DEPTH)


def test_track_frames_equals_the_restated_loop(ctx, scene, tracked):
    """Six frames 1 - 2 cm and under 1 degree off into an empty volume: poses, status and the final state as the restated loop gives
    them, and refined poses that are better than the priors (the measure and the figures are in test_registration_cpu.py)."""
    s = scene
    pq, pt, wq, wt, wstatus, wtsdf, wweight = tracked
    vol = reconstruct.TSDFVolume(I.LO, I.DIMS, I.VS, I.TRUNC)
    q, t, status = registration.track_frames(vol, s['depths'], s['K'], pq, pt, max_depth=MAX_DEPTH)
    assert status.dtype == np.int32 and np.array_equal(status, wstatus) and (status == 0).all()
    assert same_bits(q, wq) and same_bits(t, wt)
    assert same_bits(vol.tsdf, wtsdf) and same_bits(vol.weight, wweight)
    prior, refined = I.tracking_errors(pq, pt, pq, pt, s['q'], s['t']), I.tracking_errors(pq, pt, q, t, s['q'], s['t'])
    assert refined[0] < prior[0] and refined[1] < prior[1]


def test_track_frames_on_the_device(ctx, scene, tracked):
    import torch
    s = scene
    pq, pt, wq, wt, wstatus, wtsdf, wweight = tracked
    vol = reconstruct.TSDFVolume(I.LO, I.DIMS, I.VS, I.TRUNC)
    q, t, status = registration.track_frames(vol, torch.from_numpy(s['depths']).cuda(), s['K'], pq, pt, max_depth=MAX_DEPTH)
    assert q.is_cuda and t.is_cuda and status.is_cuda and vol.on_device
    assert same_bits(q.cpu().numpy(), wq) and same_bits(t.cpu().numpy(), wt) and np.array_equal(status.cpu().numpy(), wstatus)
    assert same_bits(vol.tsdf.cpu().numpy(), wtsdf) and same_bits(vol.weight.cpu().numpy(), wweight)
    only = reconstruct.TSDFVolume(I.LO, I.DIMS, I.VS, I.TRUNC, device=True)     # integrate=False: only the frame that meets the empty volume
    registration.track_frames(only, s['depths'][:3], s['K'], pq[:3], pt[:3], max_depth=MAX_DEPTH, integrate=False)
    first = R.integrate(np.zeros_like(wtsdf), np.zeros_like(wweight), I.LO, I.VS, I.TRUNC, 64, s['depths'][:1], s['K'], pq[:1], pt[:1], 1.0, MAX_DEPTH)
    assert same_bits(only.tsdf.cpu().numpy(), first[0]) and same_bits(only.weight.cpu().numpy(), first[1])
