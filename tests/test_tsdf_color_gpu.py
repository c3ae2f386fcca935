"""The TSDF colour channel on the GPU against its NumPy restatement (tests/tsdf_color_ref.py): tsdf and weight against
tsdf_ref.integrate, the colour state bit for bit (compared as integer views), vertex colours and the coloured flags exactly."""
import ctypes as C

import numpy as np
import pytest

import f3d
import tsdf_ref as R
import tsdf_color_ref as CR
from poison import fill_array, poisoned_empty
from Fusion3DSeg.segUtils import reconstruct, registration

pytestmark = pytest.mark.gpu

DIMS, VS, LO, TRUNC, H, W, MAX_DEPTH = CR.DIMS, CR.VS, CR.LO, CR.TRUNC, CR.H, CR.W, CR.MAX_DEPTH


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


def same_bits(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(bits(got), bits(want))


def same_state(got, want):
    return all(same_bits(g, x) for g, x in zip(got, want)) and len(got) == len(want)


def zeros(dims=DIMS):
    s = tuple(dims[::-1])
    return np.zeros(s, np.float32), np.zeros(s, np.float32), np.zeros(s + (4,), np.float32)


def copies(state):
    return tuple(np.array(a) for a in state)


def images(seed, F, hc, wc):
    return np.random.default_rng(seed).integers(0, 256, (F, hc, wc, 3), dtype=np.uint8)


def raw_depths(depths, dtype, scale):
    with np.errstate(invalid='ignore'):
        raw = depths * scale
        if dtype == np.uint16:
            raw = np.where(np.isfinite(raw), np.clip(np.round(raw), 0, 65535), 0)
        return raw.astype(dtype)


def integrate(ctx, state, lo, depths, rgb, K, q, t, max_weight=64, scale=1.0, max_depth=MAX_DEPTH, vs=VS, trunc=TRUNC):
    """The library's colour entry on `state` in place (host pointers)."""
    h, w = depths.shape[1:]
    ctx.tsdf_integrate_color(*state, lo, vs, trunc, max_weight, depths, rgb, f3d.views_build(K, w, h, q, t, max_depth), scale, max_depth)
    return state


@pytest.fixture(scope='module')
def ctx():
    return f3d.default_context()


@pytest.fixture(scope='module')
def frames():
    K, q, t, depths = CR.base_frames()
    depths.setflags(write=False)
    return K, q, t, depths


@pytest.fixture(scope='module')
def base_rgb():
    rgb = images(1, 5, 150, 180)
    rgb.setflags(write=False)
    return rgb


@pytest.fixture(scope='module')
def base_state(frames, base_rgb):
    """The reference state of the base case (float64 depths, scale 1, 150 x 180 colour images), shared by the tests that start from it."""
    K, q, t, depths = frames
    state = CR.integrate_color(*zeros(), LO, VS, TRUNC, 64, depths, base_rgb, K, q, t, 1.0, MAX_DEPTH)
    for a in state:
        a.setflags(write=False)
    wc = state[2][..., 3]
    assert wc.max() >= 3 and (wc < state[1]).any() and ((wc == 0) & (state[1] > 0)).any()     # clamped samples moved the TSDF alone
    return state


# ------------------------------------------------------------------------------------------------ integrate
@pytest.mark.parametrize('scale', [1.0, 1000.0])
@pytest.mark.parametrize('dtype', [np.float64, np.float32, np.uint16])
@pytest.mark.parametrize('hc,wc', [(40, 48), (80, 96), (150, 180), (7, 5)])
def test_integrate_equals_the_restatement(ctx, frames, hc, wc, dtype, scale):
    K, q, t, depths = frames
    raw, rgb = raw_depths(depths, dtype, scale), images(hc, 5, hc, wc)
    want = CR.integrate_color(*zeros(), LO, VS, TRUNC, 64, raw, rgb, K, q, t, scale, MAX_DEPTH)
    plain = R.integrate(*zeros()[:2], LO, VS, TRUNC, 64, raw, K, q, t, scale, MAX_DEPTH)
    assert same_bits(want[0], plain[0]) and same_bits(want[1], plain[1])
    got = integrate(ctx, zeros(), LO, raw, rgb, K, q, t, scale=scale)
    assert same_bits(got[0], plain[0]) and same_bits(got[1], plain[1])
    assert same_bits(got[2], want[2])
    assert (got[2][..., 3] > 1).any() and not got[2][got[2][..., 3] == 0].any()


@pytest.mark.parametrize('F', [1, 63, 64, 65, 130])
def test_frame_ballot(ctx, F):
    """The ring over a volume of two x tiles, the second partial: more frames than one ballot holds, applied in ascending order."""
    g = R.RING
    K, q, t, depths = R.ring_scene(F)
    rgb = images(F, F, 9, 11)
    want = CR.integrate_color(*zeros(g['dims']), g['lo'], g['vs'], g['trunc'], 64, depths, rgb, K, q, t, 1.0, g['max_depth'])
    got = integrate(ctx, zeros(g['dims']), g['lo'], depths, rgb, K, q, t, max_depth=g['max_depth'], vs=g['vs'], trunc=g['trunc'])
    assert same_state(got, want)
    assert (want[2][..., 3] > 0).sum() > 100
    assert F == 1 or (want[1][:, :, 64:] > 0).any()                     # the second x tile is seen (though never in band)
    if F == 130:
        assert want[2][..., 3].max() == 64                              # the colour weight saturates, too


@pytest.mark.parametrize('dims,lo', [((1, 29, 21), (0.1, -0.7, 0.55)), ((1, 1, 1), (0.5, 0.4, 1.45)), ((130, 3, 2), (-3.2, 0.3, 1.4))])
def test_thin_volumes(ctx, frames, dims, lo):
    K, q, t, depths = frames
    lo, rgb = np.array(lo), images(7, 5, 33, 21)
    want = CR.integrate_color(*zeros(dims), lo, VS, TRUNC, 64, depths, rgb, K, q, t, 1.0, MAX_DEPTH)
    assert want[1].any() and (want[2][..., 3] > 0).any()
    assert same_state(integrate(ctx, zeros(dims), lo, depths, rgb, K, q, t), want)


@pytest.mark.parametrize('max_weight', [3, 64])
def test_prior_state_and_split_calls(ctx, frames, base_rgb, max_weight):
    """From a random prior state (fractional colours; weights 0, max_weight and between): untouched voxels keep their bits, wc
    saturates at max_weight, and two calls over [0, a) and [a, F) equal one call."""
    K, q, t, depths = frames
    rng = np.random.default_rng(17 + max_weight)
    prior = (rng.uniform(-1, 1, DIMS[::-1]).astype(np.float32), rng.integers(0, max_weight + 1, DIMS[::-1]).astype(np.float32),
             CR.random_color_state(rng, DIMS[::-1], max_weight))
    want = CR.integrate_color(*prior, LO, VS, TRUNC, max_weight, depths, base_rgb, K, q, t, 1.0, MAX_DEPTH)
    touched = (bits(want[2]) != bits(prior[2])).any(axis=-1)
    assert touched.any() and not touched.all() and want[2][..., 3].max() == max_weight
    assert ((prior[2][..., 3] == max_weight) & touched).any()           # a saturated weight stays, its colour still moves
    got = integrate(ctx, copies(prior), LO, depths, base_rgb, K, q, t, max_weight=max_weight)
    assert same_state(got, want)
    for a in (1, 2, 4):
        split = copies(prior)
        for part in (slice(0, a), slice(a, 5)):
            integrate(ctx, split, LO, depths[part], base_rgb[part], K, q[part], t[part], max_weight=max_weight)
        assert same_state(split, want)


def test_no_frames_is_a_no_op(ctx, base_state):
    state = copies(base_state)
    ctx.tsdf_integrate_color(*state, LO, VS, TRUNC, 64, np.zeros((0, H, W)), np.zeros((0, 3, 3, 3), np.uint8), np.zeros((0, f3d.VIEW_DOUBLES)), 1.0,
                             MAX_DEPTH)
    assert same_state(state, base_state)


@pytest.fixture(scope='module')
def mixed_state(frames, base_rgb):
    """Depth-only calls between colour calls on one volume: frames 0 and 2 without colour, 4 with, 1 without."""
    K, q, t, depths = frames
    tsdf, weight, color = zeros()
    for sel, with_color in [([0, 2], False), ([4], True), ([1], False)]:
        if with_color:
            tsdf, weight, color = CR.integrate_color(tsdf, weight, color, LO, VS, TRUNC, 64, depths[sel], base_rgb[sel], K, q[sel], t[sel], 1.0, MAX_DEPTH)
        else:
            tsdf, weight = R.integrate(tsdf, weight, LO, VS, TRUNC, 64, depths[sel], K, q[sel], t[sel], 1.0, MAX_DEPTH)
    return tsdf, weight, color


def test_depth_only_frames_between_colour_frames(ctx, frames, base_rgb, mixed_state):
    K, q, t, depths = frames
    state = zeros()
    for sel, with_color in [([0, 2], False), ([4], True), ([1], False)]:
        views = f3d.views_build(K, W, H, q[sel], t[sel], MAX_DEPTH)
        if with_color:
            ctx.tsdf_integrate_color(*state, LO, VS, TRUNC, 64, depths[sel], base_rgb[sel], views, 1.0, MAX_DEPTH)
        else:
            ctx.tsdf_integrate(state[0], state[1], LO, VS, TRUNC, 64, depths[sel], views, 1.0, MAX_DEPTH)
    assert same_state(state, mixed_state)
    rgb, colored = CR.vertex_colors(*mixed_state, 1.0)
    assert (colored == 0).any() and (colored == 1).any() and not rgb[colored == 0].any()
    check_colors(ctx, mixed_state, 1.0)


# ------------------------------------------------------------------------------------------------ vertex colours
def check_colors(ctx, state, min_weight=1.0):
    tsdf, weight, color = copies(state)
    want_v, want_t = R.extract(tsdf, weight, LO, VS, min_weight)
    want_rgb, want_colored = CR.vertex_colors(tsdf, weight, color, min_weight)
    verts, tris, rgb, colored = ctx.tsdf_extract_colors(tsdf, weight, color, LO, VS, min_weight)
    assert same_bits(verts, want_v) and np.array_equal(tris, want_t)
    assert rgb.dtype == np.uint8 and colored.dtype == np.uint8 and rgb.shape == want_rgb.shape and colored.shape == want_colored.shape
    assert np.array_equal(colored, want_colored)
    assert np.array_equal(rgb, want_rgb)
    assert same_state((tsdf, weight, color), state)
    return rgb, colored


def random_state(seed=5):
    rng = np.random.default_rng(seed)
    tsdf = rng.uniform(-1, 1, DIMS[::-1]).astype(np.float32)
    weight = rng.integers(0, 4, DIMS[::-1]).astype(np.float32)
    weight[rng.random(weight.shape) < 0.6] = 3
    return tsdf, weight, CR.random_color_state(rng, DIMS[::-1], 64)


@pytest.mark.parametrize('min_weight', [1.0, 2.0])
def test_vertex_colours_equal_the_restatement(ctx, base_state, min_weight):
    rgb, colored = check_colors(ctx, base_state, min_weight)
    assert len(rgb) > 300 and colored.all() and len(np.unique(rgb)) > 50
    rgb, colored = check_colors(ctx, random_state(), min_weight)        # 11 scan tiles; edges with both, one and no coloured end
    assert len(rgb) > 1000 and (colored == 0).any() and (colored == 1).any()


def test_vertex_colours_without_an_active_cell(ctx):
    state = zeros((6, 5, 4))
    verts, tris, rgb, colored = ctx.tsdf_extract_colors(*state, LO, VS)
    assert rgb.shape == (0, 3) and colored.shape == (0,)


def count(ctx, state):
    nv, nt = C.c_int64(0), C.c_int64(0)
    assert ctx._lib.f3d_tsdf_extract_count(ctx._h, f3d._ptr(state[0]), f3d._ptr(state[1]), *DIMS, 1.0, C.byref(nv), C.byref(nt)) == 0
    return nv.value, nt.value


def colors_call(ctx, color, rgb, colored, dims=DIMS):
    return ctx._lib.f3d_tsdf_extract_colors(ctx._h, f3d._ptr(color), *dims, f3d._ptr(rgb), f3d._ptr(colored))


def test_vertex_colours_in_the_counted_sequence(ctx, base_state):
    """colored = NULL; the colours without a fill, before it and after it; other calls of the context in between; a poison or a
    reserve in between ends the sequence, and the colours ask for the count."""
    state = copies(base_state)
    want_v, want_t = R.extract(state[0], state[1], LO, VS, 1.0)
    want_rgb, want_colored = CR.vertex_colors(*state, 1.0)
    nv, nt = count(ctx, state)
    assert (nv, nt) == (len(want_v), len(want_t))
    rgb, colored = fill_array(np.empty((nv, 3), np.uint8), 0xA5), fill_array(np.empty(nv, np.uint8), 0xA5)
    assert colors_call(ctx, state[2], rgb, None) == 0                   # no fill yet, no flags wanted
    assert np.array_equal(rgb, want_rgb)
    pts = np.random.default_rng(3).uniform(-1, 1, (4000, 3))
    ctx.rotate(pts, [0.9, 0.1, -0.2, 0.3])
    ctx.radius_graph(pts, 0.1)
    small = zeros((5, 4, 3))
    ctx.tsdf_integrate_color(*small, LO, VS, TRUNC, 64, np.ones((1, H, W)), np.zeros((1, 2, 2, 3), np.uint8),
                             f3d.views_build(np.eye(3), W, H, [[1.0, 0, 0, 0]], [[0.0, 0, 0]], 1.0))
    verts, tris = np.empty((nv, 3)), np.empty((nt, 3), np.int32)
    assert colors_call(ctx, state[2], rgb, colored, (36, 29, 21)) == f3d.ERR_INVALID       # other dims
    assert ctx._lib.f3d_tsdf_extract_fill(ctx._h, *DIMS, f3d._ptr(LO), VS, f3d._ptr(verts), f3d._ptr(tris)) == 0
    rgb[...] = 0xA5
    assert colors_call(ctx, state[2], rgb, colored) == 0                # after the fill, with the flags
    assert np.array_equal(rgb, want_rgb) and np.array_equal(colored, want_colored)
    assert same_bits(verts, want_v) and np.array_equal(tris, want_t)
    for a, b in [(None, rgb), (state[2], None)]:
        keep = rgb.copy()
        assert ctx._lib.f3d_tsdf_extract_colors(ctx._h, f3d._ptr(a), *DIMS, f3d._ptr(b), f3d._ptr(colored)) == f3d.ERR_INVALID
        assert np.array_equal(rgb, keep)
    own = f3d.Context(0)
    try:
        for interrupt in (lambda: own.debug_poison(0x5A), lambda: own.reserve_tsdf(4 * state[0].size)):
            count(own, state)
            interrupt()
            rgb[...] = 0xA5
            assert colors_call(own, state[2], rgb, colored) == f3d.ERR_INVALID
            assert (rgb == 0xA5).all()
            count(own, state)
            assert colors_call(own, state[2], rgb, colored) == 0 and np.array_equal(rgb, want_rgb)
        fresh = f3d.Context(0)
        try:
            assert colors_call(fresh, state[2], rgb, colored) == f3d.ERR_INVALID           # never counted
        finally:
            fresh.close()
    finally:
        own.close()


# ------------------------------------------------------------------------------------------------ launch shape, poison
@pytest.mark.parametrize('which', ['tsdf', 'process'])
@pytest.mark.parametrize('cap', [1, 3])
def test_results_do_not_depend_on_the_launch_shape(frames, base_rgb, base_state, which, cap):
    """One and three blocks per launch: the integrate tiles and the vertex-colour loop take dozens of passes over the base volume."""
    K, q, t, depths = frames
    own = f3d.Context(0)
    try:
        own.debug_grid_cap(0)
        own.debug_grid_cap_stats()
        (own.debug_tsdf_grid_cap if which == 'tsdf' else own.debug_grid_cap)(cap)
        try:
            got = integrate(own, zeros(), LO, depths, base_rgb, K, q, t)
            assert same_state(got, base_state)
            for min_weight in (1.0, 3.0):
                check_colors(own, got, min_weight)
        finally:
            own.debug_grid_cap(0)
            own.debug_tsdf_grid_cap(0)
        calls, lowered = own.debug_grid_cap_stats()
        print(f'{which} cap {cap}: {calls} grids sized under the process-wide cap, {lowered} lowered')
        if which == 'process':
            assert calls >= lowered >= 3                                # the integrate launch and the extract launches of two meshes
    finally:
        own.debug_grid_cap(0)
        own.close()


@pytest.mark.parametrize('byte', [0x00, 0xFF, 0x5A])
def test_nothing_depends_on_uninitialised_memory(frames, base_rgb, base_state, byte):
    K, q, t, depths = frames
    own = f3d.Context(0)
    try:
        check_colors(own, random_state(9))                              # the scratch, staging and kept buffers exist and hold other values
        own.debug_poison(byte)
        with poisoned_empty(byte):
            got = integrate(own, zeros(), LO, depths, base_rgb, K, q, t)
        assert same_state(got, base_state)
        own.debug_poison(byte)
        want_rgb, want_colored = CR.vertex_colors(*base_state, 1.0)
        with poisoned_empty(byte):
            _, _, rgb, colored = own.tsdf_extract_colors(*got, LO, VS, 1.0)
        assert np.array_equal(rgb, want_rgb) and np.array_equal(colored, want_colored)
        want_rgb, want_colored = CR.vertex_colors(*random_state(), 1.0)
        own.debug_poison(byte)
        with poisoned_empty(byte):
            _, _, rgb, colored = own.tsdf_extract_colors(*random_state(), LO, VS, 1.0)
        assert np.array_equal(rgb, want_rgb) and np.array_equal(colored, want_colored) and (colored == 0).any()
    finally:
        own.close()


# ------------------------------------------------------------------------------------------------ routes and the context
def test_device_route_equals_host_route(ctx, frames, base_rgb, base_state):
    import torch
    K, q, t, depths = frames
    host = reconstruct.TSDFVolume(LO, DIMS, VS, TRUNC, color=True).integrate(depths, K, q, t, 1.0, MAX_DEPTH, colors=base_rgb)
    assert same_state((host.tsdf, host.weight, host.color), base_state)
    hv, ht, hrgb, hcol = host.extract_mesh(2, colors=True)
    want_rgb, want_colored = CR.vertex_colors(*base_state, 2.0)
    assert np.array_equal(hrgb, want_rgb) and np.array_equal(hcol, want_colored)
    plain = host.extract_mesh(2)
    assert len(plain) == 2 and same_bits(plain[0], hv) and np.array_equal(plain[1], ht)
    dev = reconstruct.TSDFVolume(LO, DIMS, VS, TRUNC, device=True, color=True)
    assert dev.on_device and dev.color.is_cuda and dev.color.shape == DIMS[::-1] + (4,)
    dev.integrate(torch.from_numpy(depths.copy()).cuda(), K, q, t, 1.0, MAX_DEPTH, colors=torch.from_numpy(base_rgb.copy()).cuda())
    assert same_state((dev.tsdf.cpu().numpy(), dev.weight.cpu().numpy(), dev.color.cpu().numpy()), base_state)
    dv, dt, drgb, dcol = dev.extract_mesh(2, colors=True)
    assert drgb.is_cuda and dcol.is_cuda and drgb.dtype == torch.uint8 and dcol.dtype == torch.uint8
    assert same_bits(dv.cpu().numpy(), hv) and np.array_equal(dt.cpu().numpy(), ht)
    assert np.array_equal(drgb.cpu().numpy(), hrgb) and np.array_equal(dcol.cpu().numpy(), hcol)
    fed = reconstruct.TSDFVolume(LO, DIMS, VS, TRUNC, color=True)       # NumPy depths, device colours: the state moves to the device
    fed.integrate(depths, K, q, t, 1.0, MAX_DEPTH, colors=torch.from_numpy(base_rgb.copy()).cuda())
    assert fed.on_device and same_bits(fed.color.cpu().numpy(), base_state[2])
    before = fed.color.clone()
    fed.integrate(depths[:2], K, q[:2], t[:2], 1.0, MAX_DEPTH)          # without colours: the depth-only entry, color untouched
    assert torch.equal(fed.color, before) and not same_bits(fed.weight.cpu().numpy(), base_state[1])
    got = reconstruct.reconstruct_mesh(depths, K, q, t, LO, DIMS, VS, TRUNC, max_depth=MAX_DEPTH, min_weight=2, colors=base_rgb)
    assert len(got) == 4 and same_bits(got[0], hv) and np.array_equal(got[2], hrgb) and np.array_equal(got[3], hcol)


def test_strict_reserved_context_allocates_nothing(frames, base_rgb, base_state):
    import torch
    K, q, t, depths = frames
    own = f3d.Context(0)
    try:
        own.reserve_tsdf(DIMS[0] * DIMS[1] * DIMS[2])
        tsdf, weight = (torch.zeros(DIMS[::-1], dtype=torch.float32, device='cuda') for _ in range(2))
        color = torch.zeros(DIMS[::-1] + (4,), dtype=torch.float32, device='cuda')
        dd, drgb = torch.from_numpy(depths.copy()).cuda(), torch.from_numpy(base_rgb.copy()).cuda()
        dviews = torch.from_numpy(f3d.views_build(K, W, H, q, t, MAX_DEPTH)).cuda()
        torch.cuda.synchronize()
        own.set_strict(True)
        before = own.alloc_count
        own.tsdf_integrate_color_dev(tsdf.data_ptr(), weight.data_ptr(), color.data_ptr(), DIMS, LO, VS, TRUNC, 64, dd.data_ptr(), 0, drgb.data_ptr(), 5,
                                     H, W, 150, 180, 1.0, MAX_DEPTH, dviews.data_ptr())
        nv, nt = own.tsdf_extract_count_dev(tsdf.data_ptr(), weight.data_ptr(), DIMS, 1.0)
        rgb = torch.full((nv, 3), 0xA5, dtype=torch.uint8, device='cuda')
        colored = torch.full((nv,), 0xA5, dtype=torch.uint8, device='cuda')
        own.tsdf_extract_colors_dev(tsdf.data_ptr(), color.data_ptr(), DIMS, rgb.data_ptr(), colored.data_ptr())
        own.synchronize()
        assert own.alloc_count == before
        assert same_state((tsdf.cpu().numpy(), weight.cpu().numpy(), color.cpu().numpy()), base_state)
        want_rgb, want_colored = CR.vertex_colors(*base_state, 1.0)
        assert np.array_equal(rgb.cpu().numpy(), want_rgb) and np.array_equal(colored.cpu().numpy(), want_colored)
        with pytest.raises(ValueError):                                 # a colour state that is not 16-byte aligned
            own.tsdf_extract_colors_dev(tsdf.data_ptr(), color.data_ptr() + 4, DIMS, rgb.data_ptr(), colored.data_ptr())
        with pytest.raises(ValueError):
            own.tsdf_integrate_color_dev(tsdf.data_ptr(), weight.data_ptr(), color.data_ptr() + 8, DIMS, LO, VS, TRUNC, 64, dd.data_ptr(), 0,
                                         drgb.data_ptr(), 5, H, W, 150, 180, 1.0, MAX_DEPTH, dviews.data_ptr())
        own.synchronize()
        assert same_bits(color.cpu().numpy(), base_state[2])
    finally:
        own.close()


# ------------------------------------------------------------------------------------------------ the Python surface
def test_fusion_reconstruct_mesh_with_colours(ctx):
    from fusion_scenes import copy_frames, curved_capture
    from Fusion3DSeg.fusion import Fusion
    h, w = 24, 32
    K, q, t, frames = curved_capture(h, w, 3, 7, quirks=False)
    lo, dims, voxel = np.array([-0.85, -0.8, 0.65]), (44, 38, 31), 0.04     # the capture's box grown by trunc
    fu = Fusion.from_frames(K, w, h, q, t, copy_frames(frames))
    plain = fu.reconstruct_mesh(voxel, lo=lo, dims=dims, max_depth=4.0)
    verts, tris, vc = fu.reconstruct_mesh(voxel, lo=lo, dims=dims, max_depth=4.0, colors=True)
    assert same_bits(verts, plain[0]) and np.array_equal(tris, plain[1]) and len(verts) > 100
    assert vc.dtype == np.float64 and vc.shape == (len(verts), 3) and vc.min() >= 0.0 and vc.max() <= 1.0
    # the restated route: the library's depth images, the colours made bytes by write_triangle_mesh's rule
    pts = np.stack([f[1].reshape(h, w, 3) for f in frames])
    valid = np.stack([f[4].reshape(h, w) for f in frames])
    depths = reconstruct.depth_images(pts, q, t, valid)
    rgb = np.stack([np.round(np.clip(f[3], 0.0, 1.0) * 255.0).astype(np.uint8).reshape(h, w, 3) for f in frames])
    z = tuple(dims[::-1])
    state = CR.integrate_color(np.zeros(z, np.float32), np.zeros(z, np.float32), np.zeros(z + (4,), np.float32), lo, voxel, 4 * voxel, 64, depths, rgb,
                               K, q, t, 1.0, 4.0)
    want_rgb, want_colored = CR.vertex_colors(*state, 1.0)
    assert want_colored.all() and len(np.unique(want_rgb, axis=0)) > 10
    assert np.array_equal(vc, want_rgb.astype(np.float64) / 255.0)
    import torch
    dev_frames = [(n, torch.from_numpy(p).cuda(), torch.from_numpy(nr).cuda(), torch.from_numpy(c).cuda(), torch.from_numpy(v).cuda())
                  for n, p, nr, c, v in copy_frames(frames)]
    dv, dt, dvc = Fusion.from_frames(K, w, h, q, t, dev_frames).reconstruct_mesh(voxel, lo=lo, dims=dims, max_depth=4.0, colors=True)
    assert dvc.is_cuda and dvc.dtype == torch.float64 and same_bits(dv.cpu().numpy(), verts) and np.array_equal(dvc.cpu().numpy(), vc)


def test_track_frames_with_colours(ctx):
    """The poses do not depend on the colours; the colour state is that of the restated loop: each frame integrated, with its
    image, at the pose the tracker took for it."""
    import icp_ref as I
    import torch
    K, q, t, depths = R.scene(I.EYES[:4], [(0.05, -0.02, 1.0)] * 4, I.H, I.W)
    pq, pt = I.tracking_priors(q, t)
    rgb = images(23, 4, 60, 72)
    z = np.zeros(I.DIMS[::-1], np.float32)
    wq, wt, wstatus, wtsdf, wweight = I.track_frames(z, z, I.LO, I.VS, I.TRUNC, 64, depths, K, pq, pt, 1.0, I.MAX_DEPTH)
    state = (z, z, np.zeros(z.shape + (4,), np.float32))
    for f in range(4):
        state = CR.integrate_color(*state, I.LO, I.VS, I.TRUNC, 64, depths[f:f + 1], rgb[f:f + 1], K, wq[f:f + 1], wt[f:f + 1], 1.0, I.MAX_DEPTH)
    assert same_bits(state[0], wtsdf) and same_bits(state[1], wweight)
    vol = reconstruct.TSDFVolume(I.LO, I.DIMS, I.VS, I.TRUNC, color=True)
    gq, gt, status = registration.track_frames(vol, depths, K, pq, pt, max_depth=I.MAX_DEPTH, colors=rgb)
    assert np.array_equal(status, wstatus) and same_bits(gq, wq) and same_bits(gt, wt)
    assert same_state((vol.tsdf, vol.weight, vol.color), state)
    dev = reconstruct.TSDFVolume(I.LO, I.DIMS, I.VS, I.TRUNC, color=True)
    dq, dt, _ = registration.track_frames(dev, depths, K, pq, pt, max_depth=I.MAX_DEPTH, colors=torch.from_numpy(rgb).cuda())
    assert dq.is_cuda and dev.on_device and same_bits(dq.cpu().numpy(), wq) and same_bits(dev.color.cpu().numpy(), state[2])


# ------------------------------------------------------------------------------------------------ bad arguments
def test_library_refuses_bad_arguments(ctx, frames, base_rgb, base_state):
    K, q, t, depths = frames
    views = f3d.views_build(K, W, H, q, t, MAX_DEPTH)
    state = copies(base_state)
    for kw in [dict(voxel=0.0), dict(voxel=np.inf), dict(trunc=0.0), dict(trunc=np.nan), dict(max_weight=0.5), dict(max_weight=2.0 ** 25),
               dict(depth_scale=0.0), dict(max_depth=np.inf)]:
        a = dict(voxel=VS, trunc=TRUNC, max_weight=64, depth_scale=1.0, max_depth=MAX_DEPTH)
        a.update(kw)
        with pytest.raises(ValueError):
            ctx.tsdf_integrate_color(*state, LO, a['voxel'], a['trunc'], a['max_weight'], depths, base_rgb, views, a['depth_scale'], a['max_depth'])
    lib = ctx._lib

    def call(tsdf=state[0], weight=state[1], color=state[2], depth=depths, depth_type=0, rgb=base_rgb, hc=150, wc=180, v=views, lo=LO, nframes=5):
        return lib.f3d_tsdf_integrate_color(ctx._h, f3d._ptr(tsdf), f3d._ptr(weight), f3d._ptr(color), *DIMS, f3d._ptr(lo), VS, TRUNC, 64.0, f3d._ptr(depth),
                                            depth_type, f3d._ptr(rgb), nframes, H, W, hc, wc, 1.0, MAX_DEPTH, f3d._ptr(v))

    for bad in [dict(tsdf=None), dict(weight=None), dict(color=None), dict(depth=None), dict(rgb=None), dict(v=None), dict(lo=None),
                dict(depth_type=3), dict(hc=0), dict(wc=0), dict(hc=-150), dict(wc=-1), dict(hc=1 << 16, wc=1 << 15), dict(nframes=-1)]:
        assert call(**bad) == f3d.ERR_INVALID, bad
    assert same_state(state, base_state)
    assert call(nframes=0, depth=None, rgb=None, v=None) == 0           # no frames: a no-op that needs no frames
    assert same_state(state, base_state)
    assert call() == 0 and not same_bits(state[2], base_state[2])       # and the good call goes through
