"""TSDF reconstruction on the GPU against its NumPy restatement (tests/tsdf_ref.py): tsdf, weight and vertices bit for bit (compared
as integer views), triangles and counts exactly."""
import ctypes as C

import numpy as np
import pytest

import f3d
import tsdf_ref as R
from Fusion3DSeg.segUtils import reconstruct

pytestmark = pytest.mark.gpu

DIMS, VS, LO, TRUNC = (37, 29, 21), 0.05, np.array([-0.9, -0.7, 0.55]), 0.2      # no dim is a multiple of a wave (64) or of the 4 rows of a block
H, W, MAX_DEPTH = 40, 48, 4.0
# camera 0 in front of the volume, 1 inside it, 2 sees only its far corner, 3 looks away from it, 4 from the side with an unnormalised quaternion
EYES = [(0.0, 0.0, 0.0), (-0.5, 0.3, 0.8), (1.5, 1.2, 0.9), (0.0, 0.0, -1.0), (0.6, -0.4, 0.3)]
TARGETS = [(0.0, 0.0, 1.0), (0.05, 0.0, 1.2), (1.0, 0.8, 1.7), (0.0, 0.0, -3.0), (0.0, 0.0, 1.1)]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


def same_bits(got, want):
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(bits(got), bits(want))


def zeros(dims=DIMS):
    return np.zeros(dims[::-1], np.float32), np.zeros(dims[::-1], np.float32)


@pytest.fixture(scope='module')
def ctx():
    return f3d.default_context()


@pytest.fixture(scope='module')
def frames():
    """The sphere-and-wall scene from the five poses, with holes: 0, NaN, +inf and depths beyond max_depth."""
    K, q, t, depths = R.scene(EYES, TARGETS, H, W)
    q[4] = 1.3 * q[4]
    depths[0, 5:9, 7:12] = 0.0
    depths[0, 20, 3:30] = np.nan
    depths[1, 11:14, 20:26] = np.inf
    depths[4, 30:34, 10:20] = 50.0
    depths[1, 0, 0] = -1.0
    depths.setflags(write=False)
    return K, q, t, depths


def in_image(K, q, t):
    """per voxel: projects into the image of the pose (the per-voxel rules 1 and 2 of the header)."""
    c = R.voxel_centres(LO, DIMS, VS)
    cam = R.O.rotate(R.O.quat_inverse(q), c - t[None, :])
    h0, h1, h2 = (sum(K[r, k] * cam[:, k] for k in range(3)) for r in range(3))
    with np.errstate(all='ignore'):
        return ((h2 > 0) & (h0 / h2 >= 0) & (h0 / h2 < W) & (h1 / h2 >= 0) & (h1 / h2 < H)).reshape(DIMS[::-1])


def test_scene_exercises_the_cull(frames):
    K, q, t, _ = frames
    inside_volume = np.all((t[1] > LO) & (t[1] < LO + np.array(DIMS) * VS))
    assert inside_volume
    corner = in_image(K, q[2], t[2])
    assert 0 < corner.mean() < 0.2                                     # most x-runs are culled whole ...
    per_run = corner.reshape(-1, DIMS[0]).sum(axis=1)
    assert ((per_run > 0) & (per_run < DIMS[0])).any()                 # ... and some straddle a frustum bound
    assert not in_image(K, q[3], t[3]).any()                           # wholly outside
    assert in_image(K, q[0], t[0]).mean() > 0.3


def raw_depths(depths, dtype, scale):
    with np.errstate(invalid='ignore'):
        raw = depths * scale
        if dtype == np.uint16:
            raw = np.where(np.isfinite(raw), np.clip(np.round(raw), 0, 65535), 0)
        return raw.astype(dtype)


@pytest.fixture(scope='module')
def base_state(frames):
    """The reference state of the base case (float64 depths, scale 1), shared by the tests that extract from it."""
    K, q, t, depths = frames
    tsdf, weight = R.integrate(*zeros(), LO, VS, TRUNC, 64, depths, K, q, t, 1.0, MAX_DEPTH)
    tsdf.setflags(write=False)
    weight.setflags(write=False)
    return tsdf, weight


@pytest.mark.parametrize('scale', [1.0, 1000.0])
@pytest.mark.parametrize('dtype', [np.float64, np.float32, np.uint16])
def test_integrate_equals_the_restatement(ctx, frames, dtype, scale):
    K, q, t, depths = frames
    raw = raw_depths(depths, dtype, scale)
    want_t, want_w = R.integrate(*zeros(), LO, VS, TRUNC, 64, raw, K, q, t, scale, MAX_DEPTH)
    assert want_w.max() >= 3 and (want_w == 0).any() and (want_t < 0).any() and (want_t > 0).any()
    tsdf, weight = zeros()
    ctx.tsdf_integrate(tsdf, weight, LO, VS, TRUNC, 64, raw, f3d.views_build(K, W, H, q, t, MAX_DEPTH), scale, MAX_DEPTH)
    assert same_bits(weight, want_w)
    assert same_bits(tsdf, want_t)


def test_views_built_for_another_image_change_nothing(ctx, frames, base_state):
    """The planes stored in the views play no part: views built for another image size and far distance give the same state."""
    K, q, t, depths = frames
    tsdf, weight = zeros()
    ctx.tsdf_integrate(tsdf, weight, LO, VS, TRUNC, 64, depths, f3d.views_build(K, 7, 5, q, t, 0.3), 1.0, MAX_DEPTH)
    assert same_bits(tsdf, base_state[0]) and same_bits(weight, base_state[1])


def test_two_calls_equal_one(ctx, frames, base_state):
    K, q, t, depths = frames
    tsdf, weight = zeros()
    for part in (slice(0, 2), slice(2, 5)):
        ctx.tsdf_integrate(tsdf, weight, LO, VS, TRUNC, 64, depths[part], f3d.views_build(K, W, H, q[part], t[part], MAX_DEPTH), 1.0, MAX_DEPTH)
    assert same_bits(tsdf, base_state[0]) and same_bits(weight, base_state[1])


def test_max_weight_saturates(ctx, frames):
    K, q, t, depths = frames
    want_t, want_w = R.integrate(*zeros(), LO, VS, TRUNC, 2, depths, K, q, t, 1.0, MAX_DEPTH)
    assert want_w.max() == 2 and (R.integrate(*zeros(), LO, VS, TRUNC, 64, depths, K, q, t, 1.0, MAX_DEPTH)[1] > 2).any()
    tsdf, weight = zeros()
    ctx.tsdf_integrate(tsdf, weight, LO, VS, TRUNC, 2, depths, f3d.views_build(K, W, H, q, t, MAX_DEPTH), 1.0, MAX_DEPTH)
    assert same_bits(tsdf, want_t) and same_bits(weight, want_w)


@pytest.mark.parametrize('dims,lo', [((1, 29, 21), (0.1, -0.7, 0.55)), ((1, 1, 1), (0.5, 0.4, 1.45)), ((130, 3, 2), (-3.2, 0.3, 1.4))])
def test_thin_volumes(ctx, frames, dims, lo):
    K, q, t, depths = frames
    lo = np.array(lo)
    want_t, want_w = R.integrate(*zeros(dims), lo, VS, TRUNC, 64, depths, K, q, t, 1.0, MAX_DEPTH)
    assert want_w.any()
    tsdf, weight = zeros(dims)
    ctx.tsdf_integrate(tsdf, weight, lo, VS, TRUNC, 64, depths, f3d.views_build(K, W, H, q, t, MAX_DEPTH), 1.0, MAX_DEPTH)
    assert same_bits(tsdf, want_t) and same_bits(weight, want_w)


def test_no_frames_is_a_no_op(ctx, base_state):
    tsdf, weight = base_state[0].copy(), base_state[1].copy()
    ctx.tsdf_integrate(tsdf, weight, LO, VS, TRUNC, 64, np.zeros((0, H, W)), np.zeros((0, f3d.VIEW_DOUBLES)), 1.0, MAX_DEPTH)
    assert same_bits(tsdf, base_state[0]) and same_bits(weight, base_state[1])


def test_library_refuses_bad_arguments(ctx, frames):
    K, q, t, depths = frames
    views = f3d.views_build(K, W, H, q, t, MAX_DEPTH)
    tsdf, weight = zeros()
    for kw in [dict(voxel=0.0), dict(voxel=np.inf), dict(trunc=0.0), dict(trunc=np.nan), dict(max_weight=0.5), dict(max_weight=2.0 ** 25),
               dict(depth_scale=0.0), dict(max_depth=np.inf)]:
        a = dict(voxel=VS, trunc=TRUNC, max_weight=64, depth_scale=1.0, max_depth=MAX_DEPTH)
        a.update(kw)
        with pytest.raises(ValueError):
            ctx.tsdf_integrate(tsdf, weight, LO, a['voxel'], a['trunc'], a['max_weight'], depths, views, a['depth_scale'], a['max_depth'])
    assert not tsdf.any() and not weight.any()
    with pytest.raises(ValueError):
        ctx.tsdf_extract(tsdf, weight, LO, VS, 0.5)
    with pytest.raises(ValueError):
        ctx.tsdf_extract(tsdf, weight, LO, 0.0, 1.0)
    lib, nv, nt = ctx._lib, C.c_int64(7), C.c_int64(7)
    assert lib.f3d_tsdf_integrate(ctx._h, f3d._ptr(tsdf), f3d._ptr(weight), 37, 29, 21, f3d._ptr(LO), VS, TRUNC, 64.0, f3d._ptr(depths), 3, 5, H, W, 1.0,
                                  MAX_DEPTH, f3d._ptr(views)) == f3d.ERR_INVALID              # unknown depth type
    assert lib.f3d_tsdf_extract_count(ctx._h, None, f3d._ptr(weight), 37, 29, 21, 1.0, C.byref(nv), C.byref(nt)) == f3d.ERR_INVALID
    assert lib.f3d_tsdf_extract_count(ctx._h, f3d._ptr(tsdf), f3d._ptr(weight), 2048, 2048, 512, 1.0, C.byref(nv), C.byref(nt)) == f3d.ERR_INVALID
    assert (nv.value, nt.value) == (7, 7)


# ------------------------------------------------------------------------------------------------ extract
def check_extract(ctx, tsdf, weight, lo, vs, min_weight=1.0):
    want_v, want_t = R.extract(tsdf, weight, lo, vs, min_weight)
    verts, tris = ctx.tsdf_extract(np.ascontiguousarray(tsdf).copy(), np.ascontiguousarray(weight).copy(), lo, vs, min_weight)
    assert (len(verts), len(tris)) == (len(want_v), len(want_t))
    assert tris.dtype == np.int32 and np.array_equal(tris, want_t)
    assert same_bits(verts, want_v)
    return verts, tris


def test_extract_of_the_integrated_state(ctx, base_state):
    verts, tris = check_extract(ctx, *base_state, LO, VS, 1.0)
    assert len(verts) > 500 and len(tris) > 1000
    cut_v, cut_t = check_extract(ctx, *base_state, LO, VS, 3.0)
    assert 0 < len(cut_t) < len(tris)
    assert R.edge_stats(cut_t)[1] == 1                                 # unobserved voxels cut the surface: open borders


def test_extract_without_an_active_cell(ctx):
    tsdf, weight = zeros((6, 5, 4))
    for t, w in [(tsdf, weight), (tsdf + 0.5, weight + 1), (tsdf - 0.5, weight + 1), (tsdf - 0.5, weight)]:
        verts, tris = check_extract(ctx, t, w, LO, VS)
        assert verts.shape == (0, 3) and tris.shape == (0, 3)
    verts, tris = check_extract(ctx, np.full((1, 1, 1), -0.5, np.float32), np.ones((1, 1, 1), np.float32), LO, VS)
    assert len(verts) == 0 and len(tris) == 0


def test_extract_of_one_active_cell(ctx):
    tsdf, weight = np.full((2, 2, 2), 0.5, np.float32), np.ones((2, 2, 2), np.float32)
    tsdf[1, 0, 1] = -0.25
    verts, tris = check_extract(ctx, tsdf, weight, LO, VS)
    assert verts.shape == (1, 3) and tris.shape == (0, 3)


def test_extract_with_signed_zeros(ctx):
    rng = np.random.default_rng(11)
    tsdf = rng.uniform(-1, 1, (9, 8, 7)).astype(np.float32)
    tsdf[rng.random(tsdf.shape) < 0.2] = 0.0
    tsdf[rng.random(tsdf.shape) < 0.2] = -0.0
    assert (bits(tsdf) == np.int32(-2 ** 31)).any() and (bits(tsdf) == 0).any()
    verts, _ = check_extract(ctx, tsdf, np.ones_like(tsdf), LO, VS)
    assert np.isfinite(verts).all()


def test_extract_of_a_checkerboard(ctx):
    k, j, i = np.meshgrid(np.arange(6), np.arange(11), np.arange(13), indexing='ij')
    tsdf = np.where((i + j + k) % 2 == 0, -0.5, 0.25).astype(np.float32)
    verts, tris = check_extract(ctx, tsdf, np.ones_like(tsdf), LO, VS)
    assert len(verts) == 5 * 10 * 12                                   # every cell is active


@pytest.mark.parametrize('min_weight', [1.0, 2.0])
def test_extract_of_a_random_state(ctx, min_weight):
    """22533 voxels = 11 scan tiles: active cells and quads on both sides of every tile and block edge."""
    rng = np.random.default_rng(5)
    tsdf = rng.uniform(-1, 1, DIMS[::-1]).astype(np.float32)
    weight = rng.integers(0, 4, DIMS[::-1]).astype(np.float32)
    weight[rng.random(weight.shape) < 0.6] = 3
    verts, tris = check_extract(ctx, tsdf, weight, LO, VS, min_weight)
    assert len(tris) > 0


SCAN_EDGES = [(15, 17), (16, 16), (1, 257), (23, 89), (32, 64), (3, 683)]   # 255, 256, 257 (a scan block), 2047, 2048, 2049 (a scan tile)


@pytest.mark.parametrize('a,b', SCAN_EDGES)
def test_extract_counts_at_the_scan_edges(ctx, a, b):
    """A slab crossed by the plane between its two z layers: (nx - 1)(ny - 1) active cells, (nx - 2)(ny - 2) quads."""
    assert a * b in [n + d for n in (256, f3d.TSDF_SCAN_TILE) for d in (-1, 0, 1)]
    for grow in (1, 2):                                                # the cells, then the quads, number a * b
        nx, ny = a + grow, b + grow
        tsdf = np.stack([np.full((ny, nx), -0.3, np.float32), np.full((ny, nx), 0.5, np.float32)])
        verts, tris = check_extract(ctx, tsdf, np.ones_like(tsdf), LO, VS)
        assert len(verts) == (nx - 1) * (ny - 1) and len(tris) == 2 * (nx - 2) * (ny - 2)
        assert a * b in (len(verts), len(tris) // 2)


SUMS_EDGES = [(120, 128, 34), (128, 128, 32), (128, 137, 30)]            # 255, 256 and 257 scan tiles


@pytest.mark.parametrize('dims', SUMS_EDGES)
def test_extract_across_the_blocks_of_the_tile_sums(ctx, dims):
    """k_tsdf_scan_sums scans the tile sums 256 at a time with a carry: volumes of 255, 256 and 257 tiles, random states whose
    active cells and quads lie in every tile, so the ranks and offsets behind the 256th tile need the carry."""
    n = dims[0] * dims[1] * dims[2]
    assert -(-n // f3d.TSDF_SCAN_TILE) == {34: 255, 32: 256, 30: 257}[dims[2]]
    rng = np.random.default_rng(dims[2])
    tsdf = rng.uniform(-1, 1, dims[::-1]).astype(np.float32)
    weight = (rng.random(dims[::-1]) < 0.93).astype(np.float32)
    verts, tris = check_extract(ctx, tsdf, weight, LO, VS)
    assert len(verts) > 100000 and len(tris) > 100000


def test_results_do_not_depend_on_the_launch_shape(frames, base_state):
    """Three blocks per launch: every grid-stride loop (integrate tiles, codes, cells, quads, vertices, triangles) takes dozens of
    passes over the base volume, and the results are the same bits."""
    K, q, t, depths = frames
    own = f3d.Context(0)
    try:
        own.debug_tsdf_grid_cap(3)
        tsdf, weight = zeros()
        own.tsdf_integrate(tsdf, weight, LO, VS, TRUNC, 64, depths, f3d.views_build(K, W, H, q, t, MAX_DEPTH), 1.0, MAX_DEPTH)
        assert same_bits(tsdf, base_state[0]) and same_bits(weight, base_state[1])
        for min_weight in (1.0, 3.0):
            check_extract(own, tsdf, weight, LO, VS, min_weight)
        with pytest.raises(ValueError):
            own.debug_tsdf_grid_cap(-1)
    finally:
        own.close()


def test_reserving_ends_a_counted_sequence(base_state):
    own = f3d.Context(0)
    try:
        tsdf, weight = base_state[0].copy(), base_state[1].copy()
        nv, nt = C.c_int64(0), C.c_int64(0)
        assert own._lib.f3d_tsdf_extract_count(own._h, f3d._ptr(tsdf), f3d._ptr(weight), *DIMS, 1.0, C.byref(nv), C.byref(nt)) == 0
        own.reserve_tsdf(4 * tsdf.size)                                # may move the scratch that holds the ranks
        verts, tris = np.empty((nv.value, 3)), np.empty((nt.value, 3), np.int32)
        assert own._lib.f3d_tsdf_extract_fill(own._h, *DIMS, f3d._ptr(LO), VS, f3d._ptr(verts), f3d._ptr(tris)) == f3d.ERR_INVALID
        check_extract(own, tsdf, weight, LO, VS)
    finally:
        own.close()


def test_extract_of_surfaces_that_touch_the_faces(ctx):
    """Planes that run through the whole volume, along every axis and in both orientations, and a tilted one: the quads stop one
    cell short of every face the surface touches (the four cells of an edge must be in range)."""
    dims = (7, 6, 5)
    c = R.voxel_centres(np.zeros(3), dims, 1.0)
    normals = [s * np.eye(3)[a] for a in range(3) for s in (1.0, -1.0)] + [np.array([0.5, -0.3, 0.8])]
    for n in normals:
        off = float(n @ (np.array(dims) / 2.0 + 0.2))
        tsdf = np.clip((c @ n - off) / 2.0, -1, 1).astype(np.float32).reshape(dims[::-1])
        verts, tris = check_extract(ctx, tsdf, np.ones_like(tsdf), LO, VS)
        assert len(tris) > 0 and R.edge_stats(tris)[1] == 1


# ------------------------------------------------------------------------------------------------ routes and the context
def test_device_route_equals_host_route(ctx, frames, base_state):
    import torch
    K, q, t, depths = frames
    host = reconstruct.TSDFVolume(LO, DIMS, VS, TRUNC).integrate(depths, K, q, t, 1.0, MAX_DEPTH)
    assert same_bits(host.tsdf, base_state[0]) and same_bits(host.weight, base_state[1])
    hv, ht = host.extract_mesh(2)
    dev = reconstruct.TSDFVolume(LO, DIMS, VS, TRUNC, device=True)
    assert dev.on_device
    dev.integrate(torch.from_numpy(depths.copy()).cuda(), K, q, t, 1.0, MAX_DEPTH)
    assert same_bits(dev.tsdf.cpu().numpy(), host.tsdf) and same_bits(dev.weight.cpu().numpy(), host.weight)
    dv, dt = dev.extract_mesh(2)
    assert dv.is_cuda and dt.is_cuda and dt.dtype == torch.int32
    assert same_bits(dv.cpu().numpy(), hv) and np.array_equal(dt.cpu().numpy(), ht)
    fed = reconstruct.TSDFVolume(LO, DIMS, VS, TRUNC).integrate(torch.from_numpy(raw_depths(depths, np.float32, 1.0)).cuda(), K, q, t, 1.0, MAX_DEPTH)
    assert fed.on_device                                               # fed device tensors: the state moves to the device
    want = R.integrate(*zeros(), LO, VS, TRUNC, 64, raw_depths(depths, np.float32, 1.0), K, q, t, 1.0, MAX_DEPTH)
    assert same_bits(fed.tsdf.cpu().numpy(), want[0])


def test_strict_reserved_context_allocates_nothing(frames, base_state):
    import torch
    K, q, t, depths = frames
    own = f3d.Context(0)
    try:
        n = DIMS[0] * DIMS[1] * DIMS[2]
        own.reserve_tsdf(n)
        tsdf, weight = (torch.zeros(DIMS[::-1], dtype=torch.float32, device='cuda') for _ in range(2))
        dd, dviews = torch.from_numpy(depths.copy()).cuda(), torch.from_numpy(f3d.views_build(K, W, H, q, t, MAX_DEPTH)).cuda()
        torch.cuda.synchronize()
        own.set_strict(True)
        before = own.alloc_count
        own.tsdf_integrate_dev(tsdf.data_ptr(), weight.data_ptr(), DIMS, LO, VS, TRUNC, 64, dd.data_ptr(), 0, 5, H, W, 1.0, MAX_DEPTH, dviews.data_ptr())
        nv, nt = own.tsdf_extract_count_dev(tsdf.data_ptr(), weight.data_ptr(), DIMS, 1.0)
        verts = torch.empty((nv, 3), dtype=torch.float64, device='cuda')
        tris = torch.empty((nt, 3), dtype=torch.int32, device='cuda')
        own.tsdf_extract_fill_dev(tsdf.data_ptr(), DIMS, LO, VS, verts.data_ptr(), tris.data_ptr())
        own.synchronize()
        assert own.alloc_count == before
        want_v, want_t = R.extract(*base_state, LO, VS, 1.0)
        assert same_bits(tsdf.cpu().numpy(), base_state[0])
        assert same_bits(verts.cpu().numpy(), want_v) and np.array_equal(tris.cpu().numpy(), want_t)
        with pytest.raises(MemoryError):                               # a larger volume would have to grow the scratch
            own.tsdf_extract_count_dev(tsdf.data_ptr(), weight.data_ptr(), (DIMS[0], DIMS[1], 2 * DIMS[2]), 1.0)
    finally:
        own.close()


def test_other_calls_between_count_and_fill(ctx, base_state):
    tsdf, weight = base_state[0].copy(), base_state[1].copy()
    want_v, want_t = R.extract(tsdf, weight, LO, VS, 1.0)
    lib, nv, nt = ctx._lib, C.c_int64(0), C.c_int64(0)
    assert lib.f3d_tsdf_extract_count(ctx._h, f3d._ptr(tsdf), f3d._ptr(weight), *DIMS, 1.0, C.byref(nv), C.byref(nt)) == 0
    assert (nv.value, nt.value) == (len(want_v), len(want_t))
    rng = np.random.default_rng(3)
    pts = rng.uniform(-1, 1, (4000, 3))
    ctx.rotate(pts, [0.9, 0.1, -0.2, 0.3])
    ctx.radius_graph(pts, 0.1)
    ctx.tsdf_integrate(*zeros((5, 4, 3)), LO, VS, TRUNC, 64, np.ones((1, H, W)), f3d.views_build(np.eye(3), W, H, [[1.0, 0, 0, 0]], [[0.0, 0, 0]], 1.0))
    verts, tris = np.empty((nv.value, 3)), np.empty((nt.value, 3), np.int32)
    assert lib.f3d_tsdf_extract_fill(ctx._h, 36, 29, 21, f3d._ptr(LO), VS, f3d._ptr(verts), f3d._ptr(tris)) == f3d.ERR_INVALID   # other dims
    assert lib.f3d_tsdf_extract_fill(ctx._h, *DIMS, f3d._ptr(LO), VS, f3d._ptr(verts), f3d._ptr(tris)) == 0
    assert same_bits(verts, want_v) and np.array_equal(tris, want_t)


# ------------------------------------------------------------------------------------------------ end to end
def test_reconstructed_mesh_feeds_the_mesh_route(ctx):
    from Fusion3DSeg import fusion
    from Fusion3DSeg.segUtils import meshUtils
    eyes = [(0.0, 0.0, 0.0), (-0.5, 0.1, 0.1), (0.5, -0.1, 0.1), (0.0, 0.45, 0.15), (0.0, -0.45, 0.15), (0.3, 0.3, 0.0)]
    K, q, t, depths = R.scene(eyes, [(0.05, -0.02, 1.0)] * 6, H, W)
    verts, tris = reconstruct.reconstruct_mesh(depths, K, q, t, LO, DIMS, VS, max_depth=MAX_DEPTH)
    want = R.extract(*R.integrate(*zeros(), LO, VS, 4 * VS, 64, depths, K, q, t, 1.0, MAX_DEPTH), LO, VS, 1.0)
    assert same_bits(verts, want[0]) and np.array_equal(tris, want[1]) and len(tris) > 1000
    # the sphere's front is reconstructed where it is: a vertex lies in a cell with a sign change, within a cell diagonal of the surface
    near = (np.linalg.norm(verts - R.SPHERE_C, axis=1) < R.SPHERE_R + 2 * VS) & (verts[:, 2] < R.SPHERE_C[2] - 0.1)   # the cap every camera sees
    assert near.sum() > 50 and np.abs(np.linalg.norm(verts[near] - R.SPHERE_C, axis=1) - R.SPHERE_R).max() <= np.sqrt(3.0) * VS
    offsets, neighbours = meshUtils.face_adjacency(tris, len(verts))
    assert offsets.shape == (len(tris) + 1,) and offsets[-1] == len(neighbours) and len(neighbours) > len(tris)
    depth, uv2tri, straddling = fusion.render_mesh_lookups(verts, tris, K, q, t, (H, W), MAX_DEPTH)
    assert depth.shape == (6, H, W) and uv2tri.shape == (6, H * W) and straddling.shape == (6,)
    seen = uv2tri[0].reshape(H, W) >= 0
    assert seen.mean() > 0.5
    centre = depth[0][H // 2, W // 2]                                  # the pixel that looks at the sphere's near pole
    assert abs(centre - depths[0, H // 2, W // 2]) <= np.sqrt(3.0) * VS
    masks = np.zeros((6, H, W), np.uint8)
    masks[:, :, W // 2:] = 1
    classes = meshUtils.label_faces(verts, tris, K, q, t, masks, MAX_DEPTH, nclasses=2)
    assert classes.shape == (len(tris),) and set(np.unique(classes)) <= {0, 1, 2} and (classes == 0).any() and (classes == 1).any()


def test_fusion_reconstruct_mesh(ctx):
    from fusion_scenes import copy_frames, curved_capture
    from Fusion3DSeg.fusion import Fusion
    h, w = 24, 32
    K, q, t, frames = curved_capture(h, w, 3, 7, quirks=False)
    fu = Fusion.from_frames(K, w, h, q, t, copy_frames(frames))
    verts, tris = fu.reconstruct_mesh(0.03, max_depth=4.0)
    assert verts.dtype == np.float64 and tris.dtype == np.int32 and len(verts) > 100 and len(tris) > 100
    assert tris.min() >= 0 and tris.max() < len(verts)
    pts = np.concatenate([f[1][f[4]] for f in frames])
    assert (verts >= pts.min(axis=0) - 0.12 - 0.03).all() and (verts <= pts.max(axis=0) + 0.12 + 0.03).all()
    spent = [(n, p, nr, c, np.zeros_like(v)) for n, p, nr, c, v in copy_frames(frames)]     # what fuse leaves of the valid masks
    with pytest.raises(ValueError, match='valid'):
        Fusion.from_frames(K, w, h, q, t, spent).reconstruct_mesh(0.03, lo=np.zeros(3), dims=(4, 4, 4))
    # bounds from the fused cloud (inside the frames' box, so the volume only shrinks), and frames of device tensors
    fused = fu.reconstruct_mesh(0.03, max_depth=4.0, points=pts[::3])
    assert len(fused[1]) > 100 and fused[1].max() < len(fused[0])
    import torch
    dev_frames = [(n, torch.from_numpy(p).cuda(), torch.from_numpy(nr).cuda(), torch.from_numpy(c).cuda(), torch.from_numpy(v).cuda())
                  for n, p, nr, c, v in copy_frames(frames)]
    dv, dt = Fusion.from_frames(K, w, h, q, t, dev_frames).reconstruct_mesh(0.03, max_depth=4.0)
    assert dv.is_cuda and same_bits(dv.cpu().numpy(), verts) and np.array_equal(dt.cpu().numpy(), tris)


def test_depth_images_invert_unproject_depth(ctx, frames):
    """depth -> f3d_unproject_depth -> depth_images is a rotation there and back, which is not exact.  Measured against the NumPy
    restatement of the same two steps (oracle unproject_depth, then the z of rotate(p - t, inverse(q))) on these frames: at most
    1.43e-14, which is 2 ulps of the largest depth (the 50 m hole value; 2.7e-15 on the depths below 2 m).  The bound below adds a
    margin of 4 more ulps of the largest depth."""
    K, q, t, depths = frames
    sel = [0, 1, 4]
    d = np.where(np.isfinite(depths[sel]) & (depths[sel] > 0), depths[sel], 0.0)
    pts = np.stack([ctx.unproject_depth(d[k], K, q[f], t[f], 1.0).reshape(H, W, 3) for k, f in enumerate(sel)])
    valid = d > 0
    got = reconstruct.depth_images(pts, q[sel], t[sel], valid)
    assert got.shape == d.shape and got.dtype == np.float64
    assert (got[~valid] == 0).all()
    ref = np.stack([R.O.rotate(R.O.quat_inverse(q[f]), R.O.unproject_depth(d[k], K, q[f], t[f], 1.0) - t[f][None, :])[:, 2].reshape(H, W)
                    for k, f in enumerate(sel)])
    tol = 1.43e-14 + 4 * np.spacing(d.max())
    print('depth_images: max |restatement - depth| =', np.abs(ref - d)[valid].max(), ' max |library - depth| =', np.abs(got - d)[valid].max())
    assert np.abs(ref - d)[valid].max() <= tol
    assert np.abs(got - d)[valid].max() <= tol
    pts[0, 3, 4, 1] = np.nan
    assert reconstruct.depth_images(pts, q[sel], t[sel])[0, 3, 4] == 0
