"""The frame cull of k_tsdf_integrate at its bounds, bit for bit against the NumPy restatement (tests/tsdf_ref.py), which culls nothing:
more frames than one ballot of 64 takes, one camera per bound of the cull, voxels that sit exactly on the bounds, a scene far from the
origin and a general K.  That each scene reaches its path is shown on the restatement alone in tests/test_tsdf_cpu.py."""
import numpy as np
import pytest

import f3d
import tsdf_ref as R

pytestmark = pytest.mark.gpu


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


def same_bits(got, want):
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(bits(got), bits(want))


def zeros(dims):
    return np.zeros(dims[::-1], np.float32), np.zeros(dims[::-1], np.float32)


@pytest.fixture(scope='module')
def ctx():
    return f3d.default_context()


# ------------------------------------------------------------------------------------------------ more frames than one ballot
G = R.RING


def ring_views(K, q, t):
    return f3d.views_build(K, G['w'], G['h'], q, t, G['max_depth'])


def gpu_ring(ctx, state, K, q, t, depths, lo=G['lo'], max_weight=64, scale=1.0):
    ctx.tsdf_integrate(*state, lo, G['vs'], G['trunc'], max_weight, depths, ring_views(K, q, t), scale, G['max_depth'])


@pytest.fixture(scope='module')
def rings():
    """F -> (K, q, t, depths, the restated state after the F frames of the ring), computed once per F."""
    made = {}

    def get(F):
        if F not in made:
            K, q, t, depths = R.ring_scene(F)
            want = R.integrate(*zeros(G['dims']), G['lo'], G['vs'], G['trunc'], 64, depths, K, q, t, 1.0, G['max_depth'])
            for a in (q, t, depths) + want:
                a.setflags(write=False)
            made[F] = (K, q, t, depths, want)
        return made[F]
    return get


@pytest.mark.parametrize('F', [63, 64, 65, 128, 130])
def test_frames_around_the_ballot_of_64(ctx, rings, F):
    K, q, t, depths, want = rings(F)
    state = zeros(G['dims'])
    gpu_ring(ctx, state, K, q, t, depths)
    assert same_bits(state[1], want[1])
    assert same_bits(state[0], want[0])
    if F >= 128:
        assert want[1].max() == 64                                      # the default max_weight saturates


@pytest.mark.parametrize('split', [64, 1])
def test_130_frames_split_in_two_calls(ctx, rings, split):
    K, q, t, depths, want = rings(130)
    state = zeros(G['dims'])
    for part in (slice(0, split), slice(split, 130)):
        gpu_ring(ctx, state, K, q[part], t[part], depths[part])
    assert same_bits(state[0], want[0]) and same_bits(state[1], want[1])


def test_130_frames_without_saturation(ctx, rings):
    K, q, t, depths, _ = rings(130)
    want = R.integrate(*zeros(G['dims']), G['lo'], G['vs'], G['trunc'], 1e6, depths, K, q, t, 1.0, G['max_depth'])
    assert want[1].max() > 64
    state = zeros(G['dims'])
    gpu_ring(ctx, state, K, q, t, depths, max_weight=1e6)
    assert same_bits(state[0], want[0]) and same_bits(state[1], want[1])


def test_130_frames_with_three_blocks(rings):
    """Three blocks take the 32 tiles of the volume in turn, each tile through three ballots."""
    K, q, t, depths, want = rings(130)
    own = f3d.Context(0)
    try:
        own.debug_tsdf_grid_cap(3)
        state = zeros(G['dims'])
        gpu_ring(own, state, K, q, t, depths)
        assert same_bits(state[0], want[0]) and same_bits(state[1], want[1])
    finally:
        own.close()


@pytest.mark.parametrize('dtype,scale', [(np.float32, 1.0), (np.uint16, 1000.0)])
def test_65_frames_of_other_depth_types(ctx, rings, dtype, scale):
    K, q, t, depths, _ = rings(65)
    raw = (np.round(depths * scale) if dtype == np.uint16 else depths * scale).astype(dtype)
    want = R.integrate(*zeros(G['dims']), G['lo'], G['vs'], G['trunc'], 64, raw, K, q, t, scale, G['max_depth'])
    assert want[1].max() >= 10 and (want[1] == 0).any()
    state = zeros(G['dims'])
    gpu_ring(ctx, state, K, q, t, raw, scale=scale)
    assert same_bits(state[0], want[0]) and same_bits(state[1], want[1])


# ------------------------------------------------------------------------------------------------ each bound on its own
@pytest.mark.parametrize('rule', list(R.BOUND_CAMERAS))
def test_one_camera_per_bound(ctx, rule):
    g = R.BOUNDS
    K, q, t, depth, max_depth = R.bound_scene(rule)
    want = R.integrate(*zeros(g['dims']), g['lo'], g['vs'], g['trunc'], 64, depth[None], K, q[None], t[None], 1.0, max_depth)
    assert want[1].sum() >= 500
    state = zeros(g['dims'])
    ctx.tsdf_integrate(*state, g['lo'], g['vs'], g['trunc'], 64, depth[None], f3d.views_build(K, g['w'], g['h'], q, t, max_depth), 1.0, max_depth)
    assert same_bits(state[1], want[1])
    assert same_bits(state[0], want[0])


def test_all_bound_cameras_in_one_call(ctx):
    """The six cameras as the frames of one call, twice over (12 lanes of the ballot, each with its own verdict per run); max_depth is
    the far camera's, so every camera meets the far bound as well."""
    g = R.BOUNDS
    scenes = [R.bound_scene(rule) for rule in R.BOUND_CAMERAS] * 2
    K, max_depth = scenes[0][0], R.BOUND_CAMERAS['far']['max_depth']
    q, t, depths = (np.array([s[k] for s in scenes]) for k in (1, 2, 3))
    want = R.integrate(*zeros(g['dims']), g['lo'], g['vs'], g['trunc'], 64, depths, K, q, t, 1.0, max_depth)
    assert want[1].max() >= 4 and (want[1] == 0).any()
    state = zeros(g['dims'])
    ctx.tsdf_integrate(*state, g['lo'], g['vs'], g['trunc'], 64, depths, f3d.views_build(K, g['w'], g['h'], q, t, max_depth), 1.0, max_depth)
    assert same_bits(state[0], want[0]) and same_bits(state[1], want[1])


# ------------------------------------------------------------------------------------------------ ties on the bounds
@pytest.mark.parametrize('volume', list(R.TIE_VOLUMES))
def test_voxels_on_the_bounds(ctx, volume):
    g, vol = R.TIES, R.TIE_VOLUMES[volume]
    depth = np.full((1, g['h'], g['w']), g['max_depth'])
    want = R.integrate(*zeros(vol['dims']), vol['lo'], g['vs'], g['trunc'], 64, depth, g['K'], g['wxyz'][None], g['t'][None], 1.0, g['max_depth'])
    assert (want[0] == -1.0).any() and (want[1] == 0).any()
    state = zeros(vol['dims'])
    views = f3d.views_build(g['K'], g['w'], g['h'], g['wxyz'], g['t'], g['max_depth'])
    ctx.tsdf_integrate(*state, vol['lo'], g['vs'], g['trunc'], 64, depth, views, 1.0, g['max_depth'])
    assert same_bits(state[1], want[1])
    assert same_bits(state[0], want[0])


# ------------------------------------------------------------------------------------------------ off the origin, a general K
def test_65_frames_away_from_the_origin(ctx, rings):
    K, q, t, depths, _ = rings(65)
    lo, there = G['lo'] + R.FAR_SHIFT, t + R.FAR_SHIFT
    want = R.integrate(*zeros(G['dims']), lo, G['vs'], G['trunc'], 64, depths, K, q, there, 1.0, G['max_depth'])
    assert want[1].max() >= 10 and (want[1] == 0).any()
    state = zeros(G['dims'])
    gpu_ring(ctx, state, K, q, there, depths, lo=lo)
    assert same_bits(state[0], want[0]) and same_bits(state[1], want[1])


def test_65_frames_through_a_K_with_skew(ctx, rings):
    _, q, t, depths, _ = rings(65)
    want = R.integrate(*zeros(G['dims']), G['lo'], G['vs'], G['trunc'], 64, depths, R.SKEW_K, q, t, 1.0, G['max_depth'])
    assert want[1].max() >= 10 and (want[1] == 0).any()
    state = zeros(G['dims'])
    gpu_ring(ctx, state, R.SKEW_K, q, t, depths)
    assert same_bits(state[0], want[0]) and same_bits(state[1], want[1])
