"""The sample range of k_tsdf_raycast at its bounds, bit for bit against the NumPy restatement (tests/icp_ref.py), which marches every
sample: rays along the axes and beside the faces, rays through edges and corners, marches clipped at either end, a distant camera and
a scene far from the origin.  That each case reaches its path is shown on the restatement alone in tests/test_registration_cpu.py."""
import numpy as np
import pytest

import f3d
import icp_ref as I

pytestmark = pytest.mark.gpu

CASES = I.ray_cases()


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def same_bits(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(bits(got), bits(want))


@pytest.fixture(scope='module')
def ctx():
    return f3d.default_context()


@pytest.fixture(scope='module')
def states():
    """voxel size -> (tsdf, weight) of the sphere, made once"""
    made = {}

    def get(vs):
        if vs not in made:
            made[vs] = I.ray_volume(vs)[:2]
            for a in made[vs]:
                a.setflags(write=False)
        return made[vs]
    return get


def check(ctx, case, state):
    want = I.ray_case_maps(case, state)
    got = ctx.tsdf_raycast(np.array(state[0]), np.array(state[1]), case['lo'], case['vs'], 1.0, case['K'], case['q'], case['t'], I.RAY_H, I.RAY_W,
                           case['near'], case['step'], case['nsteps'])
    for g, x in zip(got, want):
        assert same_bits(g, x)
    return want


@pytest.mark.parametrize('name', list(CASES))
def test_raycast_case_equals_the_restatement(ctx, states, name):
    case = CASES[name]
    vertex, normal, depth = check(ctx, case, states(case['vs']))
    hit = depth > 0
    if name in ('near-beyond', 'ends-before'):
        assert not hit.any() and np.isnan(vertex).all() and np.isnan(normal).all()
    else:
        assert hit.sum() >= 5 and (~hit).any()
    shape = (I.RAY_H, I.RAY_W)
    if name in ('beside', 'beside-high'):
        assert not hit.reshape(shape)[:, I.RAY_W // 2].any()
    if name in ('just-outside', 'just-outside-low'):
        assert not hit.reshape(shape)[I.RAY_H // 2].any()


@pytest.mark.parametrize('blocks', [3, 1])
def test_raycast_cases_with_capped_grids(states, blocks):
    """The 15 x 17 image is six tiles, four to a block: one block takes them in two passes, three blocks leave one idle."""
    own = f3d.Context(0)
    try:
        own.debug_tsdf_grid_cap(blocks)
        for name in ('axis-y', 'corner3', 'beside'):
            check(own, CASES[name], states(CASES[name]['vs']))
    finally:
        own.close()
