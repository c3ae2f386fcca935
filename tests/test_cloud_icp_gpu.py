"""Cloud-to-cloud ICP on the GPU against its NumPy restatement (tests/cloud_icp_ref.py): sums, pairs, poses, stats and status bit for
bit (floats compared as integer views); ties, missing normals, sources without a neighbour; the lost rules; launch shapes, uninitialised
memory, a strict context; segUtils.alignment on both routes; and the hand-off from torch of the two f3d.clouds functions behind a stalled
stream and from strided inputs (the cases tests/route_cases.py will carry once they move onto Context)."""
import numpy as np
import pytest

import f3d
import cloud_icp_ref as R
import icp_ref as I
import stalled_streams as S
from f3d import clouds as CL
from poison import poisoned_empty
from Fusion3DSeg.segUtils import alignment

pytestmark = pytest.mark.gpu

IDENT = np.array([1.0, 0.0, 0.0, 0.0])
ZERO = np.zeros(3)
MAX_DIST = 0.08
MODES = [R.PLANE, R.POINT]


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def same_bits(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and got.dtype == want.dtype == np.float64 and np.array_equal(bits(got), bits(want))


def same_ints(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and got.dtype == want.dtype == np.int32 and np.array_equal(got, want)


@pytest.fixture(scope='module')
def ctx():
    return f3d.default_context()


def check_sums(ctx, source, target, normals, mode, q, t, max_dist):
    want, want_pairs = R.cloud_icp_sums(source, target, normals, mode, q, t, max_dist)
    got, pairs = ctx.cloud_icp_sums(source, target, normals if mode == R.PLANE else None, mode, q, t, max_dist, pairs=True)
    assert same_ints(pairs, want_pairs) and same_bits(got, want)
    assert same_bits(ctx.cloud_icp_sums(source, target, normals if mode == R.PLANE else None, mode, q, t, max_dist), want)     # pairs not wanted
    return want, want_pairs


def check_rounds(ctx, source, target, normals, mode, q, t, max_dist, iterations, min_pairs):
    want = R.cloud_icp(source, target, normals, mode, q, t, max_dist, iterations, min_pairs)
    pose, stats, status = ctx.cloud_icp(source, target, normals if mode == R.PLANE else None, mode, q, t, max_dist, iterations, min_pairs)
    assert status == want[2] and same_bits(stats, want[1]) and same_bits(pose, want[0])
    return want


# ------------------------------------------------------------------------------------------------ bit for bit
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('n', [1, 63, 255, 256, 257, 700])
def test_sums_pairs_and_rounds_equal_the_restatement(ctx, n, mode):
    """n source points (one lane, a wave less one, a chunk less one, a chunk, a chunk and one, three chunks) against m = 900 targets,
    float32 and float64 on either side: the sums with the pairs, and 4 rounds."""
    for sdtype in (np.float64, np.float32):
        for tdtype in (np.float64, np.float32):
            source, target, normals, q, t = R.cloud_pair(n, sdtype=sdtype, tdtype=tdtype)
            assert source.dtype == sdtype and target.dtype == tdtype
            sums, pairs = check_sums(ctx, source, target, normals, mode, q, t, MAX_DIST)
            assert sums[28] == (pairs >= 0).sum() and (n < 63 or sums[28] >= 0.9 * n)
            _, stats, status = check_rounds(ctx, source, target, normals, mode, q, t, MAX_DIST, 4, 6)
            assert (status == I.OK) == (n >= 63)


@pytest.mark.parametrize('mode', MODES)
def test_a_third_of_the_sources_has_no_neighbour(ctx, mode):
    """max_dist = 0.04 leaves 0.351 of the 700 sources of the scene without a target in the restatement."""
    source, target, normals, q, t = R.cloud_pair(700)
    sums, pairs = check_sums(ctx, source, target, normals, mode, q, t, 0.04)
    left_out = float((pairs < 0).mean())
    print(f'without a neighbour: {left_out:.3f}')
    assert 0.2 <= left_out <= 0.5 and sums[28] == (pairs >= 0).sum()
    check_rounds(ctx, source, target, normals, mode, q, t, 0.04, 4, 6)


def lattice():
    """Integer-lattice targets 6 x 6 x 4 in a shuffled order, and sources on the midpoints of their cells' faces and bodies: four or
    eight targets at exactly the same distance."""
    rng = np.random.default_rng(5)
    g = np.stack(np.meshgrid(np.arange(6.0), np.arange(6.0), np.arange(4.0), indexing='ij'), axis=-1).reshape(-1, 3)
    g = g[rng.permutation(len(g))]
    cells = np.stack(np.meshgrid(np.arange(5.0), np.arange(5.0), np.arange(3.0), indexing='ij'), axis=-1).reshape(-1, 3)
    source = np.concatenate([cells + [0.5, 0.5, 0.0], cells + [0.5, 0.5, 0.5], cells + [0.0, 0.5, 0.5]])
    return source, g, np.tile([0.0, 0.0, 1.0], (len(g), 1))


@pytest.mark.parametrize('mode', MODES)
def test_exact_distance_ties_go_to_the_lower_index(ctx, mode):
    source, target, normals = lattice()
    for t in (ZERO, np.array([1.0, 0.0, -1.0])):                          # the identity rotation and an integer shift are exact
        for dtype in (np.float64, np.float32):
            _, pairs = check_sums(ctx, source.astype(dtype), target.astype(dtype), normals, mode, IDENT, t, 1.0)
            d2 = R.K.dist2(source + t, target)
            tied = (d2 == d2.min(axis=1, keepdims=True)).sum(axis=1)
            paired = pairs >= 0
            assert paired.sum() > 100 and (tied[paired] >= 2).all() and (tied[paired] >= 4).sum() > 50
            lowest = np.array([np.flatnonzero(row == row.min())[0] for row in d2])
            assert np.array_equal(pairs[paired], lowest[paired])
    check_rounds(ctx, source, target, normals, mode, IDENT, ZERO, 1.0, 2, 6)


def test_a_nan_normal_drops_the_pair_and_keeps_the_index(ctx):
    source, target, normals, q, t = R.cloud_pair(700)
    _, clean = R.cloud_icp_sums(source, target, normals, R.PLANE, q, t, MAX_DIST)
    holes = np.unique(clean[clean >= 0])[::5]
    normals = normals.copy()
    normals[holes[0::3], 0] = np.nan
    normals[holes[1::3], 1] = np.inf
    normals[holes[2::3], 2] = -np.inf
    sums, pairs = check_sums(ctx, source, target, normals, R.PLANE, q, t, MAX_DIST)
    hit = np.isin(pairs, holes)
    assert same_ints(pairs, clean) and hit.sum() > 50 and sums[28] == (pairs >= 0).sum() - hit.sum()
    check_rounds(ctx, source, target, normals, R.PLANE, q, t, MAX_DIST, 3, 6)
    check_sums(ctx, source, target, normals, R.POINT, q, t, MAX_DIST)      # point mode does not read them


@pytest.mark.parametrize('mode', MODES)
def test_sources_outside_the_reach_box(ctx, mode):
    """A third of the sources far from the target, a third within a few cells of its box on every side, a third inside."""
    source, target, normals, q, t = R.cloud_pair(300, sdtype=np.float64)
    rng = np.random.default_rng(8)
    source = source.copy()
    source[:100] += rng.choice([-1.0, 1.0], size=(100, 3)) * rng.uniform(5.0, 50.0, size=(100, 3))
    edge = rng.integers(0, 3, size=100)
    source[100:200, :] = rng.uniform(-1.0, 1.0, size=(100, 3))
    source[np.arange(100, 200), edge] = rng.choice([-1.0, 1.0], size=100) * (1.0 + rng.uniform(0.0, 3.0 * MAX_DIST, size=100))
    sums, pairs = check_sums(ctx, source, target, normals, mode, IDENT, ZERO, MAX_DIST)
    assert (pairs[:100] < 0).all() and (pairs[200:] >= 0).sum() > 50
    check_rounds(ctx, source, target, normals, mode, q, t, MAX_DIST, 3, 6)


# ------------------------------------------------------------------------------------------------ status
def test_a_single_plane_is_lost_in_round_0(ctx):
    """A plane fixes three of the six degrees of freedom: the third pivot is exactly 0, the pose stays, the later rows are {0, 0, 1}."""
    rng = np.random.default_rng(2)
    target = np.concatenate([rng.uniform(-1.0, 1.0, size=(400, 2)), np.zeros((400, 1))], axis=1)
    normals = np.tile([0.0, 0.0, 1.0], (400, 1))
    source = target[:300] + [0.01, -0.01, 0.02]
    q, t = I.moved(IDENT, ZERO, (0.1, 0.2, 0.9), 0.5, np.array([0.01, 0.0, 0.0]))
    pose, stats, status = check_rounds(ctx, source, target, normals, R.PLANE, q, t, 0.2, 4, 6)
    assert status == I.LOST and same_bits(pose, np.concatenate([q, t])) and stats[0, 0] > 250 and stats[0, 2] == I.LOST
    assert np.array_equal(stats[1:], [[0.0, 0.0, 1.0]] * 3)
    assert check_rounds(ctx, source, target, normals, R.POINT, q, t, 0.2, 4, 6)[2] == I.OK       # points fix all six


@pytest.mark.parametrize('mode', MODES)
def test_too_few_pairs_is_lost(ctx, mode):
    source, target, normals, q, t = R.cloud_pair(257)
    pose, stats, status = check_rounds(ctx, source, target, normals, mode, q, t, MAX_DIST, 3, 258)
    assert status == I.LOST and same_bits(pose, np.concatenate([q, t])) and 200 < stats[0, 0] < 258 and np.array_equal(stats[1:], [[0.0, 0.0, 1.0]] * 2)
    mid = check_rounds(ctx, source, target, normals, mode, q, t, MAX_DIST, 3, 6)
    assert mid[2] == I.OK and not same_bits(mid[0], pose)


@pytest.mark.parametrize('mode', MODES)
def test_an_empty_source(ctx, mode):
    _, target, normals, q, t = R.cloud_pair(5)
    for empty in (np.zeros((0, 3)), np.zeros((0, 3), np.float32)):
        sums, pairs = check_sums(ctx, empty, target, normals, mode, q, t, MAX_DIST)
        assert np.array_equal(bits(sums), np.zeros(29, np.int64)) and pairs.shape == (0,)
        pose, stats, status = check_rounds(ctx, empty, target, normals, mode, q, t, MAX_DIST, 3, 6)
        assert status == I.LOST and np.array_equal(stats, [[0.0, 0.0, 1.0]] * 3) and same_bits(pose, np.concatenate([q, t]))


def test_the_c_entries_refuse_what_the_header_says(ctx):
    """Past the Python checks: the C entries themselves, with nothing written."""
    source, target, normals, q, t = R.cloud_pair(63)
    lib, p = ctx._lib, f3d._ptr
    sums, pose, stats, status = np.full(29, 7.0), np.full(7, 7.0), np.full((2, 3), 7.0), np.full(1, 7, np.int32)

    def sums_rc(src=source, tgt=target, nrm=normals, mode=0, q=q, t=t, max_dist=MAX_DIST, n=None, m=None):
        return lib.f3d_cloud_icp_sums(ctx._h, p(src), 0, len(src) if n is None else n, p(tgt), 0, len(tgt) if m is None else m, p(nrm), mode, p(q), p(t),
                                      max_dist, p(sums), None)

    nan_src, nan_tgt = source.copy(), target.copy()
    nan_src[5, 1], nan_tgt[100, 2] = np.nan, np.inf
    for kw in [dict(nrm=None), dict(mode=2), dict(m=0), dict(n=2 ** 31), dict(m=2 ** 31), dict(src=nan_src), dict(tgt=nan_tgt), dict(max_dist=0.0),
               dict(max_dist=np.inf), dict(max_dist=1e300), dict(q=np.zeros(4)), dict(t=np.array([0.0, np.nan, 0.0])), dict(n=-1)]:
        assert sums_rc(**kw) == f3d.ERR_INVALID, kw
    assert (sums == 7.0).all()
    assert sums_rc(nrm=None, mode=1) == 0 and not (sums == 7.0).any()
    for iterations, min_pairs in [(0, 6), (2, 5)]:
        assert lib.f3d_cloud_icp(ctx._h, p(source), 0, 63, p(target), 0, 900, p(normals), 0, p(q), p(t), MAX_DIST, iterations, min_pairs, p(pose), p(stats),
                                 p(status)) == f3d.ERR_INVALID
    assert lib.f3d_cloud_icp(ctx._h, p(nan_src), 0, 63, p(target), 0, 900, p(normals), 0, p(q), p(t), MAX_DIST, 2, 6, p(pose), p(stats),
                             p(status)) == f3d.ERR_INVALID
    assert (pose == 7.0).all() and (stats == 7.0).all() and status[0] == 7
    with pytest.raises(ValueError, match='NaN or infinity'):
        ctx.cloud_icp_sums(nan_src, target, normals, 0, q, t, MAX_DIST)


# ------------------------------------------------------------------------------------------------ launch shapes, poison, strict
@pytest.fixture(scope='module')
def big():
    """5000 sources (20 chunks: 5 blocks of the terms kernel) against 900 targets, and what the restatement gives for them."""
    source, target, normals, q, t = R.cloud_pair(5000, sdtype=np.float32)
    out = dict(source=source, target=target, normals=normals, q=q, t=t)
    for mode in MODES:
        out[mode] = (R.cloud_icp_sums(source, target, normals, mode, q, t, MAX_DIST), R.cloud_icp(source, target, normals, mode, q, t, MAX_DIST, 3, 100))
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def check_big(own, b):
    for mode in MODES:
        nrm = b['normals'] if mode == R.PLANE else None
        (want_sums, want_pairs), want = b[mode]
        sums, pairs = own.cloud_icp_sums(b['source'], b['target'], nrm, mode, b['q'], b['t'], MAX_DIST, pairs=True)
        assert same_bits(sums, want_sums) and same_ints(pairs, want_pairs)
        pose, stats, status = own.cloud_icp(b['source'], b['target'], nrm, mode, b['q'], b['t'], MAX_DIST, 3, 100)
        assert status == want[2] == I.OK and same_bits(stats, want[1]) and same_bits(pose, want[0])


@pytest.mark.parametrize('cap', [1, 3])
def test_results_do_not_depend_on_the_launch_shape(big, cap):
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
        assert calls >= lowered > 0 and lowered >= 8                    # the terms launches alone: 2 modes x (1 + 3 rounds) of 5 blocks each
    finally:
        own.debug_grid_cap(0)
        own.close()


@pytest.mark.parametrize('byte', [0x00, 0xFF, 0x5A])
def test_results_do_not_depend_on_uninitialised_memory(big, byte):
    own = f3d.Context(0)
    try:
        check_big(own, big)                                             # the scratch and staging buffers exist and hold other values
        own.debug_poison(byte)
        with poisoned_empty(byte):                                      # the outputs the bindings allocate are pre-filled
            check_big(own, big)
    finally:
        own.close()


def device_inputs(torch, b):
    return {k: torch.from_numpy(np.array(b[k])).cuda() for k in ('source', 'target', 'normals')}


def device_run(torch, own, d, q, t, mode, stream=None):
    """cloud_icp_sums_dev (with pairs) and 3 rounds of cloud_icp_dev over the device tensors `d`, enqueued on `stream`."""
    n, m = len(d['source']), len(d['target'])
    f64 = lambda *shape: torch.zeros(shape, dtype=torch.float64, device='cuda')     # noqa: E731
    sums, pose, stats = f64(29), f64(7), f64(3, 3)
    pairs, status = torch.zeros(n, dtype=torch.int32, device='cuda'), torch.zeros(1, dtype=torch.int32, device='cuda')
    nrm = d['normals'].data_ptr() if mode == R.PLANE else None
    sdt, tdt = (f3d.F32 if d[k].dtype == torch.float32 else f3d.F64 for k in ('source', 'target'))
    CL.cloud_icp_sums_dev(own, d['source'].data_ptr(), sdt, n, d['target'].data_ptr(), tdt, m, nrm, mode, q, t, MAX_DIST, sums.data_ptr(),
                          pairs.data_ptr(), stream)
    CL.cloud_icp_dev(own, d['source'].data_ptr(), sdt, n, d['target'].data_ptr(), tdt, m, nrm, mode, q, t, MAX_DIST, 3, 100, pose.data_ptr(),
                     stats.data_ptr(), status.data_ptr(), stream)
    return dict(sums=sums, pairs=pairs, pose=pose, stats=stats, status=status)


def check_device(got, b, mode):
    (want_sums, want_pairs), want = b[mode]
    assert same_bits(got['sums'].cpu().numpy(), want_sums) and same_ints(got['pairs'].cpu().numpy(), want_pairs)
    assert same_bits(got['pose'].cpu().numpy(), want[0]) and same_bits(got['stats'].cpu().numpy(), want[1]) and int(got['status'][0]) == want[2]


@pytest.mark.parametrize('mode', MODES)
def test_strict_reserved_context_allocates_nothing(big, mode):
    import torch
    own = f3d.Context(0)
    try:
        own.reserve_cloud_icp(900, 5000)
        d = device_inputs(torch, big)
        torch.cuda.synchronize()
        own.set_strict(True)
        before = own.alloc_count
        got = device_run(torch, own, d, big['q'], big['t'], mode)
        own.synchronize()
        assert own.alloc_count == before
        check_device(got, big, mode)
        with pytest.raises(MemoryError):                                # a larger source than was reserved for
            more = torch.zeros((300000, 3), dtype=torch.float64, device='cuda')
            device_run(torch, own, {**d, 'source': more}, big['q'], big['t'], mode)
    finally:
        own.close()


# ------------------------------------------------------------------------------------------------ segUtils.alignment
@pytest.fixture(scope='module')
def corner():
    s = R.corner_scene()
    for a in s.values():
        a.setflags(write=False)
    return s


@pytest.mark.parametrize('method, rounds', [('plane', 12), ('point', 30)])
def test_register_clouds_on_the_exact_subset_scene(ctx, corner, method, rounds):
    """The scene and the bounds of tests/test_cloud_icp_cpu.py through the module, NumPy in and device tensors in: translation error
    < 1e-12 m, rotation angle < 1e-12 rad, all 700 paired, status OK."""
    import torch
    s = corner
    nrm = s['normals'] if method == 'plane' else None
    q, t, info = alignment.register_clouds(s['source'], s['target'], nrm, max_dist=0.15, iterations=rounds, method=method)
    err = R.pose_error(np.concatenate([q, t]), s['q_true'], s['t_true'])
    print(f'{method}, NumPy: {err[0]:.3e} m, {err[1]:.3e} rad, rmse {info["rmse"]:.3e}')
    assert isinstance(q, np.ndarray) and isinstance(t, np.ndarray) and info['stats'].shape == (rounds, 3)
    assert info['status'] == f3d.ICP_OK and info['count'] == 700 and info['fitness'] == 1.0 and (info['stats'][:, 0] == 700).all()
    assert err[0] < 1e-12 and err[1] < 1e-12 and info['rmse'] < 1e-12
    up = lambda a: None if a is None else torch.from_numpy(np.array(a)).cuda()     # noqa: E731
    dq, dt, dinfo = alignment.register_clouds(up(s['source']), up(s['target']), up(nrm), max_dist=0.15, iterations=rounds, method=method)
    assert dq.is_cuda and dt.is_cuda and dinfo['stats'].is_cuda and dinfo['status'] == f3d.ICP_OK and dinfo['count'] == 700
    derr = R.pose_error(np.concatenate([dq.cpu().numpy(), dt.cpu().numpy()]), s['q_true'], s['t_true'])
    print(f'{method}, tensors: {derr[0]:.3e} m, {derr[1]:.3e} rad')
    assert derr[0] < 1e-12 and derr[1] < 1e-12
    # what the device route returned goes back into the module as it is: as a pose to apply, to evaluate, and to start from
    dmoved = alignment.transform_points(up(s['source']), dq, dt)
    assert dmoved.is_cuda and np.abs(dmoved.cpu().numpy() - s['target'][s['picked']]).max() < 1e-12
    dev_ev = alignment.evaluate_registration(up(s['source']), up(s['target']), 0.01, dq, dt)
    assert dev_ev['count'] == 700 and dev_ev['inlier_rmse'] < 1e-12 and same_ints(dev_ev['pairs'], s['picked'].astype(np.int32))
    rq, rt, rinfo = alignment.register_clouds(up(s['source']), up(s['target']), up(nrm), max_dist=0.05, wxyz=dq, t=dt, iterations=2, method=method)
    rerr = R.pose_error(np.concatenate([rq.cpu().numpy(), rt.cpu().numpy()]), s['q_true'], s['t_true'])
    assert rinfo['status'] == f3d.ICP_OK and rinfo['count'] == 700 and rerr[0] < 1e-12 and rerr[1] < 1e-12
    ev = alignment.evaluate_registration(s['source'], s['target'], 0.01, q, t)
    assert ev['count'] == 700 and ev['fitness'] == 1.0 and ev['inlier_rmse'] < 1e-12 and same_ints(ev['pairs'], s['picked'].astype(np.int32))
    moved = alignment.transform_points(s['source'], q, t)
    assert np.abs(moved - s['target'][s['picked']]).max() < 1e-12
    start = alignment.evaluate_registration(s['source'], s['target'], 0.01, IDENT, ZERO)
    assert start['fitness'] < 0.1


@pytest.mark.parametrize('method', ['plane', 'point'])
def test_two_stages_equal_two_chained_calls(ctx, corner, method):
    import torch
    s = corner
    nrm = s['normals'] if method == 'plane' else None
    kw = dict(min_pairs=50, method=method, center=False)
    q, t, info = alignment.register_clouds(s['source'], s['target'], nrm, max_dist=(0.3, 0.1), iterations=(3, 2), **kw)
    q1, t1, info1 = alignment.register_clouds(s['source'], s['target'], nrm, max_dist=0.3, iterations=3, **kw)
    q2, t2, info2 = alignment.register_clouds(s['source'], s['target'], nrm, max_dist=0.1, iterations=2, wxyz=q1, t=t1, **kw)
    assert same_bits(q, q2) and same_bits(t, t2) and same_bits(info['stats'], np.concatenate([info1['stats'], info2['stats']]))
    assert info['status'] == f3d.ICP_OK and info['stats'].shape == (5, 3) and not same_bits(q, q1)
    want1 = R.cloud_icp(s['source'], s['target'], nrm, R.PLANE if method == 'plane' else R.POINT, IDENT, ZERO, 0.3, 3, 50)
    assert same_bits(np.concatenate([q1, t1]), want1[0]) and same_bits(info1['stats'], want1[1])
    up = lambda a: None if a is None else torch.from_numpy(np.array(a)).cuda()     # noqa: E731
    dq, dt, dinfo = alignment.register_clouds(up(s['source']), up(s['target']), up(nrm), max_dist=(0.3, 0.1), iterations=(3, 2), **kw)
    assert same_bits(dq.cpu().numpy(), q) and same_bits(dt.cpu().numpy(), t) and same_bits(dinfo['stats'].cpu().numpy(), info['stats'])
    # with the centre folded in and out the rounds linearise about another point: the same scene, both near the truth after 5 rounds
    cq, ct, cinfo = alignment.register_clouds(s['source'], s['target'], nrm, max_dist=(0.3, 0.1), iterations=(3, 2), min_pairs=50, method=method)
    for pose in (np.concatenate([q, t]), np.concatenate([cq, ct])):
        err = R.pose_error(pose, s['q_true'], s['t_true'])
        print(f'{method}: {err[0]:.3e} m, {err[1]:.3e} rad after 3 + 2 rounds')
        assert err[0] < 1e-3 and err[1] < 1e-3
    assert cinfo['status'] == f3d.ICP_OK and not same_bits(cq, q)


# ------------------------------------------------------------------------------------------------ the hand-off from torch
@pytest.mark.parametrize('mode', MODES)
def test_the_device_functions_behind_a_stalled_stream(ctx, big, mode):
    """The caller's stream sleeps; behind the sleep the inputs, which hold a decoy, are overwritten with the scene; the two functions
    are enqueued, their outputs cloned on the stream, and the inputs overwritten with the decoy again.  The prepare step of a call
    reads the target's box back, so the first call returns only after the stall: what is asserted is that every result is the
    scene's, not the decoy's, which work on another stream, or work that ran before the caller's stream got there, would have read."""
    import torch
    b = big
    decoy = dict(source=np.roll(np.array(b['source']), 17, axis=0) + np.float32(0.01), target=np.array(b['target'])[::-1] * np.float32(1.01),
                 normals=np.roll(np.array(b['normals']), 5, axis=0))
    decoy_sums, _ = R.cloud_icp_sums(decoy['source'], decoy['target'], decoy['normals'], mode, b['q'], b['t'], MAX_DIST)
    assert not same_bits(decoy_sums, b[mode][0][0])                      # the decoy would have shown in the sums,
    decoy['source'][3, 1] = np.nan                                       # and in the prepare step, which refuses a NaN
    up = lambda d: {k: torch.from_numpy(np.ascontiguousarray(d[k])).cuda() for k in ('source', 'target', 'normals')}     # noqa: E731
    caller = torch.cuda.Stream()
    src_a, src_b, t = up(b), up(decoy), up(decoy)
    with torch.cuda.stream(caller):
        for k in src_a:                                                 # the unstalled warm-up: the scratch has grown, the scene passes
            t[k].copy_(src_a[k])
        warm = device_run(torch, ctx, t, b['q'], b['t'], mode, caller.cuda_stream)
        caller.synchronize()
        check_device(warm, b, mode)
        for k in src_b:
            t[k].copy_(src_b[k])
        torch.cuda.synchronize()
        S.stall(caller)
        for k in src_a:
            t[k].copy_(src_a[k])
        got = device_run(torch, ctx, t, b['q'], b['t'], mode, caller.cuda_stream)
        snapshot = {k: v.clone() for k, v in got.items()}
        for k in src_b:
            t[k].copy_(src_b[k])
    caller.synchronize()
    check_device(snapshot, b, mode)


@pytest.mark.parametrize('method', ['plane', 'point'])
def test_strided_sliced_offset_and_retyped_inputs(ctx, corner, method):
    """register_clouds from views into larger tensors (a column slice, every other row, an offset into a flat buffer) and from float32
    normals against the same call from contiguous float64 tensors; a float32 target stays float32 and gives the same bits as float64."""
    import torch
    s = corner
    up = lambda a: torch.from_numpy(np.array(a)).cuda()                 # noqa: E731
    nrm = up(s['normals']) if method == 'plane' else None
    kw = dict(max_dist=0.15, iterations=4, method=method)
    want = alignment.register_clouds(up(s['source']), up(s['target']), nrm, **kw)
    wide = torch.zeros((700, 7), dtype=torch.float64, device='cuda')
    wide[:, 2:5] = up(s['source'])
    rows = torch.zeros((2400, 3), dtype=torch.float32, device='cuda')
    rows[::2] = up(s['target']).to(torch.float32)
    snrm = None
    if method == 'plane':
        flat = torch.zeros(3600 + 5, dtype=torch.float32, device='cuda')
        flat[5:] = nrm.to(torch.float32).reshape(-1)
        snrm = flat[5:].reshape(1200, 3)
    source, target = wide[:, 2:5], rows[::2]
    assert not source.is_contiguous() and not target.is_contiguous() and target.dtype == torch.float32
    got = alignment.register_clouds(source, target, snrm, **kw)
    assert same_bits(got[0].cpu().numpy(), want[0].cpu().numpy()) and same_bits(got[1].cpu().numpy(), want[1].cpu().numpy())
    assert same_bits(got[2]['stats'].cpu().numpy(), want[2]['stats'].cpu().numpy()) and got[2]['status'] == want[2]['status'] == f3d.ICP_OK
