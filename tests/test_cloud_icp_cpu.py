"""CPU-side checks of cloud-to-cloud ICP: the bindings exist and match the header, the device twins live in f3d.clouds, argument errors
need no device, the public surface of segUtils.alignment, and the restatement (tests/cloud_icp_ref.py): its sums against plain
J.T @ J sums, its point mode at the identity, and its convergence on the exact-subset scene."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

import f3d
import cloud_icp_ref as R
import icp_ref as I
from f3d import clouds as CL
from Fusion3DSeg.segUtils import alignment, registration

PAIRS = [('f3d_cloud_icp_sums', 'f3d_cloud_icp_sums_dev'), ('f3d_cloud_icp', 'f3d_cloud_icp_dev')]
IDENT = np.array([1.0, 0.0, 0.0, 0.0])
ZERO = np.zeros(3)


# ------------------------------------------------------------------------------------------------ bindings
def test_symbols_are_declared_and_bound():
    from conftest import ROOT
    text = (ROOT / 'include' / 'f3d.h').read_text()
    lib = f3d.library()
    for name in [n for pair in PAIRS for n in pair] + ['f3d_ctx_reserve_cloud_icp']:
        assert re.search(rf'\bint {name}\(f3d_ctx\* ctx', text), name
        fn = getattr(lib, name)
        assert name in lib._f3d_symbols
        assert fn.restype is C.c_int and fn.argtypes and fn.argtypes[0] is C.c_void_p
    for host, dev in PAIRS:
        assert list(getattr(lib, dev).argtypes) == list(getattr(lib, host).argtypes) + [C.c_void_p]
    assert int(re.search(r'#define F3D_CLOUD_ICP_PLANE (\S+)', text).group(1)) == f3d.CLOUD_ICP_PLANE == R.PLANE == 0
    assert int(re.search(r'#define F3D_CLOUD_ICP_POINT (\S+)', text).group(1)) == f3d.CLOUD_ICP_POINT == R.POINT == 1


def test_the_device_twins_live_in_f3d_clouds():
    for name in ('cloud_icp_sums', 'cloud_icp', 'reserve_cloud_icp'):
        assert callable(getattr(f3d.Context, name))
    assert not [n for n in dir(f3d.Context) if 'cloud_icp' in n and n.endswith('_dev')]
    assert CL.__all__ == ['cloud_icp_sums_dev', 'cloud_icp_dev', 'register_tensors']
    for name in CL.__all__:
        assert list(inspect.signature(getattr(CL, name)).parameters)[0] == 'ctx'
    assert 'route_cases' in CL.__doc__ and 'follow-up' in CL.__doc__


def test_public_surface():
    assert alignment.__all__ == ['register_clouds', 'evaluate_registration', 'transform_points']
    assert registration.__all__ == ['raycast', 'icp_sums', 'icp', 'track_frames']          # unchanged
    p = inspect.signature(alignment.register_clouds).parameters
    assert list(p) == ['source', 'target', 'target_normals', 'max_dist', 'wxyz', 't', 'iterations', 'min_pairs', 'method', 'center']
    assert (p['target_normals'].default, p['max_dist'].default, p['iterations'].default, p['min_pairs'].default, p['method'].default,
            p['center'].default) == (None, 0.1, 30, 100, 'plane', True)
    assert list(inspect.signature(alignment.evaluate_registration).parameters) == ['source', 'target', 'max_dist', 'wxyz', 't']
    assert list(inspect.signature(alignment.transform_points).parameters) == ['points', 'wxyz', 't']


# ------------------------------------------------------------------------------------------------ argument errors
def test_argument_errors_need_no_device():
    """A Context that was never opened has no library handle: a call that got past the checks fails with AttributeError."""
    ctx = object.__new__(f3d.Context)
    src, tgt, nrm = np.zeros((5, 3)), np.ones((7, 3)), np.tile([0.0, 0.0, 1.0], (7, 1))
    good = dict(source=src, target=tgt, target_normals=nrm, mode=f3d.CLOUD_ICP_PLANE, q_wxyz=IDENT, t=ZERO, max_dist=0.1)
    bads = [dict(mode=2), dict(mode=-1), dict(target_normals=None), dict(max_dist=0.0), dict(max_dist=-1.0), dict(max_dist=float('nan')),
            dict(max_dist=float('inf')), dict(max_dist=1e300), dict(q_wxyz=np.zeros(4)), dict(q_wxyz=[1.0, np.nan, 0.0, 0.0]),
            dict(q_wxyz=[1.0, 0.0, 0.0]), dict(t=[0.0, np.inf, 0.0]), dict(t=[0.0, 0.0]), dict(target=np.zeros((0, 3))),
            dict(source=np.zeros((5, 2))), dict(target=np.zeros(7)), dict(target_normals=np.zeros((6, 3)))]
    for bad in bads:
        with pytest.raises(ValueError):
            ctx.cloud_icp_sums(**{**good, **bad})
        with pytest.raises(ValueError):
            ctx.cloud_icp(**{**good, **bad})
    for bad in [dict(iterations=0), dict(iterations=-3), dict(min_pairs=5), dict(min_pairs=0)]:
        with pytest.raises(ValueError):
            ctx.cloud_icp(**{**good, **bad})
    for bad in [(-1, 5), (5, -1), (2 ** 31, 5), (5, 2 ** 31)]:
        with pytest.raises(ValueError):
            ctx.reserve_cloud_icp(*bad)
    with pytest.raises(AttributeError):
        ctx.cloud_icp_sums(**good)
    with pytest.raises(AttributeError):
        ctx.cloud_icp(**{**good, 'mode': f3d.CLOUD_ICP_POINT, 'target_normals': None})      # point mode reads no normals
    with pytest.raises(AttributeError):
        ctx.reserve_cloud_icp(7, 5)
    # the device-pointer functions: the same checks, pointers are plain integers here
    dev = dict(source_ptr=256, source_dtype=f3d.F64, n=5, target_ptr=512, target_dtype=f3d.F32, m=7, normals_ptr=768, mode=f3d.CLOUD_ICP_PLANE,
               q_wxyz=IDENT, t=ZERO, max_dist=0.1)
    for bad in [dict(mode=3), dict(normals_ptr=None), dict(max_dist=0.0), dict(max_dist=1e300), dict(q_wxyz=np.zeros(4)), dict(t=[np.nan, 0, 0]),
                dict(m=0), dict(n=-1), dict(n=2 ** 31), dict(m=2 ** 31)]:
        with pytest.raises(ValueError):
            CL.cloud_icp_sums_dev(ctx, **{**dev, **bad}, sums_ptr=1024)
        with pytest.raises(ValueError):
            CL.cloud_icp_dev(ctx, **{**dev, **bad}, iterations=2, min_pairs=6, pose_ptr=1024, stats_ptr=2048)
    for bad in [dict(iterations=0), dict(min_pairs=5)]:
        with pytest.raises(ValueError):
            CL.cloud_icp_dev(ctx, **dev, **{**dict(iterations=2, min_pairs=6), **bad}, pose_ptr=1024, stats_ptr=2048)
    with pytest.raises(AttributeError):
        CL.cloud_icp_sums_dev(ctx, **dev, sums_ptr=1024)
    with pytest.raises(AttributeError):
        CL.cloud_icp_dev(ctx, **dev, iterations=2, min_pairs=6, pose_ptr=1024, stats_ptr=2048)


def test_alignment_errors_come_before_any_device_call():
    src, tgt, nrm = np.zeros((5, 3)), np.ones((7, 3)), np.tile([0.0, 0.0, 1.0], (7, 1))
    for bad in [dict(method='plane'), dict(method='colour', target_normals=nrm), dict(target_normals=nrm, max_dist=0.0),
                dict(target_normals=nrm, max_dist=(0.3, 0.2), iterations=(5, 5, 5)), dict(target_normals=nrm, iterations=0),
                dict(target_normals=nrm, min_pairs=5), dict(target_normals=nrm, wxyz=(0, 0, 0, 0)), dict(method='point', t=(0, np.nan, 0)),
                dict(method='point', max_dist=(0.3, -0.1))]:
        with pytest.raises(ValueError):
            alignment.register_clouds(src, tgt, **bad)
    assert alignment._stages(0.1, 30) == ([0.1], [30]) and alignment._stages((0.3, 0.1), 5) == ([0.3, 0.1], [5, 5])
    assert alignment._stages(0.2, (4, 6)) == ([0.2, 0.2], [4, 6])


def test_transform_points_and_the_centre_fold():
    """transform_points is rotate-then-translate, and subtracting a centre c from the source turns (q, t) into (q, t + R c)."""
    rng = np.random.default_rng(0)
    p, c = rng.normal(size=(40, 3)) + 5.0, np.array([5.0, 5.1, 4.9])
    q, t = I.moved(IDENT, ZERO, (0.2, -0.5, 0.7), 25.0, np.array([0.3, -0.2, 0.1]))
    from oracle import np_ref as O
    want = O.rotate(I.normalise(q), p) + t
    assert np.abs(alignment.transform_points(p, q, t) - want).max() <= 1e-13
    assert np.abs(alignment.transform_points(p, 3.0 * np.asarray(q), t) - want).max() <= 1e-13          # the quaternion need not be unit
    import torch
    moved = alignment.transform_points(torch.from_numpy(p), torch.from_numpy(np.asarray(q)), torch.from_numpy(t))     # tensors for the pose too
    assert isinstance(moved, torch.Tensor) and np.abs(moved.numpy() - want).max() <= 1e-13
    for bad in (np.zeros((4, 2)), torch.zeros((4, 2)), torch.zeros(6)):
        with pytest.raises(ValueError):
            alignment.transform_points(bad, q, t)
    assert not [n for n in dir(f3d) if 'cloud_icp_check' in n and not n.startswith('_')]                 # the shared check is private
    assert np.abs(alignment.transform_points(p - c, q, t + f3d._quat_matrix(q) @ c) - want).max() <= 1e-13


# ------------------------------------------------------------------------------------------------ the restatement
def plain_sums(source, target, normals, mode, q, t, max_dist):
    """The 29 sums from stacked Jacobian rows and NumPy's own reductions: J.T @ J, J.T @ r, r @ r, the count."""
    from oracle import np_ref as O
    pr = O.rotate(I.normalise(q), np.asarray(source, np.float64))
    p = pr + np.asarray(t, np.float64)
    pairs = R.nearest(p, target, max_dist)
    ok = pairs >= 0
    e = (p - np.asarray(target, np.float64)[pairs])[ok]
    pr = pr[ok]
    if mode == R.PLANE:
        N = np.asarray(normals, np.float64)[pairs[ok]]
        J, r = np.concatenate([np.cross(pr, N), N], axis=1), (N * e).sum(axis=1)
    else:
        J = np.concatenate([np.concatenate([np.cross(pr, np.tile(np.eye(3)[a], (len(pr), 1))), np.tile(np.eye(3)[a], (len(pr), 1))], axis=1)
                            for a in range(3)])
        r = np.concatenate([e[:, a] for a in range(3)])
    A, b = J.T @ J, J.T @ r
    return np.concatenate([[A[a, c] for a in range(6) for c in range(a, 6)], b, [r @ r, float(ok.sum())]])


@pytest.mark.parametrize('mode', [R.PLANE, R.POINT])
@pytest.mark.parametrize('n', [1, 63, 257, 700])
def test_restated_sums_agree_with_plain_sums(mode, n):
    source, target, normals, q, t = R.cloud_pair(n)
    sums, pairs = R.cloud_icp_sums(source, target, normals, mode, q, t, 0.08)
    want = plain_sums(source, target, normals, mode, q, t, 0.08)
    assert sums[28] == want[28] == (pairs >= 0).sum() and 0 < sums[28]
    scale = np.abs(want).max()
    assert np.abs(sums - want).max() <= 1e-12 * scale
    # the order of the restated terms: one array is icp_ref.shaped_sums itself
    rows, _ = R.terms(source, target, normals, R.PLANE, q, t, 0.08)
    assert len(rows) == 1 and np.array_equal(R.shaped_sums(rows), I.shaped_sums(rows[0]))


def test_restated_nearest_breaks_ties_by_index_and_respects_the_radius():
    target = np.array([[1.0, 0.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 3.0, 0.0]])
    p = np.array([[0.0, 0.0, 0.0], [0.0, 2.0, 0.0], [0.0, 10.0, 0.0], [0.5, 0.0, 0.0]])
    assert R.nearest(p, target, 1.0).tolist() == [0, 2, -1, 0]             # three targets at distance 1: the lowest index; 1.0 is inclusive
    assert R.nearest(p, target[[1, 0, 3, 2]], 1.0).tolist() == [0, 2, -1, 1]
    assert R.nearest(p, target, 0.4).tolist() == [-1, -1, -1, -1]
    assert R.nearest(np.zeros((0, 3)), target, 1.0).shape == (0,)


def test_point_mode_at_the_identity_has_no_residual():
    _, target, _, _, _ = R.cloud_pair(5)
    sums, pairs = R.cloud_icp_sums(target, target, None, R.POINT, IDENT, ZERO, 0.05)
    assert sums[27] == 0.0 and sums[28] == len(target) and np.array_equal(pairs, np.arange(len(target)))
    assert np.array_equal(sums[21:27], np.zeros(6)) and sums[15] == sums[18] == sums[20] == len(target)
    assert np.array_equal(R.cloud_icp_sums(np.zeros((0, 3)), target, None, R.POINT, IDENT, ZERO, 0.05)[0], np.zeros(29))
    pose, stats, status = R.cloud_icp(np.zeros((0, 3)), target, None, R.POINT, IDENT, ZERO, 0.05, 3, 6)
    assert status == I.LOST and np.array_equal(stats, [[0.0, 0.0, 1.0]] * 3) and np.array_equal(pose, np.concatenate([IDENT, ZERO]))


@pytest.fixture(scope='module')
def corner():
    s = R.corner_scene()
    for a in s.values():
        a.setflags(write=False)
    return s


def test_the_corner_scene_is_what_it_says(corner):
    s = corner
    assert s['target'].shape == (1200, 3) and s['source'].shape == (700, 3) and s['normals'].shape == (1200, 3)
    assert np.array_equal(s['target'], s['target'].astype(np.float32).astype(np.float64))
    assert len(np.unique(s['picked'])) == 700
    from oracle import np_ref as O
    back = O.rotate(s['q_true'], s['source']) + s['t_true']
    assert np.abs(back - s['target'][s['picked']]).max() <= 8 * np.spacing(2.0)           # a few ulp of 2 m
    assert abs(I.rotation_angle(s['q_true'], IDENT) - np.radians(2.0)) < 1e-12 and abs(np.linalg.norm(s['t_true']) - 0.03) < 1e-15
    along = (s['target'] * s['normals']).sum(axis=1)                                    # the coordinate along the point's normal
    assert ((along == -1.0) | (along == -0.75)).all() and (along == -0.75).sum() == 150


@pytest.mark.parametrize('mode, rounds', [(R.PLANE, 12), (R.POINT, 30)])
def test_the_restatement_converges_on_the_exact_subset_scene(corner, mode, rounds):
    """At the true pose every source point coincides with a target point up to the rounding of building it (a few ulp of 2 m), so the
    fixed point is within ~1e-15 of the truth: translation error < 1e-12 m, rotation angle < 1e-12 rad, all n paired, every round OK.
    Measured with this restatement: 5.2e-16 m / 0 rad (plane, 12 rounds), 8.1e-17 m / 0 rad (point, 30 rounds)."""
    s = corner
    pose, stats, status = R.cloud_icp(s['source'], s['target'], s['normals'], mode, IDENT, ZERO, 0.15, rounds, 100)
    err = R.pose_error(pose, s['q_true'], s['t_true'])
    print(f'mode {mode}: {err[0]:.3e} m, {err[1]:.3e} rad, status {status}, sum r^2 per round {stats[:, 1]}')
    assert status == I.OK and (stats[:, 2] == I.OK).all() and (stats[:, 0] == 700).all()
    assert err[0] < 1e-12 and err[1] < 1e-12
    _, pairs = R.cloud_icp_sums(s['source'], s['target'], s['normals'], mode, pose[:4], pose[4:], 0.15)
    assert np.array_equal(pairs, s['picked'])
