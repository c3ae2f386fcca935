"""Feature fusion without a device: the NumPy restatement (tests/features_ref.py) against the hard-label restatement it generalises,
the feature-pixel rule, the Python-level argument checks and the C-ABI symbols."""
import ctypes as C

import numpy as np
import pytest

import f3d
import features_ref as FR
import render_ref as R
from f3d import synth
from Fusion3DSeg.segUtils import features, voting


def _two_walls():
    pts, far, K, q, t, masks, hw = R.two_walls()
    return pts, K, q, t, masks, hw, 10.0


def _c1():
    sc = synth.scene('C1', n=2000)
    return sc['points'], sc['K'], sc['wxyzs'], sc['translations'], sc['masks'], (sc['h'], sc['w']), sc['max_depth']


@pytest.mark.parametrize('scene', [_two_walls, _c1])
def test_one_hot_maps_give_the_hard_votes(scene):
    pts, K, q, t, masks, hw, md = scene()
    for tol in (0.05, np.inf):
        votes = R.visible_votes(pts, K, q, t, masks, md, 1, tol, ncols=134)
        sums, counts = FR.fuse(pts, K, q, t, FR.one_hot(masks, 134), hw, md, 1, tol)
        assert sums.dtype == np.float32 and counts.dtype == np.int32
        assert votes.sum() > 0
        assert np.array_equal(sums.astype(np.float64), votes)
        assert np.array_equal(counts, votes.sum(axis=1).astype(np.int32))
        assert np.array_equal(features.soft_votes(sums), votes) and features.soft_votes(sums).dtype == np.float64


def test_split_over_calls_equals_one_call():
    pts, K, q, t, masks, hw, md = _c1()
    rng = np.random.default_rng(5)
    feats = rng.standard_normal((len(t), 12, 16, 9)).astype(np.float16)
    whole = FR.fuse(pts, K, q, t, feats, hw, md)
    for a in (1, 3):
        part = FR.fuse(pts, K, q[:a], t[:a], feats[:a], hw, md)
        both = FR.fuse(pts, K, q[a:], t[a:], feats[a:], hw, md, sums=part[0], counts=part[1])
        assert np.array_equal(both[0].view(np.uint32), whole[0].view(np.uint32)) and np.array_equal(both[1], whole[1])
    assert whole[1].max() > 1                                                 # (sums of several views: the order of the adds matters)


@pytest.mark.parametrize('w,wf', [(40, 40), (40, 10), (40, 5), (40, 80), (40, 7), (48, 7), (7, 48), (5, 3), (3, 5), (960, 180), (720, 240), (1, 4)])
def test_feature_pixel_is_resize_nearest(w, wf):
    """uf = u * wf // w picks the source pixel cv2's INTER_NEAREST (voting.resize_nearest) picks when the feature map is resized to w."""
    index = np.arange(wf, dtype=np.int64)[None, :].repeat(2, axis=0)           # an index image [2, wf]
    resized = voting.resize_nearest(index, w, 2)
    uf, vf = FR.feature_pixel(np.arange(w), np.zeros(w, np.int64), (2, w), (2, wf))
    assert np.array_equal(resized[0], uf) and uf.min() >= 0 and uf.max() < wf
    column = np.arange(wf, dtype=np.int64)[:, None].repeat(2, axis=1)          # and the rows, [wf, 2]
    uf, vf = FR.feature_pixel(np.zeros(w, np.int64), np.arange(w), (w, 2), (wf, 2))
    assert np.array_equal(voting.resize_nearest(column, 2, w)[:, 0], vf)


def _good(n=5, V=2, d=4):
    return np.zeros((n, d), np.float32), np.zeros(n, np.int32), np.zeros((V, 3, 3, d), np.float16)


def test_argument_checks_raise_before_any_device_call():
    sums, counts, feats = _good()
    assert f3d.features_check(sums, counts, feats, 2, 5) == f3d.FEAT_F16
    assert f3d.features_check(sums, counts, feats.astype(np.float32), 2, 5) == f3d.FEAT_F32
    assert f3d.features_check(sums, counts) is None
    with pytest.raises(TypeError):
        f3d.features_check(sums.astype(np.float64), counts, feats)
    with pytest.raises(TypeError):
        f3d.features_check(sums, counts.astype(np.int64), feats)
    with pytest.raises(TypeError):
        f3d.features_check(sums, counts, feats.astype(np.float64))
    with pytest.raises(TypeError):
        f3d.features_check(sums, counts, feats.astype(np.uint8))
    with pytest.raises(ValueError):
        f3d.features_check(np.zeros((5, 8), np.float32)[:, ::2], counts, feats)            # non-contiguous sums
    with pytest.raises(ValueError):
        f3d.features_check(sums, counts, feats, 3, 5)                                       # V mismatch
    with pytest.raises(ValueError):
        f3d.features_check(sums, counts, feats, 2, 6)                                       # rows != points
    with pytest.raises(ValueError):
        f3d.features_check(sums, counts[:4], feats)
    with pytest.raises(ValueError):
        f3d.features_check(sums, counts, np.zeros((2, 3, 3, 5), np.float16))               # channels differ
    with pytest.raises(ValueError):
        f3d.features_check(sums, counts, np.zeros((2, 3, 3, 8), np.float16)[..., ::2])     # non-contiguous feats
    for d in (0, 4097):
        with pytest.raises(ValueError):
            f3d.features_check(np.zeros((5, d), np.float32), counts, np.zeros((2, 3, 3, d), np.float16))


def test_wrappers_check_before_they_need_a_device():
    """None of these reaches default_context(): without a device that would raise F3DUnavailable instead."""
    pts = np.zeros((5, 3))
    K, q, t = np.eye(3), np.tile([1.0, 0, 0, 0], (2, 1)), np.zeros((2, 3))
    sums, counts, feats = _good()
    with pytest.raises(TypeError):
        features.fuse_features(pts, K, q, t, feats.astype(np.float64))
    with pytest.raises(TypeError):
        features.fuse_features(pts, K, q, t, feats, sums=sums, counts=counts.astype(np.int64))
    with pytest.raises(TypeError):
        features.fuse_features(pts, K, q, t, feats, sums=sums.astype(np.float64), counts=counts)
    with pytest.raises(ValueError):
        features.fuse_features(pts, K, q, t, feats, sums=np.zeros((5, 8), np.float32)[:, ::2], counts=counts)
    with pytest.raises(ValueError):
        features.fuse_features(pts, K, q[:1], t[:1], feats)                                 # 1 view, 2 maps
    for d in (0, 4097):
        with pytest.raises(ValueError):
            features.fuse_features(pts, K, q, t, np.zeros((2, 3, 3, d), np.float16))
    with pytest.raises(ValueError):
        features.fuse_features(pts, K, q, t, feats[0])                                      # not [V, hf, wf, d]
    with pytest.raises(ValueError):
        features.fuse_features(pts, K, q, t, feats, sums=sums)                              # sums without counts
    fus = features.FeatureFusion(pts, (4, 4))
    with pytest.raises(ValueError):
        fus.features()
    with pytest.raises(ValueError):
        features.classify_features(np.zeros((3, 4), np.float32), np.zeros((2, 5), np.float32))


def test_new_symbols_are_declared_and_typed():
    lib = f3d.library()
    i32, i64, dbl, vp = C.c_int32, C.c_int64, C.c_double, C.c_void_p
    fuse = [vp, vp, i32, i64, vp, i32, i32, i32, vp, i32, i32, i32, i32, i32, dbl, vp, vp, i32]
    fin = [vp, vp, vp, i64, i32, i32, vp]
    for name, args in (('f3d_fuse_features', fuse), ('f3d_fuse_features_dev', fuse + [vp]), ('f3d_features_finalize', fin),
                       ('f3d_features_finalize_dev', fin + [vp])):
        fn = getattr(lib, name)
        assert name in lib._f3d_symbols and list(fn.argtypes) == args and fn.restype is i32, name
    assert (f3d.FEAT_F16, f3d.FEAT_F32, f3d.FEAT_MAX_D) == (0, 1, 4096)
    assert set(features.__all__) == {'fuse_features', 'FeatureFusion', 'soft_votes', 'classify_features'}
    for name in ('fuse_features', 'fuse_features_dev', 'features_finalize', 'features_finalize_dev'):
        assert callable(getattr(f3d.Context, name))


def test_finalize_restatement():
    sums = np.array([[3, 4], [0, 0], [1, 1], [6, 8]], np.float32)
    counts = np.array([1, 2, 0, 2], np.int32)
    assert np.array_equal(FR.finalize(sums, counts, False), np.array([[3, 4], [0, 0], [0, 0], [3, 4]], np.float32))
    assert np.array_equal(FR.finalize(sums, counts, True), np.array([[0.6, 0.8], [0, 0], [0, 0], [0.6, 0.8]], np.float32))
