"""Feature fusion on the GPU (f3d_fuse_features*, f3d_features_finalize* and Fusion3DSeg.segUtils.features) against the test-only
restatement (tests/features_ref.py).  The sums are a fixed sequence of float32 adds, so they are compared bit for bit; only the
normalised rows have a tolerance, derived where it is used."""
import functools

import numpy as np
import pytest

import f3d
import features_ref as FR
import render_ref as R
from f3d import synth
from Fusion3DSeg.segUtils import features

pytestmark = pytest.mark.gpu
HW = (48, 40)                                                                  # (H, W) of the samples and the z-buffer
MAX_DEPTH = 10.0
F16_MAX = 65504.0
# per channel count one feature-map size (the cross product would not fit the memory or the time of a test): 1 / 7 / 9 / 65 rows are
# not 16-byte aligned, 7 .. 65 leave a partial group or a tail, 512 (float16) fills a group of 64, 520 and 512 (float32) need two slices
MAPS_BY_D = {1: (96, 80), 7: (12, 10), 8: (96, 80), 9: (7, 5), 64: (48, 40), 65: (12, 10), 512: (7, 5), 520: (12, 10)}
MAPS_BY_CASE = [(7, (96, 80)), (512, (12, 10)), (64, (7, 5)), (9, (48, 40)), (520, (7, 5)), (1, (12, 10)), (65, (48, 40)), (8, (96, 80))]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(got, want):
    return all(g.dtype == w.dtype and g.shape == w.shape and np.array_equal(_bits(g), _bits(w)) for g, w in zip(got, want))


@pytest.fixture(scope='module')
def ctx():
    return f3d.default_context(0)


@functools.lru_cache(maxsize=None)
def _scene(n, V, tol=0.05, splat=1):
    """A seeded cloud in the synth box under V ring cameras, and the visible samples of the restatement (shared, never modified)."""
    pts = synth.cloud(n, seed=100 + n)
    q, t = synth.ring_views(V)
    K = R.pinhole(*HW)
    views = f3d.views_build(K, HW[1], HW[0], q, t, MAX_DEPTH)
    return pts, K, q, t, views, FR.visible_samples(pts, K, q, t, HW, MAX_DEPTH, splat, tol)


def _feats(V, fhw, d, dtype, seed):
    """Normal values with a few whole rows at +-65504 (the largest float16): the conversion and the rounding of large float32 sums."""
    rng = np.random.default_rng(seed)
    f = rng.standard_normal((V, fhw[0], fhw[1], d), dtype=np.float32)
    flat = f.reshape(-1, d)
    rows = rng.choice(len(flat), size=max(1, len(flat) // 16), replace=False)
    flat[rows] = np.where(rng.random((len(rows), 1)) < 0.5, F16_MAX, -F16_MAX).astype(np.float32)
    return f.astype(dtype)


def _run(ctx, pts, views, feats, tol=0.05, per=0, splat=1, sums=None, counts=None):
    d = feats.shape[3]
    sums = np.zeros((len(pts), d), np.float32) if sums is None else sums
    counts = np.zeros(len(pts), np.int32) if counts is None else counts
    return ctx.fuse_features(sums, counts, pts, views, HW[0], HW[1], feats, splat, tol, per)


def _want(n, V, feats, tol=0.05):
    pts, K, q, t, views, vis = _scene(n, V, tol)
    return FR.fuse(pts, K, q, t, feats, HW, MAX_DEPTH, 1, tol, visible=vis)


@pytest.mark.parametrize('dtype', [np.float16, np.float32])
@pytest.mark.parametrize('d', sorted(MAPS_BY_D))
def test_sums_equal_the_restatement_for_every_row_shape(ctx, d, dtype):
    n, V = 1000, 130
    pts, K, q, t, views, vis = _scene(n, V)
    feats = _feats(V, MAPS_BY_D[d], d, dtype, seed=d)
    want = _want(n, V, feats)
    assert want[1].max() > 8 and (want[1] == 0).any()                           # many views per point, and points nobody sees
    for cloud in (pts, pts.astype(np.float32)):                                 # (synth clouds hold float32 values: one restatement)
        assert _same(_run(ctx, cloud, views, feats), want), cloud.dtype
    n, V = 257, 6                                                               # few views: a group's lanes project several points at once
    pts, K, q, t, views, vis = _scene(n, V)
    assert _same(_run(ctx, pts, views, feats[:V]), _want(n, V, feats[:V]))


@pytest.mark.parametrize('V', [1, 63, 64, 65, 130])
@pytest.mark.parametrize('n', [1, 63, 64, 65, 1000])
def test_sums_equal_the_restatement_for_every_size(ctx, n, V):
    pts, K, q, t, views, vis = _scene(n, V)
    case = [1, 63, 64, 65, 1000].index(n) * 5 + [1, 63, 64, 65, 130].index(V)
    for k in (case, case + 3):                                                  # two row shapes per size, all eight over the sizes
        d, fhw = MAPS_BY_CASE[k % 8]
        dtype = (np.float16, np.float32)[(case + k // 8) % 2]
        feats = _feats(V, fhw, d, dtype, seed=case)
        cloud = pts if k % 2 else pts.astype(np.float32)
        assert _same(_run(ctx, cloud, views, feats), _want(n, V, feats)), (d, fhw, dtype)


def test_more_tiles_than_blocks(ctx):
    """33000 points in groups of 64 lanes are 8250 tiles of 4 points, more than the grid has blocks: a block walks several tiles, and
    with 65 views it stages the view records again for each of them."""
    n, V, d = 33000, 65, 264
    pts, K, q, t, views, vis = _scene(n, V, 0.05, 0)
    feats = _feats(V, (7, 5), d, np.float16, seed=9)
    want = FR.fuse(pts, K, q, t, feats, HW, MAX_DEPTH, 0, 0.05, visible=vis)
    assert want[1].sum() > 1000
    assert _same(_run(ctx, pts.astype(np.float32), views, feats, splat=0), want)


@pytest.mark.parametrize('d,dtype', [(9, np.float16), (64, np.float16), (520, np.float32)])
def test_pass_size_and_call_split_change_no_bit(ctx, d, dtype):
    n, V = 1000, 65
    pts, K, q, t, views, vis = _scene(n, V)
    feats = _feats(V, (12, 10), d, dtype, seed=7)
    want = _want(n, V, feats)
    for per in (1, 7, 0):
        assert _same(_run(ctx, pts, views, feats, per=per), want), per
    for a in (1, 33, 64):
        s, c = _run(ctx, pts, views[:a], feats[:a])
        assert _same(_run(ctx, pts, views[a:], np.ascontiguousarray(feats[a:]), sums=s, counts=c), want), a


def test_device_route_in_a_strict_reserved_context():
    import torch
    n, V, d = 1000, 65, 64
    pts, K, q, t, views, vis = _scene(n, V)
    feats = _feats(V, (12, 10), d, np.float16, seed=11)
    want = _want(n, V, feats)
    own = f3d.Context(0)
    assert _same(_run(own, pts, views, feats), want)                            # the host route, before the context turns strict
    dev = torch.device('cuda', 0)
    s = torch.cuda.Stream(dev)
    dp, dv, df = torch.from_numpy(pts).to(dev), torch.from_numpy(views).to(dev), torch.from_numpy(feats).to(dev)
    sums = torch.zeros((n, d), dtype=torch.float32, device=dev)
    counts = torch.zeros(n, dtype=torch.int32, device=dev)
    out = torch.empty_like(sums)
    torch.cuda.synchronize(dev)
    own.reserve_render(n, V, *HW)
    own.set_strict(True)
    before = own.alloc_count
    for a, b, per in ((0, 20, 0), (20, 65, 3)):
        own.fuse_features_dev(dp.data_ptr(), f3d.F64, n, dv[a:b].data_ptr(), b - a, HW[0], HW[1], df[a:b].data_ptr(), f3d.FEAT_F16, 12, 10, d,
                              1, 0.05, sums.data_ptr(), counts.data_ptr(), per, s.cuda_stream)
    own.features_finalize_dev(sums.data_ptr(), counts.data_ptr(), n, d, False, out.data_ptr(), s.cuda_stream)
    assert own.alloc_count == before
    s.synchronize()
    assert _same((sums.cpu().numpy(), counts.cpu().numpy()), want)
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(FR.finalize(*want, normalize=False)))
    with pytest.raises(MemoryError):                                            # a larger image than reserved: strict says so
        own.fuse_features_dev(dp.data_ptr(), f3d.F64, n, dv.data_ptr(), V, 4 * HW[0], 4 * HW[1], df.data_ptr(), f3d.FEAT_F16, 12, 10, d, 1, 0.05,
                              sums.data_ptr(), counts.data_ptr(), 0, s.cuda_stream)
    own.fuse_features_dev(dp.data_ptr(), f3d.F64, n, dv.data_ptr(), V, 4 * HW[0], 4 * HW[1], df.data_ptr(), f3d.FEAT_F16, 12, 10, d, 1, np.inf,
                          sums.data_ptr(), counts.data_ptr(), 0, s.cuda_stream)   # depth_tol = inf renders nothing: no keys needed
    s.synchronize()
    assert own.alloc_count == before
    own.close()


def test_empty_inputs_and_bad_arguments(ctx):
    pts, K, q, t, views, vis = _scene(63, 1)
    feats = _feats(1, (7, 5), 9, np.float16, seed=1)
    sums, counts = np.full((63, 9), 2.5, np.float32), np.full(63, 3, np.int32)
    ctx.fuse_features(sums, counts, pts, views[:0], HW[0], HW[1], feats[:0])   # V = 0
    assert (sums == 2.5).all() and (counts == 3).all()
    e = ctx.fuse_features(np.zeros((0, 9), np.float32), np.zeros(0, np.int32), pts[:0], views, HW[0], HW[1], feats)   # n = 0
    assert e[0].shape == (0, 9) and e[1].shape == (0,)
    assert ctx.features_finalize(np.zeros((0, 9), np.float32), np.zeros(0, np.int32)).shape == (0, 9)
    for kw in (dict(splat=-1), dict(splat=9), dict(depth_tol=-0.1), dict(depth_tol=np.nan), dict(views_per_pass=-1)):
        with pytest.raises(ValueError, match='fuse_features'):
            ctx.fuse_features(sums, counts, pts, views, HW[0], HW[1], feats, **kw)
    with pytest.raises(ValueError, match='fuse_features'):
        ctx.fuse_features(sums, counts, pts, views, 0, HW[1], feats)
    assert (sums == 2.5).all() and (counts == 3).all()


def test_occlusion_on_two_walls(ctx):
    pts, far, K, q, t, masks, hw = R.two_walls()
    views = f3d.views_build(K, hw[1], hw[0], q, t, MAX_DEPTH)
    near_side = slice(0, 3)                                                     # the cameras at x = -1: the wall at x = 2 is the far one
    onehot = FR.one_hot(masks, 134)
    rng = np.random.default_rng(2)
    feats = rng.standard_normal((6, 24, 32, 9)).astype(np.float16)
    for tol in (0.05, np.inf):
        zero = lambda d: (np.zeros((len(pts), d), np.float32), np.zeros(len(pts), np.int32))   # noqa: E731
        got = ctx.fuse_features(*zero(9), pts, views[near_side], hw[0], hw[1], feats[near_side], 1, tol)
        want = FR.fuse(pts, K, q[near_side], t[near_side], feats[near_side], hw, MAX_DEPTH, 1, tol)
        assert _same(got, want)
        if tol == 0.05:
            assert (got[1][far] == 0).all() and (got[0][far] == 0).all() and (got[1][~far] > 0).all()
        else:
            assert (got[1][far] > 0).all()
        # one-hot maps are hard labels: the float64 votes of the existing kernel, exactly
        votes = ctx.vote_visible(np.zeros((len(pts), 134)), pts, views, masks, 1, tol)
        sums, counts = ctx.fuse_features(*zero(134), pts, views, hw[0], hw[1], onehot, 1, tol)
        assert np.array_equal(features.soft_votes(sums), votes) and np.array_equal(counts, votes.sum(axis=1).astype(np.int32))
        assert np.array_equal(ctx.segment_votes(features.soft_votes(sums), 133), ctx.segment_votes(votes, 133))


@pytest.mark.parametrize('d', [1, 7, 64, 65, 520])
def test_finalize(ctx, d):
    n, V = 1000, 63
    pts, K, q, t, views, vis = _scene(n, V)
    feats = _feats(V, (12, 10), d, np.float16, seed=d + 1)
    sums, counts = _want(n, V, feats)
    sums[5] = 0                                                                 # a seen point whose mean is the zero row
    assert counts[5] > 0 and (counts == 0).any()
    mean = ctx.features_finalize(sums, counts, normalize=False)
    assert np.array_equal(_bits(mean), _bits(FR.finalize(sums, counts, False)))
    assert (mean[counts == 0] == 0).all()
    # The two float64 sums of squares differ by at most d * 2^-53 relative (any order of d non-negative terms), the square roots and
    # the float64 quotients by a few 2^-53 more: far inside a float32 rounding interval, so the rounded float32 quotients are equal or,
    # at a rounding boundary, neighbours: 1 ulp.
    unit, want = ctx.features_finalize(sums, counts, normalize=True), FR.finalize(sums, counts, True)
    assert np.isfinite(unit).all()
    assert (np.abs(unit - want) <= np.spacing(np.abs(want))).all()
    assert (unit[counts == 0] == 0).all() and (unit[5] == 0).all()
    seen = counts > 0
    seen[5] = False
    assert np.allclose(np.linalg.norm(unit[seen].astype(np.float64), axis=1), 1.0, atol=1e-6)
    inplace = sums.copy()
    assert ctx.features_finalize(inplace, counts, normalize=True, out=inplace) is inplace
    assert np.array_equal(_bits(inplace), _bits(unit))


def test_feature_fusion_in_chunks_equals_one_call(ctx):
    import torch
    n, V, d = 1000, 65, 65
    pts, K, q, t, views, vis = _scene(n, V)
    feats = _feats(V, (12, 10), d, np.float16, seed=3)
    want = _want(n, V, feats)
    one = features.fuse_features(pts, K, q, t, feats, hw=HW, max_depth=MAX_DEPTH)
    assert _same(one, want)
    fus = features.FeatureFusion(pts, HW, max_depth=MAX_DEPTH)
    for a, b in ((0, 7), (7, 40), (40, 65)):
        assert fus.add(K, q[a:b], t[a:b], feats[a:b]) is fus
    assert _same((fus.sums, fus.counts), want)
    assert np.array_equal(_bits(fus.features(normalize=False)), _bits(FR.finalize(*want, normalize=False)))
    dev = torch.device('cuda', 0)                                               # device tensors in, device tensors out
    dfus = features.FeatureFusion(torch.from_numpy(pts).to(dev), HW, max_depth=MAX_DEPTH)
    for a, b in ((0, 7), (7, 40), (40, 65)):
        dfus.add(K, q[a:b], t[a:b], torch.from_numpy(feats[a:b]).to(dev))
    assert dfus.sums.is_cuda and dfus.counts.is_cuda and dfus.features().is_cuda
    assert _same((dfus.sums.cpu().numpy(), dfus.counts.cpu().numpy()), want)
    assert np.array_equal(_bits(dfus.features().cpu().numpy()), _bits(fus.features()))
    # maps at their own size: hw defaults to (hf, wf)
    own = features.fuse_features(pts, R.pinhole(12, 10), q[:4], t[:4], feats[:4], max_depth=MAX_DEPTH)
    assert _same(own, FR.fuse(pts, R.pinhole(12, 10), q[:4], t[:4], feats[:4], (12, 10), MAX_DEPTH))


def test_classify_features_recovers_the_label_map(ctx):
    """Feature maps that hold the text embedding of each pixel's label, orthonormal texts: a point's score for text k is the share of
    its visible samples labelled k (over the length of the shares), so the best text is the label most of its pixels carry."""
    import torch
    pts, far, K, q, t, masks, hw = R.two_walls()
    pts = np.concatenate([pts, [[50.0, 0, 0], [0, 50.0, 0]]])                   # two points outside every frustum
    T, d = 5, 16
    text = np.linalg.qr(np.random.default_rng(4).standard_normal((d, d)))[0][:T].astype(np.float32)
    labels = ((np.arange(hw[1])[None, None, :] // 16 + (np.arange(6)[:, None, None] >= 3)) % T) * np.ones((1, hw[0], 1), np.int64)
    votes = R.visible_votes(pts, K, q, t, labels.astype(np.uint8), MAX_DEPTH, 1, 0.05, ncols=T)
    fus = features.FeatureFusion(pts, hw, max_depth=MAX_DEPTH).add(K, q[:2], t[:2], text[labels[:2]]).add(K, q[2:], t[2:], text[labels[2:]])
    assert np.array_equal(fus.counts, votes.sum(axis=1).astype(np.int32))
    f = fus.features()
    got, score = features.classify_features(f, text, chunk=300)
    assert got.dtype == np.int64 and score.dtype == np.float32 and got.shape == score.shape == (len(pts),)
    unseen = fus.counts == 0
    assert unseen[-2:].all() and (got[unseen] == -1).all() and (score[unseen] == 0).all()
    top2 = np.sort(votes, axis=1)[:, -2:]
    clear = top2[:, 1] > top2[:, 0]                                             # a unique most frequent label
    assert clear.sum() > 0.5 * len(pts) and not clear[unseen].any()
    assert np.array_equal(got[clear], np.argmax(votes, axis=1)[clear])
    assert np.allclose(score[~unseen], votes[~unseen].max(axis=1) / np.linalg.norm(votes[~unseen], axis=1), atol=1e-5)
    g2, s2 = features.classify_features(f, text, counts=fus.counts)
    assert np.array_equal(g2, got) and np.array_equal(s2, score)
    dg, ds = features.classify_features(torch.from_numpy(f).to('cuda:0'), torch.from_numpy(text).to('cuda:0'), chunk=512)
    assert dg.is_cuda and ds.is_cuda and np.array_equal(dg.cpu().numpy(), got)
