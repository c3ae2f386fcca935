"""Occlusion-aware forward voting on the GPU: the point-splat z-buffer (f3d_render_lookups*), the visibility-tested vote
(f3d_vote_visible*) and their Fusion3DSeg.fusion entry points against the test-only restatement (tests/render_ref.py).  The contract
is deterministic, so every comparison is array_equal."""
import numpy as np
import pytest

import f3d
import render_ref as R
from f3d import synth
from Fusion3DSeg import fusion
from oracle import np_ref as O

pytestmark = pytest.mark.gpu
IMAGES = ((5, 7), (24, 40))                                                    # (H, W): many points share each pixel
MAX_DEPTH = 10.0


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


@pytest.fixture(scope='module')
def ctx():
    return f3d.default_context(0)


def _views(K, hw, q, t):
    return f3d.views_build(K, hw[1], hw[0], q, t, MAX_DEPTH)


def _votes(ctx, pts, views, masks, splat, tol, per=0, ncols=134):
    return ctx.vote_visible(np.zeros((len(pts), ncols)), pts, views, masks, splat, tol, per)


@pytest.mark.parametrize('V', [1, 2, 65])
@pytest.mark.parametrize('n', [1, 63, 64, 65, 257, 5000])
def test_lookups_and_votes_equal_the_restatement(ctx, n, V):
    """Seeded clouds in the synth box, ring cameras; both images, splat 0 / 1 / 2 (the patches clip at the borders of these small
    images), float64 and float32 storage (synth clouds hold float32 values, so one restatement serves both)."""
    pts = synth.cloud(n, seed=100 + n)
    q, t = synth.ring_views(V)
    for hw in IMAGES:
        K, masks = R.pinhole(*hw), synth.masks(V, hw[0], hw[1], 'iid', seed=n + V)
        views = _views(K, hw, q, t)
        for splat in (0, 1, 2):
            depth, uv2pt = R.lookups(pts, K, q, t, hw, MAX_DEPTH, splat)
            votes = R.visible_votes(pts, K, q, t, masks, MAX_DEPTH, splat, 0.05)
            for cloud in (pts, pts.astype(np.float32)):
                gd, gl = ctx.render_lookups(cloud, views, hw[0], hw[1], splat)
                assert _same(gd, depth) and _same(gl, uv2pt), (hw, splat, cloud.dtype)
                assert _same(_votes(ctx, cloud, views, masks, splat, 0.05), votes), (hw, splat, cloud.dtype)


def test_contended_pixels():
    """300k points x 2 wide views onto 64 x 48: 72 samples per pixel (the ring cameras stand inside the cloud's box, so the points behind
    them have none), past one grid-stride round, losing atomics the common case."""
    hw, n = (48, 64), 300_000
    pts = synth.cloud(n, seed=77)
    q, t = synth.ring_views(2)
    K, masks = R.pinhole(*hw, 0.3 * hw[1]), synth.masks(2, hw[0], hw[1], 'iid')
    depth, uv2pt = R.lookups(pts, K, q, t, hw, MAX_DEPTH, 1)
    nsamples = O.forward_votes(pts, K, q, t, masks, MAX_DEPTH).sum()
    assert nsamples > 70 * 2 * hw[0] * hw[1] and (uv2pt >= 0).all()
    gd, gl = fusion.render_lookups(pts, K, q, t, hw, MAX_DEPTH, 1)
    assert _same(gd, depth) and _same(gl, uv2pt)
    got = fusion.project_vote_argmax_visible(pts, K, q, t, masks, MAX_DEPTH, return_votes=True, splat=1, depth_tol=0.05)[1]
    assert _same(got, R.visible_votes(pts, K, q, t, masks, MAX_DEPTH, 1, 0.05))


def test_ties_go_to_the_lowest_index(ctx):
    hw = (24, 40)
    q, t = synth.ring_views(2)
    K, views = R.pinhole(*hw), _views(R.pinhole(*hw), hw, q, t)
    one = synth.cloud(400, seed=5)
    twice = np.concatenate([one, one])                                          # every point again under a second index
    for splat in (0, 1):
        depth, uv2pt = R.lookups(twice, K, q, t, hw, MAX_DEPTH, splat)
        gd, gl = ctx.render_lookups(twice, views, hw[0], hw[1], splat)
        assert _same(gd, depth) and _same(gl, uv2pt) and (gl >= 0).any() and (gl < 400).all()
    # pairs on one camera ray whose depths differ by 1e-9 and so share z32: the NEARER point carries the higher index and loses
    K1, q1, t1 = R.pinhole(*hw, 30.0), np.array([[1.0, 0, 0, 0]]), np.zeros((1, 3))
    rng = np.random.default_rng(11)
    z = rng.uniform(1.0, 3.0, 300)
    a = np.stack([rng.uniform(-0.4, 0.4, 300) * z, rng.uniform(-0.3, 0.3, 300) * z, z], axis=1)
    pairs = np.concatenate([a, a * ((z - 1e-9) / z)[:, None]])
    depth, uv2pt = R.lookups(pairs, K1, q1, t1, hw, MAX_DEPTH, 0)
    gd, gl = ctx.render_lookups(pairs, _views(K1, hw, q1, t1), hw[0], hw[1], 0)
    assert _same(gd, depth) and _same(gl, uv2pt)
    won = gl[gl >= 0]
    assert len(won) > 100 and (won < 300).mean() > 0.9                          # by index, not by float64 depth


def test_dropped_samples_reach_no_output(ctx):
    hw = (24, 40)
    q, t = synth.ring_views(3)
    K, masks = R.pinhole(*hw), synth.masks(3, hw[0], hw[1], 'iid')
    pts = synth.cloud(500, seed=9)
    eyes, lookats = f3d.frustum_data(K, hw[1], hw[0], q, t)[:2]
    special = np.array([[np.nan, 0.0, 1.0], [0.0, np.nan, np.nan], t[0], t[1], eyes[0] + 10.5 * lookats[0], [np.inf, 0.0, 1.0]])
    pts[:len(special)] = special                                                # NaN, the camera centres, beyond the far plane, infinity
    views = _views(K, hw, q, t)
    for splat in (0, 2):
        depth, uv2pt = R.lookups(pts, K, q, t, hw, MAX_DEPTH, splat)
        gd, gl = ctx.render_lookups(pts, views, hw[0], hw[1], splat)
        assert _same(gd, depth) and _same(gl, uv2pt)
        votes = _votes(ctx, pts, views, masks, splat, 0.05)
        assert _same(votes, R.visible_votes(pts, K, q, t, masks, MAX_DEPTH, splat, 0.05))
    assert not np.isin(gl[0], [0, 1, 2, 4, 5]).any() and not votes[[0, 1, 5]].any() and not votes[2].sum() > 2 and votes.sum() > 100


def test_pass_size_and_tolerance(ctx):
    """V = 65: views_per_pass 0 / 1 / 2 give the same votes; depth_tol 0 / 0.05 / inf; at inf the votes are those of the existing
    project_vote_argmax (the yardstick from before this feature) and of the oracle's forward path."""
    hw, n, V = (24, 40), 257, 65
    pts = synth.cloud(n, seed=21)
    q, t = synth.ring_views(V)
    K, masks = R.pinhole(*hw), synth.masks(V, hw[0], hw[1], 'iid')
    views = _views(K, hw, q, t)
    for tol in (0.0, 0.05, np.inf):
        want = R.visible_votes(pts, K, q, t, masks, MAX_DEPTH, 1, tol)
        for per in (0, 1, 2):
            assert _same(_votes(ctx, pts, views, masks, 1, tol, per), want), (tol, per)
    u16 = ctx.project_vote_argmax(pts, views, masks, 133, 0.5, None, return_votes=True)[1]
    assert want.sum() > n and np.array_equal(want, u16) and _same(want, O.forward_votes(pts, K, q, t, masks, MAX_DEPTH))
    assert 0 < R.visible_votes(pts, K, q, t, masks, MAX_DEPTH, 1, 0.0).sum() < want.sum()


def test_lookups_feed_the_existing_uv2pt_vote(ctx):
    hw, n, V = (24, 40), 5000, 4
    pts = synth.cloud(n, seed=31)
    q, t = synth.ring_views(V)
    K, masks = R.pinhole(*hw), synth.masks(V, hw[0], hw[1], 'iid')
    for splat in (0, 1):
        uv2pt = fusion.render_lookups(pts, K, q, t, hw, MAX_DEPTH, splat)[1]
        want = np.zeros((n, 134))
        for j, lut in enumerate(R.lookups(pts, K, q, t, hw, MAX_DEPTH, splat)[1]):
            O.vote_frame(want, lut, masks[j].reshape(-1))
        got = ctx.vote_uv2pt_batch(np.zeros((n, 134)), uv2pt, masks.reshape(V, -1), hw[0], hw[1])
        assert want.sum() > 100 and _same(got, want)


def test_two_walls():
    """The test that needs the feature: the visible vote labels the x = 1 wall 86 and the x = 2 wall 114; the plain forward path
    cannot, because both walls collect both labels."""
    pts, far, K, q, t, masks, hw = R.two_walls()
    cls, votes = fusion.project_vote_argmax_visible(pts, K, q, t, masks, MAX_DEPTH, 133, 0.5, None, True, splat=1, depth_tol=0.05)
    assert cls.dtype == np.int64 and (cls[~far] == 86).all() and (cls[far] == 114).all()
    assert _same(votes, R.visible_votes(pts, K, q, t, masks, MAX_DEPTH, 1, 0.05))
    plain, pv = fusion.project_vote_argmax(pts, K, q, t, masks, MAX_DEPTH, 133, 0.5, None, True)
    assert (pv[:, 86] == 3).all() and (pv[:, 114] == 3).all() and (plain == 86).all() and not (plain[far] == 114).any()


def _blocker():
    """A (index 0) at pixel (6, 8), depth 1; B (index 1) at pixel (6, 9), depth 2, inside A's 3 x 3 patch: B is occluded at splat 1."""
    hw = (12, 16)
    K, q, t = R.pinhole(*hw, 10.0), np.array([[1.0, 0, 0, 0]]), np.zeros((1, 3))
    pts = np.array([[0.05, 0.05, 1.0], [0.3, 0.1, 2.0]])
    assert O.points2pixel(pts, K, q[0], t[0]).T.tolist() == [[8, 6], [9, 6]]
    return hw, K, q, t, pts


def test_label_beyond_nclasses(ctx):
    import torch
    hw, K, q, t, pts = _blocker()
    views = _views(K, hw, q, t)
    masks = np.full((1, *hw), 7, np.uint8)
    masks[0, 6, 9] = 200                                                         # read by the occluded sample only: nothing happens
    votes = _votes(ctx, pts, views, masks, 1, 0.05)
    assert votes.sum() == 1 and votes[0, 7] == 1 and _same(votes, R.visible_votes(pts, K, q, t, masks, MAX_DEPTH, 1, 0.05))
    assert (fusion.project_vote_argmax_visible(pts, K, q, t, masks, MAX_DEPTH) == [7, 133]).all()
    with pytest.raises(IndexError):                                              # ... but it is a sample: without the test it is read
        _votes(ctx, pts, views, masks, 1, np.inf)
    bad = masks.copy()
    bad[0, 6, 8] = 200                                                           # read by the visible sample
    with pytest.raises(IndexError):
        R.visible_votes(pts, K, q, t, bad, MAX_DEPTH, 1, 0.05)
    with pytest.raises(IndexError, match='vote_visible'):
        _votes(ctx, pts, views, bad, 1, 0.05)
    with pytest.raises(IndexError, match='vote_visible'):
        fusion.project_vote_argmax_visible(pts, K, q, t, bad, MAX_DEPTH)
    # the _dev entry records the error in a bit of its own: a pending uv2pt error is neither consumed nor blamed
    own = f3d.Context(0)
    dev = torch.device('cuda', 0)
    s = torch.cuda.Stream(dev)
    dp, dv, dm = torch.from_numpy(pts).to(dev), torch.from_numpy(views).to(dev), torch.from_numpy(bad).to(dev)
    dvotes = torch.zeros((2, 134), dtype=torch.float64, device=dev)
    lut, lm = torch.tensor([0, 99], dtype=torch.int32, device=dev), torch.zeros(2, dtype=torch.uint8, device=dev)
    uvd = torch.zeros((6, 3), dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    own.vote_uv2pt_dev(lut.data_ptr(), lm.data_ptr(), 2, uvd.data_ptr(), 6, 3, s.cuda_stream)
    own.vote_visible_dev(dp.data_ptr(), f3d.F64, 2, dv.data_ptr(), 1, dm.data_ptr(), hw[0], hw[1], 1, 0.05, dvotes.data_ptr(), 134, 0, s.cuda_stream)
    s.synchronize()
    with pytest.raises(IndexError, match='vote_visible'):                        # the host entry consumes bit 512 alone
        _votes(own, pts, views, masks, 1, 0.05)
    assert _same(_votes(own, pts, views, masks, 1, 0.05), votes)
    with pytest.raises(IndexError, match='vote_uv2pt'):                          # the other bit was left pending
        own.take_device_error(s.cuda_stream)
    own.take_device_error(s.cuda_stream)
    own.close()


def test_device_tensors_in_and_out():
    import torch
    dev = torch.device('cuda', 0)
    hw, n, V = (24, 40), 5000, 3
    q, t = synth.ring_views(V)
    K, masks = R.pinhole(*hw), synth.masks(V, hw[0], hw[1], 'iid')
    for dtype in (np.float64, np.float32):
        pts = synth.cloud(n, seed=41, dtype=dtype)
        depth, uv2pt = fusion.render_lookups(pts, K, q, t, hw, MAX_DEPTH, 1)
        cls, votes = fusion.project_vote_argmax_visible(pts, K, q, t, masks, MAX_DEPTH, filter_classes=[86, 114, 5], return_votes=True)
        dpts, dmasks = torch.from_numpy(pts).to(dev), torch.from_numpy(masks).to(dev)
        gd, gl = fusion.render_lookups(dpts, K, q, t, hw, MAX_DEPTH, 1)
        gc, gv = fusion.project_vote_argmax_visible(dpts, K, q, t, dmasks, MAX_DEPTH, filter_classes=[86, 114, 5], return_votes=True)
        assert all(isinstance(x, torch.Tensor) and x.device == dev for x in (gd, gl, gc, gv))
        assert _same(gd.cpu().numpy(), depth) and _same(gl.cpu().numpy(), uv2pt) and _same(gc.cpu().numpy(), cls) and _same(gv.cpu().numpy(), votes)
        assert _same(cls, O.segment(votes, 133, 0.5, [86, 114, 5])) and (cls != 133).any()


def test_reserved_strict_context_allocates_nothing():
    import torch
    dev = torch.device('cuda', 0)
    hw, n, V = (24, 40), 257, 5
    pts = synth.cloud(n, seed=51)
    q, t = synth.ring_views(V)
    K, masks = R.pinhole(*hw), synth.masks(V, hw[0], hw[1], 'iid')
    views = _views(K, hw, q, t)
    own = f3d.Context(0)
    s = torch.cuda.Stream(dev)
    dp, dv, dm = torch.from_numpy(pts).to(dev), torch.from_numpy(views).to(dev), torch.from_numpy(masks).to(dev)
    depth = torch.empty((V, *hw), dtype=torch.float32, device=dev)
    uv2pt = torch.empty((V, hw[0] * hw[1]), dtype=torch.int32, device=dev)
    votes = torch.zeros((n, 134), dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    own.reserve_render(n, V, hw[0], hw[1])
    own.set_strict(True)
    before = own.alloc_count
    own.render_lookups_dev(dp.data_ptr(), f3d.F64, n, dv.data_ptr(), V, hw[0], hw[1], 1, depth.data_ptr(), uv2pt.data_ptr(), s.cuda_stream)
    for per in (0, 2):
        own.vote_visible_dev(dp.data_ptr(), f3d.F64, n, dv.data_ptr(), V, dm.data_ptr(), hw[0], hw[1], 1, 0.05, votes.data_ptr(), 134, per, s.cuda_stream)
    assert own.alloc_count == before
    own.take_device_error(s.cuda_stream)
    want = R.lookups(pts, K, q, t, hw, MAX_DEPTH, 1)
    assert _same(depth.cpu().numpy(), want[0]) and _same(uv2pt.cpu().numpy(), want[1])
    assert _same(votes.cpu().numpy(), 2 * R.visible_votes(pts, K, q, t, masks, MAX_DEPTH, 1, 0.05))      # in place: two calls add up
    with pytest.raises(MemoryError):                                             # a larger image than reserved: strict says so
        own.vote_visible_dev(dp.data_ptr(), f3d.F64, n, dv.data_ptr(), V, dm.data_ptr(), 4 * hw[0], 4 * hw[1], 1, 0.05, votes.data_ptr(), 134, 0,
                             s.cuda_stream)
    own.close()


def test_bad_arguments(ctx):
    hw, K, q, t, pts = _blocker()
    views, masks = _views(K, hw, q, t), np.zeros((1, *hw), np.uint8)
    for splat, tol, per in ((9, 0.05, 0), (-1, 0.05, 0), (1, -1.0, 0), (1, np.nan, 0), (1, 0.05, -1)):
        with pytest.raises(ValueError):
            _votes(ctx, pts, views, masks, splat, tol, per)
    with pytest.raises(ValueError):
        ctx.render_lookups(pts, views, hw[0], hw[1], 9)
    with pytest.raises(ValueError):
        fusion.project_vote_argmax_visible(pts, K, q, t, masks, splat=9)
    with pytest.raises(ValueError):
        fusion.project_vote_argmax_visible(pts, K, q, t, masks, depth_tol=-1)
    assert _votes(ctx, pts, views, masks, 0, 0.0).sum() == 2                     # the accepted ends of both ranges
    assert _votes(ctx, pts, views, masks, 8, np.inf).sum() == 2
