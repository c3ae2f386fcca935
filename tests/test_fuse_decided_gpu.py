"""Early decisions of k_fuse (csrc/f3d_fuse.hip, f3d_fuse_decide.h): a point whose outstanding views cannot lift it over the threshold
is "unlabelled" already, and a wave whose points are all decided leaves its view loops.
Results must not change: every call is compared with oracle/np_ref.py, bit for bit.  Ctx.fuse_decided() (wave-tiles that left early)
and Ctx.fuse_deferred() keep the tests from being vacuous, and show that the gates hold: no early decision at threshold 0, with vote
rows, with a filter list, with a rejected label in the masks and in the view-chunked call.  Only calls of at most 64 views decide early.

The cloud is the synthetic room shrunk to 2.5 m around the point the ring cameras look at: every camera sees all of it, so a wave
of a cell-sorted cloud has the whole ring as whole-wave views.  A few points without usable coordinates are planted in it."""
import functools

import numpy as np
import pytest

import f3d
from f3d import synth
from oracle import np_ref as O
import fused_families as FF

pytestmark = pytest.mark.gpu

H = W = 256
K = np.array([[200., 0, 128], [0, 200., 128], [0, 0, 1]])
MAX_DEPTH, NCLASSES = 10.0, 133
N_ALL = 20011
SIZES = [1, 127, 128, 129, 513, 4097, N_ALL]
VIEWS = [8, 64]
PLANTED = {5: np.nan, 300: np.inf, 2000: 1e300, 15000: -np.inf}       # index -> x coordinate


@pytest.fixture(scope='module')
def ctx():
    return f3d.default_context()


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _cloud(room=False):
    """room: the synthetic room as it is (10 m x 10 m x 3 m) -- its points see different numbers of views."""
    c = np.array([0.0, 0.0, 1.5])
    pts = (synth.cloud(N_ALL, dtype=np.float32).astype(np.float64) - c) * (1.0 if room else 0.25) + c
    pts = pts.astype(np.float32).astype(np.float64)                    # both storages hold the same points
    for i, v in PLANTED.items():
        pts[i, 0] = v
    return _frozen(pts)


def _planted(n):
    return sum(1 for i in PLANTED if i < n)


@functools.lru_cache(maxsize=None)
def _masks(V, kind):
    if kind == 'block':
        m = synth.masks(V, H, W, 'block64')
    elif kind == 'merged':                                             # four of the eight block labels shown as 86: about half of a point's votes
        m = synth.masks(V, H, W, 'block64').copy()
        m[np.isin(m, [0, 15, 114])] = 86
    elif kind == 'const':
        m = np.full((V, H, W), 86, np.uint8)
    elif kind == 'half':                                               # a view shows one label: 86 in every second view
        lab = np.where(np.arange(V) % 2 == 0, 86, np.where(np.arange(V) % 4 == 1, 114, 115))
        m = np.broadcast_to(lab.astype(np.uint8)[:, None, None], (V, H, W)).copy()
    elif kind == 'third':                                              # 86 in every third view, six other labels in the rest
        other = np.array([114, 15, 115, 132, 120, 0])
        lab = np.where(np.arange(V) % 3 == 0, 86, other[(np.arange(V) // 3 * 2 + np.arange(V) % 3 - 1) % 6])
        m = np.broadcast_to(lab.astype(np.uint8)[:, None, None], (V, H, W)).copy()
    elif kind == 'allbut1':                                            # 86 everywhere but in view 0
        m = np.full((V, H, W), 86, np.uint8)
        m[0] = 114
    elif kind == 'rejected':                                           # label 200 > nclasses, only in the last two views
        m = synth.masks(V, H, W, 'block64').copy()
        m[V - 2:, 64:192, 64:192] = 200
    else:
        raise KeyError(kind)
    return _frozen(m)


@functools.lru_cache(maxsize=None)
def _views(V):
    q, t = synth.ring_views(V)
    return q, t, _frozen(f3d.views_build(K, W, H, q, t, MAX_DEPTH))


@functools.lru_cache(maxsize=None)
def _votes(V, kind, room=False):
    """The oracle's vote rows of the whole cloud: computed once per scene, shared, read-only (a label depends on the point alone)."""
    q, t, _ = _views(V)
    with np.errstate(all='ignore'):
        return _frozen(O.forward_votes(_cloud(room), K, q, t, _masks(V, kind), MAX_DEPTH, ncols=NCLASSES + 1))


def _want(V, kind, thr, n, flt=None, room=False):
    return O.segment(_votes(V, kind, room)[:n], NCLASSES, thr, flt)


def _fuse(ctx, pts, V, kind, thr, way='sort', f32=False, flt=None, votes=False, bounds=None, nclasses=NCLASSES):
    """One fused call on a device-resident cloud -> (labels, vote rows or None, deferred counts, wave-tiles that left early)."""
    import torch
    dev = torch.device('cuda', 0)
    _, _, views = _views(V)
    x = torch.from_numpy(np.array(pts, dtype=np.float32 if f32 else np.float64)).to(dev)
    n = x.shape[0]
    dt = f3d.F32 if f32 else f3d.F64
    vd, md = torch.from_numpy(np.array(views)).to(dev), torch.from_numpy(np.array(_masks(V, kind))).to(dev)
    cls = torch.full((n,), -7, dtype=torch.int64, device=dev)
    vo = torch.full((n, nclasses + 1), 7, dtype=torch.uint16, device=dev) if votes else None
    flags = f3d.FUSE_SORT if way == 'sort' else 0
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        if bounds is None:
            ctx.project_vote_argmax_dev(x.data_ptr(), dt, n, vd.data_ptr(), V, md.data_ptr(), H, W, nclasses, thr, flt, cls.data_ptr(),
                                        None if vo is None else vo.data_ptr(), s.cuda_stream, flags=flags)
        else:
            present = torch.empty(256, dtype=torch.uint8, device=dev)
            ctx.mask_presence_dev(md.data_ptr(), V, H, W, present.data_ptr(), s.cuda_stream)
            ctx.fuse_chunked_begin_dev(present.data_ptr(), n, V, H, W, nclasses, flt, s.cuda_stream)
            for a, b in zip(bounds[:-1], bounds[1:]):
                ctx.fuse_chunk_dev(x.data_ptr(), dt, n, vd.data_ptr(), V, a, b, md.data_ptr(), H, W, nclasses, thr, flt, cls.data_ptr(),
                                   s.cuda_stream, flags=flags)
        try:
            ctx.take_device_error(s.cuda_stream)                               # clean: raises otherwise
        finally:
            s.synchronize()
    return cls.cpu().numpy(), None if vo is None else vo.cpu().numpy(), ctx.fuse_deferred(), ctx.fuse_decided()


def _same(got, want, what):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f'{what}: {bad.size} of {want.size} labels differ, the first at point {int(bad[0])}: got {int(got[bad[0]])}, want {int(want[bad[0]])}'


# ---------------------------------------------------------------------------------------------------- block masks, threshold 0.5
@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('V', VIEWS)
def test_block_masks_at_the_reference_threshold(ctx, V, n):
    """Labels equal the oracle's for sorted and caller-order clouds in both storages; the planted points are deferred.  With enough
    whole-wave views for a check (64 views, a cloud of thousands of points) wave-tiles leave early: every point of this scene ends
    unlabelled, at most 20 of 64 votes for its leader."""
    want = _want(V, 'block', 0.5, n)
    assert n < 4097 or (want == NCLASSES).mean() > 0.9                 # the scene of the issue: most points end unlabelled
    for way in ('sort', 'plain'):
        for f32 in (False, True):
            got, _, deferred, decided = _fuse(ctx, _cloud()[:n], V, 'block', 0.5, way, f32)
            print(f'V={V} n={n} {way} {"f32" if f32 else "f64"}: deferred {deferred}, wave-tiles left early {decided} of {(n + 127) // 128}')
            _same(got, want, (V, n, way, f32))
            assert deferred[0] >= _planted(n)
            if V == 64 and n >= 4097 and way == 'sort':
                assert decided > 0


# ---------------------------------------------------------------------------------------------------- labelled and unlabelled points side by side
@pytest.mark.parametrize('n', [129, 4097, N_ALL])
def test_block_masks_with_a_label_near_half_of_the_votes(ctx, n):
    """Four of the eight block labels shown as one: a point gives that label about half of its 64 votes, so labelled and unlabelled
    points sit side by side in every wave -- a point wrongly decided "unlabelled" would show, and a wave with a point that may still be
    labelled must run to its last view."""
    want = _want(64, 'merged', 0.5, N_ALL)
    assert 0.2 < (want != NCLASSES).mean() < 0.8
    for way in ('sort', 'plain'):
        for f32 in (False, True):
            got, _, deferred, decided = _fuse(ctx, _cloud()[:n], 64, 'merged', 0.5, way, f32)
            print(f'merged n={n} {way} {"f32" if f32 else "f64"}: labelled {(want[:n] != NCLASSES).mean():.3f}, deferred {deferred}, left early {decided}')
            _same(got, want[:n], (n, way, f32))


# ---------------------------------------------------------------------------------------------------- nothing to decide
@pytest.mark.parametrize('V', [8, 64])
def test_one_label_in_every_view_decides_nothing(ctx, V):
    """Every vote of a point goes to one label: its share is 1, no state of it is ever decided (b + R >= cmin[s + R] whenever b = s),
    so no wave-tile leaves early; every point a view sees is labelled."""
    want = _want(V, 'const', 0.5, N_ALL)
    seen = _votes(V, 'const')[:, 86] > 0
    assert seen.mean() > 0.9 and np.all(want[seen] == 86)
    for way in ('sort', 'plain'):
        got, _, _, decided = _fuse(ctx, _cloud(), V, 'const', 0.5, way)
        _same(got, want, (V, way))
        assert decided == 0


# ---------------------------------------------------------------------------------------------------- at the boundary
@pytest.mark.parametrize('kind,thr', [('third', 0.3), ('third', 1.0 / 3.0), ('half', 0.5), ('allbut1', 1.0)])
@pytest.mark.parametrize('V', [64])
def test_points_at_the_threshold(ctx, V, kind, thr):
    """Views that show one label each, and the room at its full size, where a point is seen by some of the ring: a point's leader holds
    about the threshold's share of its votes, and many points end with best = cmin[T] (labelled, just) or cmin[T] - 1 (unlabelled,
    just) for several totals T."""
    votes = _votes(V, kind, room=True)
    T, best = votes.sum(1).astype(np.int64), votes.max(1).astype(np.int64)
    cmin = np.array([sum(1 for c in range(t + 1) if t and np.float64(c) / np.float64(t) < thr) for t in range(V + 1)])
    at, below = (T > 0) & (best == cmin[T]), (T > 0) & (best == cmin[T] - 1)
    assert len(np.unique(T[at])) >= 3 and len(np.unique(T[below])) >= 3, (np.unique(T[at]), np.unique(T[below]))
    want = _want(V, kind, thr, N_ALL, room=True)
    assert np.all(want[at] != NCLASSES) and np.all(want[below] == NCLASSES)
    for way in ('sort', 'plain'):
        for f32 in (False, True):
            got, _, deferred, decided = _fuse(ctx, _cloud(room=True), V, kind, thr, way, f32)
            print(f'V={V} {kind} thr={thr:.3f} {way}: at {int(at.sum())}, just below {int(below.sum())}, deferred {deferred}, left early {decided}')
            _same(got, want, (V, kind, thr, way, f32))


# ---------------------------------------------------------------------------------------------------- thresholds without decisions, or with nothing else
@pytest.mark.parametrize('V', [8, 64])
def test_threshold_zero_and_beyond_one(ctx, V):
    for n in (129, N_ALL):
        for way in ('sort', 'plain'):
            got, _, _, decided = _fuse(ctx, _cloud()[:n], V, 'block', 0.0, way)
            _same(got, _want(V, 'block', 0.0, n), (V, n, way, 0.0))
            assert decided == 0                                        # the rule is off at threshold 0
            got, _, deferred, decided = _fuse(ctx, _cloud()[:n], V, 'block', 1.5, way)
            _same(got, _want(V, 'block', 1.5, n), (V, n, way, 1.5))
            assert np.all(got == NCLASSES)


# ---------------------------------------------------------------------------------------------------- the gates
@pytest.mark.parametrize('V', [64])
def test_rejected_label_in_the_last_views_is_still_flagged(ctx, V):
    """Label 200 with nclasses 133 in the masks of the last two views only, where the cloud projects: the oracle raises IndexError,
    and so does the call -- the code book knows of the label, and no view is left out."""
    q, t, _ = _views(V)
    with np.errstate(all='ignore'), pytest.raises(IndexError):
        O.forward_votes(_cloud(), K, q, t, _masks(V, 'rejected'), MAX_DEPTH, ncols=NCLASSES + 1)
    for way in ('sort', 'plain'):
        with pytest.raises(IndexError):
            _fuse(ctx, _cloud(), V, 'rejected', 0.5, way)
        assert ctx.fuse_decided() == 0
    got, _, _, _ = _fuse(ctx, _cloud(), V, 'block', 0.5)                  # the context is usable again
    _same(got, _want(V, 'block', 0.5, N_ALL), (V, 'after'))


@pytest.mark.parametrize('V', [8, 64])
def test_vote_rows_are_complete(ctx, V):
    for n in (513, N_ALL):
        for way in ('sort', 'plain'):
            got, rows, _, decided = _fuse(ctx, _cloud()[:n], V, 'block', 0.5, way, votes=True)
            _same(got, _want(V, 'block', 0.5, n), (V, n, way))
            assert np.array_equal(rows, _votes(V, 'block')[:n].astype(np.uint16))
            assert decided == 0


@pytest.mark.parametrize('V', [8, 64])
def test_view_chunked_call_equals_one_shot(ctx, V):
    for f32 in (False, True):
        one, _, _, _ = _fuse(ctx, _cloud(), V, 'block', 0.5, 'sort', f32)
        two, _, _, decided = _fuse(ctx, _cloud(), V, 'block', 0.5, 'sort', f32, bounds=[0, V // 2, V])
        assert np.array_equal(one, two)
        _same(two, _want(V, 'block', 0.5, N_ALL), (V, f32))
        assert decided == 0


@pytest.mark.parametrize('flt', [[86, 114, 115], list(range(100, 134)) + [86, 15, 0]], ids=['short', 'long'])
@pytest.mark.parametrize('V', [8, 64])
def test_filter_list_runs_as_before(ctx, V, flt):
    """A short list votes into the filter book, a long one into the presence book: neither gets an early decision."""
    for way in ('sort', 'plain'):
        got, _, _, decided = _fuse(ctx, _cloud(), V, 'block', 0.5, way, flt=flt)
        _same(got, _want(V, 'block', 0.5, N_ALL, flt), (V, way))
        assert decided == 0


@pytest.mark.parametrize('V', [8, 64])
def test_no_parked_slots(ctx, V, monkeypatch):
    """F3D_DEBUG_PARK_SLOTS=0: a deferred point is redone from nothing; labels equal."""
    monkeypatch.setenv('F3D_DEBUG_PARK_SLOTS', '0')
    for way in ('sort', 'plain'):
        for f32 in (False, True):
            got, _, _, _ = _fuse(ctx, _cloud(), V, 'block', 0.5, way, f32)
            _same(got, _want(V, 'block', 0.5, N_ALL), (V, way, f32))


# ---------------------------------------------------------------------------------------------------- the scene families
@pytest.mark.parametrize('cloud', ['random', 'plane'])
@pytest.mark.parametrize('fam', FF.FAMILIES)
def test_scene_families_at_the_reference_threshold(ctx, fam, cloud):
    """Scenes far from the origin, in other units, with rolled, skewed, wide and telephoto cameras, and their clouds of points within
    a few ulp of the frustum planes (every one of them has unproven views), at threshold 0.5."""
    _, Kf, q, t, max_depth, w, h, masks = FF.family(fam)
    pts = FF.clouds(fam)[cloud]
    views = f3d.views_build(Kf, w, h, q, t, max_depth)
    with np.errstate(all='ignore'):
        want = O.project_vote_argmax(pts, Kf, q, t, masks, max_depth, NCLASSES, 0.5, None)
    for f32 in (False, True):
        p = pts.astype(np.float32) if f32 else pts
        if f32:
            with np.errstate(all='ignore'):
                want = O.project_vote_argmax(p.astype(np.float64), Kf, q, t, masks, max_depth, NCLASSES, 0.5, None)
        got = ctx.project_vote_argmax(p, views, masks, NCLASSES, 0.5, None)
        _same(got, want, (fam, cloud, f32))
