"""smooth_votes / smooth_segment without a GPU: the C symbols are bound, the NumPy restatement does on the two scenes what the
operator is for, every argument error is raised before any device call, and get3DSeg.segment's defaults keep today's call path."""
import functools
import inspect

import numpy as np
import pytest

import f3d
import smooth_ref as R
from oracle import np_ref as O


def V():
    from Fusion3DSeg.segUtils import voting
    return voting


@functools.lru_cache(maxsize=None)
def _sheet():
    pts, votes, truth = R.noisy_sheet()
    return pts, votes, truth, R.radius_csr(pts, R.SHEET_R)


@functools.lru_cache(maxsize=None)
def _corner():
    pts, normals, votes, surface = R.corner()
    return pts, normals, votes, surface, R.radius_csr(pts, 0.05)


# ------------------------------------------------------------------------------------------------ the surface
def test_symbols_are_bound():
    lib = f3d.library()
    for name in ('f3d_smooth_votes', 'f3d_smooth_votes_dev', 'f3d_smooth_segment', 'f3d_smooth_segment_dev', 'f3d_ctx_reserve_smooth'):
        assert name in lib._f3d_symbols and getattr(lib, name).argtypes is not None, name
    for name in ('smooth_votes', 'smooth_votes_dev', 'smooth_segment', 'smooth_segment_dev', 'reserve_smooth'):
        assert callable(getattr(f3d.Context, name)), name
    assert callable(V().smooth_votes) and callable(V().smooth_segment)


# ------------------------------------------------------------------------------------------------ the restatement
def test_restated_sheet_is_clean_after_one_iteration():
    pts, votes, truth, (offs, nbrs) = _sheet()
    far = R.sheet_far(pts)
    before = O.segment(votes, R.NCLASSES, 0.5)
    wrong0, empty0 = (before != truth) & (before != R.NCLASSES), before == R.NCLASSES
    assert wrong0[far].sum() > 200 and empty0.sum() > 60                       # the noise is there: ~15 % and ~5 % of 2400 rows
    lens = np.diff(offs)
    assert 15 <= np.median(lens) <= 25
    after = R.smooth_segment(votes, offs, nbrs, R.NCLASSES, 0.5)
    assert (after != R.NCLASSES).all()                                         # no unclassified point
    assert (after[far] == truth[far]).all()                                    # no wrong label beyond r of the boundary
    twice = R.smooth_segment(votes, offs, nbrs, R.NCLASSES, 0.5, iterations=2)
    assert (twice[far] == truth[far]).all() and (twice != R.NCLASSES).all()


def test_restated_corner_leaks_plain_and_not_gated():
    pts, normals, votes, surface, (offs, nbrs) = _corner()
    assert R.corner_leaks(votes, surface) == 0
    assert R.corner_leaks(R.smooth(votes, offs, nbrs), surface) > 0
    gated = R.smooth(votes, offs, nbrs, normals=normals, cos_angle=np.cos(np.radians(30.0)))
    assert R.corner_leaks(gated, surface) == 0
    assert (gated.sum(1) >= votes.sum(1)).all()                                # the gate keeps the own surface's neighbours


def test_restated_order_is_row_order():
    """(1e16 + 1) + 1 != 1e16 + (1 + 1) in float64: the restated sum follows the row, and skips the point itself wherever it stands."""
    v = np.array([[1e16], [1.0], [1.0], [-1e16]])
    offs, nbrs = np.array([0, 4, 4, 4, 4]), np.array([1, 0, 2, 3], np.int32)
    assert R.smooth(v, offs, nbrs)[0, 0] == ((1e16 + 1.0) + 1.0) + -1e16 == 0.0
    offs, nbrs = np.array([0, 4, 4, 4, 4]), np.array([3, 1, 2, 0], np.int32)
    assert R.smooth(v, offs, nbrs)[0, 0] == ((1e16 + -1e16) + 1.0) + 1.0 == 2.0
    twice = R.smooth(v, np.array([0, 2, 2, 2, 2]), np.array([1, 1], np.int32))[0, 0]                   # a duplicate counts twice,
    assert twice == (1e16 + 1.0) + 1.0 and twice != 1e16 + 2.0                                         # one add after the other
    assert R.smooth(v, np.array([0, 0, 2, 2, 2]), np.array([2, 2], np.int32))[1, 0] == 3.0
    with pytest.raises(IndexError):
        R.smooth(v, offs, np.array([3, 1, 2, 4], np.int32))


# ------------------------------------------------------------------------------------------------ argument errors
class _FakeDeviceTensor:
    is_cuda = True

    def __init__(self, shape, dtype):
        self.shape, self.dtype, self.device = shape, dtype, None


@pytest.fixture
def no_device(monkeypatch):
    def boom(*a, **k):
        raise AssertionError('a device call was reached')
    monkeypatch.setattr(f3d, 'default_context', boom)
    monkeypatch.setattr(f3d, 'Context', boom)


def test_argument_errors_come_before_any_device_call(no_device):
    sv, ss = V().smooth_votes, V().smooth_segment
    votes = np.zeros((6, 5))
    adj = (np.arange(7, dtype=np.int64), np.zeros(6, np.int32))
    nrm, col = np.zeros((6, 3)), np.zeros((6, 3), np.float32)
    for call in (lambda **k: sv(k.pop('votes', votes), k.pop('adj', adj), **k),
                 lambda **k: ss(k.pop('votes', votes), k.pop('adj', adj), 4, **k)):
        with pytest.raises(ValueError, match=r'\[N, ncols\]'):
            call(votes=np.zeros(6))
        with pytest.raises(ValueError, match=r'\[N, ncols\]'):
            call(votes=np.zeros((6, 5, 1)))
        with pytest.raises(ValueError, match='256 columns'):
            call(votes=np.zeros((6, 257)))
        with pytest.raises(ValueError, match='256 columns'):
            call(votes=np.zeros((6, 0)))
        with pytest.raises(ValueError, match='iterations'):
            call(iterations=0)
        for w in (-1.0, float('inf'), float('nan')):
            with pytest.raises(ValueError, match='self_weight'):
                call(self_weight=w)
        with pytest.raises(ValueError, match='normals and angle'):
            call(normals=nrm)
        with pytest.raises(ValueError, match='normals and angle'):
            call(angle=30.0)
        with pytest.raises(ValueError, match='colors and max_color_dist'):
            call(colors=col)
        with pytest.raises(ValueError, match='colors and max_color_dist'):
            call(max_color_dist=0.1)
        with pytest.raises(ValueError, match='max_color_dist'):
            call(colors=col, max_color_dist=-0.1)
        with pytest.raises(ValueError, match=r'normals must be \[6, 3\]'):
            call(normals=np.zeros((5, 3)), angle=30.0)
        with pytest.raises(ValueError, match=r'colors must be \[6, 3\]'):
            call(colors=np.zeros((6, 4)), max_color_dist=0.1)
        with pytest.raises(TypeError, match='float64 or uint16'):
            call(votes=np.zeros((6, 5), np.float32))
        with pytest.raises(TypeError, match='float64 or uint16'):
            call(votes=np.zeros((6, 5), np.int64))
        with pytest.raises(TypeError, match='normals'):
            call(normals=np.zeros((6, 3), np.float32), angle=30.0)
        with pytest.raises(TypeError, match='colors'):
            call(colors=np.zeros((6, 3), np.uint8), max_color_dist=0.1)
        with pytest.raises(ValueError, match='offsets'):
            call(adj=(adj[0][:-1], adj[1]))
        with pytest.raises(ValueError, match='offsets'):
            call(adj=(adj[0], adj[1][:-1]))
        import torch
        with pytest.raises(TypeError, match='host adjacency'):                     # host data with a device CSR
            call(adj=(_FakeDeviceTensor((7,), torch.int64), _FakeDeviceTensor((6,), torch.int32)))
        with pytest.raises(TypeError, match='device CSR'):                         # and device data with a host CSR
            call(votes=_FakeDeviceTensor((6, 5), torch.float64))
        with pytest.raises(TypeError, match='float64 or uint16'):
            call(votes=_FakeDeviceTensor((6, 5), torch.float32))
    with pytest.raises(ValueError, match='share memory'):                          # votes_out aliasing
        sv(votes, adj, out=votes)
    with pytest.raises(ValueError, match='share memory'):
        wide = np.zeros((7, 5))
        sv(wide[:6], adj, out=wide[1:])
    with pytest.raises(ValueError, match=r'out must be \[6, 5\]'):
        sv(votes, adj, out=np.zeros((6, 4)))
    with pytest.raises(TypeError, match='out must be'):
        sv(votes, adj, out=np.zeros((6, 5), np.float32))
    with pytest.raises(IndexError, match='filter class'):
        ss(votes, adj, 4, filter_classes=[1, 5])
    with pytest.raises(ValueError, match='empty sequence'):
        ss(np.zeros((6, 1)), adj, 4, lastcol=True)


# ------------------------------------------------------------------------------------------------ get3DSeg.segment
def _patched_get3dseg(monkeypatch, adj):
    import get3DSeg
    calls = []
    pts = np.zeros((4, 3))
    norms = np.tile([0.0, 0.0, 1.0], (4, 1))

    class Voter:
        def __init__(self, *a, **k):
            pass

        def vote(self, **k):
            calls.append('vote')
            return np.ones((4, 134))

        def segment(self, threshold, filter_classes):
            calls.append(('voter.segment', threshold, tuple(filter_classes)))
            return np.zeros(4, np.int64)

    def smooth_segment(votes, adj_, nclasses, threshold, filter_classes, **kw):
        calls.append(('smooth_segment', nclasses, threshold, tuple(filter_classes), kw))
        return np.zeros(4, np.int64)

    monkeypatch.setattr(get3DSeg.Fusion, 'load_data', staticmethod(lambda d: (pts, norms, None, None, None, 1, (2, 2), adj)))
    monkeypatch.setattr(get3DSeg, 'VotingSegmentation', Voter)
    monkeypatch.setattr(get3DSeg, 'smooth_segment', smooth_segment)
    monkeypatch.setattr(get3DSeg, 'split_into_instances', lambda *a, **k: (None, None, None, None))
    for name in ('semantic_viz', 'panoptic_viz', 'master_classes', '_coco_meta'):
        monkeypatch.setattr(get3DSeg, name, lambda *a, **k: None)
    return get3DSeg, calls, norms


def test_get3dseg_defaults_keep_the_call_path(monkeypatch, tmp_path):
    import get3DSeg
    sig = inspect.signature(get3DSeg.segment).parameters
    assert sig['smooth_iterations'].default == 0 and sig['smooth_angle'].default is None
    assert list(sig)[:7] == ['dirname', 'mask_dir', 'threshold', 'nclasses', 'filter_classes', 'min_pts_per_inst', 'verbose']
    adj = [np.array([0])] * 4
    g, calls, _ = _patched_get3dseg(monkeypatch, adj)
    g.segment(tmp_path, tmp_path, verbose=False)
    assert calls == ['vote', ('voter.segment', 0.5, (86, 114, 115))]
    g, calls, _ = _patched_get3dseg(monkeypatch, None)                             # no adjacency: smoothing has nothing to run on
    g.segment(tmp_path, tmp_path, verbose=False, smooth_iterations=2)
    assert calls == ['vote', ('voter.segment', 0.5, (86, 114, 115))]


def test_get3dseg_smoothing_goes_through_smooth_segment(monkeypatch, tmp_path):
    adj = [np.array([0])] * 4
    g, calls, norms = _patched_get3dseg(monkeypatch, adj)
    g.segment(tmp_path, tmp_path, verbose=False, smooth_iterations=2)
    assert calls == ['vote', ('smooth_segment', 133, 0.5, (86, 114, 115), {'iterations': 2})]
    g, calls, norms = _patched_get3dseg(monkeypatch, adj)
    g.segment(tmp_path, tmp_path, verbose=False, smooth_iterations=1, smooth_angle=30.0)
    (name, ncls, thr, flt, kw), = calls[1:]
    assert name == 'smooth_segment' and kw['iterations'] == 1 and kw['angle'] == 30.0 and np.array_equal(kw['normals'], norms)
