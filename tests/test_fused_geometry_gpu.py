"""The fused tiers (k_fuse, the float64 middle tier, the reference-arithmetic tier) and the single-view kernels on the scene
families of fused_families.py: scenes far from the origin, in millimetres and kilometres, rolled / skewed / wide / telephoto
cameras, quaternions far from unit norm, and clouds whose points sit within 3 ulp of the frustum planes.  Every error bound of the
accelerators has a term proportional to a magnitude of the scene; here those terms dominate.  Labels, uint16 vote rows, uv and
inside are compared BIT FOR BIT with the oracle (f3d.views_build gives the oracle's planes bit for bit for every family:
test_fused_families_cpu.py).  Needs a real MI355X: run with `-m gpu`."""
from types import SimpleNamespace

import numpy as np
import pytest

import f3d
import fused_families as FF
from oracle import np_ref as O
from test_gpu_parity import _dev_fuse, _dev_fuse_chunked

# the families' arrays are shared and read-only; the helpers hand them to torch.from_numpy only to copy them to the device
pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings('ignore:The given NumPy array is not writable')]

FLT = [86, 114, 115]
SETTINGS = [(0.0, None), (0.5, None), (0.0, FLT), (0.5, FLT)]               # (threshold, filter_classes)
CLOUDS = ('random', 'plane')


@pytest.fixture(scope='module')
def ctx():
    return f3d.default_context()


@pytest.fixture(scope='module', params=FF.FAMILIES)
def fam(request):
    """One family at a time (module-scoped parameter: pytest runs all tests of a family together): its view table and, computed on
    first use and then shared, the oracle's vote matrix of each (cloud, storage) and the labels it segments to."""
    name = request.param
    _, K, q, t, max_depth, w, h, masks = FF.family(name)
    clouds = FF.clouds(name)
    votes, labels = {}, {}

    def points(cloud, f32=False):
        return clouds[cloud].astype(np.float32) if f32 else clouds[cloud]

    def want_votes(cloud, f32=False):
        if (cloud, f32) not in votes:
            with np.errstate(all='ignore'):
                votes[(cloud, f32)] = O.forward_votes(points(cloud, f32).astype(np.float64), K, q, t, masks, max_depth, ncols=134)
        return votes[(cloud, f32)]

    def want(cloud, thr, flt, f32=False):
        key = (cloud, f32, thr, None if flt is None else tuple(flt))
        if key not in labels:
            labels[key] = O.segment(want_votes(cloud, f32), 133, thr, flt)
        return labels[key]

    return SimpleNamespace(name=name, K=K, q=q, t=t, max_depth=max_depth, w=w, h=h, masks=masks, V=len(t),
                           views=f3d.views_build(K, w, h, q, t, max_depth), points=points, want_votes=want_votes, want=want)


def _report(*fields):
    print('\nFUSED_FAMILIES', *fields)


# ---- a. the one-shot fused call through the host entry: labels and the full vote matrix --------------------------------------
@pytest.mark.parametrize('f32', [False, True], ids=['f64', 'f32'])
@pytest.mark.parametrize('cloud', CLOUDS)
def test_one_shot_labels_and_votes_bit_exact(ctx, fam, cloud, f32):
    """float32 storage is compared with the oracle on the WIDENED float32 cloud: at shift4e6 that cloud is quantised to 0.25-0.5 m
    and is simply another legal cloud at 1e7."""
    pts = fam.points(cloud, f32)
    for thr, flt in SETTINGS:
        got, votes = ctx.project_vote_argmax(pts, fam.views, fam.masks, 133, thr, flt, return_votes=True)
        assert votes.dtype == np.uint16 and np.array_equal(votes, fam.want_votes(cloud, f32)), (fam.name, cloud, f32, thr, flt)
        bad = got != fam.want(cloud, thr, flt, f32)
        assert not bad.any(), (fam.name, cloud, f32, thr, flt, int(bad.sum()))
        assert np.array_equal(ctx.project_vote_argmax(pts, fam.views, fam.masks, 133, thr, flt), got)     # the call without a vote matrix


# ---- b. the device entry on a side stream, caller order and sorted in the call -------------------------------------------------
@pytest.mark.parametrize('cloud', CLOUDS)
def test_device_entry_caller_order_and_sorted(ctx, fam, cloud):
    pts = fam.points(cloud)
    for thr, flt in ((0.0, None), (0.5, FLT)):
        for flags in (0, f3d.FUSE_SORT):
            got = _dev_fuse(ctx, pts, fam.views, fam.masks, flt, thr, flags)
            assert np.array_equal(got, fam.want(cloud, thr, flt)), (fam.name, cloud, thr, flt, flags)
    got = _dev_fuse(ctx, pts, fam.views, fam.masks, None, 0.0, f3d.FUSE_SORT, f32=True)
    assert np.array_equal(got, fam.want(cloud, 0.0, None, f32=True)), (fam.name, cloud, 'f32')


# ---- c. the view-chunked call: every deferred point is redone from nothing by the float64 tier ---------------------------------
@pytest.mark.parametrize('cloud', CLOUDS)
def test_chunked_call_equals_one_shot(ctx, fam, cloud):
    pts = fam.points(cloud)
    bounds = [0, 3, fam.V]
    for thr, flt in ((0.0, None), (0.5, FLT)):
        one = _dev_fuse(ctx, pts, fam.views, fam.masks, flt, thr, f3d.FUSE_SORT)
        assert np.array_equal(one, fam.want(cloud, thr, flt)), (fam.name, cloud, thr, flt)
        for presence, flags in (('own', f3d.FUSE_SORT), ('own', 0), ('all', f3d.FUSE_SORT)):      # 'all': no presence table (None)
            got = _dev_fuse_chunked(ctx, pts, fam.views, fam.masks, flt, thr, flags, bounds, presence=presence)
            assert np.array_equal(got, one), (fam.name, cloud, thr, flt, presence, flags)
        if fam.name in ('shift1e5', 'tele'):                                                         # the coded exchange
            for presence in ('own', 'all'):
                got = _dev_fuse_chunked(ctx, pts, fam.views, fam.masks, flt, thr, f3d.FUSE_SORT, bounds, presence=presence, coded=True)
                assert np.array_equal(got, one), (fam.name, cloud, thr, flt, presence, 'coded')


# ---- d. the lower tiers really ran -----------------------------------------------------------------------------------------------
def test_on_plane_cloud_reaches_the_reference_arithmetic_tier(ctx, fam):
    """A point within 3 ulp of a plane lies inside the float64 cull's band of 64 eps |p|_1: the float32 kernel must defer it
    (counts[0]) and only the reference's own arithmetic can decide it (counts[1])."""
    for cloud in CLOUDS:
        pts = fam.points(cloud)
        got = ctx.project_vote_argmax(pts, fam.views, fam.masks, 133, 0.0, None)
        counts = ctx.fuse_deferred()
        _report('deferred', fam.name, cloud, 'n', len(pts), 'mid', counts[0], 'exact', counts[1])
        assert np.array_equal(got, fam.want(cloud, 0.0, None))
        if cloud == 'plane':
            assert counts[0] > 0 and counts[1] > 0, (fam.name, counts)
        # the host entry leaves a cloud this small in caller order (one box per 128 scattered points: the float32 tier proves little);
        # cell-sorted in the call, the float32 tier works on compact boxes
        got = _dev_fuse(ctx, pts, fam.views, fam.masks, None, 0.0, f3d.FUSE_SORT)
        sorted_counts = ctx.fuse_deferred()
        _report('deferred_sorted', fam.name, cloud, 'n', len(pts), 'mid', sorted_counts[0], 'exact', sorted_counts[1])
        assert np.array_equal(got, fam.want(cloud, 0.0, None))
        if cloud == 'plane':
            assert sorted_counts[0] > 0 and sorted_counts[1] > 0, (fam.name, sorted_counts)
        elif fam.name == 'base':
            assert sorted_counts[0] < len(pts), sorted_counts                # the float32 tier really finishes points


# ---- e. every accelerated decision next to the exact arithmetic ------------------------------------------------------------------
def test_fastpath_audit_no_wrong_pixel_no_wrong_cull(ctx, fam):
    for cloud in CLOUDS:
        pairs, fb, wrong, cullwrong = ctx.fastpath_audit(fam.points(cloud), fam.views, fam.w, fam.h)
        _report('audit', fam.name, cloud, 'pairs', pairs, 'fallbacks', fb, 'share', round(fb / max(pairs, 1), 4), 'wrong', wrong,
                'cullwrong', cullwrong)
        assert pairs > 0 and wrong == 0 and cullwrong == 0, (fam.name, cloud, pairs, fb, wrong, cullwrong)
        if fam.name == 'base':
            assert fb < pairs, (cloud, pairs, fb)                            # the fast branch really decides something


# ---- f. the single-view kernels --------------------------------------------------------------------------------------------------
def _check_single_views(ctx, name, K, q, t, max_depth, w, h, views, clouds):
    ppts, pnrm = O.frustum_planes(K, w, h, q, t, max_depth)
    for cloud, pts in clouds.items():
        for stored in (pts, pts.astype(np.float32)):
            wide = stored.astype(np.float64)
            for j in (0, len(t) - 1):
                uv, ins = ctx.project_view(stored, views[j])
                with np.errstate(all='ignore'):
                    want_uv = O.points2pixel(wide, K, q[j], t[j])
                    want_ins = O.point_inside_polyhedra(wide, ppts[j], pnrm[j])
                assert uv.dtype == np.int32 and np.array_equal(uv, want_uv), (name, cloud, stored.dtype, j)
                assert np.array_equal(ins, want_ins), (name, cloud, stored.dtype, j, int((ins != want_ins).sum()))


def test_project_view_uv_and_inside_bit_exact(ctx, fam):
    _check_single_views(ctx, fam.name, fam.K, fam.q, fam.t, fam.max_depth, fam.w, fam.h, fam.views,
                        {c: fam.points(c) for c in CLOUDS})


def test_project_view_telephoto_inside_the_room(ctx):
    """tele_near: f = 5000 with the eyes inside the room -- pixel coordinates beyond +-32768 (the int32 conversion; for the audit
    the |U|, |V| < 32768 guard of the centre rows).  Its views see almost nothing, so it says nothing about votes."""
    pts, K, q, t, max_depth, w, h, _ = FF.family('tele_near')
    views = f3d.views_build(K, w, h, q, t, max_depth)
    uv0 = O.points2pixel(pts, K, q[0], t[0])
    assert (np.abs(uv0.astype(np.int64)) >= 32768).any(0).sum() >= 100
    _check_single_views(ctx, 'tele_near', K, q, t, max_depth, w, h, views, FF.clouds('tele_near'))
    pairs, fb, wrong, cullwrong = ctx.fastpath_audit(pts, views, w, h)
    _report('audit', 'tele_near', 'random', 'pairs', pairs, 'fallbacks', fb, 'wrong', wrong, 'cullwrong', cullwrong)
    assert wrong == 0 and cullwrong == 0, (pairs, fb, wrong, cullwrong)
