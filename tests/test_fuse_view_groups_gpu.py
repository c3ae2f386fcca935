"""The fused call across its 64-view groups (k_fuse, k_fuse_mid, k_fuse_exact: csrc/f3d_fuse.hip; layout: csrc/f3d_fuse_todo.h).
k_fuse works through a call's views in groups of 64, and what hands a half-finished point on to k_fuse_mid -- the open-view masks
umask[slot * ngroups + g], the zero-fill of the groups before a point took its slot, the zero masks after it, the parked bins, the
fallbacks beyond park_slots slots, beyond 16 groups and beyond a bin of 255 -- exists only because there can be several groups.
The clouds of tests/group_scenes.py place points within a few ulp of the frustum planes of CHOSEN views, so every such point leaves
that view open, in group view // 64; every call is compared with oracle/np_ref.py on every point, bit for bit, labels as int64 and
vote rows as uint16.  Two forms of cloud: spread over whole frustum planes (GS.cloud: wave boxes of metres, most views without a
centre row, so nearly every point is deferred with open views in ALL groups -- dense masks, every group edge) and compact
(GS.compact_cloud: one small patch per wave, where a point leaves open its owner view and no other -- masks that exist through the
zero-fill and the zero words alone).

Storages: float64 storage holds the on-plane points as built (3 ulp of float64 from their planes: k_fuse defers them, k_fuse_mid cannot
prove them either, the reference's own arithmetic decides: fuse_deferred()[1] > 0).  float32 storage holds them rounded to float32 --
half a float32 ulp from their planes, still inside k_fuse's margin (deferred) but 1e8 times k_fuse_mid's, which proves them: there
fuse_deferred()[1] may be 0 and is printed, not asserted.  The oracle's rows are computed per form.

Non-vacuity, asserted before any comparison: k_fuse deferred at least half of the call's on-plane points (a floor, not an estimate:
such a point lies far inside the float32 margin of its owner view, and only the points on the far plane whose pixel lies outside
the image by more than the margin -- under half of a fifth -- are proven out by another plane); the oracle votes for at least 90 %
of them; no call above 64 views decides early (the gate is cnv <= 64 in launch_fuse_t: the line to change ON PURPOSE when early
decisions are extended).  Counts are printed per call.  A HIP error ends the module: nothing more is started on the device."""
import functools

import numpy as np
import pytest

import f3d
import group_scenes as GS
from test_poison_gpu import stop_on_hip_error

pytestmark = pytest.mark.gpu

NC = GS.NCLASSES
H, W = GS.H, GS.W
EDGE_VIEWS = [63, 64, 65, 127, 128, 129, 241, 242, 255, 256, 257, 1024, 1025]
SMALL_N = [1, 2, 63, 64, 65, 127, 128, 129, 513]
# owner sets at 193 views (four groups, the last of one view): where the open views lie
CHOSEN = {'group0': (0, 63), 'group3': (192,), 'group1': (64, 127), 'groups0and3': (0, 63, 192), 'every': GS.group_edge_owners(193)}
CLOUD_A = {V: (GS.group_edge_owners(V), 8, 200) for V in EDGE_VIEWS}          # (owners, per, random points) of part (a), (f)
CLOUD_B = {V: (GS.group_edge_owners(V), 8, 400) for V in (65, 129)}           # on-plane points first, 520 / 600 points in all
CLOUD_E = (tuple(range(0, 300, 13)), 12, 500)
CLOUD_G = {V: (GS.group_edge_owners(V), 8, 400) for V in (130, 255, 256)}


@pytest.fixture(scope='module')
def ctx():
    return f3d.default_context()


@functools.lru_cache(maxsize=None)
def _stream():
    import torch
    return torch.cuda.Stream(torch.device('cuda', 0))


@functools.lru_cache(maxsize=8)
def _dev(V, kind):
    """The view table and the masks of a scene on the device."""
    import torch
    dev = torch.device('cuda', 0)
    return torch.from_numpy(np.array(GS.scene(V).views)).to(dev), torch.from_numpy(np.array(GS.masks(V, kind))).to(dev)


def _fuse(ctx, pts, V, kind, thr, flt=None, way='sort', f32=False, votes=False, bounds=None):
    """One fused call on a device-resident cloud, device entry on a side stream, outputs sentinel-filled
    -> (labels int64, vote rows uint16 or None, fuse_deferred(), fuse_decided())."""
    import torch
    dev = torch.device('cuda', 0)
    vd, md = _dev(V, kind)
    x = torch.from_numpy(np.array(pts, dtype=np.float32 if f32 else np.float64)).to(dev)
    n = x.shape[0]
    dt = f3d.F32 if f32 else f3d.F64
    cls = torch.full((n,), -7, dtype=torch.int64, device=dev)
    vo = torch.full((n, NC + 1), 7, dtype=torch.uint16, device=dev) if votes else None
    flags = f3d.FUSE_SORT if way == 'sort' else 0
    flt = None if flt is None else list(flt)
    s = _stream()
    s.wait_stream(torch.cuda.current_stream(dev))
    try:
        with torch.cuda.stream(s):
            if bounds is None:
                ctx.project_vote_argmax_dev(x.data_ptr(), dt, n, vd.data_ptr(), V, md.data_ptr(), H, W, NC, thr, flt, cls.data_ptr(),
                                            None if vo is None else vo.data_ptr(), s.cuda_stream, flags=flags)
            else:
                present = torch.empty(256, dtype=torch.uint8, device=dev)
                ctx.mask_presence_dev(md.data_ptr(), V, H, W, present.data_ptr(), s.cuda_stream)
                ctx.fuse_chunked_begin_dev(present.data_ptr(), n, V, H, W, NC, flt, s.cuda_stream)
                for a, b in zip(bounds[:-1], bounds[1:]):
                    ctx.fuse_chunk_dev(x.data_ptr(), dt, n, vd.data_ptr(), V, a, b, md.data_ptr(), H, W, NC, thr, flt, cls.data_ptr(),
                                       s.cuda_stream, flags=flags)
            try:
                ctx.take_device_error(s.cuda_stream)                           # clean: raises otherwise
            finally:
                s.synchronize()
        out = cls.cpu().numpy(), None if vo is None else vo.cpu().numpy(), ctx.fuse_deferred(), ctx.fuse_decided()
    except RuntimeError as e:
        stop_on_hip_error(f'fused call, {V} views, {kind}, {n} points', e)
        raise
    return out


def _same(got, rows, want_labels, want_rows, what):
    assert got.dtype == np.int64 and np.array_equal(got, want_labels), \
        f'{what}: {int((got != want_labels).sum())} of {len(got)} labels differ, the first at point {int(np.flatnonzero(got != want_labels)[0])}'
    if rows is not None:
        want = want_rows.astype(np.uint16)
        assert rows.dtype == np.uint16 and np.array_equal(rows, want), \
            f'{what}: vote rows differ at {int((rows != want).any(1).sum())} of {len(want)} points, the first {int(np.flatnonzero((rows != want).any(1))[0])}'


def _scene_is_not_vacuous(V, kind, cloud, f32, n=None):
    """The oracle's side: -> on-plane points among the first n of the cloud; at least 90 % of the cloud's on-plane points have a vote."""
    owner = GS.points(V, *cloud, f32)[1][:n]
    assert GS.voted_share(V, kind, *cloud, f32) >= 0.9
    return int((owner >= 0).sum())


def _deferred_enough(deferred, decided, V, on_plane, f32, what, chunked=False):
    print(f'{what}: deferred {deferred[0]}, of those to the reference arithmetic {deferred[1]}, on-plane points {on_plane}, left early {decided}')
    assert 2 * deferred[0] >= on_plane, what                                   # the floor: half of the on-plane points
    if on_plane and not f32:
        assert deferred[1] > 0, what                                           # (float32 storage: see the module's docstring)
    if V > 64 or chunked:
        assert decided == 0, what                                              # the gate cnv <= 64: change this line on purpose with it


def _run_settings(ctx, V, kind, cloud, settings, ways, vote_rows, n=None):
    """Every (setting, order, storage, with / without vote rows) of one cloud under one mask kind."""
    for f32 in (False, True):
        pts = GS.points(V, *cloud, f32)[0][:n]
        on_plane = _scene_is_not_vacuous(V, kind, cloud, f32, n)
        for thr, flt in settings:
            want = GS.labels(V, kind, *cloud, f32, thr, flt)[:n]
            want_rows = GS.votes(V, kind, *cloud, f32)[:n]
            for way in ways:
                for votes in vote_rows:
                    what = f'V={V} {kind} n={len(pts)} thr={thr} flt={flt} {way} {"f32" if f32 else "f64"} rows={votes}'
                    got, rows, deferred, decided = _fuse(ctx, pts, V, kind, thr, flt, way, f32, votes)
                    _deferred_enough(deferred, decided, V, on_plane, f32, what)
                    _same(got, rows, want, want_rows, what)


# ---------------------------------------------------------------------------------------------------- the scenes themselves
@pytest.mark.parametrize('V', EDGE_VIEWS + [193, 300, 130])
def test_on_plane_points_of_a_scene_end_labelled_and_unlabelled(V):
    """Per number of views: at threshold 0 and at 0.5, under at least one of the two mask kinds, the on-plane points of the scene's
    cloud hold both labelled and unlabelled points -- a tier that lost or invented the votes of an open view would change a label."""
    cloud = CLOUD_A.get(V) or {193: (CHOSEN['every'], 40, 0), 300: CLOUD_E, 130: CLOUD_G[130]}[V]
    for f32 in (False, True):
        for thr in (0.0, 0.5):
            assert GS.labelled_and_unlabelled(V, ('block64', 'iid'), *cloud, f32, thr), (V, f32, thr)


# ---------------------------------------------------------------------------------------------------- (a) every boundary
@pytest.mark.parametrize('kind', ['block64', 'iid'])
@pytest.mark.parametrize('V', EDGE_VIEWS)
def test_group_boundaries(ctx, V, kind):
    """Open views in the first and the last view of every group (of groups 0, 7, 15, 16 beyond 257 views): a last group of exactly 64
    views (64, 128, 256, 1024), a last group of ONE view (65, 129, 257, 1025), the guarded vote off at 241 and on at 242 views, the
    hand-off to k_fuse_exact from 256, and no parked slots at all at 1025 (17 groups)."""
    _run_settings(ctx, V, kind, CLOUD_A[V], GS.SETTINGS, ('sort', 'plain'), (False, True))


# ---------------------------------------------------------------------------------------------------- (b) small clouds
@pytest.mark.parametrize('n', SMALL_N)
@pytest.mark.parametrize('V', [65, 129])
def test_small_clouds_of_several_groups(ctx, V, n):
    """The first n points of a cloud whose on-plane points come first: fewer points than a wave, a wave-tile, a block's tile, and just
    beyond each; every point has a parked slot (park_slots == n)."""
    for kind in ('block64', 'iid'):
        _run_settings(ctx, V, kind, CLOUD_B[V], GS.SETTINGS[:2], ('sort', 'plain'), (False, True), n=n)


# ---------------------------------------------------------------------------------------------------- (c) open views in chosen groups
FORMS = {'spread': (40, 'sort'), 'compact': ('compact', 'plain')}              # form of the cloud -> (per of GS.points, order of the call)


@pytest.mark.parametrize('form', sorted(FORMS))
@pytest.mark.parametrize('where', sorted(CHOSEN))
def test_open_views_in_chosen_groups_under_poisoned_scratch(where, form):
    """193 views, four groups: owners only in group 0 (the later groups must write zero masks), only in group 3 (the earlier groups
    must be zero-filled when the slot is taken), only in group 1 (both), in groups 0 and 3, in every group.  No random points: every
    wave has slotted points.  Each cloud runs unpoisoned, after a 0xFF fill and after a 0x5A fill of a strict, reserved context's
    scratch: a mask word nobody wrote would then hold open views that were never left open, and the votes of those views count twice.

    spread: `per` 40 points on each plane of every owner, over the whole frustum, cell-sorted.  A wave's box is then metres wide, most
    views have no centre row for it and leave every point they may see open: the masks of ALL groups are densely set (the counts of part (a) show it: 276 of a cloud's
    280 points are deferred, nearly all of its 200 random points among them).  compact: one wave's worth of points per owner, a patch of one plane a few decimetres
    across, in caller order (GS.compact_cloud): every view has a row, and a point leaves open its owner view alone -- so with owners in
    group 3 only a point takes its slot in group 3 and the masks of groups 0..2 exist through the zero-fill alone, and with owners
    in group 0 only the masks of groups 1..3 are the zero words written for a slotted point."""
    per, way = FORMS[form]
    V, cloud = 193, (CHOSEN[where], per, 0)
    n = len(GS.points(V, *cloud)[0])
    own = f3d.Context(0)
    try:
        own.reserve(n, V, H, W)
        own.set_strict(True)
        a0 = own.alloc_count
        for pattern in (None, 0xFF, 0x5A):
            for kind in ('block64', 'iid'):
                for f32 in (False, True):
                    pts = GS.points(V, *cloud, f32)[0]
                    on_plane = _scene_is_not_vacuous(V, kind, cloud, f32)
                    assert on_plane == n
                    if pattern is not None:
                        buffers, nbytes = own.debug_poison(pattern)
                        assert buffers > 4 and nbytes > n * 4
                    what = f'V={V} owners {where} {form} {kind} {"f32" if f32 else "f64"} poison {pattern}'
                    got, rows, deferred, decided = _fuse(own, pts, V, kind, 0.5, None, way, f32, True)
                    _deferred_enough(deferred, decided, V, on_plane, f32, what)
                    _same(got, rows, GS.labels(V, kind, *cloud, f32, 0.5, None), GS.votes(V, kind, *cloud, f32), what)
                    assert own.alloc_count == a0, what                         # the run met the poisoned buffers, not fresh ones
    finally:
        own.close()


# ---------------------------------------------------------------------------------------------------- (d) slot overflow with several groups
@pytest.mark.parametrize('form', sorted(FORMS))
@pytest.mark.parametrize('V', [129, 193])
def test_parked_slot_overflow_with_several_groups(ctx, V, form, monkeypatch):
    """F3D_DEBUG_PARK_SLOTS unset, 0, 1, 7 and half of the deferred points: a point beyond the parked slots is redone from nothing,
    whichever group took its slot; the number of deferred points does not depend on the slots.  Owners in every group, both forms of (c)."""
    per, way = FORMS[form]
    cloud = (GS.group_edge_owners(V), per, 0)
    try:
        for kind in ('block64', 'iid'):
            for f32 in (False, True):
                pts = GS.points(V, *cloud, f32)[0]
                on_plane = _scene_is_not_vacuous(V, kind, cloud, f32)
                want, want_rows = GS.labels(V, kind, *cloud, f32, 0.5, None), GS.votes(V, kind, *cloud, f32)
                first = None
                for slots in (None, '0', '1', '7', 'half'):
                    if slots is None:
                        monkeypatch.delenv('F3D_DEBUG_PARK_SLOTS', raising=False)
                    else:
                        forced = first // 2 if slots == 'half' else int(slots)
                        monkeypatch.setenv('F3D_DEBUG_PARK_SLOTS', str(forced))
                    what = f'V={V} {form} {kind} {"f32" if f32 else "f64"} slots={slots}'
                    got, rows, deferred, decided = _fuse(ctx, pts, V, kind, 0.5, None, way, f32, True)
                    _deferred_enough(deferred, decided, V, on_plane, f32, what)
                    if slots is None:
                        first = deferred[0]
                    else:
                        assert deferred[0] == first > forced, what             # the overflow path ran
                    _same(got, rows, want, want_rows, what)
    finally:
        monkeypatch.delenv('F3D_DEBUG_PARK_SLOTS', raising=False)


# ---------------------------------------------------------------------------------------------------- (e) bins above 255
@pytest.mark.parametrize('kind', ['const', 'block64', 'merged2', 'iid'])
def test_bins_above_255_at_300_views(ctx, kind):
    """300 views, owners every 13th view.  const (label 86 everywhere) and block64 select the dword-bin instance, iid the any-alphabet
    one.  Under const the oracle counts more than 255 votes for 86 at 19 of the 1440 on-plane points (asserted: at least 10): a parked
    slot cannot hold such a bin (the refusal to park of the BIN32 instance), the byte that wraps inside k_fuse_mid sends the point on,
    and k_fuse_exact finishes it through the third counter.  block64 spreads a point's votes over eight labels: at most 44 for one at
    300 views, and with its labels merged into two, seven to one (merged2), at most 258 -- at 1 to 4 of the RANDOM points, at none of the
    on-plane ones (per 12, 24, 40 tried).  So block64 runs as it is, the scan of several dword bins finding nothing to refuse, and
    merged2 beside it, asserted to hold a bin above 255 at some point of the cloud."""
    V = 300
    for f32 in (False, True):
        rows = GS.votes(V, kind, *CLOUD_E, f32)
        own = GS.points(V, *CLOUD_E, f32)[1] >= 0
        over_own, over_all = int((rows[own].max(1) > 255).sum()), int((rows.max(1) > 255).sum())
        print(f'V={V} {kind} {"f32" if f32 else "f64"}: a bin above 255 at {over_own} on-plane points, {over_all} points in all; the fullest bin {int(rows.max())}')
        if kind == 'const':
            assert over_own >= 10
        elif kind == 'merged2':
            assert over_all >= 1
        else:
            assert over_all == 0 and rows.max() < 255
    _run_settings(ctx, V, kind, CLOUD_E, GS.SETTINGS[1::-1], ('sort', 'plain'), (False, True))


# ---------------------------------------------------------------------------------------------------- (f) the middle instances
@pytest.mark.parametrize('kind', ['alpha30', 'alpha80'])
@pytest.mark.parametrize('V', [65, 129])
def test_middle_instances_with_tables_in_global_memory(ctx, V, kind):
    """Alphabets of 30 and 80 labels (32 and 82 codes): with more than 64 views km2 = km3, the packed instances that read the view
    tables from global memory, 12 < codes <= 48 and 48 < codes <= 100."""
    assert len(np.unique(GS.masks(V, kind))) == int(kind[5:])
    _run_settings(ctx, V, kind, CLOUD_A[V], GS.SETTINGS, ('sort', 'plain'), (False, True))


# ---------------------------------------------------------------------------------------------------- (g) view chunks against groups
CUTS = [[0, 130], [0, 64, 130], [0, 65, 130], [0, 63, 64, 65, 129, 130], [0, 1, 130]]


@pytest.mark.parametrize('kind', ['block64', 'iid'])
def test_view_chunks_cut_at_and_beside_the_group_edges(ctx, kind):
    """130 views in chunks: a chunk is a launch of its own with its own groups (view v of a chunk from v0 is lane (v - v0) % 64 of group
    (v - v0) // 64), its bins carried in HBM.  Every cut list equals the one-shot call and the oracle; a chunked call parks nothing and
    decides nothing early."""
    V, cloud = 130, CLOUD_G[130]
    for f32 in (False, True):
        pts = GS.points(V, *cloud, f32)[0]
        on_plane = _scene_is_not_vacuous(V, kind, cloud, f32)
        want = GS.labels(V, kind, *cloud, f32, 0.5, None)
        one, _, deferred, decided = _fuse(ctx, pts, V, kind, 0.5, None, 'sort', f32)
        _deferred_enough(deferred, decided, V, on_plane, f32, f'V={V} {kind} {"f32" if f32 else "f64"} one shot')
        _same(one, None, want, None, (V, kind, f32, 'one shot'))
        for cuts in CUTS:
            got, _, deferred, decided = _fuse(ctx, pts, V, kind, 0.5, None, 'sort', f32, bounds=cuts)
            _deferred_enough(deferred, decided, V, on_plane, f32, f'V={V} {kind} {"f32" if f32 else "f64"} cuts {cuts}', chunked=True)
            assert np.array_equal(got, one), cuts
            _same(got, None, want, None, (V, kind, f32, cuts))


def test_view_chunks_at_255_views_and_their_refusal_at_256(ctx):
    """255 views is the most a chunked call takes (an 8-bit carried bin cannot wrap); at 256 f3d_fuse_chunked_begin_dev answers with
    its error, not with a result, and the one-shot call still serves the scene."""
    V, cloud, kind = 255, CLOUD_G[255], 'block64'
    for f32 in (False, True):
        pts = GS.points(V, *cloud, f32)[0]
        on_plane = _scene_is_not_vacuous(V, kind, cloud, f32)
        got, _, deferred, decided = _fuse(ctx, pts, V, kind, 0.5, None, 'sort', f32, bounds=[0, 63, 64, 65, 192, 255])
        _deferred_enough(deferred, decided, V, on_plane, f32, f'V={V} {kind} {"f32" if f32 else "f64"} chunked', chunked=True)
        _same(got, None, GS.labels(V, kind, *cloud, f32, 0.5, None), None, (V, f32))
    V, cloud = 256, CLOUD_G[256]
    pts = GS.points(V, *cloud)[0]
    with pytest.raises(ValueError, match=r'fuse_chunked_begin: bad arguments \(1\.\.255 views'):
        _fuse(ctx, pts, V, kind, 0.5, None, 'sort', False, bounds=[0, 128, 256])
    got, _, deferred, decided = _fuse(ctx, pts, V, kind, 0.5)                 # the context is usable, and the scene is served in one shot
    _deferred_enough(deferred, decided, V, _scene_is_not_vacuous(V, kind, cloud, False), False, f'V={V} one shot after the refusal')
    _same(got, None, GS.labels(V, kind, *cloud, False, 0.5, None), None, V)
