"""The certified hull (csrc/f3d_hull.hip) and the candidate pipeline (csrc/f3d_obb.hip) in the band between general position and exact
degeneracy, against the exact reference of hull_ref.py -- not against Qhull, which merges facets within its own tolerance and cannot
referee there.  The claim under test is "prove or defer": a set the kernel reports OK has exactly the exact hull's vertices and a box
that contains the set; a set it cannot prove comes back DEFERRED with a zero box.  Needs a GPU.

The inputs are hull_ref.family(name) at hull_ref.SEED; the class counts the rules rely on (at least 200 sets per family, 30
hull-degenerate, 100 simplicial) are conditions on those inputs and are checked on the CPU by test_hull_ref_cpu.py."""
from fractions import Fraction

import numpy as np
import pytest

import f3d
import hull_ref as H

pytestmark = pytest.mark.gpu

OK, FEW, DEFERRED = f3d.OBB_OK, f3d.OBB_FEW, f3d.OBB_DEFERRED


def slack_for(P):
    """64 * 2^-53 * (max |coordinate| + diameter).  Derivation: the kernel forms the mean m (|m| <= max |coordinate|), the differences
    p - m (<= diameter), three-term projections on unit axes (<= diameter), half the sum of two of them, and the centre m + R h
    (<= max |coordinate| + diameter): each of containment and tightness accumulates under ten roundings of quantities bounded by
    max |coordinate| + diameter, each at most 2^-53 of that relatively; R is orthonormal to a few 2^-53 (Jacobi rotations), which
    acts on a vector no longer than the diameter.  64 is headroom over those ten-odd terms.  The test itself evaluates R^T (p - c)
    in exact rationals, so none of the slack is spent on the test's own rounding."""
    return 64 * 2.0 ** -53 * (float(np.abs(P).max()) + H.diameter(P))


def check_rules(P, cls, box, status, verts, tag):
    """Rules 1 to 5 for one set.  Returns the status."""
    n = len(P)
    # 1: the status is one of the three, FEW only below 4 points, a box that is not OK is all zero
    assert status in (OK, FEW, DEFERRED), tag
    assert status != FEW or n < 4, tag
    if status != OK:
        assert (box == 0).all(), tag
    # 2: a degenerate hull or a non-finite coordinate is never certified
    if not cls.finite or cls.hull_degenerate:
        assert status != OK, (tag, 'certified a hull with four points on a supporting plane')
    if status != OK:
        return status
    # 3: the vertex flags are the exact boundary points
    assert np.array_equal(np.asarray(verts, bool), cls.boundary), (tag, np.flatnonzero(verts), np.flatnonzero(cls.boundary))
    c, R, e = box[0:3], box[3:12].reshape(3, 3), box[12:15]
    vidx = np.flatnonzero(cls.boundary)
    # 4: the box of the reference where the axes are well conditioned (the tolerances of test_obb_fit_kernel_hull_vertices_and_boxes)
    rc, rR, re, gap = H.box_from_vertices(P, vidx)
    if gap > 1e-3:
        scale = np.abs(P).max()
        tol = 1e-9 * scale / gap
        assert np.abs(c - rc).max() < tol and np.abs(e - re).max() < tol, (tag, gap)
        assert np.allclose(np.abs(np.sum(R * rR, axis=0)), 1.0, atol=1e-7 / gap), (tag, gap)
    # 5: for any gap -- a proper rotation in the sign convention of f3d.h, a box that contains the set and touches it on all six faces
    assert abs(np.linalg.det(R) - 1.0) < 1e-12 and np.allclose(R.T @ R, np.eye(3), atol=1e-12), tag
    assert R[np.abs(R[:, 0]).argmax(), 0] > 0 and R[np.abs(R[:, 1]).argmax(), 1] > 0, tag
    slack = Fraction(slack_for(P))
    half = [Fraction(float(v)) / 2 for v in e]
    t = H.box_coordinates(box, P)
    for a in range(3):
        assert all(abs(row[a]) <= half[a] + slack for row in t), (tag, a, 'a point outside the box')
        assert max(t[i][a] for i in vidx) >= half[a] - slack and min(t[i][a] for i in vidx) <= -half[a] + slack, (tag, a, 'a face no vertex touches')
    return status


def _in_band(e):
    return e['cls'].finite and not e['cls'].hull_degenerate and not e['cls'].clear


def _family_run(name):
    ctx = f3d.default_context()
    entries = H.family(name)
    boxes, status, verts = ctx.obb_fit([e['P'] for e in entries], want_vertices=True)
    share = {}
    for i, e in enumerate(entries):
        st = check_rules(e['P'], e['cls'], boxes[i], int(status[i]), verts[i], (name, i, e.get('k'), e.get('thickness'), e.get('solid')))
        # 6: a clear set is always certified
        if e['cls'].clear:
            assert st == OK, (name, i, 'a clear set was deferred', e['P'])
        elif _in_band(e):                                            # 7: certifying an in-band set is allowed, never required: reported only
            key = e.get('k', e.get('thickness', e.get('solid', e.get('shifted'))))
            got = share.setdefault(key, [0, 0])
            got[0] += st == OK; got[1] += 1
    print(f'{name}: {int((status == OK).sum())} OK, {int((status == DEFERRED).sum())} deferred of {len(entries)};',
          'in-band certified per class:', {k: f'{v[0]}/{v[1]}' for k, v in share.items()})
    return entries, boxes, status, verts


@pytest.mark.parametrize('name', H.ULP_FAMILIES)
def test_ulp_families_prove_or_defer(name):
    """A point k ulps off a facet plane, off a point on a hull edge (its midpoint or quarter point), off another vertex
    (k = 0, +-1, +-2, +-4, +-2^10, +-2^20, +-2^30).
    k = 0 must defer; whatever is certified has the exact vertex set -- including whether the moved point is one.
    In-band sets certified on the MI355X (not asserted), per k: see IN_BAND_MEASURED."""
    entries, boxes, status, verts = _family_run(name)
    assert all(status[i] == DEFERRED for i, e in enumerate(entries) if e['k'] == 0)


@pytest.mark.parametrize('name', ['lattice', 'far_f32', 'sliver', 'symmetric', 'clear'])
def test_quantised_far_thin_and_symmetric_sets_prove_or_defer(name):
    """lattice: points of a 6^3 grid, plain and shifted by 2^20.  far_f32: float32 coordinates near 1e4.  sliver: dyadic sheets 0, 2^-45,
    2^-30 and 1e-7 thick, rotated; thickness 0 is exactly flat and must defer.  symmetric: regular solids whose eigenvalues tie to rounding
    (rule 4 is out of reach there, rule 5 is not).  clear: general position with margins 2^20 above the filter's bound -- always OK.
    One condition was added to `clear` after the first run on the MI355X: lattice set 0 (6 points, no four coplanar) was deferred
    because two of its points have parallel (x, z) offsets from the lexicographic minimum a, so they lie in one plane with a and the
    wrap's virtual start point a + (0, E, 0) (wave_hull's first wrap_edge compares exactly those).  hull_ref.start_points_clear() asks
    the 2^-30 margin of the 4-subsets that hold a and that virtual point as well."""
    entries, boxes, status, verts = _family_run(name)
    if name == 'sliver':
        assert all(status[i] == DEFERRED for i, e in enumerate(entries) if e['thickness'] == 0.0)
    if name in ('far_f32', 'clear'):
        assert (status == OK).all()


# In-band (non-degenerate, not clear) sets the kernel certified on the MI355X at hull_ref.SEED, as printed by the tests above.
# Reported, never asserted: a deferral is always a right answer.
IN_BAND_MEASURED = """
facet_ulp   129 of 212 OK.  k = +1: 5/15, -1: 2/15, +2: 8/15, -2: 5/15, +4: 10/15, -4: 9/15, +-2^10: 30/30, +-2^20: 29/29
            (every k = +-2^30 set is clear)
edge_ulp    102 of 212 OK.  k = +1: 0/15, -1: 1/15, +2: 1/15, -2: 3/15, +4: 4/15, -4: 4/15, +2^10: 15/15, -2^10: 14/15, +-2^20: 30/30,
            +-2^30: 4/4
vertex_ulp   76 of 212 OK.  k = +-1, +-2, +-4: 0/90, +2^10: 11/15, -2^10: 12/15, +2^20: 12/15, -2^20: 12/15, +2^30: 8/9, -2^30: 8/8
lattice      18 of 200 OK.  plain: 3/24, shifted by 2^20: 3/24
far_f32     200 of 200 OK (all clear)
sliver       85 of 200 OK.  thickness 2^-45: 17/50, 2^-30: 35/50, 1e-7: 26/43
symmetric   188 of 201 OK.  tetrahedron: 67/67, octahedron: 2/2 (65 are clear), cube: 54/67
clear       200 of 200 OK
"""


def _all_sets():
    return [e for name in H.FAMILIES for e in H.family(name)]


def test_same_bits_on_a_second_call_and_on_the_vertices_alone():
    """The fit is a function of the input: a second call returns the same bits.  And of the vertex set alone: fitting only the
    flagged vertices of an OK set returns the bits of the fit of the whole set -- wherever that second fit is certified, which it
    must be for every clear set.  Measured on the MI355X: 998 of 998 OK sets were certified again from their vertices; with an
    earlier draw of the slivers 3 of 1002 were deferred, which rule 7 allows (their vertices meet in the tournament in another order)."""
    ctx = f3d.default_context()
    sets = [e['P'] for e in _all_sets()]
    boxes, status, verts = ctx.obb_fit(sets, want_vertices=True)
    boxes2, status2, verts2 = ctx.obb_fit(sets, want_vertices=True)
    assert np.array_equal(boxes.view(np.int64), boxes2.view(np.int64)) and np.array_equal(status, status2)
    assert all(np.array_equal(a, b) for a, b in zip(verts, verts2))
    ok = np.flatnonzero(status == OK)
    assert len(ok) >= 500                                            # the clear sets alone are more than that (rule 6)
    b3, s3, v3 = ctx.obb_fit([sets[i][verts[i]] for i in ok], want_vertices=True)
    entries = _all_sets()
    alone = np.flatnonzero(s3 == OK)
    print(f'vertices alone: {len(alone)} of {len(ok)} OK; deferred alone:', [(entries[i]['family'], entries[i].get('k')) for i in ok[s3 != OK]])
    # the vertices of an in-band set are an in-band set, and meet in the tournament in another order: rule 7 lets the kernel defer them.
    # The vertices of a clear set are clear (same minimum, same E, fewer 4-subsets): those must be certified again.
    assert all(s3[j] == OK for j, i in enumerate(ok) if entries[i]['cls'].clear)
    assert ((s3 == OK) | (s3 == DEFERRED)).all() and (b3[s3 != OK] == 0).all() and len(alone) >= 500
    assert np.array_equal(b3[alone].view(np.int64), boxes[ok[alone]].view(np.int64))
    assert all(v3[j].all() for j in alone)


# ---------------------------------------------------------------------------------------------------------------- launch shapes
GRID = 65536                                      # k_obb_fit and k_obb_small_hulls launch min(n, 65536) blocks and stride by the grid
TWINS = 70


def _first_seventy(rng):
    """70 sets of at most 8 points that mix OK, FEW, exactly flat (DEFERRED) and in-band sets, deferred and OK ones alternating."""
    out = []
    for i in range(TWINS):
        kind = i % 5
        if kind == 0:                                                # exactly flat: deferred in the middle of the wrap, frontier in use
            p = np.empty((int(rng.integers(5, 9)), 3)); p[:, :2] = H.dyadic(rng.uniform(-1, 1, (len(p), 2))); p[:, 2] = 0.5
        elif kind in (1, 3):                                         # general position
            p = rng.normal(size=(int(rng.integers(5, 9)), 3))
        elif kind == 2:                                              # in band: a point a few ulps off the plane of three others
            p = H.dyadic(rng.uniform(0.25, 1, (7, 3)))
            p[6] = (p[0] + p[1] + 2 * p[2]) / 4
            p[6, i % 3] = H.ulp_move(float(p[6, i % 3]), (1, -1, 4, -1024, 2 ** 20)[i // 5 % 5])
        else:
            p = rng.normal(size=(int(rng.integers(0, 4)), 3))        # FEW
        out.append(np.ascontiguousarray(p))
    return out


def test_fit_block_stride_and_lds_reuse():
    """65536 + 70 sets in one launch: the grid is capped at 65536 blocks, so blocks 0..69 fit a second set with the LDS frontier
    (and registers) the first one left behind.  Set k + 65536 is a copy of set k: the twin rows are bit-identical, and 200 sampled
    sets obey rules 1 to 5.  Block k fits set k and then its twin, so what follows a deferred set in a block is that set again: an OK
    set right after a DEFERRED one would need the two twins to differ."""
    ctx = f3d.default_context()
    rng = np.random.default_rng(65)
    first = _first_seventy(rng)
    sizes = rng.integers(5, 9, GRID - TWINS)
    bulk = rng.normal(size=(int(sizes.sum()), 3))
    quant = rng.random(len(sizes)) < 0.25                            # a quarter on a coarse grid: coplanar quadruples, duplicates
    cuts = np.cumsum(sizes)[:-1]
    middle = np.split(bulk, cuts)
    middle = [np.round(p * 2) / 2 if q else p for p, q in zip(middle, quant)]
    sets = first + middle + [p.copy() for p in first]
    assert len(sets) == GRID + TWINS
    boxes, status, verts = ctx.obb_fit(sets, want_vertices=True)
    seen = set(status[:TWINS].tolist())
    assert seen == {OK, FEW, DEFERRED}, seen
    for k in range(TWINS):
        assert status[k] == status[k + GRID] and np.array_equal(boxes[k].view(np.int64), boxes[k + GRID].view(np.int64)), k
        assert np.array_equal(verts[k], verts[k + GRID]), k
    sample = list(range(TWINS)) + list(GRID + np.arange(0, TWINS, 7)) + rng.choice(np.arange(TWINS, GRID), 120, replace=False).tolist()
    assert len(sample) == 200
    tally = {OK: 0, FEW: 0, DEFERRED: 0}
    for k in sample:
        tally[check_rules(sets[k], H.classify(sets[k]), boxes[k], int(status[k]), verts[k], ('stride', k))] += 1
    print('block-stride sample:', tally)
    assert tally[OK] >= 80 and tally[DEFERRED] >= 20


# ---------------------------------------------------------------------------------------------------------------- the candidates pipeline
def _pipeline(x_np, dtype, ids, nids, min_members):
    """group_by_id_dev -> obb_candidates_dev, then gather_points_dev -> obb_fit_dev on the candidates, all on the device."""
    import torch
    ctx = f3d.default_context()
    dev = torch.device('cuda', 0)
    n = len(ids)
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        x, di = torch.from_numpy(x_np).to(dev), torch.from_numpy(ids).to(dev)
        order = torch.empty(n, dtype=torch.int32, device=dev); keys = torch.empty(n, dtype=torch.int32, device=dev)
        starts = torch.empty(nids + 2, dtype=torch.int64, device=dev)
        cand = torch.full((n,), -1, dtype=torch.int32, device=dev); cs = torch.empty(nids + 1, dtype=torch.int64, device=dev)
        ctx.group_by_id_dev(di.data_ptr(), n, nids, order.data_ptr(), keys.data_ptr(), starts.data_ptr(), s.cuda_stream)
        ctx.obb_candidates_dev(x.data_ptr(), dtype, n, order.data_ptr(), keys.data_ptr(), starts.data_ptr(), nids, min_members,
                               cand.data_ptr(), cs.data_ptr(), s.cuda_stream)
        s.synchronize()
        total = int(cs[nids].item())
        assert 0 <= total <= n
        gathered = torch.empty((max(total, 1), 3), dtype=torch.float64, device=dev)
        boxes = torch.empty((nids, 15), dtype=torch.float64, device=dev); status = torch.empty(nids, dtype=torch.int32, device=dev)
        isvert = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
        ctx.gather_points_dev(x.data_ptr(), dtype, cand.data_ptr(), total, gathered.data_ptr(), s.cuda_stream)
        ctx.obb_fit_dev(gathered.data_ptr(), cs.data_ptr(), nids, total, boxes.data_ptr(), status.data_ptr(), isvert.data_ptr(), None, s.cuda_stream)
        s.synchronize()
    return dict(order=order.cpu().numpy(), starts=starts.cpu().numpy(), cand=cand.cpu().numpy(), cs=cs.cpu().numpy(), total=total,
                gathered=gathered.cpu().numpy()[:total], boxes=boxes.cpu().numpy(), status=status.cpu().numpy(),
                isvert=isvert.cpu().numpy()[:total].astype(bool))


def _cast(p, dtype):
    """The cloud as the kernel gets it, and the float64 values those coordinates are."""
    if dtype == f3d.F32:
        q = np.ascontiguousarray(p, np.float32)
        return q, q.astype(np.float64)
    q = np.ascontiguousarray(p, np.float64)
    return q, q


def _fillers(rng, core, cls, count, dtype):
    """Points strictly inside every exact supporting plane of the core (checked on the values the kernel gets): centroid + lambda *
    (convex combination - centroid), lambda <= 0.5.  None when the core leaves no room for them in this dtype."""
    centroid = core.mean(0)
    got = np.empty((0, 3))
    for _ in range(4):
        w = rng.dirichlet(np.ones(len(core)), count)
        f = centroid + rng.uniform(0.0, 0.5, (count, 1)) * (w @ core - centroid)
        f = _cast(f, dtype)[1]
        got = np.concatenate([got, f[H.side_of_hull(core, cls, f) > 0]])     # redraw whatever is not strictly inside
        if len(got) >= count:
            return got[:count]
    return None


@pytest.fixture(scope='module')
def scenes():
    """One cloud per dtype: instances made of a family set as core plus 300..2000 interior fillers, at separate centres, and the
    special instances; shuffled, with ids outside [0, nids) mixed in.  Built once, left unchanged."""
    out = {}
    for dtype in (f3d.F64, f3d.F32):
        rng = np.random.default_rng(77)
        cores = [e for name in H.FAMILIES for e in H.family(name)[3::23]]
        pts, ids, inst = [], [], []
        for e in cores:
            core = _cast(e['P'], dtype)[1]
            cls = H.classify(core)
            if not len(cls.sup_tri):                                 # flat (as built, or once cast): the explicit flat instance covers that
                continue
            fill = _fillers(rng, core, cls, int(rng.integers(300, 2001)), dtype)
            if fill is None:
                continue
            k = len(inst)
            inst.append(dict(kind='core', family=e['family'], cls=cls, rows=sum(map(len, pts)) + np.arange(len(core))))
            pts.append(np.concatenate([core, fill])); ids.append(np.full(len(core) + len(fill), k))
        special = {}
        for kind in ('small', 'empty', 'flat', 'nan'):
            k = special[kind] = len(inst)
            inst.append(dict(kind=kind))
            if kind == 'empty':
                continue
            p = rng.normal(size=(100 if kind == 'small' else 600, 3)) * 0.3 + rng.uniform(-20, 20, 3)
            if kind == 'flat':
                p[:, 2] = 1.5
            if kind == 'nan':
                p[17, 1] = np.nan
            pts.append(p); ids.append(np.full(len(p), k))
        nids = len(inst)
        stray = rng.normal(size=(500, 3)) * 5
        pts.append(stray); ids.append(rng.choice([-1, -7, nids, nids + 3, 1 << 40], len(stray)))
        pts, ids = np.concatenate(pts), np.concatenate(ids).astype(np.int64)
        perm = rng.permutation(len(ids))
        x, wide = _cast(pts[perm], dtype)                            # point i is row perm[i] of the build order
        where = np.empty(len(perm), np.int64); where[perm] = np.arange(len(perm))
        for info in inst:
            if info['kind'] == 'core':
                info['core_index'] = where[info['rows']]
        out[dtype] = dict(x=x, wide=wide, ids=ids[perm], nids=nids, inst=inst, special=special, perm=perm)
    return out


@pytest.mark.parametrize('dtype', [f3d.F64, f3d.F32], ids=['f64', 'f32'])
def test_candidates_keep_every_exact_boundary_point(scenes, dtype):
    """Per id the candidates are members in ascending point index and hold every exact boundary point of the instance: the fillers are
    strictly inside every supporting plane of the core (verified exactly), so the instance's boundary points are the core's.  The
    small, empty, flat and NaN instances keep every member (a NaN ranks as an extreme in fbits, and the inner hull then defers).  Where
    the fit of the candidates and the host-pointer fit of all members are both OK, the boxes are bit-identical."""
    ctx = f3d.default_context()
    sc = scenes[dtype]
    ids, nids, wide = sc['ids'], sc['nids'], sc['wide']
    assert len(ids) < 262144                                         # one scan block here; the three-block scan has its own test
    r = _pipeline(sc['x'], dtype, ids, nids, 256)
    cs, cand = r['cs'], r['cand']
    assert cs[0] == 0 and (np.diff(cs) >= 0).all() and int((cand != -1).sum()) == cs[nids]
    members = [np.flatnonzero(ids == k) for k in range(nids)]
    full_boxes, full_status = ctx.obb_fit([wide[m] for m in members])
    dropped = same = 0
    for k, info in enumerate(sc['inst']):
        mem, c = members[k], cand[cs[k]:cs[k + 1]]
        assert np.array_equal(c, np.sort(c)) and len(np.unique(c)) == len(c) and set(c.tolist()) <= set(mem.tolist()), k
        if info['kind'] != 'core':
            assert np.array_equal(c, mem), (k, info['kind'])
            assert r['status'][k] != OK or info['kind'] == 'small', (k, info['kind'])
            continue
        boundary = info['core_index'][info['cls'].boundary]          # point indices of the core's exact boundary points
        assert set(boundary.tolist()) <= set(c.tolist()), (k, info['family'], 'a hull vertex was filtered out')
        dropped += len(mem) - len(c)
        assert np.array_equal(r['gathered'][cs[k]:cs[k + 1]], wide[c]), k           # the gather widens, nothing else
        if r['status'][k] == OK:                                     # rules 2 and 3 for the fit of the candidates: the hull of all members
            assert not info['cls'].hull_degenerate, (k, info['family'])
            assert np.array_equal(c[r['isvert'][cs[k]:cs[k + 1]]], np.sort(boundary)), (k, info['family'])
        if r['status'][k] == OK and full_status[k] == OK:
            assert np.array_equal(r['boxes'][k].view(np.int64), full_boxes[k].view(np.int64)), (k, info['family'])
            same += 1
    print(f'dtype {dtype}: {nids} ids, {dropped} members dropped, {same} boxes compared bit for bit')
    assert dropped > 0.25 * len(ids) and same >= 10                  # the filter and the comparison are exercised (not a yield figure)


def test_scan_blocks_and_small_hull_block_stride():
    """65536 + 70 ids of 9 members, min_members 8: 590,454 points, so the mask scan runs three blocks of 262,144 positions with ids
    straddling both borders, and k_obb_small_hulls' blocks 0..69 take a second id.  Id k + 65536 has the coordinates of id k: the twins
    keep the same members; 200 sampled ids keep every exact boundary point; the starts add up to the survivors."""
    nids, per = GRID + TWINS, 9
    rng = np.random.default_rng(9)
    base = rng.normal(size=(GRID, per, 3)) * 0.2 + rng.uniform(-30, 30, (GRID, 1, 3))
    base[::4] = np.round(base[::4] * 8) / 8                          # a quarter on a grid: ties among the extremes, uncertifiable inner hulls
    base[5::40, :, 2] = base[5::40, :1, 2]                           # some exactly flat
    coords = np.concatenate([base, base[:TWINS]])                    # [nids, 9, 3]
    n = nids * per
    assert n == 590454 and n > 2 * 262144
    # point i belongs to id i % nids: every member list is strided through the cloud, ascending
    x = np.ascontiguousarray(coords.transpose(1, 0, 2).reshape(n, 3))
    ids = np.tile(np.arange(nids, dtype=np.int64), per)
    assert (9 * np.arange(nids) // 262144 != (9 * np.arange(nids) + 8) // 262144).sum() == 2      # one id straddles each border
    r = _pipeline(x, f3d.F64, ids, nids, 8)
    cs, cand = r['cs'], r['cand']
    assert cs[0] == 0 and (np.diff(cs) >= 0).all() and (np.diff(cs) <= per).all()
    assert cs[nids] == int((cand != -1).sum()) == r['total']         # the starts add up to what the compaction wrote
    assert np.array_equal(r['starts'][:nids + 1], per * np.arange(nids + 1))
    kept = cand[:cs[nids]]
    assert np.array_equal(kept % nids, np.repeat(np.arange(nids), np.diff(cs)))       # every survivor under its own id ...
    slot = kept // nids
    inner = np.ones(len(kept), bool); inner[cs[1:nids]] = False
    assert (np.diff(slot)[inner[1:]] > 0).all()                      # ... in ascending point index
    for k in range(TWINS):
        assert np.array_equal(slot[cs[k]:cs[k + 1]], slot[cs[k + GRID]:cs[k + GRID + 1]]), k
        assert r['status'][k] == r['status'][k + GRID] and np.array_equal(r['boxes'][k].view(np.int64), r['boxes'][k + GRID].view(np.int64)), k
    sample = list(range(TWINS)) + [29127, 29128, 58254, 58255] + rng.choice(np.arange(TWINS, GRID), 126, replace=False).tolist()
    assert len(sample) == 200
    dropped = 0
    for k in sample:
        cls = H.classify(coords[k])
        assert set(np.flatnonzero(cls.boundary).tolist()) <= set(slot[cs[k]:cs[k + 1]].tolist()), k
        dropped += per - (cs[k + 1] - cs[k])
    print(f'{n - r["total"]} of {n} members dropped; {dropped} in the sample')
    assert n - r['total'] > 10000                                    # the filter is at work: interior members do go


def test_extremes_on_a_lattice_quantised_cloud():
    """obb_extremes through the host entry on coordinates rounded to a 0.25 grid, where many members tie: for every id and direction
    the reported member attains the exact maximum of the float32 dot (any tied member is acceptable)."""
    ctx = f3d.default_context()
    rng = np.random.default_rng(41)
    nids, n = 37, 20_000
    ids = rng.integers(-2, nids + 3, n).astype(np.int64)
    ids[ids == 5] = 6                                                # an id without members
    centres = rng.uniform(-4, 4, (nids + 3, 3))
    pts = np.round((centres[np.clip(ids, 0, nids + 2)] + rng.normal(size=(n, 3)) * [0.4, 0.2, 0.1]) * 4) / 4
    order, starts = ctx.group_by_id(ids, nids)
    ext = ctx.obb_extremes(pts)
    assert ext.shape == (nids, 26) and (ext[5] == -1).all()
    p32 = pts.astype(np.float32)
    x, y, z = p32[:, 0], p32[:, 1], p32[:, 2]
    dots = np.stack([x, y, z, x + y, x - y, x + z, x - z, y + z, y - z, (x + y) + z, (x + y) - z, (x - y) + z, (x - y) - z])
    ties = 0
    for k in range(nids):
        mem = np.flatnonzero(ids == k)
        if k == 5:
            continue
        assert len(mem) and np.array_equal(order[starts[k]:starts[k + 1]], mem)
        for d in range(13):
            hi, lo = ext[k, 2 * d], ext[k, 2 * d + 1]
            assert ids[hi] == k and dots[d, hi] == dots[d, mem].max(), (k, d)
            assert ids[lo] == k and dots[d, lo] == dots[d, mem].min(), (k, d)
            ties += int((dots[d, mem] == dots[d, mem].max()).sum() > 1)
    assert ties > 100                                                # the grid does produce tied extremes
