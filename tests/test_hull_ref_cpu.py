"""The exact hull reference (hull_ref.py) checks itself: the filtered signs equal an all-exact evaluation, every family yields the
classes it is built for, and the per-family class counts meet the floors the GPU tests (test_hull_exact_gpu.py) rely on.  No GPU."""
import itertools

import numpy as np
import pytest

import hull_ref as H
from oracle import np_ref as O

# conditions on the inputs of the GPU tests, met by the reference alone at H.SEED
MIN_SETS = 200                                    # per family
MIN_DEGENERATE = 30                               # per family with k = 0 or thickness 0 members
MIN_SIMPLICIAL = 100                              # per ulp family
DEGENERATE_FAMILIES = H.ULP_FAMILIES + ('sliver',)


def _small(e, rows=12):
    """At most `rows` points of a family set, the moved point among them."""
    P = e['P']
    if len(P) <= rows:
        return P
    keep = list(range(rows))
    if e.get('moved', 0) >= rows:
        keep[-1] = e['moved']
    return P[keep]


@pytest.mark.parametrize('name', H.FAMILIES)
def test_filtered_signs_equal_an_all_exact_evaluation(name):
    entries = H.family(name)
    undecided = 0
    for e in entries[::len(entries) // 50][:50]:
        P = _small(e)
        tri, s = H.orient_signs(P)
        tri2, exact = H.orient_signs(P, exact_only=True)
        assert np.array_equal(tri, tri2) and np.array_equal(s, exact), e
        own = H._own(tri, len(P))
        assert (s[own] == 0).all()
        undecided += int(((s == 0) & ~own).sum())
        # antisymmetry under a swap, on an independent path through the integers: S(b, a, c, d) = -S(a, b, c, d)
        swapped, _, _ = H.signs_against(P, tri[:, [1, 0, 2]], P, exact_only=True)
        assert np.array_equal(swapped, -exact)
    print(f'{name}: {undecided} exactly-zero entries in 50 sets')


def test_signs_and_classes_of_known_shapes():
    a, b, c = [0.0, 0, 0], [1.0, 0, 0], [0.0, 1, 0]
    tri, s = H.orient_signs(np.array([a, b, c, [0.25, 0.25, 3.0], [0.25, 0.25, -2 ** -1070], [0.5, 0.5, 0.0]]))
    assert tri[0].tolist() == [0, 1, 2] and s[0].tolist() == [0, 0, 0, 1, -1, 0]      # ((b - a) x (c - a)) = +z; a denormal height still counts
    cube = np.array(list(itertools.product((0.0, 1.0), repeat=3)))
    k = H.classify(cube)
    assert k.boundary.all() and k.hull_degenerate and not k.clear and len(k.sup_tri) == 6 * 4
    k = H.classify(np.vstack([cube, [[0.5, 0.5, 0.5], [0.5, 0.5, 1.0], [0.5, 1.0, 1.0]]]))      # the centre, a face centre, an edge midpoint
    assert k.boundary.tolist() == [True] * 8 + [False, True, True] and k.hull_degenerate
    tet = np.array([[0.0, 0, 0], [1, 0.25, 0], [0.25, 1, 0.125], [0.25, 0.5, 1], [0.375, 0.375, 0.25]])
    k = H.classify(tet)
    assert k.boundary.tolist() == [True] * 4 + [False] and not k.hull_degenerate and k.clear and len(k.sup_tri) == 4
    assert H.side_of_hull(tet[:4], H.classify(tet[:4]), np.array([[0.375, 0.375, 0.25], [5.0, 5, 5], [0.5, 0.125, 0.0]])).tolist() == [1, -1, 0]
    assert H.classify(np.vstack([tet, tet[:1]])).hull_degenerate                    # a duplicated vertex: four points on its facets' planes
    flat = np.array([[0.0, 0, 1], [1, 0, 1], [0, 1, 1], [1, 1, 1], [0.5, 0.25, 1]])
    k = H.classify(flat)
    assert k.hull_degenerate and k.boundary.all() and not k.clear
    assert H.classify(tet[:3]).hull_degenerate                                      # fewer than four points: coplanar
    bad = tet.copy(); bad[2, 1] = np.nan
    k = H.classify(bad)
    assert not k.finite and not k.clear and not k.simplicial
    tie = tet.copy(); tie[1, 0] = tie[0, 0] = -1.0                                  # two candidates for the smallest x: not clear
    assert not H.classify(tie).clear and not H.classify(tie).hull_degenerate


def test_a_virtual_start_point_on_a_plane_through_input_points_is_not_clear():
    """The set the kernel deferred on the MI355X although no four of its points are coplanar: points 2 and 4 have parallel (x, z)
    offsets from the lexicographic minimum (point 0), so they share a plane with it and the wrap's virtual point a + (0, E, 0)."""
    P = np.array([[0, 1, 1], [0.5, 0, 0.25], [1, 0.25, 0.5], [0.25, 0, 0.75], [1, 0, 0.5], [0.5, 0.5, 0]])
    k = H.classify(P)
    tri, s = H.orient_signs(P)
    own = H._own(tri, len(P))
    assert (s[~own] != 0).all() and not k.hull_degenerate and k.boundary.all()
    assert not H.start_points_clear(P, 0) and not k.clear
    d2, d4 = P[2] - P[0], P[4] - P[0]
    assert d2[0] * d4[2] == d2[2] * d4[0]
    Q = P.copy(); Q[4, 2] = 0.875                                                   # off that plane: clear
    assert H.start_points_clear(Q, 0) and H.classify(Q).clear


@pytest.mark.parametrize('name', H.ULP_FAMILIES)
def test_ulp_families_are_degenerate_at_zero_and_simplicial_off_it(name):
    seen = {k: [0, 0] for k in H.ULPS}
    for e in H.family(name):
        P, cls, k, at = e['P'], e['cls'], e['k'], e['moved']
        assert np.array_equal(np.delete(P, at, axis=0), e['base'])
        side = int(H.side_of_hull(e['base'], e['base_cls'], P[at:at + 1])[0])      # of the moved point against the polytope without it
        if k == 0:
            assert cls.hull_degenerate and side == 0 and cls.boundary[at], e
        else:
            assert not cls.hull_degenerate and side != 0, e
            assert bool(cls.boundary[at]) == (side < 0), e                          # a boundary point exactly when it lies outside
            if name == 'facet_ulp':                                                 # off one plane only: the sign of k decides the side
                assert side == -int(np.sign(k) * np.sign(_outward(e))), e
        if side > 0 or k == 0:
            others = np.delete(cls.boundary, at)
            assert others.all()                                                     # nothing else stopped being a vertex
        seen[k][side < 0] += 1
    grids = [e['bits'] for e in H.family(name)]
    assert grids.count(H.FINE) >= 100 and grids.count(H.COARSE) >= 50
    fine_flat = [e for e in H.family(name) if e['k'] == 0 and e['bits'] == H.FINE]
    tri_noise = 0
    for e in fine_flat:                                                             # exactly coplanar, yet float64 sees noise: the band
        tri, s = H.orient_signs(e['P'])
        _, det, _ = H.signs_against(e['P'], tri, e['P'])
        tri_noise += int(((s == 0) & ~H._own(tri, len(e['P'])) & (det != 0)).any())
    print(name, f'{tri_noise} of {len(fine_flat)} fine-grid k = 0 sets have an exactly-zero determinant that float64 evaluates nonzero')
    assert tri_noise >= 10 or name == 'vertex_ulp'                                  # two equal rows cancel exactly in float64 too
    print(name, 'moved point (inside or on, outside) per k:', seen)
    assert all(sum(v) >= 15 for v in seen.values())
    assert sum(v[1] for k, v in seen.items() if k) >= 40 and sum(v[0] for k, v in seen.items() if k) >= 40      # both sides are exercised


def _outward(e):
    """The component, along the moved coordinate, of the outward normal of the facet the point was placed on."""
    base, t = e['base'], e['base_cls'].sup_tri[e['facet']]
    n = np.cross(base[t[1]] - base[t[0]], base[t[2]] - base[t[0]])              # S > 0 on this normal's side
    return -int(e['base_cls'].sup_inner[e['facet']]) * n[e['axis']]


@pytest.mark.parametrize('name', H.FAMILIES)
def test_family_class_counts_meet_the_floors_of_the_gpu_tests(name):
    entries = H.family(name)
    c = H.counts(entries)
    print(name, c)
    assert all(len(e['P']) <= (16 if name == 'lattice' else 32) for e in entries)
    assert c['sets'] >= MIN_SETS
    if name in DEGENERATE_FAMILIES:
        assert c['degenerate'] >= MIN_DEGENERATE
    if name in H.ULP_FAMILIES:
        assert c['simplicial'] >= MIN_SIMPLICIAL and c['clear'] >= 10               # some must be certified: rule 3 has something to bite on
    if name == 'clear':
        assert c['clear'] == c['sets']
    if name == 'far_f32':
        assert all(np.array_equal(e['P'], e['P'].astype(np.float32)) for e in entries) and c['degenerate'] == 0
    if name == 'sliver':
        for e in entries:
            assert e['cls'].hull_degenerate or e['thickness'] != 0.0
            assert not (e['thickness'] == 0.0 and not e['cls'].hull_degenerate)
    if name == 'lattice':
        for plain, far in zip(entries[0::2], entries[1::2]):                        # an exact shift changes no class
            assert np.array_equal(far['P'] - 2.0 ** 20, plain['P'])
            assert np.array_equal(plain['cls'].boundary, far['cls'].boundary) and plain['cls'].hull_degenerate == far['cls'].hull_degenerate
        assert 30 <= c['degenerate'] <= c['sets'] - 30                              # both classes in numbers
    if name == 'symmetric':
        gaps = [H.box_from_vertices(e['P'], np.flatnonzero(e['cls'].boundary))[3] for e in entries]
        assert max(gaps) < 1e-12 and c['simplicial'] >= 150                         # eigenvalues tie to rounding; the hulls are simplicial


def test_same_seed_same_sets():
    H.family.cache_clear()
    a = [e['P'].copy() for e in H.family('edge_ulp')]
    H.family.cache_clear()
    b = [e['P'] for e in H.family('edge_ulp')]
    assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def test_clear_sets_agree_with_qhull_and_the_oracle_box():
    """On a clear set Qhull has nothing to merge: the boundary points are ConvexHull(P).vertices, and the box from exact moments is the
    oracle's box (hull -> numpy mean / cov -> eigh) within the existing GPU test's tolerances."""
    from scipy.spatial import ConvexHull
    n = 0
    for name in H.FAMILIES:
        for e in H.family(name):
            if not e['cls'].clear:
                continue
            P = e['P']
            assert not e['cls'].hull_degenerate
            v = np.flatnonzero(e['cls'].boundary)
            assert np.array_equal(v, np.sort(ConvexHull(P).vertices)), (name, P)
            c, R, ext, gap = H.box_from_vertices(P, v)
            n += 1
            if gap > 1e-3:
                oc, oR, oe = O.obb_from_points(P)
                scale = np.abs(P).max()
                assert np.abs(c - oc).max() < 1e-9 * scale / gap and np.abs(ext - oe).max() < 1e-9 * scale / gap
                assert np.allclose(np.abs(np.sum(R * oR, axis=0)), 1.0, atol=1e-7 / gap)
    assert n >= 300
