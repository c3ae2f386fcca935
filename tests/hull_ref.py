"""An exact reference for the certified hull (csrc/f3d_hull.hip) and the box fitted on it, CPU only.

Nothing here wraps gifts: every triple of input points is tested against every point.  The sign of
    S(a, b, c, d) = ((b - a) x (c - a)) . (d - a)
is evaluated vectorised in float64 with Shewchuk's stage-A bound (7 + 56 eps) eps * permanent, eps = 2^-53, as a filter; whatever the
filter cannot decide is evaluated exactly (float64 values are exact rationals: every coordinate is scaled to a Python integer over one
common power-of-two denominator).  A triple whose nonzero signs all agree spans a supporting plane of the hull; the points with sign 0
on such a plane are boundary points.  Every facet plane is spanned by three input points, so the union over the supporting triples is
the whole boundary.

The set families at the bottom sit in the band between general position and exact degeneracy: a point a few ulps off a facet plane, a
hull edge or another vertex, lattice and float32-quantised coordinates, far offsets, slivers, and symmetric solids.  Coordinates are
built so that the intended coincidences are exact (dyadic bases, midpoints and weighted points that are representable)."""
import functools
import itertools
from fractions import Fraction

import numpy as np

EPS = 2.0 ** -53
ERR_A = (7.0 + 56.0 * EPS) * EPS                 # Shewchuk, orient3d stage A
CLEAR_DET = 2.0 ** -30                           # clear: |det| > CLEAR_DET * permanent on every 4-subset (2^20 above the stage-A bound)
CLEAR_X = 2.0 ** -20                             # clear: the lexicographic minimum's x is below every other x by this share of the diameter
ULPS = (0, 1, -1, 2, -2, 4, -4, 2 ** 10, -2 ** 10, 2 ** 20, -2 ** 20, 2 ** 30, -2 ** 30)


# ---------------------------------------------------------------------------------------------------------------- exact signs
def _ints(X):
    """The entries of X as Python integers over one common power-of-two denominator (object array of X's shape)."""
    ratios = [float(v).as_integer_ratio() for v in np.asarray(X, np.float64).reshape(-1)]
    den = max(d for _, d in ratios)
    out = np.empty(len(ratios), object)
    out[:] = [n * (den // d) for n, d in ratios]
    return out.reshape(np.shape(X))


def _det_rows(A, B, C):
    """Shewchuk's orient3d expression on rows (a - d, b - d, c - d); works on float64 and on object (integer) arrays."""
    bdxcdy, cdxbdy = B[..., 0] * C[..., 1], C[..., 0] * B[..., 1]
    cdxady, adxcdy = C[..., 0] * A[..., 1], A[..., 0] * C[..., 1]
    adxbdy, bdxady = A[..., 0] * B[..., 1], B[..., 0] * A[..., 1]
    det = A[..., 2] * (bdxcdy - cdxbdy) + B[..., 2] * (cdxady - adxcdy) + C[..., 2] * (adxbdy - bdxady)
    return det, (bdxcdy, cdxbdy, cdxady, adxcdy, adxbdy, bdxady)


def signs_against(P, tri, Q, skip=None, exact_only=False):
    """sign of S(P[tri[t, 0]], P[tri[t, 1]], P[tri[t, 2]], Q[q]) as int8 [len(tri), len(Q)], exact; also the float64 determinant and
    permanent.  Entries under `skip` are left 0 and never evaluated exactly.  exact_only evaluates every entry in integers."""
    P, Q, tri = np.asarray(P, np.float64), np.asarray(Q, np.float64), np.asarray(tri, np.int64).reshape(-1, 3)
    if not (np.isfinite(P).all() and np.isfinite(Q).all()):
        raise ValueError('non-finite coordinates have no orientation')
    A = P[tri[:, 0]][:, None, :] - Q[None, :, :]
    B = P[tri[:, 1]][:, None, :] - Q[None, :, :]
    C = P[tri[:, 2]][:, None, :] - Q[None, :, :]
    det, (p0, p1, p2, p3, p4, p5) = _det_rows(A, B, C)
    perm = (np.abs(p0) + np.abs(p1)) * np.abs(A[..., 2]) + (np.abs(p2) + np.abs(p3)) * np.abs(B[..., 2]) + (np.abs(p4) + np.abs(p5)) * np.abs(C[..., 2])
    bound = ERR_A * perm
    s = np.zeros(det.shape, np.int8)
    s[det > bound] = -1                          # orient3d = -S
    s[-det > bound] = 1
    todo = np.ones(det.shape, bool) if exact_only else ~(np.abs(det) > bound)
    if skip is not None:
        todo &= ~skip
        s[skip] = 0
    t, q = np.nonzero(todo)
    if len(t):
        I = _ints(np.concatenate([P, Q]))
        IP, IQ = I[:len(P)], I[len(P):]
        d, _ = _det_rows(IP[tri[t, 0]] - IQ[q], IP[tri[t, 1]] - IQ[q], IP[tri[t, 2]] - IQ[q])
        s[t, q] = [(v < 0) - (v > 0) for v in d]
    return s, det, perm


def _triples(n):
    return np.array(list(itertools.combinations(range(n), 3)), np.int64).reshape(-1, 3)


def _own(tri, n):
    own = np.zeros((len(tri), n), bool)
    own[np.arange(len(tri))[:, None], tri] = True
    return own


def orient_signs(P, exact_only=False):
    """(tri int64 [T, 3], sign int8 [T, n]): all index triples i < j < k of P and the exact sign of ((b - a) x (c - a)) . (d - a) for
    every triple against every point.  A point of its own triple has sign 0 by definition."""
    P = np.asarray(P, np.float64).reshape(-1, 3)
    tri = _triples(len(P))
    s, _, _ = signs_against(P, tri, P, skip=_own(tri, len(P)), exact_only=exact_only)
    return tri, s


class Classes:
    """What classify() found.  boundary: bool [n]; sup_tri / sup_inner: the supporting triples and the sign the hull's side has."""
    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def simplicial(self):
        return self.finite and not self.hull_degenerate


def diameter(P):
    P = np.asarray(P, np.float64)
    return float(np.sqrt(((P[:, None, :] - P[None, :, :]) ** 2).sum(-1)).max()) if len(P) else 0.0


def classify(P):
    """boundary: every input point on some supporting plane of the exact hull.  hull_degenerate: some supporting plane holds four or
    more input points (duplicates counted), or all points are coplanar.  clear: every 4-subset has |det| > 2^-30 permanent (float64
    values: their error, 2^-50 permanent, is far below the margin), the lexicographically smallest point's x is below every other x by
    more than 2^-20 of the diameter, and all coordinates are finite.  The two margins are conditions on the input, 2^20 above the
    stage-A bound, so that no correct filter can be unsure about a clear set.
    One condition more, found on the GPU (a 6-point lattice set was deferred): the wrap starts from two virtual points next to the
    lexicographic minimum a, a' = a + (0, E, 0) and a'' = a - (0, 0, E) with E the largest coordinate difference to a, and compares
    input points around the axis a - a'.  Two input points whose (x, z) offsets from a are parallel lie in one plane with a and a'
    -- the filter is rightly unsure there although no four INPUT points are coplanar.  So clear also asks |det| > 2^-30 permanent
    of every 4-subset that holds a, a' and two of the other points (a'' among them): start_points_clear()."""
    P = np.asarray(P, np.float64).reshape(-1, 3)
    n = len(P)
    if not np.isfinite(P).all():
        return Classes(n=n, finite=False, boundary=None, hull_degenerate=False, clear=False, sup_tri=None, sup_inner=None)
    tri = _triples(n)
    own = _own(tri, n)
    s, det, perm = signs_against(P, tri, P, skip=own)
    pos, neg = (s > 0).any(1), (s < 0).any(1)
    sup = pos ^ neg                                                  # spans a plane (some nonzero sign) with everything on one side
    flat = not (pos | neg).any()                                     # no triple sees a point off its plane: all coplanar (or n < 4)
    boundary = np.ones(n, bool) if flat else (s[sup] == 0).any(0)
    degenerate = flat or bool(((s[sup] == 0).sum(1) >= 4).any())
    clear = n >= 4 and bool((np.abs(det)[~own] > CLEAR_DET * perm[~own]).all())
    if clear:
        order = np.lexsort((P[:, 2], P[:, 1], P[:, 0]))
        clear = bool(P[order[1], 0] - P[order[0], 0] > CLEAR_X * diameter(P)) and start_points_clear(P, int(order[0]))
    return Classes(n=n, finite=True, boundary=boundary, hull_degenerate=degenerate, clear=clear, sup_tri=tri[sup],
                   sup_inner=np.where(pos[sup], 1, -1).astype(np.int8))


def start_points_clear(P, ia):
    """No plane through a = P[ia], the kernel's virtual point a + (0, E, 0) and another point (an input point or a - (0, 0, E)) comes
    within 2^-30 permanent of a further one."""
    a = P[ia]
    E = float(np.abs(P - a).max())
    ext = np.vstack([P, a + [0.0, E, 0.0], a - [0.0, 0.0, E]])
    others = np.array([j for j in range(len(ext)) if j not in (ia, len(P))])
    tri = np.array([[ia, len(P), j] for j in others])
    _, det, perm = signs_against(ext, tri, ext[others], skip=np.eye(len(others), dtype=bool))
    off = ~np.eye(len(others), dtype=bool)
    return bool((np.abs(det)[off] > CLEAR_DET * perm[off]).all())


def side_of_hull(P, cls, Q):
    """int8 [len(Q)]: +1 strictly inside every exact supporting plane of P's hull, -1 strictly outside one, 0 on the boundary."""
    s, _, _ = signs_against(P, cls.sup_tri, Q)
    s = s * cls.sup_inner[:, None]
    return np.where((s < 0).any(0), -1, np.where((s > 0).all(0), 1, 0)).astype(np.int8)


# ---------------------------------------------------------------------------------------------------------------- the box
def box_from_vertices(P, vertex_idx):
    """(centre, R, extent, gap): mean and covariance (divided by the count) of P[vertex_idx] in exact rationals, each rounded once to
    float64; numpy.linalg.eigh, axes by descending eigenvalue, third axis = first x second, extents of the vertices.  gap is the
    relative eigenvalue gap of test_obb_fit_kernel_hull_vertices_and_boxes: min diff / max |coordinate of P|^2."""
    P = np.asarray(P, np.float64).reshape(-1, 3)
    V = P[np.asarray(vertex_idx)]
    F = [[Fraction(float(v)) for v in row] for row in V]
    n = len(F)
    mean = [sum(r[a] for r in F) / n for a in range(3)]
    cov = np.empty((3, 3))
    for a in range(3):
        for b in range(a, 3):
            cov[a, b] = cov[b, a] = float(sum((r[a] - mean[a]) * (r[b] - mean[b]) for r in F) / n)
    mean = np.array([float(m) for m in mean])
    w, U = np.linalg.eigh(cov)
    R = U[:, np.argsort(-w, kind='stable')]
    R[:, 2] = np.cross(R[:, 0], R[:, 1])
    loc = (V - mean) @ R
    lo, hi = loc.min(0), loc.max(0)
    gap = float(np.diff(np.sort(w)).min() / np.abs(P).max() ** 2)
    return mean + R @ ((lo + hi) / 2), R, hi - lo, gap


def box_coordinates(box, Q):
    """R^T (q - c) for the rows of Q as exact rationals ([len(Q)][3] Fractions): the box's float64 entries are taken as given."""
    c = [Fraction(float(v)) for v in box[0:3]]
    R = [[Fraction(float(v)) for v in box[3 + 3 * r:6 + 3 * r]] for r in range(3)]
    out = []
    for q in np.asarray(Q, np.float64).reshape(-1, 3):
        d = [Fraction(float(q[r])) - c[r] for r in range(3)]
        out.append([R[0][a] * d[0] + R[1][a] * d[1] + R[2][a] * d[2] for a in range(3)])
    return out


# ---------------------------------------------------------------------------------------------------------------- the families
COARSE, FINE = 10, 26


def dyadic(x, bits=COARSE):
    """x rounded to multiples of 2^-bits.  Midpoints and weighted points such as (A + B + 2 C) / 4 of such values (|x| < 8) are
    representable at either grid, so the intended coincidences are exact.  On the coarse grid every product in the determinant is
    exact as well: an exactly coplanar quadruple evaluates to 0.0 and a kernel needs no error bound to notice it.  On the fine grid
    the coordinate differences still are exact but their products no longer fit 53 bits: the float64 determinant of an exactly
    coplanar quadruple is rounding noise of either sign, which only the stage-A bound tells from a real sign.  (A first version with
    the coarse grid alone passed against a kernel built with the bound set to 0: it did not reach the band.)"""
    return np.round(np.asarray(x, np.float64) * 2.0 ** bits) / 2.0 ** bits


def ulp_move(x, k):
    """x moved by k units in the last place (k > 0: towards +inf); x is finite and nonzero, and the move stays on x's side of 0."""
    bits = np.array([x], np.float64).view(np.int64)
    bits += k if x > 0 else -k
    y = float(bits.view(np.float64)[0])
    assert np.isfinite(y) and (y > 0) == (x > 0) and (k == 0 or (y > x) == (k > 0))
    return y


def rotation(rng):
    q = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    return q * np.sign(np.linalg.det(q))


def _entry(P, family, cls=None, **kw):
    P = np.ascontiguousarray(P, np.float64)
    return dict(P=P, family=family, cls=cls if cls is not None else classify(P), **kw)


def _polytope(rng, bits):
    """A simplicial dyadic polytope of 8..16 vertices: dyadic points near an ellipsoid, all of them vertices, no four on a facet plane."""
    while True:
        m = int(rng.integers(8, 17))
        v = rng.normal(size=(m, 3))
        P = dyadic(v / np.linalg.norm(v, axis=1)[:, None] * rng.uniform(0.5, 2.0, 3) + rng.integers(-2, 3, 3), bits)
        cls = classify(P)
        if cls.boundary.all() and not cls.hull_degenerate:
            return P, cls


def _best_axis(normals):
    """The coordinate axis that is least parallel to every one of the planes (rows: their normals)."""
    n = np.abs(normals / np.linalg.norm(normals, axis=1)[:, None])
    return int(n.min(0).argmax())


def _normal(P, t):
    return np.cross(P[t[1]] - P[t[0]], P[t[2]] - P[t[0]])


def _ulp_family(name, seed, per_k, per_zero):
    """per_k sets for every k != 0 of ULPS and per_zero for k = 0.  k = 0 is hull-degenerate by construction; a k != 0 member is redrawn until it is not (a move
    that happens to stay on a plane through three other points would still be degenerate)."""
    rng = np.random.default_rng([seed, {'facet_ulp': 1, 'edge_ulp': 2, 'vertex_ulp': 3}[name]])
    out = []
    for k in ULPS:
        made = 0
        while made < (per_k if k else per_zero):
            bits = FINE if made % 3 else COARSE                      # two sets in three on the fine grid
            base, bcls = _polytope(rng, bits)
            ti = int(rng.integers(len(bcls.sup_tri)))
            t = bcls.sup_tri[ti]
            if name == 'facet_ulp':                                  # (A + B + 2 C) / 4: on the facet's plane, strictly inside the facet
                x = (base[t[0]] + base[t[1]] + 2 * base[t[2]]) / 4
                axis = _best_axis(_normal(base, t)[None])
            elif name == 'edge_ulp':                                 # on the hull edge t0 - t1; its two facets decide the axis
                # the exact midpoint, or every other time the quarter point: about the midpoint the rows A - M = -(B - M) cancel
                # exactly in float64 as well, about the quarter point (A - M = -3 (B - M)) the products round differently
                x = (base[t[0]] + base[t[1]]) / 2 if made % 2 else (base[t[0]] + 3 * base[t[1]]) / 4
                both = [u for u in bcls.sup_tri if t[0] in u and t[1] in u]
                axis = _best_axis(np.array([_normal(base, u) for u in both]))
            else:                                                    # a copy of the vertex t0; every facet at that vertex decides the axis
                x = base[t[0]].copy()
                axis = _best_axis(np.array([_normal(base, u) for u in bcls.sup_tri if t[0] in u]))
            if x[axis] == 0.0:
                continue
            x[axis] = ulp_move(float(x[axis]), k)
            at = int(rng.integers(len(base) + 1))                    # the moved point takes any position in the set
            P = np.insert(base, at, x, axis=0)
            cls = classify(P)
            if k != 0 and cls.hull_degenerate:
                continue
            out.append(_entry(P, name, cls, k=k, moved=at, axis=axis, facet=ti, bits=bits, base=base, base_cls=bcls))
            made += 1
    return out


def _lattice(seed, count=100):
    rng = np.random.default_rng([seed, 4])
    cells = np.array(list(itertools.product(range(6), repeat=3)), np.float64) * 0.25
    out = []
    for i in range(count):
        m = 6 + i % 11
        P = cells[rng.choice(len(cells), m, replace=False)]
        cls = classify(P)
        out.append(_entry(P, 'lattice', cls, shifted=False))
        out.append(_entry(P + 2.0 ** 20, 'lattice', shifted=True))   # the shift is exact: the same classes, a coarser float64 grid
    return out


def _far_f32(seed, count=200):
    rng = np.random.default_rng([seed, 5])
    return [_entry((rng.normal(size=(20, 3)) * 0.15 + rng.uniform(-1e4, 1e4, 3)).astype(np.float32).astype(np.float64), 'far_f32')
            for _ in range(count)]


SLIVER_THICKNESS = (0.0, 2.0 ** -45, 2.0 ** -30, 1e-7)


def _sliver(seed, per_thickness=50):
    rng = np.random.default_rng([seed, 6])
    out = []
    for th in SLIVER_THICKNESS:
        for _ in range(per_thickness):
            m = int(rng.integers(6, 17))
            P = np.empty((m, 3))
            P[:, :2] = dyadic(rng.uniform(-2, 2, (m, 2)))
            P[:, 2] = rng.integers(-3, 4, m) * th
            if th == 0.0 and len(out) % 2:                           # exactly flat in a tilted plane, fine grid: z = x / 2 + y / 4 + c is exact
                P[:, :2] = dyadic(rng.uniform(-2, 2, (m, 2)), FINE)
                P[:, 2] = P[:, 0] / 2 + P[:, 1] / 4 + float(dyadic(rng.uniform(-1, 1)))
                P = P[:, rng.permutation(3)]
            elif th == 0.0:                                          # exactly flat, in any of the three coordinate planes, at a dyadic height
                P[:, 2] = float(dyadic(rng.uniform(-1, 1)))
                P = P[:, rng.permutation(3)]
            else:
                P = P @ rotation(rng).T
            out.append(_entry(P, 'sliver', thickness=th))
    return out


SOLIDS = {
    'tetrahedron': np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], np.float64),
    'octahedron': np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64),
    'cube': np.array(list(itertools.product((-1.0, 1.0), repeat=3))),
}


def _symmetric(seed, per_solid=67):
    """Corners of the regular solids at a dyadic size about a dyadic centre (no coordinate is 0), every coordinate of every vertex moved
    by its own 1..24 ulps: the cube's faces split into triangles, and the covariance's eigenvalues tie to rounding."""
    rng = np.random.default_rng([seed, 7])
    out = []
    for solid, corners in SOLIDS.items():
        for _ in range(per_solid):
            P = corners * float(2.0 ** rng.integers(-2, 3)) + (rng.integers(5, 13, 3) * rng.choice([-1.0, 1.0], 3))
            moves = (rng.permutation(3 * len(P)) + 1).reshape(-1, 3) * rng.choice([-1, 1], (len(P), 3))      # distinct sizes
            P = np.array([[ulp_move(float(v), int(k)) for v, k in zip(row, mrow)] for row, mrow in zip(P, moves)])
            out.append(_entry(P, 'symmetric', solid=solid))
    return out


CLEAR_SIZES = (4, 5, 6, 7, 8, 10, 12, 16, 20, 32)


def _clear(seed, count=200):
    rng = np.random.default_rng([seed, 8])
    out = []
    while len(out) < count:
        m = CLEAR_SIZES[len(out) % len(CLEAR_SIZES)]
        p = rng.normal(size=(m, 3)) * rng.uniform(0.05, 2.0, 3) if rng.integers(2) else rng.uniform(-1, 1, (m, 3)) * rng.uniform(0.1, 3.0, 3)
        P = p @ rotation(rng).T + rng.uniform(-5, 5, 3)
        cls = classify(P)
        if cls.clear:
            out.append(_entry(P, 'clear', cls))
    return out


FAMILIES = ('facet_ulp', 'edge_ulp', 'vertex_ulp', 'lattice', 'far_f32', 'sliver', 'symmetric', 'clear')
ULP_FAMILIES = FAMILIES[:3]
SEED = 2024                                       # the seed whose class counts test_hull_ref_cpu.py checks and the GPU tests rely on


@functools.lru_cache(maxsize=None)
def family(name, seed=SEED):
    """The sets of one family as a tuple of dicts: P float64 [n, 3], cls = classify(P), and what the family built (k, moved, ...)."""
    if name in ULP_FAMILIES:
        return tuple(_ulp_family(name, seed, 15, 32))
    return tuple({'lattice': _lattice, 'far_f32': _far_f32, 'sliver': _sliver, 'symmetric': _symmetric, 'clear': _clear}[name](seed))


def counts(entries):
    c = dict(sets=len(entries), degenerate=0, simplicial=0, clear=0)
    for e in entries:
        c['degenerate'] += bool(e['cls'].hull_degenerate)
        c['simplicial'] += bool(e['cls'].simplicial)
        c['clear'] += bool(e['cls'].clear)
    return c
