"""NumPy / SciPy restatement of f3d_extract_planes (include/f3d.h; the oracle of tests/test_planes_*.py) and the test scenes.

Every step follows the contract operation for operation: dot(a, b) = (a0*b0 + a1*b1) + a2*b2 with every product and sum rounded
alone, the row-order PCA sums, jacobi3 (csrc/f3d_eigen.h, restated on Python floats), the fixed-shape plane sums (chunks of 4096,
lane-strided wave sums, xor butterfly) and the synchronous attach rounds.  Besides the outputs, ``extract`` returns the MARGIN: the
smallest relative distance |value - threshold| / threshold over every predicate it evaluated (variation, angle, offset, dist).  A
scene is fit for an exact comparison only when its margin is far above rounding; that is a condition on the input, not a tolerance.
Result also carries the in-plane axes u, v, the eigenvalues lam (lambda0, lambda1, lambda2 per plane), the core flags and `members`,
the core members every plane was fitted on (before the inlier test).
"""
import math
from collections import namedtuple

import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components
from scipy.spatial import cKDTree

Result = namedtuple('Result', ['labels', 'planes', 'corners', 'counts', 'normals', 'margin', 'u', 'v', 'lam', 'core', 'members'])

DEFAULTS = dict(angle=10.0, offset=0.01, dist=0.01, max_variation=0.01, min_points=50, max_rounds=64)


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def jacobi3(a00, a01, a02, a11, a12, a22):
    """csrc/f3d_eigen.h jacobi3 -> (w [3], V [3][3] with the eigenvectors as columns)."""
    A = [[a00, a01, a02], [a01, a11, a12], [a02, a12, a22]]
    Q = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    for _ in range(16):
        off = abs(A[0][1]) + abs(A[0][2]) + abs(A[1][2])
        diag = abs(A[0][0]) + abs(A[1][1]) + abs(A[2][2])
        if not (off > 1e-300) or off <= 1e-18 * diag:
            break
        for k in range(3):
            p, q = (1 if k == 2 else 0), (1 if k == 0 else 2)
            apq = A[p][q]
            if abs(apq) <= 1e-300:
                continue
            theta = (A[q][q] - A[p][p]) / (2.0 * apq)
            t = (1.0 if theta >= 0.0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
            c = 1.0 / math.sqrt(t * t + 1.0)
            s = t * c
            app, aqq = A[p][p], A[q][q]
            A[p][p] = app - t * apq
            A[q][q] = aqq + t * apq
            A[p][q] = A[q][p] = 0.0
            r = 3 - p - q
            arp, arq = A[r][p], A[r][q]
            A[r][p] = A[p][r] = c * arp - s * arq
            A[r][q] = A[q][r] = s * arp + c * arq
            for i in range(3):
                vip, viq = Q[i][p], Q[i][q]
                Q[i][p] = c * vip - s * viq
                Q[i][q] = s * vip + c * viq
    return [A[0][0], A[1][1], A[2][2]], Q


def eig_order(w):
    """(k0, k1, k2): the smallest (ties: lowest index), the largest of the other two (ties: lowest index), the third."""
    k0 = 0
    if w[1] < w[k0]:
        k0 = 1
    if w[2] < w[k0]:
        k0 = 2
    a, b = (1 if k0 == 0 else 0), (1 if k0 == 2 else 2)
    k2 = b if w[b] > w[a] else a
    return k0, 3 - k0 - k2, k2


def sign_largest(v):
    a = 0
    if abs(v[1]) > abs(v[a]):
        a = 1
    if abs(v[2]) > abs(v[a]):
        a = 2
    return -v if v[a] < 0.0 else v


def wave_sum(x):
    """Lane l adds the items l, l + 64, ... left to right from 0.0; the 64 lanes meet in an xor butterfly 32, 16, .., 1."""
    x = np.asarray(x, np.float64)
    rows = -(-len(x) // 64)
    pad = np.zeros(rows * 64)
    pad[:len(x)] = x
    live = (np.arange(rows * 64) < len(x)).reshape(rows, 64)
    pad = pad.reshape(rows, 64)
    acc = np.zeros(64)
    for r in range(rows):
        acc = np.where(live[r], acc + pad[r], acc)
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[lane ^ off]
    return float(acc[0])


def shaped_sum(x):
    """The fixed-shape sum of the contract: chunks of 4096 items, each a wave_sum; the chunk sums summed the same way."""
    return wave_sum([wave_sum(x[k:k + 4096]) for k in range(0, len(x), 4096)])


class _Margin:
    def __init__(self):
        self.value = math.inf

    def see(self, values, threshold):
        values = np.asarray(values, np.float64).reshape(-1)
        values = values[np.isfinite(values)]
        if len(values):
            scale = abs(threshold) if threshold != 0 else 1.0
            self.value = min(self.value, float(np.min(np.abs(values - threshold))) / scale)


def _pca(p, offsets, neighbours, max_variation, margin):
    """Step 1 without normals -> (core bool [n], normals [n, 3])."""
    n = len(p)
    core, nrm = np.zeros(n, bool), np.zeros((n, 3))
    for i in range(n):
        row = neighbours[offsets[i]:offsets[i + 1]]
        seq = np.concatenate([[i], row[row != i]]).astype(np.int64)
        if len(seq) < 3:
            continue
        q = p[seq]
        s = q[0].copy()
        for k in range(1, len(seq)):
            s = s + q[k]
        d = q - s / float(len(seq))
        prod = np.stack([d[:, 0] * d[:, 0], d[:, 0] * d[:, 1], d[:, 0] * d[:, 2], d[:, 1] * d[:, 1], d[:, 1] * d[:, 2], d[:, 2] * d[:, 2]], axis=1)
        a = prod[0].copy()
        for k in range(1, len(seq)):
            a = a + prod[k]
        w, V = jacobi3(*[float(x) for x in a])
        k0, k1, k2 = eig_order(w)
        tr = (w[k0] + w[k1]) + w[k2]
        nrm[i] = [V[0][k0], V[1][k0], V[2][k0]]
        if tr > 0.0:
            margin.see(w[k0] / tr, max_variation)
            core[i] = w[k0] / tr <= max_variation
    return core, nrm


def extract(points, offsets, neighbours, normals=None, angle=10.0, offset=0.01, dist=0.01, max_variation=0.01, min_points=50, max_rounds=64,
            max_planes=None):
    """-> Result.  max_planes defaults to n // min_points (what the Python layer passes)."""
    p = np.asarray(points).astype(np.float64)
    n = len(p)
    offsets, neighbours = np.asarray(offsets, np.int64), np.asarray(neighbours, np.int64)
    cos_angle = math.cos(math.radians(float(angle)))
    max_planes = n // min_points if max_planes is None else max_planes
    margin = _Margin()
    rows = np.repeat(np.arange(n), np.diff(offsets))
    # 1 core
    if normals is not None:
        nrm = np.asarray(normals, np.float64)
        others = np.bincount(rows[neighbours != rows], minlength=n) if n else np.zeros(0, np.int64)
        core = np.isfinite(nrm).all(axis=1) & (others >= 2)
    else:
        core, nrm = _pca(p, offsets, neighbours, max_variation, margin)
    # 2 smooth edges between core points
    e = core[rows] & core[neighbours] & (rows < neighbours)
    i, j = rows[e], neighbours[e]
    with np.errstate(invalid='ignore'):
        cosv = np.abs(dot3(nrm[i], nrm[j]))
        margin.see(cosv, cos_angle)
        near = cosv >= cos_angle
        i, j = i[near], j[near]
        d = p[j] - p[i]
        off = np.maximum(np.abs(dot3(d, nrm[i])), np.abs(dot3(d, nrm[j])))
        margin.see(off, offset)
        hold = off <= offset
    graph = coo_matrix((np.ones(int(hold.sum()), np.int8), (i[hold], j[hold])), shape=(n, n))
    _, comp = connected_components(graph, directed=False)
    # 3 planes: components with at least min_points core members, numbered by ascending root (= lowest index)
    labels = np.full(n, -1, np.int32)
    members = {}
    for idx in np.flatnonzero(core):
        members.setdefault(comp[idx], []).append(idx)
    qualifying = sorted((m for m in members.values() if len(m) >= min_points), key=lambda m: m[0])
    P = min(len(qualifying), max_planes)
    cen, nP, uP, vP, lam = np.zeros((P, 3)), np.zeros((P, 3)), np.zeros((P, 3)), np.zeros((P, 3)), np.zeros((P, 3))
    for k in range(P):
        m = np.array(qualifying[k])
        labels[m] = k
        q = p[m]
        cen[k] = [shaped_sum(q[:, a]) / float(len(m)) for a in range(3)]
        d = q - cen[k]
        pairs = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
        w, V = jacobi3(*[shaped_sum(d[:, a] * d[:, b]) for a, b in pairs])
        k0, k1, k2 = eig_order(w)
        lam[k] = [w[k0], w[k1], w[k2]]
        nv, u = np.array([V[0][k0], V[1][k0], V[2][k0]]), np.array([V[0][k2], V[1][k2], V[2][k2]])
        if normals is not None:
            if dot3(nv, nrm[m[0]]) < 0.0:
                nv = -nv
        else:
            nv = sign_largest(nv)
        nP[k], uP[k] = nv, sign_largest(u)
        vP[k] = [nv[1] * uP[k][2] - nv[2] * uP[k][1], nv[2] * uP[k][0] - nv[0] * uP[k][2], nv[0] * uP[k][1] - nv[1] * uP[k][0]]

    def pdist(idx, k):
        return np.abs(dot3(p[idx] - cen[k], nP[k]))
    # 4 inliers
    for k in range(P):
        m = np.flatnonzero(labels == k)
        r = pdist(m, k)
        margin.see(r, dist)
        labels[m[r > dist]] = -1
    # 5 attach: synchronous rounds
    rounds = 0
    while rounds < max_rounds:
        rounds += 1
        nxt = labels.copy()
        for idx in np.flatnonzero(labels < 0):
            held = labels[neighbours[offsets[idx]:offsets[idx + 1]]]
            for k in np.unique(held[held >= 0]):                 # ascending: the lowest plane that accepts the point
                r = float(pdist(idx, k))
                margin.see(r, dist)
                if r <= dist:
                    nxt[idx] = k
                    break
        changed = not np.array_equal(nxt, labels)
        labels = nxt
        if not changed:
            break
    # 6 quads, plane rows
    planes, corners = np.zeros((P, 8)), np.zeros((P, 4, 3))
    for k in range(P):
        m = np.flatnonzero(labels == k)
        d = p[m] - cen[k]
        a, b = dot3(d, uP[k]), dot3(d, vP[k])
        res = dot3(d, nP[k])
        planes[k, 0:3], planes[k, 3], planes[k, 4:7] = nP[k], -dot3(nP[k], cen[k]), cen[k]
        planes[k, 7] = math.sqrt(shaped_sum(res * res) / float(len(m))) if len(m) else math.nan
        if len(m):
            for c, (ca, cb) in enumerate([(a.min(), b.min()), (a.max(), b.min()), (a.max(), b.max()), (a.min(), b.max())]):
                corners[k, c] = (cen[k] + ca * uP[k]) + cb * vP[k]
        else:
            corners[k] = math.nan
    counts = np.array([P, len(qualifying), rounds, int((labels >= 0).sum())], np.int64)
    return Result(labels, planes, corners, counts, nrm, margin.value, uP, vP, lam, core, [np.array(m) for m in qualifying[:P]])


# ------------------------------------------------------------------------------------------------ graphs and scenes
def radius_csr(points, radius):
    """Symmetric CSR adjacency without duplicate entries (rows ascending, the point itself included): (offsets int64, neighbours int32)."""
    p = np.asarray(points, np.float64)
    rows = cKDTree(p).query_ball_point(p, radius, return_sorted=True) if len(p) else []
    offsets = np.zeros(len(p) + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=offsets[1:])
    flat = np.concatenate([np.asarray(r, np.int32) for r in rows]).astype(np.int32) if len(p) else np.zeros(0, np.int32)
    return offsets, flat


def sheet(nx, ny, spacing, origin, ax_u, ax_v):
    """nx x ny grid points origin + i spacing ax_u + j spacing ax_v, and their unit normal ax_u x ax_v repeated."""
    ax_u, ax_v = np.asarray(ax_u, np.float64), np.asarray(ax_v, np.float64)
    i, j = np.meshgrid(np.arange(nx, dtype=np.float64), np.arange(ny, dtype=np.float64), indexing='ij')
    pts = np.asarray(origin, np.float64) + spacing * (i.reshape(-1, 1) * ax_u + j.reshape(-1, 1) * ax_v)
    nrm = np.cross(ax_u, ax_v)
    return pts, np.tile(nrm / np.linalg.norm(nrm), (len(pts), 1))


def noisy(pts, nrm, rng, sigma_p=0.001, sigma_n=0.02, shuffle=True):
    """Position noise, renormalised noisy normals, one shuffle for both -> (points, normals, the permutation applied)."""
    pts = pts + sigma_p * rng.standard_normal(pts.shape)
    nrm = nrm + sigma_n * rng.standard_normal(nrm.shape)
    nrm = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
    perm = rng.permutation(len(pts)) if shuffle else np.arange(len(pts))
    return np.ascontiguousarray(pts[perm]), np.ascontiguousarray(nrm[perm]), perm


# sheets whose single plane has a member count at the edge of a chunk of the plane sums (4096 members); the noise seed is one under
# which `extract` reports a margin >= 1e-6 (tests/test_planes_cpu.py asserts it)
EDGE_SHEETS = {'sheet4095': (5, 819, 4095), 'sheet4096': (64, 64, 4096), 'sheet4097': (17, 241, 4097)}


def edge_sheet(name):
    """-> (points, normals) of the named sheet of EDGE_SHEETS: nx x ny points 2 cm apart in z = 0, noisy and shuffled."""
    nx, ny, seed = EDGE_SHEETS[name]
    pts, nrm, _ = noisy(*sheet(nx, ny, 0.02, (0, 0, 0), (1, 0, 0), (0, 1, 0)), np.random.default_rng(seed))
    return pts, nrm


def room_corner(rng):
    """Three orthogonal 0.6 m faces that meet in a corner (floor z = 0, walls x = 0 and y = 0) and a slab 3 cm above the floor's level
    behind the x = 0 wall, 2 cm spacing: 4 x 900 points -> (points, normals, face id: floor 0, wall x 1, wall y 2, slab 3).  Floor and
    slab points are neighbours at a 0.05 radius across the wall's foot: parallel normals, 3 cm out of each other's tangent plane."""
    X, Y, Z = np.eye(3)
    h = 0.01                                                     # the faces start half a cell off the edges they share
    parts = [sheet(30, 30, 0.02, (h, h, 0.0), X, Y), sheet(30, 30, 0.02, (0.0, h, h), Y, Z), sheet(30, 30, 0.02, (h, 0.0, h), Z, X),
             sheet(30, 30, 0.02, (h - 0.6, h, 0.03), X, Y)]
    pts = np.concatenate([a for a, _ in parts])
    nrm = np.concatenate([b for _, b in parts])
    face = np.repeat(np.arange(4), 900)
    pts, nrm, perm = noisy(pts, nrm, rng)
    return pts, nrm, face[perm]


def same_partition(a, b):
    """True when two label arrays describe the same partition (with the same unlabelled set)."""
    a, b = np.asarray(a), np.asarray(b)
    if not np.array_equal(a < 0, b < 0):
        return False
    pairs = np.unique(np.stack([a[a >= 0], b[a >= 0]], axis=1), axis=0)
    return len(pairs) == len(np.unique(pairs[:, 0])) == len(np.unique(pairs[:, 1]))
