"""NumPy / scipy restatement of the surface-normal contract of f3d.h (f3d_estimate_normals), the checker of the kernel.

Per point i, float64: the points j of the frame with d2 = (dx*dx + dy*dy) + dz*dz < radius**2 (strict), the max_nn smallest in
(d2, j) order; (0, 0, 1) when fewer than 3 are kept, when the kept points are bit-identical or when the covariance vanishes; else
the eigenvector of the smallest eigenvalue of Open3D's cumulant covariance E[p p^T] - E[p] E[p]^T; then the flip of
RTAB2Cache.surface_normal_estimation (ios_rtab.py:242-246), restated line for line in ``orient``.
"""
import numpy as np
from scipy.spatial import cKDTree


def neighbours(points, radius, max_nn):
    """-> list of int arrays: the kept neighbours of every point, in (d2, j) order."""
    p = np.ascontiguousarray(points, np.float64)
    r2 = radius * radius
    tree = cKDTree(p)
    out = []
    for i, cand in enumerate(tree.query_ball_point(p, radius * (1 + 1e-9) + 1e-300)):   # a superset; the exact test follows
        c = np.asarray(cand, np.int64)
        t = p[i] - p[c]
        d2 = (t[:, 0] * t[:, 0] + t[:, 1] * t[:, 1]) + t[:, 2] * t[:, 2]
        keep = d2 < r2
        c, d2 = c[keep], d2[keep]
        order = np.lexsort((c, d2))[:max_nn]
        out.append(c[order])
    return out


def covariance(q):
    """Open3D's cumulant form over the points q [m,3]."""
    m = float(len(q))
    mean = q.sum(axis=0) / m
    second = np.einsum('ij,ik->jk', q, q) / m
    return second - np.outer(mean, mean)


def normals(points, radius=0.05, max_nn=30):
    """-> (unoriented normals [N,3], eigen-gap lambda1 - lambda0 [N] (inf on degenerate rows), degenerate [N] bool, kept lists)."""
    p = np.ascontiguousarray(points, np.float64)
    nb = neighbours(p, radius, max_nn)
    out = np.zeros_like(p)
    out[:, 2] = 1.0
    gap = np.full(len(p), np.inf)
    degenerate = np.ones(len(p), bool)
    for i, idx in enumerate(nb):
        if len(idx) < 3:
            continue
        q = p[idx]
        if (q.view(np.uint64) == q[:1].view(np.uint64)).all():
            continue
        C = covariance(q)
        if not C.any():
            continue
        w, V = np.linalg.eigh(C)
        v = V[:, 0]
        out[i] = v / np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
        gap[i] = w[1] - w[0]
        degenerate[i] = False
    return out, gap, degenerate, nb


def orient(points, raw_normals, cam_centre):
    """ios_rtab.py:241-246 on given unit normals (the reference's own lines)."""
    points = np.asarray(points, np.float64)
    cam_centre = np.asarray(cam_centre, np.float64)
    org_surface_normals = np.array(raw_normals, np.float64, copy=True)
    direction = points - cam_centre[None, :]
    magnitude_direction = np.linalg.norm(direction, axis=-1)
    with np.errstate(invalid='ignore', divide='ignore'):
        direction = direction / magnitude_direction[:, None]
    dirs = np.einsum('ij, ij -> i', org_surface_normals, direction)
    with np.errstate(invalid='ignore'):
        flip = dirs > 0
    org_surface_normals[flip] = -org_surface_normals[flip]
    return org_surface_normals


def orient_dots(points, raw_normals, cam_centre):
    """The dot products the flip decides on (to find rows too close to 0 to compare)."""
    direction = np.asarray(points, np.float64) - np.asarray(cam_centre, np.float64)[None, :]
    with np.errstate(invalid='ignore', divide='ignore'):
        direction = direction / np.linalg.norm(direction, axis=-1)[:, None]
    return np.einsum('ij, ij -> i', np.asarray(raw_normals, np.float64), direction)


def surface_normal_estimation(points, cam_centre, radius=0.05, max_nn=30):
    return orient(points, normals(points, radius, max_nn)[0], cam_centre)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def angle(a, b):
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=1), np.abs(np.einsum('ij,ij->i', a, b)))


def check_against_oracle(pts, radius, max_nn, got):
    """The check of estimate_normals' unoriented output `got` (tests/test_normals_gpu.py, tests/test_launch_shape_gpu.py): degenerate rows
    are (0, 0, 1) bit for bit, rows with a clear eigen-gap lie within 1e-6 rad of the oracle's normal, every row has unit length.
    -> (rows excluded for a small gap, rows compared, degenerate rows)."""
    want, gap, degenerate, nb = normals(pts, radius, max_nn)
    scale = np.array([np.mean(np.einsum('ij,ij->i', pts[k], pts[k])) if len(k) else 0.0 for k in nb])
    ok = ~degenerate & (gap >= 1e-8 * scale)
    excluded = int((~degenerate & ~ok).sum())
    assert np.array_equal(bits(got[degenerate]), bits(np.tile([0.0, 0.0, 1.0], (int(degenerate.sum()), 1))))
    ang = angle(got[ok], want[ok])
    assert ang.max(initial=0.0) <= 1e-6, ang.max()
    assert np.abs(np.linalg.norm(got, axis=1) - 1.0).max() <= 1e-14
    return excluded, int(ok.sum()), int(degenerate.sum())
