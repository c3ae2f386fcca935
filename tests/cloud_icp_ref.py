"""NumPy restatement of the cloud-to-cloud ICP contract of include/f3d.h (f3d_cloud_icp_sums, f3d_cloud_icp), operation for operation:
float64 arithmetic, every product and sum as the header writes it.  The nearest target is found by brute force (knn_ref.dist2 and the
(d2, index) rule); the sums have the chunk, lane and butterfly shape of icp_ref; the solve and the update are icp_ref's.  No grid, no
launch shape: what the library returns must equal this bit for bit.
"""
import numpy as np

from oracle import np_ref as O
import icp_ref as I
import knn_ref as K

PLANE, POINT = 0, 1
CHUNK, NSUMS = I.CHUNK, I.NSUMS
ROWS_PER_STEP = 2_000_000


def nearest(p, target, max_dist):
    """int32 [n]: per row of p the target index smallest under (d2, index) among those with d2 <= max_dist * max_dist, or -1."""
    target = np.asarray(target)
    out = np.full(len(p), -1, np.int32)
    step = max(1, ROWS_PER_STEP // max(len(target), 1))
    with np.errstate(all='ignore'):
        for a in range(0, len(p), step):
            d2 = K.dist2(p[a:a + step], target)
            ok = d2 <= max_dist * max_dist
            j = np.argmin(np.where(ok, d2, np.inf), axis=1)                # the first of equal minima: the lower index
            out[a:a + step] = np.where(ok.any(axis=1), j, -1)
    return out


def _rows(J, r, count):
    return np.stack([J[a] * J[b] for a in range(6) for b in range(a, 6)] + [J[a] * r for a in range(6)] + [r * r, count], axis=1)


def terms(source, target, normals, mode, q, t, max_dist):
    """-> (list of term arrays [n, 29], pairs int32 [n]).  PLANE: one array, the 29 terms of every pair.  POINT: three, one per unit
    axis a = 0, 1, 2, which a lane adds to its accumulators in that order for each of its points; the count's 1.0 sits in the first.
    Rows are 0.0 where a step of the header fails."""
    s, g = np.asarray(source, np.float64), np.asarray(target, np.float64)
    n = len(s)
    with np.errstate(all='ignore'):
        pr = O.rotate(I.normalise(q), s) if n else np.zeros((0, 3))
        p = pr + np.asarray(t, np.float64)[None, :]
        pairs = nearest(p, g, max_dist)
        ok = pairs >= 0
        e = p - g[np.where(ok, pairs, 0)]
        ones = np.ones(n)
        if mode == PLANE:
            N = np.asarray(normals, np.float64)[np.where(ok, pairs, 0)]
            ok = ok & np.isfinite(N).all(axis=1)
            N = np.where(ok[:, None], N, 0.0)
            r = I.dot3(N, e)
            J = [pr[:, 1] * N[:, 2] - pr[:, 2] * N[:, 1], pr[:, 2] * N[:, 0] - pr[:, 0] * N[:, 2], pr[:, 0] * N[:, 1] - pr[:, 1] * N[:, 0],
                 N[:, 0], N[:, 1], N[:, 2]]
            return [np.where(ok[:, None], _rows(J, r, ones), 0.0)], pairs
        out = []
        for a in range(3):
            N = np.zeros((n, 3))
            N[:, a] = 1.0
            r = e[:, a]
            J = [pr[:, 1] * N[:, 2] - pr[:, 2] * N[:, 1], pr[:, 2] * N[:, 0] - pr[:, 0] * N[:, 2], pr[:, 0] * N[:, 1] - pr[:, 1] * N[:, 0],
                 N[:, 0], N[:, 1], N[:, 2]]
            out.append(np.where(ok[:, None], _rows(J, r, ones if a == 0 else np.zeros(n)), 0.0))
        return out, pairs


def shaped_sums(rows):
    """The 29 totals of `rows` (a list of arrays [n, 29]): chunks of CHUNK source points; in a chunk lane l of 64 takes the points
    l, l + 64, .. in turn and adds each point's rows, one array after the other, from 0.0; the butterfly and the sum of the chunk sums
    are icp_ref.wave_sum's.  With one array this is icp_ref.shaped_sums."""
    n = len(rows[0])
    if n == 0:
        return np.zeros(NSUMS)
    if len(rows) == 1:
        return I.shaped_sums(rows[0])
    lane = np.arange(64)
    chunk_sums = []
    for k in range(0, n, CHUNK):
        acc = np.zeros((64, NSUMS))
        for g in range(k, min(k + CHUNK, n), 64):
            for x in rows:
                part = x[g:min(g + 64, k + CHUNK)]
                acc[:len(part)] = acc[:len(part)] + part
        for off in (32, 16, 8, 4, 2, 1):
            acc = acc + acc[lane ^ off]
        chunk_sums.append(acc[0])
    return I.wave_sum(np.stack(chunk_sums))


def cloud_icp_sums(source, target, normals, mode, q, t, max_dist):
    """-> (sums float64 [29], pairs int32 [n]) of the header's f3d_cloud_icp_sums."""
    rows, pairs = terms(source, target, normals, mode, q, t, max_dist)
    return shaped_sums(rows), pairs


def cloud_icp(source, target, normals, mode, q, t, max_dist, iterations, min_pairs):
    """-> (pose float64 [7], stats float64 [iterations, 3], status) of the header's f3d_cloud_icp."""
    q, t = np.asarray(q, np.float64).copy(), np.asarray(t, np.float64).copy()
    stats, lost = np.zeros((iterations, 3)), False
    for it in range(iterations):
        if lost:
            stats[it] = (0.0, 0.0, I.LOST)
            continue
        tot, _ = cloud_icp_sums(source, target, normals, mode, q, t, max_dist)
        x = I.solve(tot, min_pairs)
        stats[it] = (tot[28], tot[27], I.OK if x is not None else I.LOST)
        if x is None:
            lost = True
            continue
        q, t = I.update(q, t, x)
    return np.concatenate([q, t]), stats, I.LOST if lost else I.OK


# ------------------------------------------------------------------------------------------------ scenes of the tests
def corner_scene(m=1200, n=700, seed=11, degrees=2.0, shift=0.03):
    """A room corner: three orthogonal 2 m x 2 m planes (x = -1, y = -1, z = -1) and a 0.5 m square patch raised 0.25 m above the
    floor, m float32-representable target points with their normals.  The source is n of them taken through the inverse of a known
    pose (`degrees` about a skew axis, `shift` metres), in float64: at the true pose every source point coincides with its target
    point up to the rounding of building it.  -> dict(target float64 [m, 3], normals [m, 3], source float64 [n, 3], picked int [n],
    q_true, t_true)."""
    rng = np.random.default_rng(seed)
    per = (m - m // 8) // 3
    parts, normals = [], []
    for axis in range(3):
        uv = rng.uniform(-1.0, 1.0, size=(per if axis else m - m // 8 - 2 * per, 2))
        pts = np.insert(uv, axis, -1.0, axis=1)
        parts.append(pts)
        normals.append(np.tile(np.eye(3)[axis], (len(pts), 1)))
    uv = rng.uniform(0.0, 0.5, size=(m // 8, 2))
    parts.append(np.stack([uv[:, 0], uv[:, 1], np.full(len(uv), -0.75)], axis=1))
    normals.append(np.tile(np.eye(3)[2], (len(uv), 1)))
    target = np.concatenate(parts).astype(np.float32).astype(np.float64)
    normals = np.concatenate(normals)
    order = rng.permutation(m)
    target, normals = target[order], normals[order]
    axis = np.array([0.4, -0.7, 0.59])
    q_true, t_true = I.moved([1.0, 0.0, 0.0, 0.0], np.zeros(3), axis, degrees, np.zeros(3))
    t_true = np.array([0.6, -0.5, 0.62]) * (shift / np.linalg.norm([0.6, -0.5, 0.62]))
    picked = np.sort(rng.permutation(m)[:n])
    q_inv = I.normalise(q_true) * np.array([1.0, -1.0, -1.0, -1.0])
    source = O.rotate(q_inv, target[picked] - t_true[None, :])
    return dict(target=target, normals=normals, source=source, picked=picked, q_true=I.normalise(q_true), t_true=t_true)


def pose_error(pose, q_true, t_true):
    """(metres, radians) between a pose [7] and the true one."""
    return float(np.linalg.norm(pose[4:] - t_true)), I.rotation_angle(pose[:4], q_true)


def cloud_pair(n, m=900, seed=3, sdtype=np.float64, tdtype=np.float64):
    """A bumpy sheet of m target points with unit normals (some far from any axis) and n source points near it, moved by a small pose:
    the inputs of the bit-for-bit cases.  -> (source [n, 3] of sdtype, target [m, 3] of tdtype, normals float64 [m, 3], q, t)."""
    rng = np.random.default_rng(seed)
    uv = rng.uniform(-1.0, 1.0, size=(m, 2))
    z = 0.2 * np.sin(2.0 * uv[:, 0]) * np.cos(1.5 * uv[:, 1])
    target = np.stack([uv[:, 0], uv[:, 1], z], axis=1).astype(np.float32)
    gx, gy = 0.4 * np.cos(2.0 * uv[:, 0]) * np.cos(1.5 * uv[:, 1]), -0.3 * np.sin(2.0 * uv[:, 0]) * np.sin(1.5 * uv[:, 1])
    normals = np.stack([-gx, -gy, np.ones(m)], axis=1)
    normals /= np.linalg.norm(normals, axis=1)[:, None]
    src = target[rng.integers(0, m, size=n)].astype(np.float64) + rng.normal(scale=0.02, size=(n, 3))
    q, t = I.moved([1.0, 0.0, 0.0, 0.0], np.zeros(3), (0.3, 0.5, -0.8), 1.5, np.array([0.012, -0.02, 0.015]))
    source = src.astype(np.float32)
    return source.astype(sdtype), target.astype(tdtype), normals, q, t
