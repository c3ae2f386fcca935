"""Test-only restatement of f3d_smooth_votes / f3d_smooth_segment (include/f3d.h), NumPy, operation for operation, and the two scenes
their tests share.

One iteration: the others of point i are the entries j != i of its row, in row order; such a j contributes iff every gate that was
given holds (normals: |(a0*b0 + a1*b1) + a2*b2| >= cos_angle; colours: (dr*dr + dg*dg) + db*db <= limit*limit, float32 colours
widened first); a NaN makes a comparison false.  Per column the sum starts from self_weight * v[i] and adds the contributing rows one
after the other in row order: NumPy's elementwise float64 operations round exactly like the kernel's, one operation at a time.
Iteration t + 1 reads the whole output of iteration t.  smooth_segment is the oracle's segment (lastcol: point_voting_ref's) on that
matrix; for integer votes every order of the row total gives the same bits.
"""
import numpy as np

from oracle.np_ref import segment as segment_rows
from point_voting_ref import segment as segment_rows_lastcol


def smooth_once(v, offs, nbrs, normals=None, cos_angle=0.0, colors=None, max_color_dist=0.0, self_weight=1.0):
    v = np.asarray(v, np.float64)
    n = len(v)
    nbrs = np.asarray(nbrs, np.int64)
    col = None if colors is None else np.asarray(colors).astype(np.float64)
    limit2 = np.float64(max_color_dist) * np.float64(max_color_dist)
    out = np.empty_like(v)
    with np.errstate(all='ignore'):
        for i in range(n):
            row = nbrs[offs[i]:offs[i + 1]]
            keep = row != i
            if normals is not None:
                a, b = normals[i], normals[row]
                keep &= np.abs((a[0] * b[:, 0] + a[1] * b[:, 1]) + a[2] * b[:, 2]) >= cos_angle
            if col is not None:
                d = col[row] - col[i]
                keep &= (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2] <= limit2
            acc = np.float64(self_weight) * v[i]
            for j in row[keep]:
                acc = acc + v[j]
            out[i] = acc
    return out


def smooth(votes, offs, nbrs, normals=None, cos_angle=0.0, colors=None, max_color_dist=0.0, self_weight=1.0, iterations=1):
    """f3d_smooth_votes -> float64 [n, ncols].  A neighbour outside [0, n) raises IndexError before anything is computed."""
    v = np.asarray(votes).astype(np.float64)                                   # uint16 widens exactly
    nb = np.asarray(nbrs, np.int64)
    if ((nb < 0) | (nb >= len(v))).any():
        raise IndexError('neighbour index outside [0, n)')
    for _ in range(iterations):
        v = smooth_once(v, offs, nb, normals, cos_angle, colors, max_color_dist, self_weight)
    return v


def smooth_segment(votes, offs, nbrs, nclasses, threshold=0.5, filter_classes=None, lastcol=False, **kw):
    m = smooth(votes, offs, nbrs, **kw)
    return (segment_rows_lastcol if lastcol else segment_rows)(m, nclasses, threshold, filter_classes)


# ------------------------------------------------------------------------------------------------ graphs and scenes
def radius_csr(pts, r):
    """Brute-force radius graph: row i lists every j (i included) with squared distance <= r*r, ascending."""
    pts = np.asarray(pts, np.float64)
    d = pts[:, None, :] - pts[None, :, :]
    near = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2] <= r * r
    offs = np.zeros(len(pts) + 1, np.int64)
    np.cumsum(near.sum(1), out=offs[1:])
    return offs, np.nonzero(near)[1].astype(np.int32)


SHEET_R = 0.05                  # the sheet's graph radius
SHEET_EDGE = 0.59               # the two classes meet at x = SHEET_EDGE
SHEET_CLASSES = (1, 2)          # left, right; nclasses = 4, so column 4 is "unclassified"
NCLASSES = 4


def noisy_sheet(seed=0):
    """A 60 x 40 sheet at 2 cm with 1 mm jitter, rows shuffled; class 1 left of x = 0.59 m, class 2 right of it.  A clean row holds 8
    votes for its class; in 15 % of the rows the other class leads 5 : 3; 5 % of the rows are empty.
    -> (points [2400, 3], votes float64 [2400, 5], truth int64 [2400])."""
    rng = np.random.default_rng(seed)
    ix, iy = np.meshgrid(np.arange(60), np.arange(40), indexing='ij')
    pts = np.stack([ix * 0.02, iy * 0.02, np.zeros_like(ix, dtype=np.float64)], -1).reshape(-1, 3)
    pts = (pts + rng.uniform(-0.001, 0.001, pts.shape))[rng.permutation(len(pts))]
    left = pts[:, 0] < SHEET_EDGE
    truth = np.where(left, SHEET_CLASSES[0], SHEET_CLASSES[1]).astype(np.int64)
    other = np.where(left, SHEET_CLASSES[1], SHEET_CLASSES[0])
    u = rng.random(len(pts))
    votes = np.zeros((len(pts), NCLASSES + 1))
    rows = np.arange(len(pts))
    clean, wrong = u >= 0.20, (u >= 0.05) & (u < 0.20)
    votes[rows[clean], truth[clean]] = 8
    votes[rows[wrong], other[wrong]] = 5
    votes[rows[wrong], truth[wrong]] = 3
    return pts, votes, truth


def sheet_far(pts):
    """Points farther than the graph radius from the class boundary: no row there reaches across it."""
    return np.abs(pts[:, 0] - SHEET_EDGE) > SHEET_R


CORNER_CLASSES = (1, 2)         # floor, wall


def corner():
    """A floor (z = 0, normal +z, class 1) and a wall (x = 0, normal +x, class 2) meeting in an edge, 30 x 30 points each at 2 cm,
    clean votes of 8.  -> (points [1800, 3], normals [1800, 3], votes float64 [1800, 5], surface int64 [1800] (0 floor, 1 wall))."""
    a, b = np.meshgrid(np.arange(30) * 0.02 + 0.01, np.arange(30) * 0.02, indexing='ij')
    a, b = a.reshape(-1), b.reshape(-1)
    floor = np.stack([a, b, np.zeros_like(a)], -1)
    wall = np.stack([np.zeros_like(a), b, a], -1)
    pts = np.concatenate([floor, wall])
    surface = np.repeat([0, 1], len(a)).astype(np.int64)
    normals = np.where(surface[:, None] == 0, [0.0, 0.0, 1.0], [1.0, 0.0, 0.0])
    votes = np.zeros((len(pts), NCLASSES + 1))
    votes[np.arange(len(pts)), np.where(surface == 0, *CORNER_CLASSES)] = 8
    return pts, normals, votes, surface


def corner_leaks(smoothed, surface):
    """Rows that hold votes of the other surface's class."""
    other = np.where(surface == 0, CORNER_CLASSES[1], CORNER_CLASSES[0])
    return int((smoothed[np.arange(len(smoothed)), other] > 0).sum())
