"""Test-only NumPy restatement of the point-splat z-buffer contract of include/f3d.h (f3d_render_lookups, f3d_vote_visible), on top
of oracle.np_ref: the samples are those of O.forward_votes, the depth keys are resolved with a lexsort instead of atomics."""
import numpy as np

from f3d import synth
from oracle import np_ref as O

FLT_MIN = np.float32(np.finfo(np.float32).tiny)
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def view_samples(P, K, q, t, plane_pts, plane_nrm, H, W):
    """(index, u, v, z32) of the points that have a sample in this view."""
    idx = np.nonzero(O.point_inside_polyhedra(P, plane_pts, plane_nrm))[0]
    u, v = O.points2pixel(P[idx], K, q, t)
    with np.errstate(all='ignore'):
        z32 = O.project_uvz(P[idx], K, q, t)[2].astype(np.float32)
        ok = (u >= 0) & (u < W) & (v >= 0) & (v < H) & (z32 >= FLT_MIN) & (z32 < np.float32(np.inf))
    return idx[ok], u[ok].astype(np.int64), v[ok].astype(np.int64), z32[ok]


def view_keys(idx, u, v, z32, H, W, splat):
    """zkey uint64 [H*W] of one view: per cell the smallest (z32 bits, index) over the samples whose patch covers it."""
    zbits = z32.view(np.uint32).astype(np.uint64)
    cells, who = [], []
    for dv in range(-splat, splat + 1):
        for du in range(-splat, splat + 1):
            r, c = v + dv, u + du
            ok = (r >= 0) & (r < H) & (c >= 0) & (c < W)
            cells.append((r * W + c)[ok])
            who.append(np.nonzero(ok)[0])
    cells, who = np.concatenate(cells), np.concatenate(who)
    zkey = np.full(H * W, EMPTY, np.uint64)
    if len(cells):
        order = np.lexsort((idx[who], zbits[who], cells))
        cs, ws = cells[order], who[order]
        first = np.r_[True, cs[1:] != cs[:-1]]
        zkey[cs[first]] = (zbits[ws[first]] << np.uint64(32)) | idx[ws[first]].astype(np.uint64)
    return zkey


def unpack(zkey):
    """zkey -> (depth float32, uv2pt int32)."""
    empty = zkey == EMPTY
    depth = (zkey >> np.uint64(32)).astype(np.uint32).view(np.float32).copy()
    depth[empty] = np.inf
    uv2pt = (zkey & np.uint64(0xFFFFFFFF)).astype(np.uint32).astype(np.int64).astype(np.int32)
    uv2pt[empty] = -1
    return depth, uv2pt


def _views(points, K, wxyzs, translations, H, W, max_depth, splat):
    P = np.asarray(points, np.float64)                                          # float32 clouds are widened exactly
    ppts, pnrm = O.frustum_planes(K, W, H, wxyzs, translations, max_depth)
    for j in range(len(translations)):
        s = view_samples(P, K, wxyzs[j], translations[j], ppts[j], pnrm[j], H, W)
        yield j, s, view_keys(*s, H, W, splat)


def lookups(points, K, wxyzs, translations, hw, max_depth=10, splat=0):
    """depth float32 [V,H,W] (+inf = empty) and uv2pt int32 [V,H*W] (-1 = empty)."""
    H, W = hw
    V = len(translations)
    depth, uv2pt = np.empty((V, H, W), np.float32), np.empty((V, H * W), np.int32)
    for j, _, zkey in _views(points, K, wxyzs, translations, H, W, max_depth, splat):
        d, l = unpack(zkey)
        depth[j], uv2pt[j] = d.reshape(H, W), l
    return depth, uv2pt


def visible_votes(points, K, wxyzs, translations, masks, max_depth=10, splat=1, depth_tol=0.05, ncols=134):
    """float64 [N, ncols]: votes[i, masks[j, v, u]] += 1 for every sample within depth_tol of the front surface of its pixel."""
    masks = np.asarray(masks)
    V, H, W = masks.shape
    votes = np.zeros((len(points), ncols))
    for j, (idx, u, v, z32), zkey in _views(points, K, wxyzs, translations, H, W, max_depth, splat):
        zmin32 = unpack(zkey)[0][v * W + u]
        vis = z32.astype(np.float64) <= zmin32.astype(np.float64) + np.float64(depth_tol)
        lab = masks[j, v[vis], u[vis]].astype(np.int64)
        if (lab >= ncols).any():
            raise IndexError('the mask label of a visible sample exceeds nclasses')
        votes[idx[vis], lab] += 1                                               # the indices are unique per view
    return votes


def pinhole(H, W, focal=None):
    f = 0.8 * W if focal is None else focal
    return np.array([[f, 0.0, W / 2.0], [0.0, f, H / 2.0], [0.0, 0.0, 1.0]])


def two_walls():
    """A wall at x = 1 and one at x = 2 (2 cm grid); 3 cameras at x = -1 facing +x see label 86 everywhere, 3 at x = 4 facing -x see 114.
    From either side the far wall lies inside the silhouette of the near one, 1 m behind it.
    -> points, is_far_wall (x == 2), K, wxyzs, translations, masks, (H, W)"""
    y, z = np.meshgrid(np.arange(-0.5, 0.5001, 0.02), np.arange(-0.4, 0.4001, 0.02))
    wall = np.stack([np.zeros(y.size), y.reshape(-1), z.reshape(-1)], axis=1)
    points = np.concatenate([wall + [1.0, 0, 0], wall + [2.0, 0, 0]])
    H, W = 96, 128
    eyes = np.array([[-1.0, dy, 0.0] for dy in (-0.2, 0.0, 0.2)] + [[4.0, dy, 0.0] for dy in (-0.2, 0.0, 0.2)])
    quats = np.stack([synth._look_at_quat(e, e + [1.0 if e[0] < 1 else -1.0, 0.0, 0.0]) for e in eyes])
    masks = np.empty((6, H, W), np.uint8)
    masks[:3], masks[3:] = 86, 114
    return points, points[:, 0] == 2.0, pinhole(H, W, 60.0), quats, eyes, masks, (H, W)
