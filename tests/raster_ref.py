"""Test-only NumPy restatement of the triangle z-buffer contract of include/f3d.h (f3d_render_mesh_lookups, f3d_vote_faces,
f3d_vote_visible_mesh), operation for operation in float64: the vertex projection is oracle.np_ref.project_uvz, a triangle's
candidate box is evaluated at once (every product and sum of the contract as one NumPy operation, so nothing is contracted), and the
depth keys are resolved with a minimum per cell instead of atomics.  The loop over the triangles is Python: keep the cases small."""
import numpy as np

import render_ref as R
from oracle import np_ref as O

FLT_MIN = R.FLT_MIN
EMPTY = R.EMPTY
XY_MAX = 2.0 ** 30


def _mesh(vertices, triangles):
    P = np.asarray(vertices, np.float64)                                        # float32 vertices are widened exactly
    T = np.asarray(triangles).astype(np.int64)
    if len(T) and (T.min() < 0 or T.max() >= len(P)):
        raise IndexError('a triangle vertex index is outside [0, nv)')
    return P, T


def view_keys(P, T, K, q, t, H, W, z_far=np.inf):
    """(zkey uint64 [H*W], straddling) of one view."""
    with np.errstate(all='ignore'):
        x, y, h2 = O.project_uvz(P, K, q, t) if len(P) else (np.zeros(0),) * 3
        iz = 1.0 / h2
        z32 = h2.astype(np.float32)
        ok = (z32 >= FLT_MIN) & (z32 < np.float32(np.inf)) & (np.abs(x) <= XY_MAX) & (np.abs(y) <= XY_MAX)
    zkey = np.full((H, W), EMPTY, np.uint64)
    straddling = 0
    for ti, (a, b, c) in enumerate(T.tolist()):
        nok = int(ok[a]) + int(ok[b]) + int(ok[c])
        if nok != 3:
            straddling += nok > 0
            continue
        if a == b or b == c or a == c:
            continue
        with np.errstate(all='ignore'):
            A = (x[b] - x[a]) * (y[c] - y[a]) - (y[b] - y[a]) * (x[c] - x[a])
        if not np.isfinite(A) or A == 0.0:
            continue
        u0 = max(int(np.floor(min(x[a], x[b], x[c]))) - 1, 0)
        u1 = min(int(np.floor(max(x[a], x[b], x[c]))) + 1, W - 1)
        v0 = max(int(np.floor(min(y[a], y[b], y[c]))) - 1, 0)
        v1 = min(int(np.floor(max(y[a], y[b], y[c]))) + 1, H - 1)
        if u0 > u1 or v0 > v1:
            continue
        sx = (np.arange(u0, u1 + 1).astype(np.float64) + 0.5)[None, :]
        sy = (np.arange(v0, v1 + 1).astype(np.float64) + 0.5)[:, None]

        def directed(i, j):
            lo, hi = min(i, j), max(i, j)
            e = (x[hi] - x[lo]) * (sy - y[lo]) - (y[hi] - y[lo]) * (sx - x[lo])
            e = e if i < j else -e
            return -e if A < 0 else e

        with np.errstate(all='ignore'):
            E01, E12, E20 = directed(a, b), directed(b, c), directed(c, a)
            covered = (E01 >= 0) & (E12 >= 0) & (E20 >= 0)
            s = (E12 + E20) + E01
            z = s / ((E12 * iz[a] + E20 * iz[b]) + E01 * iz[c])
            zf = z.astype(np.float32)
            frag = covered & (s > 0) & (zf >= FLT_MIN) & (zf < np.float32(np.inf)) & (z <= z_far)
        if not frag.any():
            continue
        key = (zf.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(ti)
        box = zkey[v0:v1 + 1, u0:u1 + 1]
        box[frag] = np.minimum(box[frag], key[frag])
    return zkey.reshape(-1), straddling


def lookups(vertices, triangles, K, wxyzs, translations, hw, max_depth=10):
    """depth float32 [V,H,W] (+inf = empty), uv2tri int32 [V,H*W] (-1 = empty), straddling int64 [V]."""
    H, W = hw
    P, T = _mesh(vertices, triangles)
    V = len(translations)
    depth, uv2tri, straddling = np.empty((V, H, W), np.float32), np.empty((V, H * W), np.int32), np.zeros(V, np.int64)
    for j in range(V):
        zkey, straddling[j] = view_keys(P, T, K, wxyzs[j], translations[j], H, W, max_depth)
        d, l = R.unpack(zkey)
        depth[j], uv2tri[j] = d.reshape(H, W), l
    return depth, uv2tri, straddling


def face_votes(uv2tri, masks, nt, ncols=134):
    """float64 [nt, ncols]: the reference's vote() loop over the lookups, one row per triangle (a pair counts once per view)."""
    votes = np.zeros((nt, ncols))
    for j in range(len(uv2tri)):
        O.vote_frame(votes, uv2tri[j], np.asarray(masks[j]).reshape(-1))
    return votes


def visible_votes(points, depth, K, wxyzs, translations, masks, max_depth=10, depth_tol=0.05, ncols=134):
    """float64 [N, ncols]: the samples of render_ref (those of f3d_vote_visible) tested against the mesh depth of their pixel, an
    empty cell counting as +inf."""
    masks = np.asarray(masks)
    V, H, W = masks.shape
    P = np.asarray(points, np.float64)
    ppts, pnrm = O.frustum_planes(K, W, H, wxyzs, translations, max_depth)
    votes = np.zeros((len(P), ncols))
    for j in range(V):
        idx, u, v, z32 = R.view_samples(P, K, wxyzs[j], translations[j], ppts[j], pnrm[j], H, W)
        zmin32 = depth[j][v, u]
        vis = z32.astype(np.float64) <= zmin32.astype(np.float64) + np.float64(depth_tol)
        lab = masks[j, v[vis], u[vis]].astype(np.int64)
        if (lab >= ncols).any():
            raise IndexError('the mask label of a visible sample exceeds nclasses')
        votes[idx[vis], lab] += 1
    return votes


# ---------------------------------------------------------------------------------------------------------------- scenes
IDENTITY = (np.array([[1.0, 0.0, 0.0, 0.0]]), np.zeros((1, 3)))               # one camera at the origin looking down +z


def grid_mesh(nx, ny, origin, eu, ev, jitter=0.0, seed=0, flip=False, shuffle=False):
    """(nx + 1) x (ny + 1) vertices origin + i * eu + j * ev, interior vertices moved IN the plane by up to jitter cells, two
    triangles per cell (alternating diagonals); flip reverses every winding, shuffle permutes the triangle order.
    -> vertices float64 [nv, 3], triangles int64 [2 nx ny, 3]"""
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(nx + 1.0), np.arange(ny + 1.0), indexing='ij')
    inner = ((i > 0) & (i < nx) & (j > 0) & (j < ny)).astype(np.float64)
    i = i + inner * rng.uniform(-jitter, jitter, i.shape)
    j = j + inner * rng.uniform(-jitter, jitter, j.shape)
    verts = np.asarray(origin, np.float64) + i.reshape(-1, 1) * np.asarray(eu, np.float64) + j.reshape(-1, 1) * np.asarray(ev, np.float64)
    vid = np.arange((nx + 1) * (ny + 1)).reshape(nx + 1, ny + 1)
    a, b, c, d = vid[:-1, :-1], vid[1:, :-1], vid[1:, 1:], vid[:-1, 1:]
    odd = ((np.arange(nx)[:, None] + np.arange(ny)[None, :]) & 1).astype(bool)
    t1 = np.where(odd[..., None], np.stack([a, b, d], -1), np.stack([a, b, c], -1))
    t2 = np.where(odd[..., None], np.stack([b, c, d], -1), np.stack([a, c, d], -1))
    tris = np.concatenate([t1.reshape(-1, 3), t2.reshape(-1, 3)]).astype(np.int64)
    if flip:
        tris = tris[:, ::-1].copy()
    if shuffle:
        tris = tris[rng.permutation(len(tris))]
    return verts, tris


def plane_depth(K, H, W, origin, eu, ev, nx, ny, margin=1e-6):
    """For the identity camera and the plane of grid_mesh: (analytic camera depth float64 [H, W] of the pixel centres' rays, bool
    [H, W] whether the ray hits the grid's rectangle at least `margin` cells inside its border)."""
    origin, eu, ev = (np.asarray(a, np.float64) for a in (origin, eu, ev))
    n = np.cross(eu, ev)
    sx, sy = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    d = np.stack([(sx - K[0, 2]) / K[0, 0], (sy - K[1, 2]) / K[1, 1], np.ones_like(sx)], -1)
    with np.errstate(all='ignore'):
        z = (n @ origin) / (d @ n)
    hit = d * z[..., None] - origin
    M = np.stack([eu, ev], 1)
    ij = hit @ M @ np.linalg.inv(M.T @ M)
    inside = (z > 0) & (ij[..., 0] > margin) & (ij[..., 0] < nx - margin) & (ij[..., 1] > margin) & (ij[..., 1] < ny - margin)
    return z, inside


def lowest_touching(px, tris, H, W):
    """int [H, W]: the lowest index among the triangles whose CLOSED projection px[tri] (pixel coordinates, small dyadic numbers:
    the cross products are exact) holds the pixel's centre, -1 for none."""
    sx, sy = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    out = np.full((H, W), -1)
    for k in range(len(tris) - 1, -1, -1):
        p = px[tris[k]]
        e = [(p[(m + 1) % 3, 0] - p[m, 0]) * (sy - p[m, 1]) - (p[(m + 1) % 3, 1] - p[m, 1]) * (sx - p[m, 0]) for m in range(3)]
        inside = ((e[0] >= 0) & (e[1] >= 0) & (e[2] >= 0)) | ((e[0] <= 0) & (e[1] <= 0) & (e[2] <= 0))
        out[inside] = k
    return out


def scene_mesh(nt, seed):
    """nt triangles in the synth box (float32 values, so float32 and float64 storage agree): a soup of ~0.5 m triangles around
    synth.cloud centres -- under the ring cameras some are behind a camera, some cross its plane, most are a few pixels or less --
    and, from 257 triangles on, a jittered 8 x 8 grid mesh (shared edges) in place of the last 128."""
    from f3d import synth
    rng = np.random.default_rng(seed)
    c = synth.cloud(nt, seed=seed)
    verts = c[:, None, :] + rng.uniform(-0.4, 0.4, (nt, 3, 3))
    tris = np.stack([rng.permutation(3) + 3 * k for k in range(nt)]).astype(np.int64).reshape(nt, 3)
    verts = verts.reshape(-1, 3)
    if nt >= 257:
        gv, gt = grid_mesh(8, 8, [-1.0, -1.2, 0.6], [0.25, 0.0, 0.05], [0.0, 0.3, 0.1], jitter=0.3, seed=seed, shuffle=True)
        tris = np.concatenate([tris[:nt - 128], gt + len(verts)])
        verts = np.concatenate([verts, gv])
    return verts.astype(np.float32).astype(np.float64), tris


def dropped_scene():
    """Input that must reach no output, around ONE good triangle (the last): a repeated index (twice), a NaN, an infinite and a
    behind-the-camera corner next to good ones (3 straddling), a triangle wholly behind the camera, one wholly outside the image.
    -> vertices, triangles, K of an 8 x 8 image for the identity camera, index of the good triangle, straddling count"""
    verts = np.array([[-1.0, -1.0, 2.0], [1.0, -1.0, 2.0], [0.0, 1.0, 2.0],
                      [0.0, 0.0, -1.0], [0.5, 0.5, 2.0], [np.nan, 0.0, 2.0], [np.inf, 0.0, 2.0],
                      [-1.0, -1.0, -2.0], [1.0, -1.0, -2.0], [0.0, 1.0, -2.0],
                      [50.0, 50.0, 2.0], [51.0, 50.0, 2.0], [50.0, 51.0, 2.0]])
    tris = np.array([[0, 1, 1], [0, 4, 4], [0, 1, 5], [0, 1, 6], [7, 8, 9], [0, 1, 3], [10, 11, 12], [0, 1, 2]])
    return verts, tris, R.pinhole(8, 8, 4.0), 7, 3


def meshed_two_walls():
    """The two walls of render_ref.two_walls as grid meshes on its 2 cm grid (the cloud's points are the meshes' vertices)."""
    verts, tris, off = [], [], 0
    for xw in (1.0, 2.0):
        v, t = grid_mesh(50, 40, [xw, -0.5, -0.4], [0.0, 0.02, 0.0], [0.0, 0.0, 0.02])
        verts.append(v)
        tris.append(t + off)
        off += len(v)
    return np.concatenate(verts), np.concatenate(tris)
