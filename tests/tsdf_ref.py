"""NumPy restatement of the TSDF contract of include/f3d.h (f3d_tsdf_integrate, f3d_tsdf_extract_count -> _fill), operation for
operation: float64 arithmetic, every product, sum and division as the header writes it, float32 storage.  No culling, no scan, no
launch shape: what the library returns must equal this bit for bit.  Plus the analytic depth scenes the tests integrate
(per-pixel-centre ray casts of a sphere in front of a wall) and mesh checks.
"""
import numpy as np

from oracle import np_ref as O
from fusion_scenes import _pose, _quat_from_axes


# ------------------------------------------------------------------------------------------------ integrate
def voxel_centres(lo, dims, vs):
    """float64 [nx * ny * nz, 3] in linear order lin = (k * ny + j) * nx + i; c_a = lo[a] + ((double)idx_a + 0.5) * vs."""
    nx, ny, nz = dims
    k, j, i = np.meshgrid(np.arange(nz, dtype=np.float64), np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64), indexing='ij')
    lo = np.asarray(lo, np.float64)
    return np.stack([lo[a] + (idx.reshape(-1) + 0.5) * vs for a, idx in enumerate((i, j, k))], axis=1)


def integrate(tsdf, weight, lo, vs, trunc, max_weight, depths, K, wxyzs, translations, depth_scale=1.0, max_depth=10.0):
    """Returns the new (tsdf, weight), float32 [nz, ny, nx]; the inputs are left as they are."""
    nz, ny, nx = tsdf.shape
    K = np.asarray(K, np.float64)
    T, W = tsdf.reshape(-1).copy(), weight.reshape(-1).copy()
    c = voxel_centres(lo, (nx, ny, nz), vs)
    wmax = np.float64(np.float32(max_weight))
    depths = np.asarray(depths)
    F, h, w = depths.shape
    with np.errstate(all='ignore'):
        for f in range(F):
            t = np.asarray(translations[f], np.float64)
            cam = O.rotate(O.quat_inverse(wxyzs[f]), c - t[None, :])
            x, y, z = cam[:, 0], cam[:, 1], cam[:, 2]
            h0 = (K[0, 0] * x + K[0, 1] * y) + K[0, 2] * z
            h1 = (K[1, 0] * x + K[1, 1] * y) + K[1, 2] * z
            h2 = (K[2, 0] * x + K[2, 1] * y) + K[2, 2] * z
            ok = h2 > 0
            px, py = h0 / h2, h1 / h2
            ok &= (px >= 0) & (px < w) & (py >= 0) & (py < h)
            u = np.where(ok, np.floor(px), 0).astype(np.int64)
            v = np.where(ok, np.floor(py), 0).astype(np.int64)
            d = depths[f][v, u].astype(np.float64) / np.float64(depth_scale)
            ok &= (d > 0) & (d <= max_depth)
            sdf = d - h2
            ok &= ~(sdf < -trunc)
            val = sdf / np.float64(trunc)
            val = np.where(val > 1.0, 1.0, val)
            Wd = W.astype(np.float64)
            Tn = ((T.astype(np.float64) * Wd + val) / (Wd + 1.0)).astype(np.float32)
            Wn = np.minimum(Wd + 1.0, wmax).astype(np.float32)
            T, W = np.where(ok, Tn, T), np.where(ok, Wn, W)
    return T.reshape(nz, ny, nx), W.reshape(nz, ny, nx)


# ------------------------------------------------------------------------------------------------ extract
def extract(tsdf, weight, lo, vs, min_weight=1.0):
    """-> (verts float64 [nv, 3], tris int32 [nt, 3]) of the header's surface nets."""
    nz, ny, nx = tsdf.shape
    n = (nx, ny, nz)
    N = nx * ny * nz
    st = (1, nx, nx * ny)
    lo = np.asarray(lo, np.float64)
    S = tsdf.reshape(-1)
    obs = weight.reshape(-1) >= np.float32(min_weight)
    with np.errstate(invalid='ignore'):
        inside = obs & (S < 0)
    lin = np.arange(N, dtype=np.int64)
    P = (lin % nx, (lin // nx) % ny, lin // (nx * ny))
    # active cells
    is_cell = (P[0] <= nx - 2) & (P[1] <= ny - 2) & (P[2] <= nz - 2)
    cl = lin[is_cell]
    corners = [cl + (c & 1) * st[0] + ((c >> 1) & 1) * st[1] + (c >> 2) * st[2] for c in range(8)]
    all_obs = np.ones(len(cl), bool)
    nin = np.zeros(len(cl), np.int64)
    for at in corners:
        all_obs &= obs[at]
        nin += inside[at]
    active = np.zeros(N, bool)
    active[cl] = all_obs & (nin > 0) & (nin < 8)
    rank = np.cumsum(active) - 1
    # vertices
    al = lin[active]
    sums = [np.zeros(len(al)) for _ in range(3)]
    count = np.zeros(len(al), np.int64)
    with np.errstate(all='ignore'):
        for a in range(3):
            b, c = (a + 1) % 3, (a + 2) % 3
            for oc in (0, 1):
                for ob in (0, 1):                                       # e = 4 a + 2 oc + ob ascending
                    at0 = al + ob * st[b] + oc * st[c]
                    at1 = at0 + st[a]
                    cross = inside[at0] != inside[at1]
                    s0, s1 = S[at0].astype(np.float64), S[at1].astype(np.float64)
                    L = [None, None, None]
                    L[a], L[b], L[c] = s0 / (s0 - s1), np.float64(ob), np.float64(oc)
                    for k in range(3):
                        sums[k] = np.where(cross, sums[k] + L[k], sums[k])
                    count += cross
        verts = np.stack([lo[a] + ((P[a][active].astype(np.float64) + 0.5) + sums[a] / count.astype(np.float64)) * vs for a in range(3)], axis=1)
    # faces
    keys, quads = [], []
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        rng = (P[a] <= n[a] - 2) & (P[b] >= 1) & (P[b] <= n[b] - 2) & (P[c] >= 1) & (P[c] <= n[c] - 2)
        p = lin[rng]
        e1 = p + st[a]
        ok = obs[p] & obs[e1] & (inside[p] != inside[e1])
        A, B, C, D = p - st[b] - st[c], p - st[c], p, p - st[b]
        ok &= active[A] & active[B] & active[C] & active[D]
        p, A, B, C, D = p[ok], A[ok], B[ok], C[ok], D[ok]
        ins = inside[p]
        q = np.stack([rank[A], np.where(ins, rank[B], rank[D]), rank[C], np.where(ins, rank[D], rank[B])], axis=1)
        keys.append(3 * p + a)
        quads.append(q)
    keys, quads = np.concatenate(keys), np.concatenate(quads)
    quads = quads[np.argsort(keys, kind='stable')]
    tris = np.stack([quads[:, [0, 1, 2]], quads[:, [0, 2, 3]]], axis=1).reshape(-1, 3).astype(np.int32)
    return verts.reshape(-1, 3), tris


# ------------------------------------------------------------------------------------------------ analytic scenes
SPHERE_C, SPHERE_R = np.array([0.05, -0.02, 1.0]), 0.28
WALL_Z = 1.55                                                          # the wall is the plane z = WALL_Z, seen from z < WALL_Z


def look_at(eye, target, down=(0.0, 1.0, 0.0)):
    """(wxyz, translation) of a camera at `eye` looking at `target`."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    return _quat_from_axes(_pose(eye, target, np.asarray(down, np.float64))), eye


def intrinsics(h, w, focal=0.9):
    f = focal * w
    return np.array([[f, 0.0, w / 2.0], [0.0, f, h / 2.0], [0.0, 0.0, 1.0]])


def cast_depth(K, wxyz, t, h, w):
    """Camera-z depth float64 [h, w] of the sphere in front of the wall through every pixel centre (u + 0.5, v + 0.5); 0 = no hit."""
    uu, vv = np.meshgrid(np.arange(w) + 0.5, np.arange(h) + 0.5)
    dc = np.stack([((uu - K[0, 2]) / K[0, 0]).reshape(-1), ((vv - K[1, 2]) / K[1, 1]).reshape(-1), np.ones(h * w)], axis=1)
    D = O.rotate(np.asarray(wxyz, np.float64), dc)                     # world direction per unit of camera z
    best = np.full(h * w, np.inf)
    oc = np.asarray(t, np.float64) - SPHERE_C
    dot = lambda a, b: (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]   # noqa: E731
    qa, qb, qc = dot(D, D), 2 * dot(D, oc[None, :]), dot(oc, oc) - SPHERE_R * SPHERE_R
    disc = qb * qb - 4 * qa * qc
    with np.errstate(all='ignore'):
        s = (-qb - np.sqrt(disc)) / (2 * qa)
        hit = (disc > 0) & (s > 0)
        best[hit] = s[hit]
        s = (WALL_Z - t[2]) / D[:, 2]
        hit = (s > 0) & (s < best)
        best[hit] = s[hit]
    best[~np.isfinite(best)] = 0.0
    return best.reshape(h, w)


def scene(eyes, targets, h, w):
    """K, wxyzs [F, 4], translations [F, 3], depths float64 [F, h, w] of the sphere-and-wall scene from the given poses."""
    K = intrinsics(h, w)
    poses = [look_at(e, t) for e, t in zip(eyes, targets)]
    q, t = np.array([p[0] for p in poses]), np.array([p[1] for p in poses])
    return K, q, t, np.stack([cast_depth(K, q[f], t[f], h, w) for f in range(len(q))])


def sphere_state(dims, lo, vs, centre, radius, trunc):
    """tsdf = clamp((|c - centre| - r) / trunc) at the voxel centres, all weights 1."""
    nx, ny, nz = dims
    c = voxel_centres(lo, dims, vs) - np.asarray(centre, np.float64)[None, :]
    sd = (np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]) - radius) / trunc
    return np.clip(sd, -1.0, 1.0).astype(np.float32).reshape(nz, ny, nx), np.ones((nz, ny, nx), np.float32)


# ------------------------------------------------------------------------------------------------ scenes of the cull tests
def frame_terms(K, wxyz, t, lo, dims, vs, depth, depth_scale=1.0):
    """The per-voxel quantities of integrate's steps 1 - 4 for one frame, float64 [ny * nz, nx] each (a row is an x-run): h0, h1, h2,
    px, py, d, sdf.  px and py are NaN where h2 > 0 fails, d and sdf where the voxel has no pixel."""
    K, depth = np.asarray(K, np.float64), np.asarray(depth)
    h, w = depth.shape
    c = voxel_centres(lo, dims, vs)
    cam = O.rotate(O.quat_inverse(wxyz), c - np.asarray(t, np.float64)[None, :])
    x, y, z = cam[:, 0], cam[:, 1], cam[:, 2]
    h0 = (K[0, 0] * x + K[0, 1] * y) + K[0, 2] * z
    h1 = (K[1, 0] * x + K[1, 1] * y) + K[1, 2] * z
    h2 = (K[2, 0] * x + K[2, 1] * y) + K[2, 2] * z
    with np.errstate(all='ignore'):
        px, py = np.where(h2 > 0, h0 / h2, np.nan), np.where(h2 > 0, h1 / h2, np.nan)
        inside = (px >= 0) & (px < w) & (py >= 0) & (py < h)
        u, v = np.where(inside, np.floor(px), 0).astype(np.int64), np.where(inside, np.floor(py), 0).astype(np.int64)
        d = np.where(inside, depth[v, u].astype(np.float64) / np.float64(depth_scale), np.nan)
    rows = lambda a: a.reshape(-1, dims[0])                            # noqa: E731
    return dict(h0=rows(h0), h1=rows(h1), h2=rows(h2), px=rows(px), py=rows(py), d=rows(d), sdf=rows(d - h2))


def failed_rules(terms, h, w, max_depth, trunc):
    """Which of the contract's geometric rules each voxel fails, bool [ny * nz, nx] each.  `behind` is step 1 (h2 > 0 fails); `left`,
    `right`, `up`, `down` are the four comparisons of step 2 (for h2 > 0); `far` is h2 > max_depth + trunc, where d <= max_depth
    (step 3) and sdf >= -trunc (step 4) cannot both hold, whatever the depth."""
    px, py, h2 = terms['px'], terms['py'], terms['h2']
    with np.errstate(invalid='ignore'):
        return dict(behind=~(h2 > 0), far=h2 > max_depth + trunc, left=px < 0, right=px >= w, up=py < 0, down=py >= h)


def applied(terms, max_depth, trunc):
    """bool [ny * nz, nx]: the frame changes the voxel (every step of the contract passes)."""
    with np.errstate(invalid='ignore'):
        return (terms['d'] > 0) & (terms['d'] <= max_depth) & ~(terms['sdf'] < -trunc)


def run_counts(fails, rule):
    """(x-runs whose every voxel fails `rule` and no other rule, x-runs that hold voxels that fail it and voxels that pass it)."""
    others = np.zeros_like(fails[rule])
    for name, f in fails.items():
        if name != rule:
            others |= f
    only = fails[rule] & ~others
    return int(only.all(axis=1).sum()), int((fails[rule].any(axis=1) & ~fails[rule].all(axis=1)).sum())


def ring(F):
    """F poses that wind three times around the sphere-and-wall scene, all in front of the wall -> (eyes, targets)."""
    a = 2 * np.pi * np.arange(F) / F * 3.0
    eyes = [(0.9 * np.cos(x), 0.6 * np.sin(x), 0.15 + 0.25 * np.sin(2.3 * x)) for x in a]
    targets = [(0.05 + 0.3 * np.cos(1.7 * x), -0.02 + 0.2 * np.sin(x), 1.1) for x in a]
    return eyes, targets


# The ring's volume: 70 voxels along x are two x tiles of a wave, the second partial; it reaches from beside the sphere to beyond it.
RING = dict(dims=(70, 9, 7), vs=0.05, lo=np.array([-1.7, -0.2, 0.9]), trunc=0.2, h=20, w=24, max_depth=4.0)


def ring_scene(F):
    """K, wxyzs, translations, depths float64 [F, 20, 24] of the ring."""
    return scene(*ring(F), RING['h'], RING['w'])


FAR_SHIFT = np.array([1000.0, -2000.0, 500.0])                         # moves a scene (lo and every translation) away from the origin
# for the ring's 20 x 24 image: skew, unequal focal lengths, a principal point off the centre
SKEW_K = np.array([[21.6, 1.5, 12.3], [0.0, 19.0, 9.6], [0.0, 0.0, 1.0]])


# One camera per bound of the frame cull, over the volume of the base scene with a 20 x 24 image.  look_at's third argument is the
# image's down direction: (1, 0, 0) rolls the camera by 90 degrees, so that the x-runs of the volume cross the upper and lower bounds.
# The behind camera stands inside the volume, near its +x end, looking towards +x and tilted by 45 degrees, so that the runs of one
# corner lie wholly behind its plane; its focal length is a third of the others', so that its frustum holds most of what is in front.
BOUNDS = dict(dims=(37, 29, 21), vs=0.05, lo=np.array([-0.9, -0.7, 0.55]), trunc=0.2, h=20, w=24)
BOUND_CAMERAS = {
    'left': dict(eye=(2.46, -0.69, 0.55), target=(0.57, 0.69, 2.23), down=(0.0, 1.0, 0.0), max_depth=4.0),
    'right': dict(eye=(-2.68, -0.08, 1.35), target=(-1.33, -0.04, 1.85), down=(0.0, 1.0, 0.0), max_depth=4.0),
    'up': dict(eye=(-2.86, 0.58, 0.94), target=(-0.03, 1.14, 0.66), down=(-1.0, 0.0, 0.0), max_depth=4.0),
    'down': dict(eye=(-2.86, 0.58, 0.94), target=(-0.03, 1.14, 0.66), down=(1.0, 0.0, 0.0), max_depth=4.0),
    'far': dict(eye=(0.47, -0.57, -0.34), target=(0.16, 0.01, 1.38), down=(0.0, 1.0, 0.0), max_depth=1.5),
    'behind': dict(eye=(0.76, 0.24, 0.75), target=(1.76, -0.35, 1.56), down=(0.0, 1.0, 0.0), max_depth=4.0, focal=0.3),
}


def bound_scene(rule):
    """K, wxyz, translation, depth float64 [20, 24], max_depth of the camera that exercises `rule`.  The far camera's depths are cut
    at max_depth where they exceed it in the right half of the image, so some equal max_depth exactly."""
    cam, h, w = BOUND_CAMERAS[rule], BOUNDS['h'], BOUNDS['w']
    K = intrinsics(h, w, cam.get('focal', 0.9))
    q, t = look_at(cam['eye'], cam['target'], cam['down'])
    depth = cast_depth(K, q, t, h, w)
    if rule == 'far':
        depth[:, w // 2:] = np.minimum(depth[:, w // 2:], cam['max_depth'])
    return K, q, t, depth, cam['max_depth']


# Ties on the bounds: an identity pose at the origin, a 16 x 16 image with focal length 8 and principal point (8, 8), voxels of 1 / 16
# whose centres are odd multiples of 1 / 32, and a flat depth of 1.0 = max_depth.  Every product and sum of the projection is exact, so
# px == 0 where x == -z, px == w where x == z, py == 0 where y == -z, and h2 == max_depth + trunc in the layer z = 1.21875.
TIES = dict(vs=0.0625, trunc=0.21875, max_depth=1.0, h=16, w=16, K=np.array([[8.0, 0.0, 8.0], [0.0, 8.0, 8.0], [0.0, 0.0, 1.0]]),
            wxyz=np.array([1.0, 0.0, 0.0, 0.0]), t=np.zeros(3))
TIE_VOLUMES = {
    'wide': dict(dims=(48, 12, 14), lo=np.array([-1.5, -0.875, 0.5])),   # the image's left and right bounds cross every x-run
    'left-end': dict(dims=(6, 12, 14), lo=np.array([-0.875, -0.875, 0.5])),   # px == 0 at the last voxel of the runs of the first layer
}


# ------------------------------------------------------------------------------------------------ mesh checks
def edge_stats(tris):
    """(max uses of an undirected edge, min uses, max uses of a directed edge, undirected edge count)."""
    t = np.asarray(tris, np.int64)
    d = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    _, dc = np.unique(d[:, 0] * (t.max() + 1) + d[:, 1], return_counts=True)
    u = np.sort(d, axis=1)
    _, uc = np.unique(u[:, 0] * (t.max() + 1) + u[:, 1], return_counts=True)
    return int(uc.max()), int(uc.min()), int(dc.max()), len(uc)


def signed_volume(verts, tris):
    a, b, c = (verts[tris[:, k]] for k in range(3))
    return float(np.einsum('ij,ij->i', a, np.cross(b, c)).sum() / 6.0)
