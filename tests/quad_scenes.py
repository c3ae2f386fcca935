"""Small scenes for f3d_door_window_quads next to door_window_ref.capture_scene: a few rectangles (two triangles each) and
instances of chosen sizes, each a noisy patch on one rectangle's plane.  Points are in general position (noise > 0): a point
exactly in a mesh plane gives a minimum of 0 and QUAD_NO_CANDIDATE by the reference's own rule, which the golden `b` scene pins.
Plain NumPy; every function returns (points [n, 3], ids int64 [n], instance ids list, vertices [nv, 3], triangles int64 [nt, 3]).
"""
import numpy as np

WILD_IDS = (-7, 2 ** 40 + 3)                        # a negative id and one above 2^40 among the wanted ones


def _frames(nrm, rng):
    u = np.cross(nrm, rng.normal(size=nrm.shape))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    return u, np.cross(nrm, u)


def _rect_mesh(centre, u, w, half):
    corners = [centre + sa * half[:, :1] * u + sb * half[:, 1:] * w for sa, sb in ((-1, -1), (1, -1), (1, 1), (-1, 1))]
    verts = np.stack(corners, 1).reshape(-1, 3)
    base = 4 * np.arange(len(centre))[:, None]
    tris = np.concatenate([base + [0, 1, 2], base + [0, 2, 3]], 1).reshape(-1, 3)
    return verts, tris.astype(np.int64)


def _patch(rng, m, centre, u, w, nrm, half, noise):
    a, b = rng.uniform(-0.8, 0.8, (2, m))
    return centre + (a * half[0])[:, None] * u + (b * half[1])[:, None] * w + rng.normal(0, noise, (m, 1)) * nrm


def _instance_ids(k):
    """k distinct ids in ascending order: WILD_IDS[0], then odd numbers, WILD_IDS[1] last (from two instances on)"""
    ids = [WILD_IDS[0]] + [2 * i + 1 for i in range(k - 1)]
    if k >= 2:
        ids[-1] = WILD_IDS[1]
    return ids


def rect_scene(nrect, sizes, noise=0.02, seed=0, ntri=None, nother=0, other_ids=(2, 4)):
    """nrect random rectangles in a 20 m box (the first `ntri` triangles of their mesh, all by default); instance k has sizes[k]
    points on rectangle k % nrect; `nother` points of unwanted ids anywhere in the box.  Instance order = ascending id; the cloud
    is instance after instance, the unwanted points last."""
    rng = np.random.default_rng(seed)
    centre = rng.uniform(0, 20, (nrect, 3))
    nrm = rng.normal(size=(nrect, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    u, w = _frames(nrm, rng)
    half = rng.uniform(0.5, 2.0, (nrect, 2))
    verts, tris = _rect_mesh(centre, u, w, half)
    if ntri is not None:
        tris = tris[:ntri]
    inst = _instance_ids(len(sizes))
    pts, ids = [], []
    for k, m in enumerate(sizes):
        r = k % nrect
        pts.append(_patch(rng, m, centre[r], u[r], w[r], nrm[r], half[r], noise))
        ids.append(np.full(m, inst[k], np.int64))
    if nother:
        pts.append(rng.uniform(0, 20, (nother, 3)))
        ids.append(rng.choice(np.asarray(other_ids, np.int64), nother))
    return np.concatenate(pts), np.concatenate(ids), inst, verts, tris


def shuffled(scene, seed):
    pts, ids, inst, verts, tris = scene
    perm = np.random.default_rng(seed).permutation(len(pts))
    return pts[perm], ids[perm], inst, verts, tris


def sorted_by_id(scene):
    pts, ids, inst, verts, tris = scene
    order = np.argsort(ids, kind='stable')
    return pts[order], ids[order], inst, verts, tris


def fan_scene(nfan=136, heavy=((70, 100), (5, 69)), seed=0, noise=0.01):
    """One vertical 4 x 3 rectangle cut into `nfan` coplanar triangles around its centre (the boundary split into nfan segments),
    plus four ordinary rectangles far from it.  Instance s is spread over the fan, two points in every sector, and four in the
    sectors heavy[s]: all nfan triangles are in its band (their distance sums differ by rounding only) and the best inside count
    is shared by the sectors heavy[s]; the first of them in triangle order has to win."""
    rng = np.random.default_rng(seed)
    c, u, w = np.array([3.0, 4.0, 1.5]), np.array([0.6, 0.8, 0.0]), np.array([0.0, 0.0, 1.0])
    nrm = np.cross(u, w)
    t = np.linspace(0, 4, nfan + 1)[:-1]                        # position along the square [-1, 1]^2's boundary, scaled below
    side, f = np.floor(t).astype(int), t - np.floor(t)
    bx = np.select([side == 0, side == 1, side == 2, side == 3], [2 * f - 1, np.ones_like(f), 1 - 2 * f, -np.ones_like(f)])
    by = np.select([side == 0, side == 1, side == 2, side == 3], [-np.ones_like(f), 2 * f - 1, np.ones_like(f), 1 - 2 * f])
    rim = c + (2.0 * bx)[:, None] * u + (1.5 * by)[:, None] * w
    fverts = np.vstack([c[None], rim])
    ring = 1 + np.arange(nfan)
    ftris = np.stack([np.zeros(nfan, np.int64), ring, 1 + (np.arange(nfan) + 1) % nfan], 1)
    centre = np.array([[40.0, 40, 3], [50, 40, 3], [40, 50, 3], [50, 50, 3]])
    n4 = rng.normal(size=(4, 3))
    n4[:, 2] *= 0.2
    n4 /= np.linalg.norm(n4, axis=1, keepdims=True)
    u4, w4 = _frames(n4, rng)
    rverts, rtris = _rect_mesh(centre, u4, w4, np.full((4, 2), 1.0))
    verts, tris = np.vstack([fverts, rverts]), np.vstack([ftris, rtris + len(fverts)])
    inst = _instance_ids(len(heavy) + 1)
    pts, ids = [], []
    for s, hv in enumerate(heavy):
        per = np.full(nfan, 2)
        per[list(hv)] = 4
        sec = np.repeat(np.arange(nfan), per)
        a, b = fverts[ftris[sec, 1]], fverts[ftris[sec, 2]]
        wa, wb = rng.uniform(0.25, 0.4, (2, len(sec)))           # well inside the sector: weights (1 - wa - wb, wa, wb)
        p = c + wa[:, None] * (a - c) + wb[:, None] * (b - c) + rng.normal(0, noise, (len(sec), 1)) * nrm
        order = rng.permutation(len(p))
        pts.append(p[order])
        ids.append(np.full(len(p), inst[s], np.int64))
    pts.append(_patch(rng, 90, centre[1], u4[1], w4[1], n4[1], np.array([1.0, 1.0]), noise))     # an ordinary instance beside them
    ids.append(np.full(90, inst[-1], np.int64))
    return np.concatenate(pts), np.concatenate(ids), inst, verts, tris


def _flat_rect(x0, y0, z, dx, dy, down):
    v = np.array([[x0, y0, z], [x0 + dx, y0, z], [x0 + dx, y0 + dy, z], [x0, y0 + dy, z]], np.float64)
    return v[::-1] if down else v


def _tilted_rect(x0, y0, z, dx, dy, angle, down):
    """a dx x dy rectangle whose normal is (-sin a, 0, cos a), or its opposite for `down`"""
    ux, uz = np.cos(angle), np.sin(angle)
    v = np.array([[x0, y0, z], [x0 + dx * ux, y0, z + dx * uz], [x0 + dx * ux, y0 + dy, z + dx * uz], [x0, y0 + dy, z]], np.float64)
    return v[::-1] if down else v


# (name, tilt about y in rad, facing down): exact +z, exact -z, down on either side of 1 - |n_z| = 1.00001e-5 (np.allclose with 1),
# up on either side of cos(10 deg), and a wall
FACINGS = (('up', 0.0, False), ('down', 0.0, True), ('down_4e-3', 4.0e-3, True), ('down_5e-3', 5.0e-3, True),
           ('up_9.9deg', np.deg2rad(9.9), False), ('up_10.1deg', np.deg2rad(10.1), False), ('wall', np.pi / 2, False))


def facing_scene(seed=0, m=150, noise=0.01):
    """One 2 x 1 rectangle per entry of FACINGS, 5 m apart, with one instance of m points on each."""
    rng = np.random.default_rng(seed)
    verts, pts, ids = [], [], []
    inst = _instance_ids(len(FACINGS))
    for k, (_, angle, down) in enumerate(FACINGS):
        v = _flat_rect(5.0 * k, 1.0, 2.0, 2.0, 1.0, down) if angle == 0.0 else _tilted_rect(5.0 * k, 1.0, 2.0, 2.0, 1.0, angle, down)
        verts.append(v)
        a, b = rng.uniform(0.1, 0.9, (2, m))
        e0, e1 = v[1] - v[0], v[3] - v[0]
        nrm = np.cross(e0, e1)
        nrm /= np.linalg.norm(nrm)
        pts.append(v[0] + a[:, None] * e0 + b[:, None] * e1 + rng.normal(0, noise, (m, 1)) * nrm)
        ids.append(np.full(m, inst[k], np.int64))
    base = 4 * np.arange(len(FACINGS))[:, None]
    tris = np.concatenate([base + [0, 1, 2], base + [0, 2, 3]], 1).reshape(-1, 3).astype(np.int64)
    return np.concatenate(pts), np.concatenate(ids), inst, np.vstack(verts), tris


def with_negative_indices(scene, seed=0):
    """the same scene with half the triangle corners written as negative indices (ix - nv)"""
    pts, ids, inst, verts, tris = scene
    neg = np.random.default_rng(seed).random(tris.shape) < 0.5
    return pts, ids, inst, verts, np.where(neg, tris - len(verts), tris)


def with_zero_area_triangle(scene):
    pts, ids, inst, verts, tris = scene
    return pts, ids, inst, verts, np.vstack([tris, [[1, 1, 2]]])


def with_nan_vertex(scene):
    pts, ids, inst, verts, tris = scene
    return pts, ids, inst, np.vstack([verts, [[np.nan, 0.0, 0.0]]]), np.vstack([tris, [[0, 1, len(verts)]]])
