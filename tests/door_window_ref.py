"""Independent NumPy restatement of door_window_bbox.generate_mesh (reference :65-150) with every rounding written out.

* einsum 'mnc,nc->mn' / 'c,nc->n' / 'nc,c->n': (a0*b0 + a2*b2) + a1*b1, each product and sum rounded alone;
* np.dot / np.linalg.norm of 3-vectors: fma(x2, y2, fma(x1, y1, x0*y0)) -- the fma is evaluated exactly with fractions, so the
  result does not depend on this host's BLAS;
* np.sum(|perp|, axis=0): a sequential float64 sum in point order (np.cumsum is sequential by definition);
* np.cross: plain multiply and subtract;
* the triangle normal: cross(v1 - v0, v2 - v0) / sqrt((x*x + y*y) + z*z), left as it is for a squared norm of 0, (0, 0, 1) when
  x is NaN (the restated Open3D rule).
"""
from fractions import Fraction

import numpy as np

DOOR_WINDOW = (86, 115, 116)
COS10 = float.fromhex('0x1.f838b8c811c17p-1')
QUAD_OK, QUAD_HORIZONTAL, QUAD_NO_CANDIDATE = 0, 1, 2


def fma(a, b, c):
    a, b, c = float(a), float(b), float(c)
    if not all(np.isfinite([a, b, c])):
        return a * b + c
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def blas_dot(x, y):
    return fma(x[2], y[2], fma(x[1], y[1], float(x[0]) * float(y[0])))


def einsum3(a0, a1, a2, b0, b1, b2):
    return (a0 * b0 + a2 * b2) + a1 * b1


def cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def normals(verts, tris):
    tv = verts[tris]
    a, b = tv[:, 1] - tv[:, 0], tv[:, 2] - tv[:, 0]
    c = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)
    nn = (c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]
    with np.errstate(invalid='ignore', divide='ignore'):
        n = np.where((nn > 0)[:, None], c / np.sqrt(nn)[:, None], c)
    n[np.isnan(n[:, 0])] = [0.0, 0.0, 1.0]
    return n


def _perp(p, v0, n):
    """[M, T] (or [M] for one triangle) perpendicular distances in the einsum's order."""
    d = p[:, None, :] - v0[None] if v0.ndim == 2 else p - v0
    return einsum3(d[..., 0], d[..., 1], d[..., 2], n[..., 0], n[..., 1], n[..., 2])


def tri_dist(p, v0, n, chunk=512):
    acc = np.zeros(len(v0))
    for b in range(0, len(p), chunk):
        blk = np.abs(_perp(p[b:b + chunk], v0, n))
        acc = np.cumsum(np.vstack([acc[None], blk]), axis=0)[-1]
    return acc


def inside_count(q, tri):
    e0, e1 = tri[2] - tri[0], tri[1] - tri[0]
    v2 = q - tri[0]
    d00, d01, d11 = blas_dot(e0, e0), blas_dot(e0, e1), blas_dot(e1, e1)
    d02 = einsum3(e0[0], e0[1], e0[2], v2[:, 0], v2[:, 1], v2[:, 2])
    d12 = einsum3(e1[0], e1[1], e1[2], v2[:, 0], v2[:, 1], v2[:, 2])
    with np.errstate(divide='ignore', invalid='ignore'):
        inv = np.float64(1.0) / np.float64(d00 * d11 - d01 * d01)
        u = (d11 * d02 - d01 * d12) * inv
        v = (d00 * d12 - d01 * d02) * inv
        return int(((u >= 0) & (v >= 0) & (u + v <= 1)).sum())


def basis(nrm):
    nrm = np.asarray(nrm, np.float64)
    a = nrm / np.sqrt(blas_dot(nrm, nrm))
    arb = np.array([0.0, 0.0, 1.0])
    if abs(abs(blas_dot(a, arb)) - 1.0) <= 1e-08 + 1e-05 * 1.0:
        arb = np.array([0.0, 1.0, 0.0])
    c = cross(a, arb)
    e = cross(a, c)
    return c / np.sqrt(blas_dot(c, c)), e / np.sqrt(blas_dot(e, e))


def quad_of(points, ids, inst_id, verts, tris, nrm):
    """-> (status, chosen triangle, quad [4, 3] or None) of one instance."""
    p = points[ids == inst_id]
    tv = verts[tris]
    with np.errstate(invalid='ignore', over='ignore'):
        td = tri_dist(p, tv[:, 0], nrm)
    if np.isnan(td).any():
        return QUAD_NO_CANDIDATE, -1, None
    mn = td.min()
    cand = np.nonzero(td < mn + 0.05 * mn)[0]
    if not len(cand):
        return QUAD_NO_CANDIDATE, -1, None
    best, bt, bq = -1, -1, None
    for t in cand:
        perp = _perp(p, tv[t, 0], nrm[t])
        q = p - nrm[t][None, :] * perp[:, None]
        c = inside_count(q, tv[t])
        if c > best:
            best, bt, bq = c, int(t), q
    if COS10 < nrm[bt][2]:
        return QUAD_HORIZONTAL, bt, None
    i, j = basis(nrm[bt])
    o = bq[0]
    d = bq - o
    x = einsum3(d[:, 0], d[:, 1], d[:, 2], i[0], i[1], i[2])
    y = einsum3(d[:, 0], d[:, 1], d[:, 2], j[0], j[1], j[2])
    xmin, xmax, ymin, ymax = x.min(), x.max(), y.min(), y.max()
    quad = np.array([o + xmin * i + ymax * j, o + xmin * i + ymin * j, o + xmax * i + ymin * j, o + xmax * i + ymax * j])
    return QUAD_OK, bt, quad


def quads(points, ids, inst_ids, verts, tris):
    """-> (quads [k, 4, 3] (NaN unless ok), status int32 [k], chosen triangle int32 [k], normals [T, 3])."""
    points, verts = np.asarray(points, np.float64), np.asarray(verts, np.float64)
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    nrm = normals(verts, tris)
    k = len(inst_ids)
    out, status, tri = np.full((k, 4, 3), np.nan), np.zeros(k, np.int32), np.full(k, -1, np.int32)
    for s, iid in enumerate(inst_ids):
        st, t, q = quad_of(points, ids, iid, verts, tris, nrm)
        status[s], tri[s] = st, t
        if q is not None:
            out[s] = q
    return out, status, tri, nrm


def generate(points, ids, info, verts, tris):
    """The reference's outputs: (triangle_ids int32 [2k], quad vertices [4k, 3], quad triangles [2k, 3], colours [4k, 3]);
    ValueError where the reference raises one."""
    entries = [d for d in info if d['category_id'] in DOOR_WINDOW]
    if entries and len(tris) == 0:
        raise ValueError('attempt to get argmin of an empty sequence')
    q, st, _, _ = quads(points, ids, [d['id'] for d in entries], verts, tris)
    if (st == QUAD_NO_CANDIDATE).any():
        raise ValueError('attempt to get argmax of an empty sequence')
    keep = np.nonzero(st == QUAD_OK)[0]
    if not len(keep):
        raise ValueError('need at least one array to concatenate')
    hexrgb = [[int(entries[e]['hexcolor'].lstrip('#')[c:c + 2], 16) for c in (0, 2, 4)] for e in keep]
    return (np.repeat([entries[e]['id'] for e in keep], 2).astype(np.int32), q[keep].reshape(-1, 3),
            np.vstack([np.array([[0, 1, 2], [2, 3, 0]]) + 4 * b for b in range(len(keep))]),
            np.repeat(np.array(hexrgb, np.float64), 4, axis=0) / 255)


def capture_scene(seed=0, ninst=40, nrect=1000, smallest=1000, largest=200_000):
    """A capture-sized input: nrect random rectangles (2 triangles each; one in eight horizontal) in a 60 m box, and ninst door /
    window instances of geometrically spaced sizes, each a noisy patch (2 cm) on one rectangle's plane; points of other ids around
    them; the cloud shuffled.  -> (points, ids, info, vertices, triangles)."""
    rng = np.random.default_rng(seed)
    centre = rng.uniform(0, 60, (nrect, 3))
    nrm = rng.normal(size=(nrect, 3))
    nrm[::8] = [0.0, 0.0, 1.0]
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    u = np.cross(nrm, rng.normal(size=(nrect, 3)))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    w = np.cross(nrm, u)
    half = rng.uniform(0.5, 3.0, (nrect, 2))
    corners = [centre + sa * half[:, :1] * u + sb * half[:, 1:] * w for sa, sb in ((-1, -1), (1, -1), (1, 1), (-1, 1))]
    verts = np.stack(corners, 1).reshape(-1, 3)
    base = 4 * np.arange(nrect)[:, None]
    tris = np.concatenate([base + [0, 1, 2], base + [0, 2, 3]], 1).reshape(-1, 3)
    sizes = np.geomspace(smallest, largest, ninst).astype(np.int64)
    host = rng.choice(nrect, ninst, replace=False)
    pts, ids, info = [], [], []
    for k, (m, r) in enumerate(zip(sizes, host)):
        a, b = rng.uniform(-0.8, 0.8, (2, m))
        p = centre[r] + (a * half[r, 0])[:, None] * u[r] + (b * half[r, 1])[:, None] * w[r] + rng.normal(0, 0.02, (m, 1)) * nrm[r]
        iid = 3 * k + 1
        pts.append(p)
        ids.append(np.full(m, iid, np.int64))
        info.append({'id': int(iid), 'isthing': True, 'category_id': int(DOOR_WINDOW[k % 3]), 'area': int(m),
                     'hexcolor': '#' + ''.join(f'{int(x):02x}' for x in rng.integers(0, 256, 3))})
    other = rng.uniform(0, 60, (50_000, 3))
    pts.append(other)
    ids.append(np.full(len(other), 2, np.int64))
    info.append({'id': 2, 'isthing': False, 'category_id': 50, 'area': len(other), 'hexcolor': '#808080'})
    pts, ids = np.concatenate(pts), np.concatenate(ids)
    perm = rng.permutation(len(pts))
    return pts[perm], ids[perm], info, verts, tris
