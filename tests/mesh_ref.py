"""NumPy / SciPy restatement of Fusion3DSeg.segUtils.meshUtils (the oracle of tests/test_mesh_*.py) and the test meshes.

Clusters come from scipy.sparse.csgraph.connected_components over the shared-ordered-edge graph, relabelled by lowest triangle
index; triangle areas use the library's operation order; cluster areas are math.fsum (correctly rounded)."""
import math

import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components


def vertex_map(tris, nv):
    """CSR of vertex_triangle_mapping: (offsets int64 [V + 1], tri int32 [3M], pos int8 [3M]), rows in ascending slot order."""
    flat = np.asarray(tris).reshape(-1).astype(np.int64)
    order = np.argsort(flat, kind='stable')
    offsets = np.zeros(nv + 1, np.int64)
    np.cumsum(np.bincount(flat, minlength=nv), out=offsets[1:])
    return offsets, (order // 3).astype(np.int32), (order % 3).astype(np.int8)


def lists_of(offsets, flat):
    return [flat[offsets[v]:offsets[v + 1]].tolist() for v in range(len(offsets) - 1)]


def remove_faces(nv, tris, mask):
    mask = np.asarray(mask, bool)
    o2n = np.where(mask, 0, np.cumsum(~mask) - 1).astype(np.int64)
    nr = ~mask[tris].any(axis=1) if len(tris) else np.zeros(0, bool)
    return nr, o2n[tris[nr]].astype(tris.dtype).reshape(-1, 3), o2n


def keep_faces(verts, tris, mask):
    mask = np.asarray(mask, bool)
    kept = mask[tris].any(axis=1) if len(tris) else np.zeros(0, bool)
    flat = tris[kept].reshape(-1)
    uniq, first = np.unique(flat, return_index=True)
    by_appearance = uniq[np.argsort(first)]
    newid = np.full(len(verts), -1, np.int64)
    newid[by_appearance] = np.arange(len(by_appearance))
    return verts[by_appearance].reshape(-1, 3), newid[tris[kept]].astype(tris.dtype).reshape(-1, 3)


def triangle_areas(verts, tris):
    v = np.asarray(verts, np.float64)
    p0, p1, p2 = v[tris[:, 0]], v[tris[:, 1]], v[tris[:, 2]]
    a, b = p0 - p1, p0 - p2
    cx = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]
    cy = a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2]
    cz = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
    return 0.5 * np.sqrt((cx * cx + cy * cy) + cz * cz)


def clusters(verts, tris):
    """-> (triangle_clusters int32 [M], cluster_n_triangles int64 [P], cluster_area float64 [P] by fsum, triangle areas [M])."""
    m = len(tris)
    if m == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int64), np.zeros(0), np.zeros(0)
    t = tris.astype(np.int64)
    nv = int(t.max()) + 1
    e = np.concatenate([t[:, [0, 1]], t[:, [0, 2]], t[:, [1, 2]]])
    key = e.min(axis=1) * nv + e.max(axis=1)
    face = np.tile(np.arange(m), 3)
    order = np.argsort(key, kind='stable')
    key, face = key[order], face[order]
    same = key[1:] == key[:-1]
    graph = coo_matrix((np.ones(int(same.sum()), np.int8), (face[:-1][same], face[1:][same])), shape=(m, m))
    _, lab = connected_components(graph, directed=False)
    _, first = np.unique(lab, return_index=True)                      # relabel by lowest triangle index
    rank = np.empty(len(first), np.int64)
    rank[np.argsort(first)] = np.arange(len(first))
    cl = rank[lab].astype(np.int32)
    area = triangle_areas(verts, tris)
    n = np.bincount(cl).astype(np.int64)
    order = np.argsort(cl, kind='stable')
    cuts = np.cumsum(n)[:-1]
    ca = np.array([math.fsum(part.tolist()) for part in np.split(area[order], cuts)])
    return cl, n, ca, area


def clean_by_composition(remove_fn, cluster_fn, verts, tris, remove_mask, min_triangles, min_area):
    """clean_mesh as the composition of remove_faces_by_vertices and get_triangle_clusters (either the restatements' or the
    library's) -> (new_vertices, new_triangles, kept_vertex_mask, kept_triangle_mask)."""
    nv = len(verts)
    mask = np.zeros(nv, bool) if remove_mask is None else np.asarray(remove_mask, bool)
    nr, t1, _ = remove_fn(nv, tris, mask)
    v1 = verts[~mask]
    cl, n, a = cluster_fn((v1, t1))[:3]
    good = (n >= min_triangles) & ~(a < min_area)
    keep1 = good[cl] if len(cl) else np.zeros(0, bool)
    t2 = t1[keep1]
    ref = np.zeros(len(v1), bool)
    ref[t2.reshape(-1)] = True
    _, t3, _ = remove_fn(len(v1), t2, ~ref)
    kept_t = nr.copy()
    kept_t[nr] = keep1
    kept_v = np.zeros(nv, bool)
    kept_v[~mask] = ref
    return v1[ref], t3, kept_v, kept_t


def ref_clean(verts, tris, remove_mask, min_triangles, min_area):
    return clean_by_composition(remove_faces, lambda vt: clusters(*vt), verts, tris, remove_mask, min_triangles, min_area)


def area_bound(n, fsum):
    """|any-order float64 sum of n non-negative terms - fsum| <= (gamma_{n-1} + u) * fsum, u = 2^-53 (Higham, Accuracy and Stability,
    eq. 4.4, plus the oracle's own final rounding)."""
    u = 2.0 ** -53
    k = np.maximum(np.asarray(n, np.float64) - 1, 0)
    return (k * u / (1 - k * u) + u) * fsum


# ------------------------------------------------------------------------------------------------ test meshes
def grid_mesh(nx, ny, rng=None, jitter=0.2):
    """(nx x ny) vertices, 2 (nx - 1)(ny - 1) triangles; z and the in-plane jitter make the areas differ."""
    xs, ys = np.meshgrid(np.arange(nx, dtype=np.float64), np.arange(ny, dtype=np.float64), indexing='ij')
    verts = np.stack([xs, ys, np.zeros_like(xs)], axis=-1).reshape(-1, 3)
    if rng is not None:
        verts = verts + rng.uniform(-jitter, jitter, verts.shape)
    i, j = np.meshgrid(np.arange(nx - 1), np.arange(ny - 1), indexing='ij')
    a = (i * ny + j).reshape(-1)
    tris = np.concatenate([np.stack([a, a + ny, a + 1], axis=1), np.stack([a + 1, a + ny, a + ny + 1], axis=1)]).astype(np.int64)
    return verts, tris


def strip_mesh(m, rng):
    """One triangle strip of m triangles (m + 2 vertices), face order shuffled."""
    k = np.arange(m + 2)
    verts = np.stack([(k // 2).astype(np.float64), (k % 2).astype(np.float64), 0.01 * rng.standard_normal(m + 2)], axis=1)
    f = np.arange(m)
    tris = np.stack([f, f + 1, f + 2], axis=1).astype(np.int64)
    return verts, tris[rng.permutation(m)]


def fan(center, rim):
    """Triangles (center, rim[k], rim[k + 1])."""
    return [[center, rim[k], rim[k + 1]] for k in range(len(rim) - 1)]


def random_mesh(nv, m, rng, dtype=np.int64):
    verts = rng.uniform(-1, 1, (nv, 3))
    tris = rng.integers(0, nv, (m, 3)).astype(dtype)
    return verts, tris
