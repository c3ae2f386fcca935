"""Plain-Python restatement of the CVSegmentation contract (include/f3d.h f3d_flood_order / f3d_color_segment), the checker of
the kernels at sizes the golden file cannot hold.

Written from the contract, not from the reference's text: a deque BFS per cluster and per colour seed.
* instance_seperate: semantic classes (those not listed) first, one record each; then every listed class in the given
  order, seeds by ascending index among the points that carry the class when its turn comes.  The flood enqueues every
  unvisited neighbour, expands only same-class ones, and a popped different-class point marks its discoverer as boundary.
  A cluster smaller than minimum_points gets category 0 and its points are relabelled 0 in `classes` (in place).  At the end
  every category-0 record folds into the first one (merge_instances_by_classes with classes (0,)).
* color_segment: per seed, a FIFO flood through neutral points with a level limit and the running-mean colour test.
"""
from collections import deque

import numpy as np


def _rows(adj):
    """list of rows, or a CSR pair (offsets, neighbours)."""
    if isinstance(adj, tuple) and len(adj) == 2:
        offs, nb = adj
        return [nb[offs[i]:offs[i + 1]] for i in range(len(offs) - 1)]
    return adj


def flood_class(seed, rows, classes):
    """-> (cluster points in pop order, boundary bool [n])"""
    n = len(classes)
    c = classes[seed]
    seen = np.zeros(n, bool)
    seen[seed] = True
    found_by = {seed: seed}
    boundary = np.zeros(n, bool)
    out = []
    todo = deque([seed])
    while todo:
        p = todo.popleft()
        if classes[p] != c:
            boundary[found_by[p]] = True
            continue
        out.append(p)
        for q in rows[p]:
            q = int(q)
            if not seen[q]:
                seen[q] = True
                found_by[q] = p
                todo.append(q)
    return np.array(out, dtype=np.int64), boundary


def merge_zero(ids, info, clusters, boundaries):
    """merge_instances_by_classes(ids, info, (0,), clusters, boundaries)"""
    new_of, out_info, groups_c, groups_b = {}, [], [], []
    zero_slot = None
    for k, rec in enumerate(info):
        if rec['category_id'] == 0 and zero_slot is not None:
            new_of[rec['id']] = zero_slot
            out_info[zero_slot]['area'] += rec['area']
            groups_c[zero_slot].append(clusters[k])
            groups_b[zero_slot].append(boundaries[k])
            continue
        slot = len(out_info)
        if rec['category_id'] == 0:
            zero_slot = slot
        new_of[rec['id']] = slot
        out_info.append(rec)
        groups_c.append([clusters[k]])
        groups_b.append([boundaries[k]])
    out_ids = ids.copy()
    for old, new in new_of.items():
        out_ids[ids == old] = new
    return (len(out_info) + 1, out_ids, out_info, [np.hstack(g) for g in groups_c], [np.hstack(g) for g in groups_b])


def instance_seperate(classes, adj, instance_classes=None, minimum_points=1):
    """-> (ids range, ids, info, clusters, boundaries); `classes` is rewritten in place like the reference's self.classes."""
    rows = _rows(adj)
    n = len(classes)
    ids = np.zeros_like(classes)
    info, clusters, boundaries = [], [], []
    present = np.unique(classes)
    if instance_classes is None:
        order, next_id = present, 0
    else:
        order = np.array(instance_classes)
        for k, c in enumerate(np.setdiff1d(present, order)):
            pts = np.nonzero(classes == c)[0]
            ids[pts] = k
            info.append({'id': k, 'isthing': False, 'category_id': int(c), 'area': int(len(pts))})
            clusters.append(pts)
            boundaries.append(None)
        next_id = len(info)
    for c in order:
        todo = classes == c
        for seed in range(n):
            if not todo[seed]:
                continue
            pts, bnd = flood_class(seed, rows, classes)
            cat = 0 if len(pts) < minimum_points else c
            ids[pts] = next_id
            info.append({'id': next_id, 'isthing': True, 'category_id': int(cat), 'area': int(len(pts))})
            clusters.append(pts)
            boundaries.append(bnd)
            next_id += 1
            todo[pts] = False
            classes[pts] = cat
    m, ids, info, clusters, boundaries = merge_zero(ids, info, clusters, boundaries)
    return np.arange(m), ids, info, clusters, boundaries


def color_segment(classes_unused, adj, colors, ids, seeds, threshold, neutral_ids=(0,), max_level=10, counts=None):
    """ids updated in place and returned; `counts` (a list) receives every seed's number of accepted points."""
    rows = _rows(adj)
    n = len(ids)
    thr = np.broadcast_to(np.asarray(threshold, dtype=np.float64), (3,))
    neutral = np.isin(ids, list(neutral_ids))
    for seed in seeds:
        sid = ids[seed]
        seen = np.zeros(n, bool)
        seen[seed] = True
        mean = colors[seed].copy()
        count = 0
        todo = deque([(int(seed), 1)])
        while todo:
            p, lv = todo.popleft()
            if lv == max_level:
                continue
            c = colors[p]
            if (np.abs(mean - c).astype(np.float64) > thr).any():
                continue
            count += 1
            mean = mean + (c - mean) / count
            ids[p] = sid
            for q in rows[p]:
                q = int(q)
                if not seen[q] and neutral[q]:
                    seen[q] = True
                    todo.append((q, lv + 1))
        neutral[ids == sid] = False
        if counts is not None:
            counts.append(count)
    return ids


# ---------------------------------------------------------------- golden encoding (tests/golden/cvseg.npz holds no objects)
def encode_instances(out, prefix, store):
    """(ids range, ids, info, clusters, boundaries) -> flat arrays under `prefix`.  A boundary is kind 0 (bool array) or kind 1
    (object array, None = -1); both as int8 values."""
    rng_, ids, info, clusters, boundaries = out
    store[prefix + 'nrange'] = np.array(len(rng_))
    store[prefix + 'ids'] = ids
    store[prefix + 'info'] = np.array([[d['id'], int(d['isthing']), d['category_id'], d['area']] for d in info], np.int64).reshape(-1, 4)
    store[prefix + 'clusters'] = np.concatenate(clusters) if clusters else np.zeros(0, np.int64)
    store[prefix + 'cluster_offsets'] = np.cumsum([0] + [len(c) for c in clusters]).astype(np.int64)
    kinds, vals = [], []
    for b in boundaries:
        b = np.asarray(b)
        kinds.append(1 if b.dtype == object else 0)
        vals.append(np.array([-1 if v is None else int(bool(v)) for v in b], np.int8))
    store[prefix + 'boundary_kinds'] = np.array(kinds, np.int8)
    store[prefix + 'boundaries'] = np.concatenate(vals) if vals else np.zeros(0, np.int8)
    store[prefix + 'boundary_offsets'] = np.cumsum([0] + [len(v) for v in vals]).astype(np.int64)


def decode_instances(g, prefix):
    """-> (nrange, ids, info dicts, clusters, boundaries) as the reference returns them."""
    co, bo = g[prefix + 'cluster_offsets'], g[prefix + 'boundary_offsets']
    cl = g[prefix + 'clusters']
    clusters = [cl[co[k]:co[k + 1]] for k in range(len(co) - 1)]
    bv, kinds = g[prefix + 'boundaries'], g[prefix + 'boundary_kinds']
    boundaries = []
    for k in range(len(bo) - 1):
        v = bv[bo[k]:bo[k + 1]]
        if kinds[k]:
            boundaries.append(np.array([None if x < 0 else bool(x) for x in v], dtype=object))
        else:
            boundaries.append(v.astype(bool))
    info = [{'id': int(a), 'isthing': bool(b), 'category_id': int(c), 'area': int(d)} for a, b, c, d in g[prefix + 'info']]
    return int(g[prefix + 'nrange']), g[prefix + 'ids'], info, clusters, boundaries


def same_boundary(got, want):
    got = np.asarray(got) if not hasattr(got, 'cpu') else got.cpu().numpy()
    if (got.dtype == object) != (want.dtype == object) or got.shape != want.shape:
        return False
    if want.dtype == object:
        return all((a is None and b is None) or (a is not None and b is not None and bool(a) == bool(b)) for a, b in zip(got, want))
    return got.dtype == want.dtype and np.array_equal(got, want)


def same_instances(got, want):
    """instance_seperate's result against (n, ids, info, clusters, boundaries) of the reference or the restatement: everything exactly, the
    clusters in flood (pop) order, the boundaries as sets (same_boundary)."""
    n, ids, info, clusters, bnds = want
    assert len(got[0]) == n and np.array_equal(got[0], np.arange(n))
    assert got[1].dtype == ids.dtype and np.array_equal(got[1], ids)
    assert got[2] == info
    assert len(got[3]) == len(clusters) and len(got[4]) == len(bnds)
    for a, b in zip(got[3], clusters):
        assert a.dtype == b.dtype and np.array_equal(a, b)          # flood (pop) order
    for k in range(len(bnds)):
        assert same_boundary(got[4][k], bnds[k]), k
