"""Plain-Python restatement of the region-growing contract (include/f3d.h f3d_region_grow), the checker of the kernel at sizes
the golden file cannot hold.

Written from the contract, not from the reference's text: one deque flood with the four start rules as arguments.  A queue entry
carries its level (the seeds have level 1).  A popped entry at level == max_level, or whose value is further than the threshold
from the running mean in any channel, is dropped.  Any other entry enqueues its never-enqueued neighbours in row order, and --
unless it is one of the seeds of a `given` flood -- joins the cluster and the mean: npts += 1, sma += (value - sma) / npts, in the
values' dtype.  The deque pops in the same order as the reference's list.pop(0).
"""
from collections import deque

import numpy as np


def rows_of(adj):
    """list of rows, or a CSR pair (offsets, neighbours)."""
    if isinstance(adj, tuple) and len(adj) == 2:
        offs, nb = adj
        return [nb[offs[i]:offs[i + 1]] for i in range(len(offs) - 1)]
    return adj


class _CsrRows:
    def __init__(self, offs, flat):
        self.offs, self.flat = offs, flat

    def __getitem__(self, p):
        return self.flat[self.offs[p]:self.offs[p + 1]]


def grow(values, adj, seeds, sma0, npts0, threshold, max_level, given):
    """-> accepted points int64, in acceptance order.  values [n] or [n, 3]; threshold a scalar or per channel."""
    if isinstance(adj, tuple) and len(adj) == 2:                 # CSR: plain lists iterate much faster than array slices
        offs, flat = np.asarray(adj[0]).tolist(), np.asarray(adj[1]).tolist()
        rows = _CsrRows(offs, flat)
    else:
        rows = adj
    values = np.asarray(values)
    seen = np.zeros(len(values), bool)
    seeds = [int(s) for s in np.asarray(seeds).reshape(-1)]
    seen[seeds] = True
    todo = deque((s, 1) for s in seeds)
    sma, npts = values.dtype.type(sma0) if values.ndim == 1 else np.asarray(sma0, values.dtype), int(npts0)
    thr = np.asarray(threshold, np.float64)
    out = []
    while todo:
        p, level = todo.popleft()
        if level == max_level:
            continue
        v = values[p]
        if np.any(np.abs(sma - v) > thr):
            continue
        if not (given and level == 1):
            npts += 1
            sma = sma + (v - sma) / npts
            out.append(p)
        for q in rows[p]:
            q = int(q)
            if not seen[q]:
                seen[q] = True
                todo.append((q, level + 1))
    return np.array(out, dtype=np.int64)


def depth_points(distance, adj, instance_points, threshold, max_level):
    pts = np.asarray(instance_points)
    return grow(distance, adj, pts, np.average(distance[pts], axis=0), len(pts), threshold, max_level, True)


def depth_point(distance, adj, picked, threshold, max_level):
    pts = np.asarray(picked)
    return grow(distance, adj, pts, np.average(distance[pts], axis=0), len(pts), threshold, max_level, False)


def color_points(colors, adj, instance_points, threshold, max_level):
    pts = np.asarray(instance_points)
    return grow(colors, adj, pts, np.average(colors[pts], axis=0), len(pts), threshold, max_level, True)


def color_point(colors, adj, picked, threshold, max_level):
    return grow(colors, adj, [int(picked)], colors[int(picked)], 0, threshold, max_level, False)


def plane_distance_bound(points, plane_point, normal):
    """Bound on |computed - exact| of |((dx nx + dy ny) + dz nz)| with dx = x - px rounded, in float64 (u = 2^-53).  Each
    difference carries one rounding, each product one more, and the x and y terms pass through two additions (the z term through
    one): every term carries at most four factors (1 + d), |d| <= u, so |error| <= gamma_4 S with gamma_4 = 4u / (1 - 4u) and
    S = |dx nx| + |dy ny| + |dz nz| over the exact differences (the issue's 3u S plus the subtraction's u S).  S is evaluated here
    in float64 with five roundings per term and two additions, so the evaluated sum is at least S (1 - u)^7 >= S (1 - 7u); the
    factor (1 + 16u) covers 1 / ((1 - 4u)(1 - 7u)) and the rounding of the final products.  |.| itself is exact."""
    u = 2.0 ** -53
    d = np.abs(np.asarray(points, np.float64) - np.asarray(plane_point, np.float64)) * np.abs(np.asarray(normal, np.float64))
    return 4.0 * u * (1.0 + 16.0 * u) * d.sum(axis=1)


class _Plane:
    def __init__(self, normal):
        self.normal = np.asarray(normal, np.float64)


def plane_table(normals, index_offsets, index_values, bbox_points):
    """The plane table and bounding-point map the depth wrappers take, from flat arrays: row k = [object with .normal, set of the
    plane's point indices, key of its quad in the map, its quad [4, 3]]."""
    table = np.empty((len(normals), 4), dtype=object)
    bounding = {}
    for k in range(len(normals)):
        table[k, 0] = _Plane(normals[k])
        table[k, 1] = set(int(i) for i in index_values[index_offsets[k]:index_offsets[k + 1]])
        table[k, 2] = k
        table[k, 3] = np.array(bbox_points[k], np.float64)
        bounding[k] = np.array(bbox_points[k], np.float64)
    return table, bounding


def shuffled_csr(offsets, neighbours):
    """The same graph with every row reordered by a fixed hash of (row, neighbour): a deterministic shuffle that needs no storage."""
    offsets, nb = np.asarray(offsets, np.int64), np.asarray(neighbours, np.int64)
    row = np.repeat(np.arange(len(offsets) - 1, dtype=np.int64), np.diff(offsets))
    key = ((nb + 1) * 2654435761 + row * 40503) % (1 << 32)
    order = np.lexsort((key, row))
    return offsets, nb[order].astype(np.int32)


def golden_graph(g, gi):
    """CSR pair of graph gi of tests/golden/refinement.npz (graph 1 is graph 0 with reordered rows)."""
    offs, nb = g['g0_offsets'], g['g0_neighbours']
    return (offs, nb) if gi == 0 else shuffled_csr(offs, nb)


def golden_case(g, k):
    """-> (kind, CSR pair, values, seeds, threshold, max_level, expected cluster) of flood case k"""
    values = {'dist': g['dist'], 'col': g['colors'], 'col32': g['colors'].astype(np.float32)}[str(g[f'c{k}_values'])]
    thr = g[f'c{k}_threshold']
    return (str(g[f'c{k}_kind']), golden_graph(g, int(g[f'c{k}_graph'])), values, g[f'c{k}_seeds'],
            float(thr) if thr.ndim == 0 else thr, int(g[f'c{k}_max_level']), g[f'c{k}_cluster'])
