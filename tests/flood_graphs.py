"""Input recipes for the ordered floods (f3d_flood_order, f3d_color_segment, f3d_region_grow) at the sizes where their block
shares, batches and 1024-entry chunks change behaviour.  Plain NumPy; nothing here touches the GPU.

Every graph is a CSR pair (offsets int64 [n + 1], neighbours int32 [offsets[n]]) that meets the preconditions of include/f3d.h
(f3d_flood_order): rows are symmetric, hold no entry twice and stay inside [0, n).  `layered` also lists the row's own node first;
`relabel` keeps it but moves it anywhere in the row (a row may or may not list its own node, and the floods never follow it).
"""
import numpy as np

# level widths; a breadth-first search from the first node has exactly these level sizes
CHUNK_EDGES = [1, 1023, 1, 1024, 1, 1025, 2, 2049, 3]      # the 1024-entry chunks of k_color_grow / k_region_grow / f3d_flood_place
CARRY_EDGES = [1, 2500, 5000, 3]                            # every node of the wide levels has children: expanders past 1024 place some
SHARE_EDGES = [1, 1024, 1025, 7]                            # FO_GRID = 1024 block shares of f3d_flood_order: one entry each, then two
BATCH_EDGE = [1, 300, 262145 + 300]                         # a frontier above 1024 * 256: a second batch in k_fo_count / k_fo_apply
BATCH_TAIL_EVERY = 64                                       # tailed(BATCH_EDGE, 64): that frontier's entries have children in every share
PATH_DEPTHS = (1, 7, 8, 9, 16, 17)                          # around the FO_CHUNK = 8 levels between two frontier readbacks


def PATH(d):
    return [1] * d


def level_starts(widths):
    return np.concatenate([[0], np.cumsum(widths)]).astype(np.int64)


def level_of(widths):
    """level (0-based) of every node of layered(widths)"""
    return np.repeat(np.arange(len(widths)), widths)


def parent_of(widths):
    """parent node of every node of layered(widths); -1 for the first"""
    st = level_starts(widths)
    par = np.full(st[-1], -1, np.int64)
    for l in range(1, len(widths)):
        c = -(-widths[l] // widths[l - 1])
        par[st[l]:st[l + 1]] = st[l - 1] + np.arange(widths[l]) // c
    return par


def from_edges(n, u, v, self_first=True):
    """CSR of the undirected edges (u[e], v[e]), each given once and u != v: row i = [i,] then its neighbours in ascending order.
    Symmetric and duplicate-free as long as no edge is given twice."""
    u, v = np.asarray(u, np.int64), np.asarray(v, np.int64)
    src = np.concatenate([np.arange(n) if self_first else np.zeros(0, np.int64), u, v])
    dst = np.concatenate([np.arange(n) if self_first else np.zeros(0, np.int64), v, u])
    key = np.where(src == dst, -1, dst)                      # the row's own node sorts first
    order = np.lexsort((key, src))
    offs = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(src, minlength=n), out=offs[1:])
    return offs, dst[order].astype(np.int32)


def layered(widths):
    """Levels of widths[0], widths[1], ... nodes, numbered level by level; node j of level l is joined to node
    j // ceil(w_l / w_{l-1}) of level l - 1.  Row i = [i, its parent, its children in ascending order]: symmetric, duplicate-free,
    the row's own node first (the preconditions of include/f3d.h).  A breadth-first search from node 0 has level sizes exactly
    `widths`, and as every node's children are consecutive and follow those of the node before it, a FIFO flood that rejects
    nothing pops the nodes as arange(n)."""
    widths = [int(w) for w in widths]
    assert widths and widths[0] >= 1 and all(w >= 1 for w in widths)
    par = parent_of(widths)
    child = np.arange(1, len(par), dtype=np.int64)
    return from_edges(len(par), par[1:], child)


def tailed(widths, every):
    """layered(widths) plus one more node joined to every `every`-th node of the last level (the new nodes are numbered last, in
    that order): one more level whose parents are spread over the whole level before it.  As built a flood still pops arange(n)."""
    par = parent_of(widths)
    last = level_starts(widths)[-2] + np.arange(0, widths[-1], every)
    par = np.concatenate([par, last])
    return from_edges(len(par), par[1:], np.arange(1, len(par), dtype=np.int64))


def relabel(csr, perm, rng):
    """The same graph with node i renamed perm[i] and every row shuffled by `rng`.  Node data moves with
    data_new[perm] = data_old."""
    offs, nb = np.asarray(csr[0], np.int64), np.asarray(csr[1], np.int64)
    perm = np.asarray(perm, np.int64)
    n = len(offs) - 1
    deg = np.diff(offs)
    row = perm[np.repeat(np.arange(n, dtype=np.int64), deg)]
    order = np.lexsort((rng.random(len(nb)), row))
    out = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(perm, weights=deg, minlength=n).astype(np.int64), out=out[1:])
    return out, perm[nb][order].astype(np.int32)


def moved(data, perm):
    """node data of the relabelled graph"""
    out = np.empty_like(data)
    out[perm] = data
    return out


def disjoint_union(graphs, cross_edges=()):
    """Several graphs in one cloud, component after component; cross_edges = (u, v) pairs of union indices, u != v, each pair once
    and not an edge of a component: appended to both rows.  -> (CSR pair, first node of every component [len(graphs) + 1])"""
    starts = np.concatenate([[0], np.cumsum([len(g[0]) - 1 for g in graphs])]).astype(np.int64)
    rows = []
    for g, s in zip(graphs, starts):
        offs, nb = np.asarray(g[0], np.int64), np.asarray(g[1], np.int64)
        rows.extend((nb[offs[i]:offs[i + 1]] + s).tolist() for i in range(len(offs) - 1))
    for u, v in cross_edges:
        assert u != v and v not in rows[u] and u not in rows[v]
        rows[u].append(int(v))
        rows[v].append(int(u))
    offs = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return (offs, np.concatenate([np.asarray(r, np.int32) for r in rows])), starts


def check_rows(csr):
    """symmetric, duplicate-free, in range; raises AssertionError"""
    offs, nb = np.asarray(csr[0], np.int64), np.asarray(csr[1], np.int64)
    n = len(offs) - 1
    assert offs[0] == 0 and offs[-1] == len(nb) and (np.diff(offs) >= 0).all()
    assert len(nb) == 0 or (nb.min() >= 0 and nb.max() < n)
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(offs))
    fwd = row * n + nb
    assert len(np.unique(fwd)) == len(fwd), 'a row holds an entry twice'
    assert np.array_equal(np.sort(fwd), np.sort(nb * n + row)), 'rows are not symmetric'


def bfs_levels(csr, source, allowed=None):
    """level sizes of a breadth-first search from `source` (through nodes with allowed[node] only)"""
    offs, nb = np.asarray(csr[0], np.int64), np.asarray(csr[1], np.int64)
    n = len(offs) - 1
    seen = np.zeros(n, bool) if allowed is None else ~np.asarray(allowed, bool)
    seen[source] = True
    front, sizes = np.array([source], np.int64), []
    while len(front):
        sizes.append(len(front))
        lo, deg = offs[front], offs[front + 1] - offs[front]
        idx = np.repeat(lo - np.concatenate([[0], np.cumsum(deg)[:-1]]), deg) + np.arange(deg.sum())
        front = np.unique(nb[idx])
        front = front[~seen[front]]
        seen[front] = True
    return sizes


def variants(csr, seed, keep_first=False):
    """(name, CSR pair, perm) of the graph as built (perm = identity: a flood pops in index order) and relabelled by a seeded
    permutation with shuffled rows; keep_first: node 0 keeps its index (it stays the smallest of its cluster: the flood's seed)"""
    n = len(csr[0]) - 1
    rng = np.random.default_rng(seed)
    perm = np.concatenate([[0], 1 + rng.permutation(n - 1)]).astype(np.int64) if keep_first else rng.permutation(n)
    return (('built', csr, np.arange(n)), ('relabelled', relabel(csr, perm, rng), perm))


# ------------------------------------------------------------------------------------------------ reject recipes
def reject_colors(widths, seed, dtype=np.float64, nchan=3, noise=0.02):
    """Values of layered(widths) for the running-mean floods.  A node's value is its level's centre 0.5 + 0.1 * level / nlevels plus
    noise: the centre drifts away from the running mean, so with a threshold of a few times the noise the test of an entry depends
    on the mean that the entries before it left, to the last bit.  A seeded quarter of the nodes is 0.5 above the centre in one
    seeded channel, far outside any such threshold.  The nodes of levels of at most four nodes and their parents sit on the centre
    exactly, so that the flood reaches every level.  -> values [n, nchan] (or [n] for nchan 1) of `dtype`, the mask of the far
    nodes."""
    rng = np.random.default_rng(seed)
    lv = level_of(widths)
    n = len(lv)
    narrow = np.asarray(widths)[lv] <= 4
    keep = narrow.copy()
    keep[parent_of(widths)[narrow & (lv > 0)]] = True
    val = 0.5 + 0.1 * lv[:, None] / len(widths) + np.where(keep[:, None], 0.0, rng.normal(0, noise, (n, nchan)))
    far = (rng.random(n) < 0.25) & ~keep
    val[np.nonzero(far)[0], rng.integers(0, nchan, int(far.sum()))] += 0.5
    val = val.astype(dtype)
    return (val[:, 0].copy() if nchan == 1 else val), far


def flood_trace(csr, seed_nodes, accepts):
    """Replays the FIFO flood the three kernels share with the acceptance given as accepts[node] (taken from a restatement's
    result): -> per level (queue, positions in the queue of the entries that expand, children enqueued by each of those).  It
    states what a recipe covers; the checked results come from the restatements themselves."""
    offs, nb = np.asarray(csr[0], np.int64).tolist(), np.asarray(csr[1], np.int64).tolist()
    seen = np.zeros(len(offs) - 1, bool)
    queue = [int(s) for s in seed_nodes]
    seen[queue] = True
    out = []
    while queue:
        ok = [k for k, p in enumerate(queue) if accepts[p]]
        nxt, nchild = [], []
        for k in ok:
            p, before = queue[k], len(nxt)
            for q in nb[offs[p]:offs[p + 1]]:
                if not seen[q]:
                    seen[q] = True
                    nxt.append(q)
            nchild.append(len(nxt) - before)
        out.append((np.array(queue, np.int64), np.array(ok, np.int64), np.array(nchild, np.int64)))
        queue = nxt
    return out


def carry_coverage(trace, chunk=1024):
    """-> (every level above `chunk` entries has an accepted and a rejected entry in each of its chunks of two or more entries,
           and some such level exists: the staging loop carries
           its counts across chunks both ways,
           some entry at position >= chunk of a level's list of expanding entries has children: the placement adds a carry)"""
    mixed, carried = any(len(q) > chunk for q, _, _ in trace), False
    for queue, ok, nchild in trace:
        if len(queue) > chunk:
            acc = np.zeros(len(queue), bool)
            acc[ok] = True
            for c0 in range(0, len(queue), chunk):
                if len(queue) - c0 >= 2:                     # a chunk of one entry cannot hold both
                    mixed = mixed and bool(acc[c0:c0 + chunk].any() and not acc[c0:c0 + chunk].all())
        carried = carried or bool(nchild[chunk:].sum() > 0)
    return mixed, carried


# ------------------------------------------------------------------------------------------------ composed inputs
UNION_WIDTHS = (PATH(9), SHARE_EDGES, [1, 700, 900], [1], [1, 2])
UNION_CLASSES = (2, 1, 2, 3, 1)


def class_union():
    """Five components of different depths and classes UNION_CLASSES in one cloud, with cross edges between components of
    different class (so some points are boundary points).  -> (CSR pair, classes int64 [n])"""
    graphs = [layered(w) for w in UNION_WIDTHS]
    st = np.concatenate([[0], np.cumsum([sum(w) for w in UNION_WIDTHS])])
    cross = [(st[0] + 4, st[1] + 3), (st[1] + 1500, st[2] + 10), (st[2] + 1200, st[3]), (st[3], st[4] + 1), (st[2] - 1, st[0] + 8),
             (st[0], st[4])]
    csr, starts = disjoint_union(graphs, cross)
    return csr, np.repeat(np.asarray(UNION_CLASSES, np.int64), np.diff(starts))


def batch_classes(split, tails=False):
    """classes of layered(BATCH_EDGE) (or of tailed(BATCH_EDGE, BATCH_TAIL_EVERY)): one class, or (split) the second half of level 1 and its children in a class of their own.
    Level 1's nodes are joined through the first node only, so the split gives one large cluster and 150 of up to 876 points each, all of
    them in flight together with a frontier above 262 144 entries."""
    cls = np.full(sum(BATCH_EDGE), 4, np.int64)
    if split:
        par = parent_of(BATCH_EDGE)
        second = np.zeros(len(cls), bool)
        second[1 + BATCH_EDGE[1] // 2:1 + BATCH_EDGE[1]] = True
        second[1 + BATCH_EDGE[1]:] = second[par[1 + BATCH_EDGE[1]:]]
        cls[second] = 6
    if tails:                                               # a tail has its parent's class
        cls = np.concatenate([cls, cls[1 + BATCH_EDGE[1]::BATCH_TAIL_EVERY]])
    return cls


def seeded_colors(seed=1):
    """Input of the several-seeds colour case: components A and B = layered(CHUNK_EDGES), C = layered([1, 5, 9]), one edge between
    a level-1 node of A and one of B.  B's colours are 0.3 below A's and C's 0.3 above.  ids: 0 and 9 are neutral; A's first node
    carries 9 itself, B's 5, C's 7; some far nodes carry the non-neutral 3, and some nodes of C carry 9.  Seeds: B's first node
    (its flood reaches A's node over the edge and rejects it), A's first node (whose id is a neutral one: every 9 stops being
    neutral, also in C), a node of A that A's flood took (id 9 again; its mean starts afresh, so it takes
    children that A's flood rejected), C's first node.
    -> (CSR pair, colours float64 [n, 3], ids int64 [n], seeds, neutral ids, (a, b) the joined nodes)"""
    na = sum(CHUNK_EDGES)
    a, b = 5, na + 7
    csr, starts = disjoint_union([layered(CHUNK_EDGES), layered(CHUNK_EDGES), layered([1, 5, 9])], [(a, b)])
    ca, fa = reject_colors(CHUNK_EDGES, seed)
    cb, fb = reject_colors(CHUNK_EDGES, seed + 1)
    cc, fc = reject_colors([1, 5, 9], seed + 2)
    colors = np.vstack([ca, cb - 0.3, cc + 0.3])
    far = np.concatenate([fa, fb, fc])
    far[[a, b]] = False
    colors[a], colors[b] = ca[0], cb[0] - 0.3
    rng = np.random.default_rng(seed + 3)
    ids = np.where(rng.random(len(far)) < 0.1, 9, 0).astype(np.int64)
    ids[far & (rng.random(len(far)) < 0.3)] = 3
    ids[starts[2] + 3], ids[starts[2] + 8] = 9, 9
    ids[0], ids[na], ids[starts[2]] = 9, 5, 7
    seeds = np.array([na, 0, level_starts(CHUNK_EDGES)[4], starts[2]], np.int64)   # A's one node of level 4: 1025 children
    return csr, colors, ids, seeds, (0, 9), (a, b)


STAR = [1, 3099]
SEED_COUNTS = (1, 1023, 1024, 1025, 3000)


def star_values(seed, dtype=np.float64, nchan=1):
    """Values on layered(STAR): two thirds of the nodes near 1.0 (noise 0.02), one third at 1.5; the first node near 1.0.  With
    the threshold 0.25 and the mean starting as the seeds' average (about 1.17), the seeds at 1.5 fail the test and expand nothing."""
    rng = np.random.default_rng(seed)
    n = sum(STAR)
    val = 1.0 + rng.normal(0, 0.02, (n, nchan))
    far = rng.random(n) < 1 / 3
    far[0] = False
    val[far] += 0.5
    val = val.astype(dtype)
    return (val[:, 0].copy() if nchan == 1 else val), far


def star_seeds(count, far, perm, seed):
    """`count` distinct nodes other than the first, in seeded random order, the first of them a near one; relabelled by perm"""
    rng = np.random.default_rng(seed)
    order = 1 + rng.permutation(len(far) - 1)
    first = int(np.argmax(~far[order]))
    order[[0, first]] = order[[first, 0]]
    return perm[order[:count]]
