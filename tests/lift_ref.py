"""Mask lifting restated in plain Python / NumPy from the contract in include/f3d.h (f3d_lift_overlaps / f3d_lift_instances): sets,
dicts and np.unique, no kernels.  Also the hand-built scenes the CPU and GPU tests share."""
from types import SimpleNamespace

import numpy as np


def incidence(luts, inst, npoints, max_ids):
    """-> (rows: point -> ascending list of its segments, sizes int32 [S]).  Raises the contract's IndexError."""
    luts, inst = np.asarray(luts, np.int64), np.asarray(inst, np.int64)
    nf, hw = luts.shape
    if (inst > max_ids).any() or (luts >= npoints).any():
        raise IndexError('lift: an instance id exceeds max_ids, or a lookup is not below npoints')
    f = np.repeat(np.arange(nf, dtype=np.int64), hw).reshape(nf, hw)
    ok = (luts >= 0) & (inst > 0)
    g = f[ok] * max_ids + (inst[ok] - 1)
    pairs = np.unique(np.stack([luts[ok], g], axis=1), axis=0) if ok.any() else np.zeros((0, 2), np.int64)
    rows = {}
    for p, s in pairs.tolist():                                  # np.unique sorted them by (point, segment)
        rows.setdefault(p, []).append(s)
    sizes = np.bincount(pairs[:, 1], minlength=nf * max_ids).astype(np.int32)
    return rows, sizes


def segment_overlaps(luts, inst, npoints, max_ids):
    """-> (sizes int32 [S], pairs int32 [P, 2] ascending, counts int32 [P])."""
    rows, sizes = incidence(luts, inst, npoints, max_ids)
    cnt = {}
    for row in rows.values():
        for i, a in enumerate(row):
            for b in row[i + 1:]:
                cnt[(a, b)] = cnt.get((a, b), 0) + 1
    keys = sorted(cnt)
    return sizes, np.array(keys, np.int32).reshape(-1, 2), np.array([cnt[k] for k in keys], np.int32)


def lift_instances(luts, inst, npoints, max_ids=None, ratio=0.5, min_overlap=10, seg_classes=None, min_points=1):
    inst = np.asarray(inst)
    if max_ids is None:
        max_ids = max(1, int(inst.max())) if inst.size else 1
    rows, sizes = incidence(luts, inst, npoints, max_ids)
    _, pairs, counts = segment_overlaps(luts, inst, npoints, max_ids)
    nseg = len(sizes)
    parent = list(range(nseg))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    for (a, b), c in zip(pairs.tolist(), counts.tolist()):
        if c < min_overlap or not (float(c) >= np.float64(ratio) * np.float64(min(sizes[a], sizes[b]))):
            continue
        if seg_classes is not None and seg_classes[a] != seg_classes[b]:
            continue
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)                    # the root is the minimum index
    roots = sorted({find(g) for g in range(nseg) if sizes[g] > 0})
    number = {r: k + 1 for k, r in enumerate(roots)}
    seg2inst = np.array([number[find(g)] if sizes[g] > 0 else 0 for g in range(nseg)], np.int32).reshape(nseg)

    ids, support, seen = np.zeros(npoints, np.int32), np.zeros(npoints, np.uint16), np.zeros(npoints, np.uint16)
    for p, row in rows.items():
        seen[p] = min(len(row), 65535)
        count = {}
        for g in row:
            count[seg2inst[g]] = count.get(seg2inst[g], 0) + 1
        best = min(count, key=lambda i: (-count[i], i))          # the largest count, a tie to the smaller id
        ids[p], support[p] = best, min(count[best], 65535)

    wins = np.bincount(ids, minlength=len(roots) + 1)
    keep = [i for i in range(1, len(roots) + 1) if wins[i] >= min_points]
    renumber = np.zeros(len(roots) + 1, np.int32)
    renumber[keep] = np.arange(1, len(keep) + 1)
    ids = renumber[ids]
    support[ids == 0] = 0
    seg2inst = renumber[seg2inst]
    inst_points = np.bincount(ids, minlength=len(keep) + 1).astype(np.int64)
    return SimpleNamespace(ids=ids, support=support, seen=seen, seg2inst=seg2inst, inst_points=inst_points)


def split_by_lift(ids, lifted):
    pairs = sorted(set(zip(np.asarray(ids).tolist(), np.asarray(lifted).tolist())))
    rank = {pr: k for k, pr in enumerate(pairs)}
    return np.array([rank[pr] for pr in zip(np.asarray(ids).tolist(), np.asarray(lifted).tolist())], np.int64)


def flood_components(points, radius):
    """Number of connected components of the radius graph (a NumPy flood)."""
    pts = np.asarray(points, np.float64)
    d2 = ((pts[:, None, :] - pts[None, :, :]) ** 2).sum(-1)
    adj = d2 <= radius * radius
    label = np.full(len(pts), -1)
    ncomp = 0
    for s in range(len(pts)):
        if label[s] >= 0:
            continue
        stack, label[s] = [s], ncomp
        while stack:
            u = stack.pop()
            for v in np.nonzero(adj[u] & (label < 0))[0]:
                label[v] = ncomp
                stack.append(v)
        ncomp += 1
    return ncomp


# ------------------------------------------------------------------------------------------------ hand-built scenes
def frames_from_sets(npoints, frames, hw=None, max_ids=None):
    """frames: per frame a dict {id: iterable of points}.  -> (luts int32 [F, HW], inst uint16 [F, HW]); one pixel per (point, id),
    the rest of a frame empty (lut -1, id 0)."""
    need = max(sum(len(list(pts)) for pts in fr.values()) for fr in frames)
    hw = max(need, 1) if hw is None else hw
    luts, inst = np.full((len(frames), hw), -1, np.int32), np.zeros((len(frames), hw), np.uint16)
    for f, fr in enumerate(frames):
        k = 0
        for i, pts in fr.items():
            for p in pts:
                luts[f, k], inst[f, k] = p, i
                k += 1
    return luts, inst


def two_boxes(seed=0):
    """Two 4 x 4 x 4 boxes of unit spacing that touch (x = 0..3 and x = 4..7): 128 points, point p of box b = 64 b + ...  Six frames
    each see both boxes whole and give them local ids in shuffled order (with a decoy id in between).
    -> (points [128, 3], luts, inst, max_ids = 3, box [128])."""
    g = np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(4), indexing='ij'), -1).reshape(-1, 3).astype(np.float64)
    points = np.vstack([g, g + [4.0, 0.0, 0.0]])
    box = np.repeat([0, 1], 64)
    rng = np.random.default_rng(seed)
    frames = []
    for f in range(6):
        a, b = rng.permutation(3)[:2] + 1                          # two of the ids 1..3, in any order
        order = rng.permutation(128)
        fr = {int(a): [p for p in order if box[p] == 0], int(b): [p for p in order if box[p] == 1]}
        frames.append(fr if f % 2 else dict(reversed(list(fr.items()))))
    luts, inst = frames_from_sets(128, frames)
    return points, luts, inst, 3, box


def chain(overlap_ab=6, overlap_bc=6):
    """Three segments a (frame 0), b (frame 1), c (frame 2) of 12 points each: a and b share overlap_ab points, b and c share
    overlap_bc, a and c none.  a = 0..11, b = 12 - overlap_ab .. , c follows b.  -> (npoints, luts, inst)."""
    a = list(range(0, 12))
    b = list(range(12 - overlap_ab, 24 - overlap_ab))
    c = list(range(b[-1] + 1 - overlap_bc, b[-1] + 13 - overlap_bc))
    luts, inst = frames_from_sets(c[-1] + 1, [{1: a}, {1: b}, {1: c}])
    return c[-1] + 1, luts, inst


def threshold_pair(overlap):
    """Segment a (frame 0) = 8 points, segment b (frame 1) = 12 points sharing `overlap` of them."""
    a = list(range(8))
    b = list(range(8 - overlap, 20 - overlap))
    luts, inst = frames_from_sets(b[-1] + 1, [{1: a}, {1: b}])
    return b[-1] + 1, luts, inst


def random_scene(seed, n, nf, hw, k, hit=0.6, skew=3.0, no_id=0.1):
    """Lookups hit `hit` of the pixels; the hits crowd towards the low point indices (u^skew), so that points are seen many times,
    also several times within a frame and with different ids; `no_id` of the pixels carry id 0."""
    rng = np.random.default_rng(seed)
    luts = np.floor(n * rng.random((nf, hw)) ** skew).astype(np.int32)
    luts[rng.random((nf, hw)) >= hit] = -1
    luts[rng.random((nf, hw)) < 0.01] = -7                          # any negative value means none
    inst = rng.integers(1, k + 1, (nf, hw)).astype(np.uint16)
    inst[rng.random((nf, hw)) < no_id] = 0
    return luts, inst
