"""Brute-force restatement of the hybrid k-nearest search and the label transfer (include/f3d.h: f3d_knn_query,
f3d_transfer_labels), the oracle of tests/test_transfer_*.py.  NumPy only, float64 throughout (float32 inputs widen exactly)."""
import numpy as np

PAIRS_PER_CHUNK = 2_000_000


def dist2(queries, data):
    """float64 [n, m]: (dx*dx + dy*dy) + dz*dz, the parenthesisation of the kernels' candidate test."""
    q, d = np.asarray(queries, np.float64), np.asarray(data, np.float64)
    t0, t1, t2 = (q[:, None, c] - d[None, :, c] for c in range(3))
    return (t0 * t0 + t1 * t1) + t2 * t2


def knn(data, queries, k, radius):
    """-> (idx int32 [n, k], dist2 float64 [n, k], counts int32 [n], matches int64 [n]).  Row q: the min(k, matches[q]) data indices with
    d2 <= radius*radius that are smallest under (d2, index), in that order, padded with -1 / +inf; matches[q] = all of them.
    k is not limited to 32 here (the tests look one slot past the cut)."""
    data, queries = np.asarray(data), np.asarray(queries)
    m, n = len(data), len(queries)
    r = float(radius)
    idx = np.full((n, k), -1, np.int32)
    d2o = np.full((n, k), np.inf, np.float64)
    matches = np.zeros(n, np.int64)
    step = max(1, PAIRS_PER_CHUNK // max(m, 1))
    index = np.arange(m)
    for a in range(0, n, step):
        d2 = dist2(queries[a:a + step], data)
        ok = d2 <= r * r if r >= 0.0 else np.zeros(d2.shape, bool)             # radius < 0 or NaN: nothing matches
        key = np.where(ok, d2, np.inf)
        order = np.lexsort((np.broadcast_to(index, d2.shape), key), axis=-1)[:, :k]
        cnt = ok.sum(axis=1)
        kept = np.arange(order.shape[1])[None, :] < np.minimum(cnt, k)[:, None]
        idx[a:a + step, :order.shape[1]] = np.where(kept, order, -1)
        d2o[a:a + step, :order.shape[1]] = np.where(kept, np.take_along_axis(d2, order, axis=1), np.inf)
        matches[a:a + step] = cnt
    return idx, d2o, np.minimum(matches, k).astype(np.int32), matches


def cut(row, k):
    """The answer for a smaller k from the answer for a larger one: (idx, dist2, counts) of knn(..., k, ...)."""
    idx, d2, _, matches = row
    return idx[:, :k], d2[:, :k], np.minimum(matches, k).astype(np.int32)


def plurality_row(labels_in_row, fill):
    """(winner, support) of one kept row, by the stated rule: the label with the most occurrences, ties to the label whose first
    occurrence comes earliest; an empty row gives (fill, 0).  Plain Python, the pin of `plurality`."""
    best, win = 0, fill
    seen = []
    for x in labels_in_row:
        if x not in seen:
            seen.append(x)
    for x in seen:                                                             # in order of first occurrence
        c = sum(1 for y in labels_in_row if y == x)
        if c > best:
            best, win = c, x
    return win, best


def plurality(idx, labels, fill):
    """-> (out int64 [n], support int32 [n]) of the rows `idx` (-1 padded) over int64 `labels`."""
    labels = np.asarray(labels, np.int64)
    valid = idx >= 0
    lab = labels[np.where(valid, idx, 0)]
    same = (lab[:, :, None] == lab[:, None, :]) & valid[:, :, None] & valid[:, None, :]
    cnt = same.sum(axis=2)                                                     # occurrences of slot s's label in its row (0: empty slot)
    first = cnt.argmax(axis=1)                                                 # the first slot with the largest count
    rows = np.arange(len(idx))
    support = cnt[rows, first].astype(np.int32)
    out = np.where(support > 0, lab[rows, first], np.int64(fill))
    return out.astype(np.int64), support


def transfer(data, labels, queries, k, radius, fill=-1):
    idx = knn(data, queries, k, radius)[0]
    return plurality(idx, labels, fill)
