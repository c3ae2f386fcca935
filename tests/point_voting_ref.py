"""Test-only restatement of PointVotingSegmentation (Fusion3DSeg/segUtils/voting.py of the reference), NumPy + sklearn, vectorised.

Written from the semantics, not from the reference's text:
* search: pixel q pairs with every cloud index i whose float64 squared distance is <= r*r (sklearn's KDTree.query_radius);
* vote: per frame every DISTINCT (i, mask[q]) cell and every distinct (i, last column) cell gets +1 (NumPy's buffered fancy-index
  ``+=``), the label statement first, so a label equal to the last column's index adds 2 there;
* a label beyond the last column raises IndexError before the frame writes anything, but only if its pixel has a neighbour;
  non-finite queries raise sklearn's ValueError; earlier frames stay applied;
* segment: the total is the last column, the unfiltered candidates are the columns before it.
"""
import numpy as np
from sklearn.neighbors import KDTree


def make_tree(cloud):
    return KDTree(np.asarray(cloud), leaf_size=2)


def get_nns(tree, queries, radius):
    """(int32 indices of all queries flattened in sklearn's order, per-query counts)."""
    nns = tree.query_radius(np.asarray(queries), r=radius)
    freq = np.array([len(x) for x in nns])
    return np.hstack(nns).astype(np.int32), freq


def vote_frame(votes, tree, queries, mask_flat, radius):
    """One frame, in place on votes [M, ncols]."""
    idx, freq = get_nns(tree, queries, radius)
    if idx.shape[0] == 0:
        return
    ncols = votes.shape[1]
    labels = np.repeat(np.asarray(mask_flat).reshape(-1), freq).astype(np.int64)
    if (labels >= ncols).any():
        raise IndexError(f'index {labels.max()} is out of bounds for axis 1 with size {ncols}')
    flat = votes.reshape(-1)
    flat[np.unique(idx.astype(np.int64) * ncols + labels)] += 1
    flat[np.unique(idx).astype(np.int64) * ncols + (ncols - 1)] += 1


def vote(votes, cloud, frames, masks, radius, tree=None):
    """frames: iterable of [hw, 3]; masks: matching iterable of flat uint8 masks, None = the mask file is absent."""
    tree = make_tree(cloud) if tree is None else tree
    for q, m in zip(frames, masks):
        if m is None:
            continue
        vote_frame(votes, tree, q, m, radius)
    return votes


def segment(votes, nclasses, threshold, filter_classes=None):
    votes = np.asarray(votes)
    total = votes[:, -1]
    cand = votes[:, :-1] if filter_classes is None else votes[:, list(filter_classes)]
    cls = np.argmax(cand, axis=1)
    best = cand[np.arange(len(cand)), cls]
    ratio = np.divide(best, total, out=np.zeros(len(cand)), where=total > 0)
    cls[~(total > 0) | ((total > 0) & (ratio < threshold)) | (best == 0)] = nclasses
    if filter_classes is not None:
        for i, c in enumerate(filter_classes):                 # sequential: a class id below the list length is remapped again
            cls[cls == i] = c
    return cls
