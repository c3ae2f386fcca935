"""Hybrid k-nearest search and label transfer without a GPU: the C-ABI surface, the argument checks that precede any launch, and
the brute-force restatement (tests/knn_ref.py) itself -- against sklearn's KDTree on tie-free data, and its plurality rule on
hand-made rows."""
import re

import numpy as np
import pytest
from sklearn.neighbors import KDTree

import f3d
import knn_ref as R
from conftest import ROOT

NEW_SYMBOLS = ['f3d_knn_query', 'f3d_knn_query_dev', 'f3d_transfer_labels', 'f3d_transfer_labels_dev', 'f3d_ctx_reserve_knn']


def test_library_exports_and_header_declares_the_new_entries():
    lib = f3d.library()
    text = re.sub(r'/\*.*?\*/', '', (ROOT / 'include' / 'f3d.h').read_text(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), f'{name} is not exported by libf3d_hip.so'
        assert name in lib._f3d_symbols
        assert re.search(r'\bint\s+%s\s*\(' % name, text), f'{name} is not declared in include/f3d.h'


@pytest.mark.parametrize('k', [0, 33, -1])
def test_k_out_of_range_raises_before_any_launch(k):
    ctx = f3d.Context.__new__(f3d.Context)              # no f3d_ctx behind it: anything but the argument check would fail differently
    pts = np.zeros((4, 3))
    with pytest.raises(ValueError, match='k must be in'):
        ctx.knn_query(pts, pts, k, 0.1)
    with pytest.raises(ValueError, match='k must be in'):
        ctx.transfer_labels(pts, np.zeros(4, np.int64), pts, k, 0.1)
    with pytest.raises(ValueError, match='k must be in'):
        ctx.knn_query_dev(0, f3d.F64, 4, 0, f3d.F64, 4, k, 0.1, 0)
    with pytest.raises(ValueError, match='k must be in'):
        ctx.transfer_labels_dev(0, f3d.F64, 4, 0, 0, f3d.F64, 4, k, 0.1, -1, 0)


def test_public_surface_checks_k_and_label_dtype_without_a_device():
    from Fusion3DSeg.segUtils import transfer
    pts = np.zeros((4, 3))
    for k in (0, 33):
        with pytest.raises(ValueError, match='k must be in'):
            transfer.nearest_points(pts, pts, 0.1, k=k)
        with pytest.raises(ValueError, match='k must be in'):
            transfer.transfer_labels(pts, np.zeros(4, np.int64), pts, 0.1, k=k)
    with pytest.raises(TypeError, match='integer or bool'):
        transfer.transfer_labels(pts, np.zeros(4, np.float32), pts, 0.1)
    with pytest.raises(ValueError, match='one entry per cloud point'):
        transfer.transfer_labels(pts, np.zeros(5, np.int64), pts, 0.1)


@pytest.mark.parametrize('k', [1, 5, 32])
def test_restatement_agrees_with_sklearn_on_tie_free_data(k):
    rng = np.random.default_rng(k)
    data, queries = rng.uniform(-1, 1, (1500, 3)), rng.uniform(-1, 1, (700, 3))
    r = 0.3
    idx, d2, counts, matches = R.knn(data, queries, k, r)
    dist, ind = KDTree(data).query(queries, k=k)                       # sorted by distance; no ties in random float64 data
    assert (np.diff(np.sort(R.dist2(queries[:50], data), axis=1), axis=1) > 0).all()
    within = R.dist2(queries, data)[np.arange(len(queries))[:, None], ind] <= r * r
    assert np.array_equal(within, np.sort(within, axis=1)[:, ::-1])   # the cut at the radius is a prefix
    assert np.array_equal(idx, np.where(within, ind, -1))
    assert np.array_equal(counts, within.sum(axis=1)) and (matches > k).any()
    assert k < 32 or (counts < k).any()                                # the radius cuts some rows short
    assert np.array_equal(np.isinf(d2), idx < 0)


def test_restatement_breaks_distance_ties_by_index_and_pads():
    data = np.array([[1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, 0, 0.5], [0, -1, 0], [5, 5, 5]], float)
    q = np.array([[0, 0, 0], [9, 9, 9]], float)
    idx, d2, counts, matches = R.knn(data, q, 4, 1.0)                  # 1.0 * 1.0: the four unit points are exactly on it
    assert idx.tolist() == [[3, 0, 1, 2], [-1, -1, -1, -1]]
    assert d2[0].tolist() == [0.25, 1.0, 1.0, 1.0] and np.isinf(d2[1]).all()
    assert counts.tolist() == [4, 0] and matches.tolist() == [5, 0]
    for r in (-1.0, float('nan')):
        assert (R.knn(data, q, 3, r)[0] == -1).all()
    assert R.cut((idx, d2, counts, matches), 2)[0].tolist() == [[3, 0], [-1, -1]]


def test_plurality_rule_on_hand_made_rows():
    a, b, fill = 7, -3, -99
    assert R.plurality_row([a, b, b, a], fill) == (a, 2)
    assert R.plurality_row([b, a, a], fill) == (a, 2)
    assert R.plurality_row([], fill) == (fill, 0)
    assert R.plurality_row([b, a], fill) == (b, 1)
    # the vectorised form used by the GPU tests follows it: labels of data points 0..3 are [a, b, b, a]
    labels = np.array([a, b, b, a, 2 ** 40], np.int64)
    idx = np.array([[0, 1, 2, 3], [1, 0, 3, -1], [-1, -1, -1, -1], [4, 1, -1, -1], [2, 0, 3, 1]], np.int32)
    out, support = R.plurality(idx, labels, fill)
    assert out.tolist() == [a, a, fill, 2 ** 40, b] and support.tolist() == [2, 2, 0, 1, 2]
    rng = np.random.default_rng(0)
    labels = rng.integers(-2, 3, 50) * (2 ** 33)
    idx = rng.integers(-1, 50, (300, 6)).astype(np.int32)
    idx = np.where(np.arange(6)[None, :] < rng.integers(0, 7, 300)[:, None], np.abs(idx), -1).astype(np.int32)
    out, support = R.plurality(idx, labels, fill)
    want = [R.plurality_row([int(labels[j]) for j in row if j >= 0], fill) for row in idx]
    assert out.tolist() == [w[0] for w in want] and support.tolist() == [w[1] for w in want]
