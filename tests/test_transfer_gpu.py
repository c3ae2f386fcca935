"""Hybrid k-nearest search (f3d_knn_query) and label transfer (f3d_transfer_labels) on the GPU against the brute-force restatement
of tests/knn_ref.py, bit for bit: every K instantiation and boundary over small and odd shapes and both dtypes, distance ties at the
cut and at the radius, plurality ties, degenerate clouds, the error contract, the context's separate state, and the mesh route of
Fusion3DSeg.segUtils.transfer on device tensors."""
import functools

import numpy as np
import pytest

import f3d
import knn_ref as R
from Fusion3DSeg.segUtils import meshUtils, transfer

pytestmark = pytest.mark.gpu

KS = [1, 2, 5, 8, 9, 32]                                  # every K instantiation (1, 4, 8, 16, 32) and each boundary
PALETTE = np.array([-7, 0, 3, 2 ** 33 + 5, 2 ** 40, -2 ** 35], np.int64)
FILL = -5


def _same(got, want):
    for g, w, dt in zip(got, want, (np.int32, np.float64, np.int32)):
        assert g.dtype == dt and g.shape == w.shape
        assert np.array_equal(g, w)


def _check_both(ctx, data, labels, queries, k, r, want_rows):
    """knn_query and transfer_labels of one input against the restated rows (idx, dist2, counts) for this k."""
    _same(ctx.knn_query(data, queries, k, r), want_rows)
    out, support = ctx.transfer_labels(data, labels, queries, k, r, fill=FILL)
    wout, wsup = R.plurality(want_rows[0], labels, FILL)
    assert out.dtype == np.int64 and support.dtype == np.int32
    assert np.array_equal(out, wout) and np.array_equal(support, wsup)
    return out, support


# ------------------------------------------------------------------------------------------------ shapes
@functools.lru_cache(maxsize=None)
def _shape_case(n, m, ddt, qdt):
    rng = np.random.default_rng(7919 * n + m)
    data = rng.uniform(-0.5, 0.5, (m, 3)).astype(ddt)
    queries = rng.uniform(-0.5, 0.5, (n, 3))
    near = np.arange(0, n, 3)                             # every third query sits near a data point: matches also when m is 1 or 2
    queries[near] = data[rng.integers(0, m, len(near))].astype(np.float64) + rng.uniform(-0.05, 0.05, (len(near), 3))
    queries[1::11] += 5.0                                 # outside the reach box
    queries = queries.astype(qdt)
    labels = PALETTE[rng.integers(0, len(PALETTE), m)]
    r = 0.15                                              # about 42 of 3000 points: rows shorter and longer than 32
    return data, queries, r, labels, R.knn(data, queries, 32, r)


@pytest.mark.parametrize('qdt', [np.float32, np.float64], ids=['q32', 'q64'])
@pytest.mark.parametrize('ddt', [np.float32, np.float64], ids=['d32', 'd64'])
@pytest.mark.parametrize('m', [1, 2, 65, 3000])
@pytest.mark.parametrize('n', [1, 63, 64, 65, 257, 5000])
def test_shapes_dtypes_and_every_k(n, m, ddt, qdt):
    data, queries, r, labels, row = _shape_case(n, m, ddt, qdt)
    ctx = f3d.default_context()
    for k in KS:
        _check_both(ctx, data, labels, queries, k, r, R.cut(row, k))
    if n >= 63:
        assert row[3].max() > 0 and row[3].min() == 0    # matched and empty rows
    if n == 5000 and m == 3000:
        assert (row[3] > 32).sum() > 100 and (row[3] < 32).sum() > 100 and (row[3] == 0).sum() > 100


# ------------------------------------------------------------------------------------------------ ties
@functools.lru_cache(maxsize=None)
def _tie_case():
    rng = np.random.default_rng(3)
    data = np.round(rng.uniform(-0.5, 0.5, (6000, 3)) * 32) / 32
    queries = np.round(rng.uniform(-0.5, 0.5, (4000, 3)) * 32) / 32
    labels = rng.integers(0, 4, 6000)
    r = 3 / 32
    return data, queries, r, labels, R.knn(data, queries, 40, r)


def test_tie_recipe_still_exercises_the_rules():
    """The lattice recipe, with the counts measured when it was written: 18 971 pairs exactly on r*r, rows of 2 to 37 matches; rows with
    a tie at the cut 1703 / 2277 / 2659 / 75 for k = 1 / 5 / 8 / 32; rows shorter than k 66 at k = 8 and 3889 at k = 32; 975 rows with
    a shared top count at k = 8.  (The 66 short rows at k = 8 are asserted above 50: the recipe cannot give more.)"""
    data, queries, r, labels, row = _tie_case()
    idx, d2, _, matches = row
    assert (d2 == r * r).sum() > 100 and matches.min() >= 1 and matches.max() < 40
    for k, floor in ((1, 100), (5, 100), (8, 100), (32, 50)):
        assert ((matches > k) & (d2[:, k - 1] == d2[:, k])).sum() > floor
    assert (matches < 8).sum() > 50 and (matches < 32).sum() > 100
    i8 = R.cut(row, 8)[0]
    valid = i8 >= 0
    lab = labels[np.where(valid, i8, 0)]
    cnt = ((lab[:, :, None] == lab[:, None, :]) & valid[:, :, None] & valid[:, None, :]).sum(axis=2)
    top = cnt.max(axis=1, keepdims=True)
    first = lab[np.arange(len(lab)), cnt.argmax(axis=1)][:, None]
    assert (((cnt == top) & valid & (lab != first)).any(axis=1)).sum() > 100   # another label shares the top count


@pytest.mark.parametrize('k', [1, 5, 8, 32])
def test_ties_at_the_cut_at_the_radius_and_in_the_vote(k):
    data, queries, r, labels, row = _tie_case()
    _check_both(f3d.default_context(), data, labels, queries, k, r, R.cut(row, k))


# ------------------------------------------------------------------------------------------------ degenerate inputs
def test_identical_points_give_the_lowest_indices():
    rng = np.random.default_rng(11)
    data = rng.uniform(-1, 1, (200, 3))
    where = np.sort(rng.choice(200, 40, replace=False))
    data[where] = [0.25, -0.5, 0.125]                     # 40 bit-identical points
    q = np.array([[0.25, -0.5, 0.125]])
    idx, d2, counts = f3d.default_context().knn_query(data, q, 32, 0.01)
    assert np.array_equal(idx[0], where[:32]) and (d2 == 0).all() and counts[0] == 32
    _same((idx, d2, counts), R.knn(data, q, 32, 0.01)[:3])


def test_a_clump_within_reach_of_every_query():
    rng = np.random.default_rng(12)
    data = np.concatenate([rng.uniform(-1, 1, (500, 3)), rng.normal(0, 0.004, (3000, 3))])
    queries = rng.normal(0, 0.004, (64, 3))
    labels = PALETTE[rng.integers(0, len(PALETTE), len(data))]
    row = R.knn(data, queries, 8, 0.05)
    assert row[3].min() >= 2900
    _check_both(f3d.default_context(), data, labels, queries, 8, 0.05, row[:3])


def test_padding_outside_the_reach_box_and_without_a_match():
    rng = np.random.default_rng(13)
    data = rng.uniform(0, 1, (2000, 3))
    inside = rng.uniform(0, 1, (300, 3))
    far = rng.uniform(-1, 1, (50, 3)) * 0.2 + rng.choice([-10.0, 10.0], (50, 3))
    edge = rng.uniform(0, 1, (50, 3))
    edge[:, 0] = 1.0 + 0.01                               # within a cell of the box, past the radius of most points
    queries = np.concatenate([far, inside, edge])
    labels = rng.integers(-3, 3, 2000)
    r = 0.04
    ctx = f3d.default_context()
    for k in (1, 8):
        want = R.knn(data, queries, k, r)
        assert (want[3] == 0).sum() > 100 and (want[3] > 0).sum() > 20
        idx, d2, counts = ctx.knn_query(data, queries, k, r)
        _same((idx, d2, counts), want[:3])
        assert (idx[:50] == -1).all() and np.isposinf(d2[:50]).all() and (counts[:50] == 0).all()
        out, support = _check_both(ctx, data, labels, queries, k, r, want[:3])
        assert (out[:50] == FILL).all() and (support[:50] == 0).all()
        assert np.array_equal(support == 0, want[3] == 0) and (out[want[3] == 0] == FILL).all()


@pytest.mark.parametrize('radius', [-1.0, float('nan')])
def test_negative_and_nan_radius_give_empty_rows(radius):
    rng = np.random.default_rng(14)
    data, queries = rng.uniform(0, 1, (100, 3)), rng.uniform(0, 1, (70, 3))
    queries[:10] = data[:10]
    ctx = f3d.default_context()
    idx, d2, counts = ctx.knn_query(data, queries, 5, radius)
    assert (idx == -1).all() and np.isposinf(d2).all() and (counts == 0).all()
    out, support = ctx.transfer_labels(data, np.arange(100), queries, 5, radius, fill=FILL)
    assert (out == FILL).all() and (support == 0).all()


@functools.lru_cache(maxsize=None)
def _side_stream():
    import torch
    return torch.cuda.Stream()


def _handle(torch):
    """The stream handle for *_dev calls (the null handle would select the context's own stream); what torch has enqueued so far is
    complete when this returns."""
    torch.cuda.synchronize()
    return _side_stream().cuda_stream


def _dev_outputs(torch, n, k):
    """Sentinel-filled idx, dist2, counts / support, out; complete when this returns."""
    outs = (torch.full((n, k), 77, dtype=torch.int32, device='cuda'), torch.full((n, k), 77.0, dtype=torch.float64, device='cuda'),
            torch.full((n,), 77, dtype=torch.int32, device='cuda'), torch.full((n,), 77, dtype=torch.int64, device='cuda'))
    torch.cuda.synchronize()
    return outs


@pytest.mark.parametrize('case', ['radius', 'empty', 'nan_data', 'inf_queries'])
def test_errors_are_value_errors_and_write_nothing(case):
    import torch
    rng = np.random.default_rng(15)
    data, queries, radius = rng.uniform(0, 1, (50, 3)), rng.uniform(0, 1, (30, 3)), 0.2
    if case == 'radius':
        radius = 1e300
    elif case == 'empty':
        data = data[:0]
    elif case == 'nan_data':
        data[17, 1] = np.nan
    else:
        queries[29, 2] = np.inf
    ctx = f3d.default_context()
    labels = np.arange(len(data), dtype=np.int64)
    with pytest.raises(ValueError):
        ctx.knn_query(data, queries, 4, radius)
    with pytest.raises(ValueError):
        ctx.transfer_labels(data, labels, queries, 4, radius)
    d, q, lab = torch.from_numpy(data).cuda(), torch.from_numpy(queries).cuda(), torch.from_numpy(labels).cuda()
    idx, d2, counts, out = _dev_outputs(torch, 30, 4)
    stream = _handle(torch)
    with pytest.raises(ValueError):
        ctx.knn_query_dev(d.data_ptr(), f3d.F64, len(d), q.data_ptr(), f3d.F64, 30, 4, radius, idx.data_ptr(), d2.data_ptr(), counts.data_ptr(),
                          stream)
    with pytest.raises(ValueError):
        ctx.transfer_labels_dev(d.data_ptr(), f3d.F64, len(d), lab.data_ptr(), q.data_ptr(), f3d.F64, 30, 4, radius, -1, out.data_ptr(),
                                counts.data_ptr(), stream)
    torch.cuda.synchronize()
    assert (idx == 77).all() and (d2 == 77.0).all() and (counts == 77).all() and (out == 77).all()


def test_no_queries_is_nothing_to_do():
    ctx = f3d.default_context()
    idx, d2, counts = ctx.knn_query(np.zeros((3, 3)), np.zeros((0, 3)), 4, 0.1)
    assert idx.shape == (0, 4) and d2.shape == (0, 4) and counts.shape == (0,)
    out, support = ctx.transfer_labels(np.zeros((3, 3)), np.arange(3), np.zeros((0, 3)), 4, 0.1)
    assert out.shape == (0,) and support.shape == (0,)


# ------------------------------------------------------------------------------------------------ consistency
def test_k32_rows_are_the_radius_query_rows():
    data, queries, r, _, row = _tie_case()
    ctx = f3d.default_context()
    idx, _, counts = ctx.knn_query(data, queries, 32, r)
    offs, nb = ctx.radius_query(data, queries, r)
    lens = np.diff(offs)
    assert np.array_equal(np.minimum(lens, 32), counts)
    short = np.flatnonzero(lens <= 32)
    assert len(short) > 1000
    for q in short:
        assert np.array_equal(np.sort(idx[q, :counts[q]]), nb[offs[q]:offs[q + 1]])


def test_host_equals_dev_and_two_calls_return_identical_bits():
    import torch
    data, queries, r, labels, row = _tie_case()
    data, queries = data.astype(np.float32), queries[:1000]
    ctx = f3d.default_context()
    k = 8
    host = ctx.knn_query(data, queries, k, r)
    hout = ctx.transfer_labels(data, labels, queries, k, r, fill=FILL)
    d, q, lab = torch.from_numpy(data).cuda(), torch.from_numpy(queries).cuda(), torch.from_numpy(labels).cuda()
    stream = _handle(torch)
    for _ in range(2):
        idx, d2, counts, out = _dev_outputs(torch, len(q), k)
        sup = torch.full((len(q),), 77, dtype=torch.int32, device='cuda')
        torch.cuda.synchronize()
        ctx.knn_query_dev(d.data_ptr(), f3d.F32, len(d), q.data_ptr(), f3d.F64, len(q), k, r, idx.data_ptr(), d2.data_ptr(), counts.data_ptr(), stream)
        ctx.transfer_labels_dev(d.data_ptr(), f3d.F32, len(d), lab.data_ptr(), q.data_ptr(), f3d.F64, len(q), k, r, FILL, out.data_ptr(),
                                sup.data_ptr(), stream)
        torch.cuda.synchronize()
        _same((idx.cpu().numpy(), d2.cpu().numpy(), counts.cpu().numpy()), host)
        assert np.array_equal(out.cpu().numpy(), hout[0]) and np.array_equal(sup.cpu().numpy(), hout[1])
    # the optional outputs left out
    idx2 = torch.empty_like(idx)
    out2 = torch.empty_like(out)
    ctx.knn_query_dev(d.data_ptr(), f3d.F32, len(d), q.data_ptr(), f3d.F64, len(q), k, r, idx2.data_ptr(), None, None, stream)
    ctx.transfer_labels_dev(d.data_ptr(), f3d.F32, len(d), lab.data_ptr(), q.data_ptr(), f3d.F64, len(q), k, r, FILL, out2.data_ptr(), None, stream)
    torch.cuda.synchronize()
    assert torch.equal(idx2, idx) and torch.equal(out2, out)


def test_a_knn_call_between_the_passes_of_radius_query():
    import torch
    data, queries, r, labels, row = _tie_case()
    other = np.random.default_rng(16).uniform(-0.5, 0.5, (777, 3))       # the knn call searches another cloud, at another radius
    ctx = f3d.default_context()
    want_offs, want_nb = ctx.radius_query(data, queries, r)
    d, q, o = torch.from_numpy(data).cuda(), torch.from_numpy(queries).cuda(), torch.from_numpy(other).cuda()
    stream = _handle(torch)
    offs = torch.empty(len(q) + 1, dtype=torch.int64, device='cuda')
    nnz = ctx.radius_query_dev(d.data_ptr(), f3d.F64, len(d), q.data_ptr(), f3d.F64, len(q), r, offs.data_ptr(), stream)
    idx, d2, counts, _ = _dev_outputs(torch, len(q), 5)
    ctx.knn_query_dev(o.data_ptr(), f3d.F64, len(o), q.data_ptr(), f3d.F64, len(q), 5, 0.21, idx.data_ptr(), d2.data_ptr(), counts.data_ptr(), stream)
    nb = torch.empty(nnz, dtype=torch.int32, device='cuda')
    ctx.radius_query_fill_dev(q.data_ptr(), f3d.F64, len(q), offs.data_ptr(), nb.data_ptr(), stream)
    torch.cuda.synchronize()
    assert np.array_equal(offs.cpu().numpy(), want_offs) and np.array_equal(nb.cpu().numpy(), want_nb)
    _same((idx.cpu().numpy(), d2.cpu().numpy(), counts.cpu().numpy()), R.knn(other, queries, 5, 0.21)[:3])


def test_host_calls_between_the_host_passes_of_both_radius_searches():
    import ctypes as C
    rng = np.random.default_rng(20)
    data, queries, other = rng.uniform(0, 1, (1500, 3)), rng.uniform(0, 1, (900, 3)), rng.uniform(0, 1, (2500, 3))
    labels = rng.integers(-4, 4, 2500)
    r = 0.08
    ctx = f3d.default_context()
    want_graph, want_query = ctx.radius_graph(data, r), ctx.radius_query(data, queries, r)
    lib, h, ptr = ctx._lib, ctx._h, lambda a: C.c_void_p(a.ctypes.data)
    goffs, qoffs = np.zeros(len(data) + 1, np.int64), np.zeros(len(queries) + 1, np.int64)
    gnnz, qnnz = C.c_int64(0), C.c_int64(0)
    assert lib.f3d_radius_graph_count(h, ptr(data), f3d.F64, len(data), r, ptr(goffs), C.byref(gnnz)) == 0
    assert lib.f3d_radius_query_count(h, ptr(data), f3d.F64, len(data), ptr(queries), f3d.F64, len(queries), r, ptr(qoffs), C.byref(qnnz)) == 0
    row = R.knn(other, queries, 9, 0.11)
    _check_both(ctx, other, labels, queries, 9, 0.11, row[:3])         # larger inputs and outputs than the pending searches'
    gnb, qnb = np.empty(gnnz.value, np.int32), np.empty(qnnz.value, np.int32)
    assert lib.f3d_radius_graph_fill(h, len(data), ptr(gnb)) == 0
    assert lib.f3d_radius_query_fill(h, len(queries), ptr(qnb)) == 0
    assert np.array_equal(goffs, want_graph[0]) and np.array_equal(gnb, want_graph[1])
    assert np.array_equal(qoffs, want_query[0]) and np.array_equal(qnb, want_query[1])


def test_strict_context_does_not_allocate_after_reserve_knn():
    import torch
    data, queries, _, labels, _ = _tie_case()
    queries = queries[:500]
    d, q, lab = torch.from_numpy(data).cuda(), torch.from_numpy(queries).cuda(), torch.from_numpy(labels).cuda()
    stream = _handle(torch)
    ctx = f3d.Context(0)
    try:
        ctx.reserve_knn(len(d))
        ctx.set_strict(True)
        before = ctx.alloc_count
        for r in (0.004, 0.3):                            # a fine grid (the cell table at its cap) and a coarse one
            idx, d2, counts, out = _dev_outputs(torch, len(q), 8)
            ctx.knn_query_dev(d.data_ptr(), f3d.F64, len(d), q.data_ptr(), f3d.F64, len(q), 8, r, idx.data_ptr(), d2.data_ptr(), counts.data_ptr(),
                              stream)
            ctx.transfer_labels_dev(d.data_ptr(), f3d.F64, len(d), lab.data_ptr(), q.data_ptr(), f3d.F64, len(q), 8, r, FILL, out.data_ptr(), None,
                                    stream)
            torch.cuda.synchronize()
            want = R.knn(data, queries, 8, r)
            _same((idx.cpu().numpy(), d2.cpu().numpy(), counts.cpu().numpy()), want[:3])
            assert np.array_equal(out.cpu().numpy(), R.plurality(want[0], labels, FILL)[0])
        assert ctx.alloc_count == before
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ transfer (public surface)
def test_k1_is_the_nearest_points_label_and_empty_rows_get_fill():
    data, queries, r, _, row = _tie_case()
    rng = np.random.default_rng(17)
    labels = PALETTE[rng.integers(0, len(PALETTE), len(data))]
    queries = np.concatenate([queries[:1500], queries[:40] + 7.0])
    idx, _, counts = transfer.nearest_points(data, queries, r, k=1)
    out, support = transfer.transfer_labels(data, labels, queries, r, k=1, fill=-99, return_support=True)
    assert out.dtype == np.int64 and support.dtype == np.int32
    assert np.array_equal(out[:1500], labels[idx[:1500, 0]]) and (support[:1500] == 1).all()
    assert (out[1500:] == -99).all() and (support[1500:] == 0).all() and (counts[1500:] == 0).all()
    assert (labels < 0).any() and (labels >= 2 ** 33).any()


def test_label_dtypes_round_trip_and_bool_stays_bool():
    import torch
    data, queries, r, labels, row = _tie_case()
    queries = np.concatenate([queries[:800], queries[:20] + 7.0])
    want, _ = R.transfer(data, labels, queries, 5, r, fill=3)
    for dt in (np.int32, np.uint8, np.int64):
        got = transfer.transfer_labels(data, labels.astype(dt), queries, r, k=5, fill=3)
        assert got.dtype == dt and np.array_equal(got, want.astype(dt))
    bits = labels >= 2
    wbits, _ = R.transfer(data, bits.astype(np.int64), queries, 5, r, fill=1)
    got = transfer.transfer_labels(data, bits, queries, r, k=5, fill=7)               # fill coerced: bool(7)
    assert got.dtype == bool and np.array_equal(got, wbits.astype(bool)) and got[800:].all()
    tgot, tsup = transfer.transfer_labels(torch.from_numpy(data).cuda(), torch.from_numpy(bits).cuda(), torch.from_numpy(queries).cuda(), r, k=5,
                                          fill=7, return_support=True)
    assert tgot.is_cuda and tgot.dtype == torch.bool and tsup.dtype == torch.int32
    assert np.array_equal(tgot.cpu().numpy(), got)
    t32 = transfer.transfer_labels(torch.from_numpy(data).cuda(), torch.from_numpy(labels.astype(np.int32)).cuda(), queries, r, k=5, fill=3)
    assert t32.is_cuda and t32.dtype == torch.int32 and np.array_equal(t32.cpu().numpy(), want.astype(np.int32))
    tidx, td2, tcnt = transfer.nearest_points(torch.from_numpy(data).cuda(), torch.from_numpy(queries).cuda(), r, k=5)
    _same((tidx.cpu().numpy(), td2.cpu().numpy(), tcnt.cpu().numpy()), R.knn(data, queries, 5, r)[:3])


def test_labels_no_query_reaches_do_not_matter():
    rng = np.random.default_rng(18)
    data = rng.uniform(0, 1, (3000, 3))
    queries = rng.uniform(0, 0.5, (500, 3))
    labels = rng.integers(0, 5, 3000)
    k, r = 8, 0.08
    reached = np.zeros(3000, bool)
    idx = R.knn(data, queries, k, r)[0]
    reached[idx[idx >= 0]] = True
    assert (~reached).sum() > 1000
    poisoned = np.where(reached, labels, np.int64(-2 ** 62))
    ctx = f3d.default_context()
    a = ctx.transfer_labels(data, labels, queries, k, r, fill=FILL)
    b = ctx.transfer_labels(data, poisoned, queries, k, r, fill=FILL)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.array_equal(a[0], R.plurality(idx, labels, FILL)[0])


# ------------------------------------------------------------------------------------------------ mesh route
@functools.lru_cache(maxsize=None)
def _mesh_case():
    s, g = 0.01, 60
    ii, jj = np.meshgrid(np.arange(g), np.arange(g), indexing='ij')
    cloud = np.stack([ii.ravel() * s, jj.ravel() * s, np.zeros(g * g)], 1)
    remove = cloud[:, 0] < 0.5 * (g - 1) * s                                   # a half-plane
    grid_v = cloud + np.array([0.4 * s, 0.4 * s, 0.0])
    v = lambda i, j: i * g + j
    a, b = ii[:-1, :-1].ravel(), jj[:-1, :-1].ravel()
    tris = np.concatenate([np.stack([v(a, b), v(a + 1, b), v(a, b + 1)], 1), np.stack([v(a + 1, b), v(a + 1, b + 1), v(a, b + 1)], 1)])
    assert len(tris) == 2 * 59 * 59
    patch_v = np.array([[0, 0, 1.0], [s, 0, 1.0], [0, s, 1.0], [s, s, 1.0]]) + np.array([0.1, 0.1, 0.0])     # farther than r away
    patch_t = np.array([[0, 1, 2], [1, 3, 2]]) + g * g
    rng = np.random.default_rng(19)
    tris = rng.permutation(np.concatenate([tris, patch_t]))
    return cloud, remove, np.concatenate([grid_v, patch_v]), tris.astype(np.int64), s


@pytest.mark.parametrize('k,rs', [(1, 0.7), (4, 1.3)])
def test_mesh_route_on_device_tensors(k, rs):
    import torch
    cloud, remove, verts, tris, s = _mesh_case()
    r = rs * s
    tc, tr, tv, tt = (torch.from_numpy(x).cuda() for x in (cloud, remove, verts, tris))
    for unmatched in (False, True):
        want = R.transfer(cloud, remove.astype(np.int64), verts, k, r, fill=int(unmatched))[0].astype(bool)
        got = transfer.vertex_mask_from_points(tc, tr, tv, r, k=k, unmatched=unmatched)
        assert got.is_cuda and got.dtype == torch.bool and np.array_equal(got.cpu().numpy(), want)
        assert (want[-4:] == unmatched).all() and 1000 < want[:-4].sum() < 2600
        assert np.array_equal(transfer.vertex_mask_from_points(cloud, remove, verts, r, k=k, unmatched=unmatched), want)
    want_mask = R.transfer(cloud, remove.astype(np.int64), verts, k, r, fill=0)[0].astype(bool)
    got = transfer.clean_mesh_by_points(tv, tt, tc, tr, r, k=k, min_triangles=3)
    want = meshUtils.clean_mesh(tv, tt, torch.from_numpy(want_mask).cuda(), min_triangles=3)
    assert len(got) == 4 and all(g.is_cuda for g in got)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and torch.equal(g, w)
    assert not got[2][-4:].any() and 0 < got[3].sum() < len(tris)              # the 2-triangle patch is a small fragment
    # the masks feed the face filters as they are
    nr, rem, _ = meshUtils.remove_faces_by_vertices(len(verts), tt, transfer.vertex_mask_from_points(tc, tr, tv, r, k=k))
    assert torch.equal(nr, ~torch.from_numpy(want_mask).cuda()[tt].any(dim=1))
    kv, kt = meshUtils.keep_faces_by_vertices(tv, tt, transfer.vertex_mask_from_points(tc, tr, tv, r, k=k))
    assert len(kt) == int(torch.from_numpy(want_mask).cuda()[tt].any(dim=1).sum())
