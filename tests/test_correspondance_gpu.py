"""segUtils.correspondance on the GPU: the radius query (f3d_radius_query_*) against the reference's golden and against sklearn's
KDTree inverted by a stable sort, rows compared in order; host entries against _dev entries; the count -> other call -> fill
interleaving; the device-resident path from depth frames to PointCorrespondance on tensors; degenerate clouds through all three
callers of the shared grid walk (radius graph, radius query, point vote)."""
import ctypes as C

import numpy as np
import pytest
from sklearn.neighbors import KDTree

import f3d
from Fusion3DSeg.segUtils.correspondance import PointCorrespondance

pytestmark = pytest.mark.gpu


def _sklearn_csr(sparse, dense, r):
    """KDTree(dense, leaf_size=2).query_radius(sparse, r) inverted per dense point, sparse indices ascending (a stable sort)."""
    nb = KDTree(dense, leaf_size=2).query_radius(sparse, r=r)
    sp = np.repeat(np.arange(len(sparse), dtype=np.int64), [len(x) for x in nb])
    dn = np.concatenate(nb).astype(np.int64) if len(nb) else np.zeros(0, np.int64)
    order = np.argsort(dn, kind='stable')
    offs = np.zeros(len(dense) + 1, np.int64)
    np.cumsum(np.bincount(dn, minlength=len(dense)), out=offs[1:])
    return offs, sp[order].astype(np.int32)


def _check(sparse, dense, r, ctx=None):
    ctx = ctx or f3d.default_context()
    got = ctx.radius_query(sparse, dense, r)
    want = _sklearn_csr(sparse, dense, r)
    assert np.array_equal(got[0], want[0]) and got[0].dtype == np.int64
    assert np.array_equal(got[1], want[1]) and got[1].dtype == np.int32
    return got


def test_golden_merge_maps_and_get_point(golden):
    g = golden('correspondance')
    F, h, w = (int(x) for x in g['a_hw'])
    pc = PointCorrespondance(g['a_sparse'], g['a_dense'], float(g['a_radius']), F, (h, w))
    assert np.array_equal(pc.csr.offsets, g['a_offsets']) and np.array_equal(pc.csr.indices, g['a_indices'])
    assert pc.merge_maps.ndim == int(g['a_ndim'])
    idx, freq = pc.get_point(g['a_images'], g['a_coords'])
    assert idx.dtype == g['a_point_indices'].dtype and np.array_equal(idx, g['a_point_indices'])
    assert freq.dtype == g['a_point_frequency'].dtype and np.array_equal(freq, g['a_point_frequency'])
    lens = np.diff(g['a_offsets'])
    assert lens.max() > 32                                             # rows past the in-thread sort (the clump at camera 1)
    mb = PointCorrespondance.get_merge_maps(g['b_sparse'], g['b_dense'], 0.0)
    assert mb.ndim == int(g['b_ndim']) == 2 and mb.shape == tuple(g['b_shape'])
    assert np.array_equal(mb.astype(np.int64).reshape(-1), g['b_indices'])


def _quantised(rng, n, m, span=2.0):
    dense = np.round(rng.uniform(-span, span, (n, 3)) * 64) / 64
    sparse = np.round(rng.uniform(-span, span, (m, 3)) * 64) / 64
    return sparse, dense


@pytest.mark.parametrize('k', [1, 3, 8])
def test_quantised_lattice_ties_are_inclusive(k):
    rng = np.random.default_rng(k)
    sparse, dense = _quantised(rng, 20000, 30000, span=1.0)
    offs, nb = _check(sparse, dense, k / 64)
    d = dense[np.repeat(np.arange(len(dense)), np.diff(offs))] - sparse[nb]
    assert (((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) == (k / 64) ** 2).sum() > 100   # exactly on r*r


def test_dropouts_at_camera_centres_and_a_clump():
    rng = np.random.default_rng(7)
    sparse, dense = _quantised(rng, 40000, 20000)
    cams = np.array([[0.0, 0.0, 0.0], [0.5, 0.25, -0.125], [1.0, -0.5, 0.75]])
    drop = rng.random(len(dense)) < 0.15
    dense[drop] = cams[rng.integers(0, 3, drop.sum())]
    clump = cams[1] + rng.normal(0, 0.01, (3000, 3))                    # > 1000 cloud points within r of the dropout pixels
    sparse = np.concatenate([sparse[:10000], clump, sparse[10000:]])
    offs, nb = _check(sparse, dense, 0.05)
    assert np.diff(offs).max() > 2500 and np.diff(offs)[drop].min() >= 0


def test_a_row_longer_than_the_lds_sort():
    rng = np.random.default_rng(8)
    sparse = rng.normal(0, 0.02, (20000, 3))
    dense = np.concatenate([np.zeros((5, 3)), rng.uniform(-1, 1, (2000, 3))])
    offs, _ = _check(sparse, dense, 0.5)
    assert np.diff(offs)[:5].min() > 8192


def test_float32_inputs_are_widened_exactly():
    rng = np.random.default_rng(9)
    sparse, dense = _quantised(rng, 20000, 20000)
    s32 = (sparse + rng.normal(0, 1e-3, sparse.shape)).astype(np.float32)
    d32 = (dense + rng.normal(0, 1e-3, dense.shape)).astype(np.float32)
    ctx = f3d.default_context()
    for s, d in ((s32, d32), (s32, dense), (sparse, d32)):
        got = ctx.radius_query(s, d, 0.07)
        want = _sklearn_csr(s.astype(np.float64), d.astype(np.float64), 0.07)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_queries_far_outside_the_cloud_and_radius_edges():
    rng = np.random.default_rng(10)
    sparse, dense = _quantised(rng, 5000, 5000)
    far = np.concatenate([dense, dense[:500] + [40.0, 0.0, 0.0], dense[:500] * 1e6])
    _check(sparse, far, 0.1)
    dup = np.concatenate([sparse[:100], sparse[:100]])
    offs, nb = _check(sparse, dup, 0.0)                                 # r = 0: exact duplicates only
    assert (np.diff(offs) >= 1).all()
    ctx = f3d.default_context()
    for r in (-0.1, float('nan')):
        offs, nb = ctx.radius_query(sparse, dense, r)
        assert (offs == 0).all() and len(nb) == 0
    with pytest.raises(ValueError):
        ctx.radius_query(sparse, dense, float('inf'))
    for bad in (np.nan, np.inf, -np.inf):
        q = dense.copy()
        q[17, 1] = bad
        with pytest.raises(ValueError):
            ctx.radius_query(sparse, q, 0.1)                            # flagged by the count pass
        with pytest.raises(ValueError):
            ctx.radius_query(q, dense, 0.1)                             # the data's bounding box
    with pytest.raises(ValueError):
        ctx.radius_query(np.zeros((0, 3)), dense, 0.1)
    offs, nb = ctx.radius_query(sparse, np.zeros((0, 3)), 0.1)
    assert list(offs) == [0] and len(nb) == 0


def _degenerate_clouds():
    rng = np.random.default_rng(14)
    flat = np.concatenate([rng.uniform(0, 100, (4000, 2)), np.zeros((4000, 1))], axis=1)
    lattice = np.stack(np.meshgrid(np.arange(9.0), np.arange(7.0), np.arange(5.0), indexing='ij'), -1).reshape(-1, 3)
    return {'one_point': (np.array([[0.25, -1.5, 3.0]]), 0.1),
            'identical_points': (np.tile([[0.5, -0.25, 2.0]], (70, 1)), 0.05),                # a 1 x 1 x 1 grid
            'flat': (flat, 2.5),                                                               # one axis has dim 1
            'lattice_r1': (lattice, 1.0),                                                      # ties exactly on r * r, points on
            'lattice_sqrt2': (lattice, float(np.sqrt(2.0))),                                   # the upper faces of the box
            'offset': (rng.uniform(0, 1, (3000, 3)) + [1e6, -2e6, 3e5], 0.08)}


@pytest.mark.parametrize('name', list(_degenerate_clouds()))
def test_degenerate_clouds_through_graph_query_and_vote(name):
    P, r = _degenerate_clouds()[name]
    n, ncols = len(P), 6
    ctx = f3d.default_context()
    want = [np.sort(row) for row in KDTree(P).query_radius(P, r)]
    want_offs = np.concatenate([[0], np.cumsum([len(row) for row in want])])
    goffs, gnb = ctx.radius_graph(P, r)
    qoffs, qnb = ctx.radius_query(P, P, r)
    assert np.array_equal(goffs, qoffs) and np.array_equal(qoffs, want_offs)
    graph_rows = np.concatenate([np.sort(gnb[goffs[i]:goffs[i + 1]]) for i in range(n)])
    assert np.array_equal(graph_rows, qnb) and np.array_equal(qnb, np.concatenate(want))
    labels = (np.arange(n) % 5).astype(np.uint8)
    expect = np.zeros((n, ncols))
    for j, row in enumerate(want):                                      # row j: the pixels within r of point j (the relation is symmetric)
        expect[j, labels[row]] = 1
    expect[:, -1] = 1                                                   # every point is its own neighbour
    votes = ctx.point_vote_frames(np.zeros((n, ncols)), P, P[None], labels[None], r)
    assert np.array_equal(votes, expect)


def test_host_entries_equal_dev_entries():
    import torch
    ctx = f3d.default_context()
    dev = torch.device('cuda', ctx.device)
    rng = np.random.default_rng(11)
    sparse, dense = _quantised(rng, 30000, 20000)
    want = ctx.radius_query(sparse, dense.astype(np.float32), 0.09)
    s = torch.from_numpy(sparse).to(dev)
    d = torch.from_numpy(dense.astype(np.float32)).to(dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    offs = torch.empty(len(d) + 1, dtype=torch.int64, device=dev)
    nnz = ctx.radius_query_dev(s.data_ptr(), f3d.F64, len(s), d.data_ptr(), f3d.F32, len(d), 0.09, offs.data_ptr(), stream)
    nb = torch.empty(nnz, dtype=torch.int32, device=dev)
    ctx.radius_query_fill_dev(d.data_ptr(), f3d.F32, len(d), offs.data_ptr(), nb.data_ptr(), stream)
    torch.cuda.synchronize(dev)
    assert nnz == want[0][-1] and np.array_equal(offs.cpu().numpy(), want[0]) and np.array_equal(nb.cpu().numpy(), want[1])
    with pytest.raises(ValueError):                                    # the fill must name the counted queries
        ctx.radius_query_fill_dev(s.data_ptr(), f3d.F64, len(d), offs.data_ptr(), nb.data_ptr(), stream)


def test_count_then_other_calls_then_fill():
    ctx = f3d.Context(f3d.default_context().device)
    lib = ctx._lib
    rng = np.random.default_rng(12)
    sparse, dense = _quantised(rng, 20000, 15000)
    want = _sklearn_csr(sparse, dense, 0.08)

    def count():
        offs = np.zeros(len(dense) + 1, np.int64)
        nnz = C.c_int64(0)
        ctx._check(lib.f3d_radius_query_count(ctx._h, sparse.ctypes.data, f3d.F64, len(sparse), dense.ctypes.data, f3d.F64, len(dense),
                                              0.08, offs.ctypes.data, C.byref(nnz)))
        return offs, np.empty(nnz.value, np.int32)
    offs, nb = count()
    # entries that use the staging buffers and the radius graph's scratch, and the patch entries (nine staging buffers)
    other = rng.uniform(-1, 1, (50000, 3))
    ctx.radius_graph(other, 0.05)
    ctx.rotate(other, [1.0, 0.0, 0.0, 0.0])
    h, w = 16, 16
    pts = rng.uniform(0, 1, (h * w, 3))
    ctx.patch_seeds_sums(pts, np.tile([0.0, 0.0, 1.0], (h * w, 1)), pts, np.arange(h * w)[::-1], np.ones(h * w, np.uint8), h, w, 1, 0.1, 0.5)
    ctx._check(lib.f3d_radius_query_fill(ctx._h, len(dense), nb.ctypes.data))
    assert np.array_equal(offs, want[0]) and np.array_equal(nb, want[1])
    offs, nb = count()
    ctx.radius_query(other[:1000], other[1000:3000], 0.2)              # another query replaces the state: the fill is refused
    with pytest.raises(ValueError):
        ctx._check(lib.f3d_radius_query_fill(ctx._h, len(dense), nb.ctypes.data))
    ctx.close()


def test_device_path_end_to_end():
    """depth -> frames_world_dev -> Fusion.from_frames(...).fuse_device -> PointCorrespondance on tensors == the host path."""
    import torch
    from RTAB_utils import ios_rtab
    from Fusion3DSeg.fusion import Fusion
    dev = torch.device('cuda', f3d.default_context().device)
    F, H, W = 4, 48, 64
    K = np.array([[52.5, 0.0, 32.0], [0.0, 52.5, 24.0], [0.0, 0.0, 1.0]])
    rng = np.random.default_rng(13)
    v = np.arange(H, dtype=np.float64)[:, None] + np.zeros((1, W))
    with np.errstate(divide='ignore'):
        d = np.minimum(2.5, np.where(v > 24.5, 52.5 * 1.0 / (v - 24.0), np.inf))
    depth = np.stack([np.round(d * 1000 + rng.normal(0, 1.0, d.shape)).astype(np.uint16) for _ in range(F)])
    depth[rng.random(depth.shape) < 0.1] = 0                            # dropouts: their points sit at the camera centres
    odo_xyzw = np.tile([0.0, 0.0, 0.0, 1.0], (F, 1))
    odo_xyz = np.stack([[0.03 * j, 0.0, 0.0] for j in range(F)])
    pts, nrm = ios_rtab.frames_world_dev(depth, K, odo_xyzw, odo_xyz)
    clr = torch.from_numpy(rng.uniform(0, 1, (F, H * W, 3))).to(dev)
    valid = torch.from_numpy((depth > 0).reshape(F, -1).astype(np.uint8)).to(dev)
    frames = [(str(j), pts[j], nrm[j], clr[j], valid[j]) for j in range(F)]
    np.random.seed(3)
    cloud = Fusion.from_frames(K, W, H, odo_xyzw[:, [3, 0, 1, 2]], odo_xyz, frames).fuse_device()[0]
    assert cloud.is_cuda and len(cloud) > 100
    dense = pts.reshape(-1, 3)
    pc = PointCorrespondance(cloud, dense, 0.05, F, (H, W))
    host = PointCorrespondance(cloud.cpu().numpy(), dense.cpu().numpy(), 0.05, F, (H, W))
    assert pc.csr.offsets.is_cuda and pc.pcdimgs.is_cuda and pc.pcd2xy.is_cuda and pc.imgids.is_cuda
    for a, b in zip(pc.csr, host.csr):
        assert np.array_equal(a.cpu().numpy(), b)
    for a, b in ((pc.pcdimgs, host.pcdimgs), (pc.pcd2xy, host.pcd2xy), (pc.imgids, host.imgids)):
        a = a.cpu().numpy()
        assert a.dtype == b.dtype and np.array_equal(a, b)
    images = np.array([0, 3, -1, 2, 1])
    coords = np.array([[0, 0], [63, 47], [-1, -2], [32, 30], [10, 40]])
    gi, gf = pc.get_point(torch.from_numpy(images).to(dev), torch.from_numpy(coords).to(dev))
    hi, hf = host.get_point(images, coords)
    assert gi.is_cuda and gi.dtype == torch.int32 and gf.dtype == torch.int64
    assert np.array_equal(gi.cpu().numpy(), hi) and np.array_equal(gf.cpu().numpy(), hf) and hf.sum() > 0
    with pytest.raises(IndexError):
        pc.get_point(torch.tensor([0], device=dev), torch.tensor([[W, 0]], device=dev))
    bad = dense.clone()
    bad[5, 0] = float('nan')
    with pytest.raises(ValueError):
        PointCorrespondance(cloud, bad, 0.05, F, (H, W))
