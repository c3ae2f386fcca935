"""CVSegmentation on the GPU (f3d_flood_order, f3d_color_segment): bit-exact against the reference golden and, at ~200k points,
against the restatement tests/cvseg_ref.py."""
import copy

import numpy as np
import pytest

import f3d
import cvseg_ref as R

pytestmark = pytest.mark.gpu


def _graph(g, gi):
    offs, nb = g[f'g{gi}_offsets'], g[f'g{gi}_neighbours']
    return g[f'g{gi}_classes'], [nb[offs[i]:offs[i + 1]] for i in range(len(offs) - 1)], (offs, nb)


def test_instance_seperate_matches_reference_golden(golden):
    from Fusion3DSeg.segUtils.cv import CVSegmentation
    g = golden('cvseg')
    for k in range(int(g['nicases'])):
        cls, rows, csr = _graph(g, int(g[f'i{k}_graph']))
        ic = g[f'i{k}_instance_classes'].tolist() if g[f'i{k}_has_instance_classes'] else None
        for adj in (rows, csr):
            mine = cls.copy()
            seg = CVSegmentation(mine, adj)
            got = seg.instance_seperate(ic, int(g[f'i{k}_minimum_points']))
            R.same_instances(got, R.decode_instances(g, f'i{k}_'))
            assert np.array_equal(mine, g[f'i{k}_classes_after']), k         # the caller's classes, rewritten in place
            assert seg.floods and all(f.stats['levels'] >= 1 for f in seg.floods)


def test_color_segment_matches_reference_golden(golden):
    from Fusion3DSeg.segUtils.cv import CVSegmentation
    g = golden('cvseg')
    for k in range(int(g['nccases'])):
        cls, rows, csr = _graph(g, int(g[f'c{k}_graph']))
        thr = float(g[f'c{k}_threshold']) if g[f'c{k}_threshold_is_scalar'] else tuple(g[f'c{k}_threshold'])
        for adj in (rows, csr):
            ids = g[f'c{k}_ids_in'].copy()
            out = CVSegmentation(cls.copy(), adj).color_segment(g[f'c{k}_colors'], ids, g[f'c{k}_seeds'], thr,
                                                                tuple(g[f'c{k}_neutral_ids'].tolist()), int(g[f'c{k}_max_level']))
            assert out is ids and np.array_equal(ids, g[f'c{k}_ids_out']), k


def _scene(seed=5):
    from fusion_scenes import curved_capture
    from scipy.spatial import cKDTree
    _, _, _, frames = curved_capture(300, 400, 2, seed)
    pts = np.concatenate([p[v & np.isfinite(p).all(1)] for _, p, _, _, v in frames])
    clr = np.concatenate([c[v & np.isfinite(p).all(1)] for _, p, _, c, v in frames]).astype(np.float64)
    pts = pts[:200_000]
    clr = clr[:200_000]
    d, _ = cKDTree(pts[::50]).query(pts[::50], k=2)
    r = float(np.median(d[:, 1])) * 0.6                              # ~ 10-20 neighbours at full density
    s = 0.35
    q = np.floor(pts / s).astype(np.int64)
    cls = ((q[:, 0] + 2 * q[:, 1] + 3 * q[:, 2]) % 4).astype(np.int64)  # spatial blobs: hundreds of clusters, some tiny
    return pts, clr, cls, r


def test_large_scene_matches_restatement():
    from Fusion3DSeg.fusion import radius_adjacency
    from Fusion3DSeg.segUtils.cv import CVSegmentation
    pts, clr, cls, r = _scene()
    offs, nb = radius_adjacency(pts, r / 2, as_csr=True)
    deg = np.diff(offs)
    assert 4 < deg.mean() < 80, deg.mean()
    for ic, mp in ((None, 1), ([3, 1, 0], 40)):
        want_cls, mine = cls.copy(), cls.copy()
        want = R.instance_seperate(want_cls, (offs, nb), ic, mp)
        seg = CVSegmentation(mine, (offs, nb))
        got = seg.instance_seperate(ic, mp)
        assert np.array_equal(mine, want_cls)
        R.same_instances(got, (len(want[0]), want[1], want[2], want[3], list(want[4])))
        assert len(got[3]) > 10
        print(f'{len(cls)} points, {len(got[3])} clusters, floods {[f.stats for f in seg.floods]}')
    ids = got[1].copy()
    ids[np.isin(ids, [i for i, d in enumerate(got[2]) if d['category_id'] in (1, 2)])] = 0      # a neutral region
    touch = np.add.reduceat((ids == 0)[nb].astype(np.int64), offs[:-1]) > 0                      # rows are never empty (self)
    seeds = np.random.default_rng(1).choice(np.nonzero((ids != 0) & touch)[0], 40, replace=False)
    clr = (clr - clr.min(0)) / np.maximum(clr.max(0) - clr.min(0), 1e-12)
    for dt, thr, ml in ((np.float64, 0.2, 10), (np.float32, (0.25, 0.2, 0.3), 25)):
        c = clr.astype(dt)
        want = R.color_segment(None, (offs, nb), c, ids.copy(), seeds, thr, (0,), ml)
        got_ids = CVSegmentation(cls.copy(), (offs, nb)).color_segment(c, ids.copy(), seeds, thr, (0,), ml)
        assert np.array_equal(got_ids, want)
        assert (want != ids).sum() > 50


def _dev_inputs(g, k):
    import torch
    cls, rows, (offs, nb) = _graph(g, int(g[f'i{k}_graph']))
    return (torch.as_tensor(cls, device='cuda'), torch.as_tensor(offs, device='cuda'), torch.as_tensor(nb.astype(np.int32), device='cuda'))


def test_dev_paths_under_sync_debug_and_strict_context(golden):
    import torch
    g = golden('cvseg')
    cls, rows, (offs, nb) = _graph(g, 0)
    n = len(cls)
    host = f3d.default_context()
    want = host.flood_order(cls, offs, nb, [5, 7, 0, 9])
    cc = host.color_segment(g['c0_colors'], offs, nb, g['c0_ids_in'].copy(), g['c0_seeds'], 0.3, (0,), 10)[0]
    ctx = f3d.Context(0)
    ctx.reserve_cvseg(n)
    dc, do, dn = (torch.as_tensor(cls, device='cuda'), torch.as_tensor(offs, device='cuda'),
                  torch.as_tensor(nb.astype(np.int32), device='cuda'))
    root, order = torch.empty(n, dtype=torch.int64, device='cuda'), torch.empty(n, dtype=torch.int64, device='cuda')
    coffs, flags = torch.empty(n + 1, dtype=torch.int64, device='cuda'), torch.empty(n, dtype=torch.uint8, device='cuda')
    clr = torch.as_tensor(g['c0_colors'], device='cuda')
    ids = torch.as_tensor(g['c0_ids_in'].copy(), device='cuda')
    seeds = torch.as_tensor(g['c0_seeds'], device='cuda')
    acc = torch.zeros(1, dtype=torch.int64, device='cuda')
    st = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    ctx.set_strict(True)
    before = ctx.alloc_count
    torch.cuda.set_sync_debug_mode('error')
    try:
        stats = ctx.flood_order_dev(dc.data_ptr(), n, do.data_ptr(), dn.data_ptr(), [5, 7, 0, 9], root.data_ptr(), order.data_ptr(),
                                    coffs.data_ptr(), flags.data_ptr(), st)
        ctx.color_segment_dev(clr.data_ptr(), f3d.F64, n, do.data_ptr(), dn.data_ptr(), ids.data_ptr(), seeds.data_ptr(), len(seeds), 0.3,
                              (0,), 10, acc.data_ptr(), st)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert ctx.alloc_count == before
    ctx.take_device_error(st)
    m, L = stats['clusters'], stats['points']
    assert np.array_equal(root.cpu().numpy(), want[0]) and np.array_equal(order[:L].cpu().numpy(), want[1])
    assert np.array_equal(coffs[:m + 1].cpu().numpy(), want[2]) and np.array_equal(flags.cpu().numpy().astype(bool), want[3])
    assert np.array_equal(ids.cpu().numpy(), cc) and int(acc.item()) > 0
    with pytest.raises(MemoryError):                                     # a larger cloud than reserved: no silent allocation
        ctx.flood_order_dev(dc.data_ptr(), n, do.data_ptr(), dn.data_ptr(), list(range(5000)), root.data_ptr(), order.data_ptr(),
                            coffs.data_ptr(), flags.data_ptr(), st)
    ctx.close()


def test_device_tensors_stay_on_device(golden):
    import torch
    from Fusion3DSeg.segUtils.cv import CVSegmentation
    g = golden('cvseg')
    for k in (2, 4):
        dc, do, dn = _dev_inputs(g, k)
        ic = g[f'i{k}_instance_classes'].tolist()
        got = CVSegmentation(dc, (do, dn)).instance_seperate(ic, int(g[f'i{k}_minimum_points']))
        n, ids, info, clusters, bnds = R.decode_instances(g, f'i{k}_')
        assert got[1].is_cuda and np.array_equal(got[1].cpu().numpy(), ids) and got[2] == info
        assert all(c.is_cuda and np.array_equal(c.cpu().numpy(), w) for c, w in zip(got[3], clusters))
        assert all(R.same_boundary(got[4][i], bnds[i]) for i in range(len(bnds)))
        assert np.array_equal(dc.cpu().numpy(), g[f'i{k}_classes_after'])
    cls, rows, (offs, nb) = _graph(g, int(g['c5_graph']))
    ids = torch.as_tensor(g['c5_ids_in'].copy(), device='cuda')
    out = CVSegmentation(torch.as_tensor(cls, device='cuda'), (torch.as_tensor(offs, device='cuda'), torch.as_tensor(nb, device='cuda'))) \
        .color_segment(torch.as_tensor(g['c5_colors'], device='cuda'), ids, torch.as_tensor(g['c5_seeds'], device='cuda'),
                       float(g['c5_threshold']) if g['c5_threshold_is_scalar'] else tuple(g['c5_threshold']),
                       tuple(g['c5_neutral_ids'].tolist()), int(g['c5_max_level']))
    assert out is ids and np.array_equal(ids.cpu().numpy(), g['c5_ids_out'])


def test_interleaved_with_components_and_split_into_instances(golden):
    from Fusion3DSeg.segUtils.cv import CVSegmentation, split_into_instances
    g = golden('cvseg')
    sp = golden('split_instances')
    soffs, sflat = sp['adj_offsets'], sp['adj_flat']
    sadj = [sflat[soffs[i]:soffs[i + 1]] for i in range(len(soffs) - 1)]
    ctx = f3d.default_context()
    cls, rows, (offs, nb) = _graph(g, 1)
    root0 = ctx.components_same_class(cls, offs, nb)
    split0 = split_into_instances(sp['classes'], sadj, 133, [86, 114, 115], 5)
    for k in range(int(g['nicases'])):
        c2, rows2, _ = _graph(g, int(g[f'i{k}_graph']))
        ic = g[f'i{k}_instance_classes'].tolist() if g[f'i{k}_has_instance_classes'] else None
        R.same_instances(CVSegmentation(c2.copy(), rows2).instance_seperate(ic, int(g[f'i{k}_minimum_points'])),
                        R.decode_instances(g, f'i{k}_'))
        assert np.array_equal(ctx.components_same_class(cls, offs, nb), root0)
        s = split_into_instances(sp['classes'], sadj, 133, [86, 114, 115], 5)
        assert np.array_equal(s[1], split0[1]) and np.array_equal(s[3], split0[3]) and s[2] == split0[2]


def test_bad_indices_raise_for_their_own_operation(golden):
    g = golden('cvseg')
    cls, rows, (offs, nb) = _graph(g, 0)
    ctx = f3d.default_context()
    bad = nb.astype(np.int32).copy()
    bad[7] = len(cls) + 5
    with pytest.raises(IndexError, match='flood_order'):
        ctx.flood_order(cls, offs, bad, [5, 7])
    ids = g['c0_ids_in'].copy()
    with pytest.raises(IndexError, match='color_segment'):
        ctx.color_segment(g['c0_colors'], offs, nb, ids, [len(cls) + 1], 0.3)
    root = ctx.components_same_class(cls, offs, nb)                    # the context is clean afterwards
    assert np.array_equal(root, ctx.flood_order(cls, offs, nb, [5])[0])


def test_color_segment_neighbour_index_error_comes_from_the_kernel(golden):
    """A bad neighbour index in a row the flood expands is found inside the kernel (its own error bit), on both paths."""
    import torch
    from Fusion3DSeg.segUtils.cv import CVSegmentation
    g = golden('cvseg')
    cls, rows, (offs, nb) = _graph(g, int(g['c0_graph']))
    seed = int(g['c0_seeds'][0])
    bad = nb.astype(np.int32).copy()
    bad[offs[seed]] = len(cls) + 9                                      # the seed is accepted, so its row is walked
    ctx = f3d.default_context()
    ids = g['c0_ids_in'].copy()
    with pytest.raises(IndexError, match='color_segment'):
        ctx.color_segment(g['c0_colors'], offs, bad, ids, [seed], 0.3)
    assert np.array_equal(ids, g['c0_ids_in'])                         # the host entry writes nothing back on an IndexError
    dids = torch.as_tensor(g['c0_ids_in'].copy(), device='cuda')
    seg = CVSegmentation(torch.as_tensor(cls, device='cuda'), (torch.as_tensor(offs, device='cuda'), torch.as_tensor(bad, device='cuda')))
    with pytest.raises(IndexError, match='color_segment'):
        seg.color_segment(torch.as_tensor(g['c0_colors'], device='cuda'), dids, [seed], 0.3)
    with pytest.raises(ValueError, match='colours'):                   # a colour tensor of the wrong shape never reaches the kernel
        seg.color_segment(torch.zeros((len(cls) - 1, 3), dtype=torch.float64, device='cuda'), dids, [seed], 0.3)
    root = ctx.components_same_class(cls, offs, nb)                    # the context is clean afterwards
    assert np.array_equal(root, ctx.flood_order(cls, offs, nb, [5])[0])


def test_device_path_on_a_side_stream_follows_the_callers_work(golden):
    """Device inputs written by torch just before the call (no synchronisation in between) are the ones the kernels read."""
    import torch
    from Fusion3DSeg.segUtils.cv import CVSegmentation
    g = golden('cvseg')
    k = 2
    cls, rows, (offs, nb) = _graph(g, int(g[f'i{k}_graph']))
    dc = torch.full((len(cls),), 77, dtype=torch.int64, device='cuda')
    for _ in range(3):
        dc.add_(0)
    dc.copy_(torch.as_tensor(cls, device='cuda'))                     # enqueued on the caller's stream
    got = CVSegmentation(dc, (torch.as_tensor(offs, device='cuda'), torch.as_tensor(nb.astype(np.int32), device='cuda'))) \
        .instance_seperate(g[f'i{k}_instance_classes'].tolist(), int(g[f'i{k}_minimum_points']))
    n, ids, info, clusters, bnds = R.decode_instances(g, f'i{k}_')
    assert np.array_equal(got[1].cpu().numpy(), ids) and got[2] == info
    assert np.array_equal(dc.cpu().numpy(), g[f'i{k}_classes_after'])
