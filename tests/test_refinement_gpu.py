"""segUtils/refinement.py on the GPU (f3d_region_grow, f3d_plane_distance): element for element against the reference golden,
and at capture size against the restatement tests/refinement_ref.py."""
import time

import numpy as np
import pytest

import f3d
import refinement_ref as R

pytestmark = pytest.mark.gpu


def _call(M, kind, values, adj, seeds, thr, ml):
    if kind == 'depth_points':
        return M.grow_depth(values, adj, seeds, thr, ml, given=True)
    if kind == 'depth_point':
        return M.grow_depth(values, adj, seeds, thr, ml)
    if kind == 'color_points':
        return M.grow_color(values, adj, seeds, thr, ml, given=True)
    return M.grow_color(values, adj, int(seeds), thr, ml)


def _find(g, kind, max_level, nseeds):
    """index of the golden case of that kind, level limit and seed count on graph 0 with float64 values"""
    for k in range(int(g['ncases'])):
        if (str(g[f'c{k}_kind']), int(g[f'c{k}_max_level']), g[f'c{k}_seeds'].size, int(g[f'c{k}_graph'])) == (kind, max_level, nseeds, 0) \
                and str(g[f'c{k}_values']) != 'col32' and len(g[f'c{k}_cluster']):
            return k
    raise KeyError((kind, max_level, nseeds))


def _dev(adj):
    import torch
    return torch.as_tensor(adj[0], device='cuda'), torch.as_tensor(np.asarray(adj[1], np.int32), device='cuda')


def test_every_golden_flood_through_the_host_entry(golden):
    from Fusion3DSeg.segUtils import refinement as M
    g = golden('refinement')
    sets = (_find(g, 'depth_points', 5, 130), _find(g, 'color_point', 5, 1))
    for k in range(int(g['ncases'])):
        kind, (offs, nb), val, seeds, thr, ml, want = R.golden_case(g, k)
        rows = [nb[offs[i]:offs[i + 1]] for i in range(len(offs) - 1)]
        for adj in ((offs, nb), rows) + (([set(r.tolist()) for r in rows],) if k in sets else ()):
            if isinstance(adj[0], set):                                                 # the reference's list[set]: rows in set order
                want = getattr(R, kind)(val, [list(a) for a in adj], seeds, thr, ml)
            got = _call(M, kind, val, adj, seeds, thr, ml)
            assert isinstance(got, np.ndarray) and got.dtype == np.int64
            assert np.array_equal(got, want), (k, kind, len(got), len(want))            # acceptance order included


def test_every_golden_flood_through_the_device_entry(golden):
    import torch
    from Fusion3DSeg.segUtils import refinement as M
    g = golden('refinement')
    side = torch.cuda.Stream()
    for k in range(int(g['ncases'])):
        kind, adj, val, seeds, thr, ml, want = R.golden_case(g, k)
        dadj, dval = _dev(adj), torch.as_tensor(val, device='cuda')
        got = _call(M, kind, dval, dadj, seeds, thr, ml)                                 # the default stream, host seeds
        assert got.is_cuda and got.dtype == torch.int64
        assert np.array_equal(got.cpu().numpy(), want), (k, kind)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                                                   # a side stream, device seeds
            dseeds = torch.as_tensor(seeds, device='cuda')
            got = _call(M, kind, dval * 1.0, dadj, dseeds if dseeds.dim() else int(seeds), thr, ml)
            grown = torch.zeros(len(val), dtype=torch.bool, device='cuda')
            grown[got] = True                                                           # consumed on the same stream, no sync between
        torch.cuda.current_stream().wait_stream(side)
        assert np.array_equal(got.cpu().numpy(), want), (k, kind)
        assert int(grown.sum()) == len(want)


def _wrapper_args(g, name, adj):
    vertex = np.hstack([g['points'], g['colors']])
    if name.startswith('depth'):
        table, bounding = R.plane_table(g['plane_normals'], g['plane_index_offsets'], g['plane_index_values'], g['plane_quads'])
        return (table, vertex, list(g['selected_vertices']), bounding, adj)
    return (vertex, adj)


def test_public_wrappers_match_reference_golden(golden, tmp_path):
    from get3DSeg import PointCloud, write_ply
    from Fusion3DSeg.segUtils import refinement as M
    g = golden('refinement')
    adj = R.golden_graph(g, 0)
    changed = []
    for k in range(int(g['nruns'])):
        name, where, pick = str(g[f'r{k}_name']), str(g[f'r{k}_where']), g[f'r{k}_pick'].tolist()
        kw = {a: (int(v) if a == 'max_level' else float(v)) for a, v in zip(g[f'r{k}_kw_names'].tolist(), g[f'r{k}_kw_values'].tolist())}
        # the segmentation passed directly
        ids = g['ids'].copy()
        out_ids, pcd = getattr(M, name)(*_wrapper_args(g, name, adj), str(tmp_path / 'unused'), selected_point=pick, instance_id=ids,
                                        seg_colors=g['seg_colors'], **kw)
        assert out_ids is ids and np.array_equal(out_ids, g[f'r{k}_ids']), (k, name)
        assert np.array_equal(pcd.colors, g[f'r{k}_colors']) and np.array_equal(pcd.points, g['points']), (k, name)
        # read from ids.npy + pcd.ply under outputpath, where the reference looks for them
        d = tmp_path / f'run{k}'
        (d / where).mkdir(parents=True)
        np.save(d / where / 'ids.npy', g['ids'])
        write_ply(d / where / 'pcd.ply', PointCloud(g['points'], g['seg_colors']))
        out_ids, pcd = getattr(M, name)(*_wrapper_args(g, name, adj), str(d), selected_point=pick, **kw)
        assert np.array_equal(out_ids, g[f'r{k}_ids']) and np.array_equal(pcd.colors, g[f'r{k}_colors']), (k, name, 'files')
        changed.append(int((out_ids != g['ids']).sum()))
        if k == 0:
            M.save_ids_ply(pcd, out_ids, str(d))                                        # the next call finds cv_segmentation first
            again, _ = M.depth_floodfill_dl(*_wrapper_args(g, name, adj), str(d), selected_point=pick, depth_threshold=0.01, max_level=2)
            assert np.array_equal(again, out_ids)
    assert changed[4] == 0 and all(c > 0 for i, c in enumerate(changed) if i != 4)


def _capture(n=1_000_000, seed=11):
    """A wall of n points (10 x 10, lifted by a slow wave + noise) with ~10 neighbours per point, and two instances of > 10^5 points:
    a disc (one depth at its rim, so a depth flood leaves it) and a stripe across the colour gradient (a colour flood leaves it
    sideways, where its seeds are near the mean colour, and not at its ends, where they fail the threshold and do not expand)."""
    from Fusion3DSeg.fusion import radius_adjacency
    rng = np.random.default_rng(seed)
    xy = rng.uniform(0, 10, (n, 2))
    pts = np.stack([xy[:, 0], xy[:, 1], 0.02 * np.sin(xy[:, 0]) + rng.normal(0, 0.004, n)], 1)
    col = np.clip(np.stack([xy[:, 0] / 10, xy[:, 1] / 10, np.full(n, 0.5)], 1) + rng.normal(0, 0.02, (n, 3)), 0, 1)
    r = np.sqrt(10.0 / (np.pi * n / 100.0))
    adj = radius_adjacency(pts, r / 2, as_csr=True)
    return pts, col, adj, np.nonzero(((xy - 5) ** 2).sum(1) < 4.0)[0], np.nonzero(np.abs(xy[:, 0] - 5) < 0.8)[0]


def test_capture_size_matches_restatement():
    """~1 M points, the first queue is an instance of > 10^5 points (> 100 LDS chunks), max_level 50, all four variants."""
    from Fusion3DSeg.segUtils import refinement as M
    pts, col, adj, inst, stripe = _capture()
    deg = np.diff(adj[0])
    assert len(inst) >= 100_000 and len(stripe) >= 100_000 and 4 < deg.mean() < 40, (len(inst), len(stripe), deg.mean())
    dist = f3d.default_context().plane_distance(pts, [0, 0, 0], [0, 0, 1.0])
    assert np.array_equal(dist, np.abs(pts[:, 2]))                                       # exact for an axis normal
    picks = [int(inst[0]), int(inst[len(inst) // 2]), int(inst[-1])]
    for kind, val, seeds, thr in (('depth_points', dist, inst, 0.01), ('color_points', col, stripe, 0.1),
                                  ('depth_point', dist, picks, 0.01), ('color_point', col, picks[1], 0.1),
                                  ('color_points', col.astype(np.float32), stripe, np.array([0.1, 0.08, 0.1]))):
        t0 = time.perf_counter()
        want = getattr(R, kind)(val, adj, seeds, thr, 50)
        t1 = time.perf_counter()
        got = _call(M, kind, val, adj, seeds, thr, 50)
        t2 = time.perf_counter()
        print(f'{kind} {val.dtype}: {len(want)} points grown; restatement {t1 - t0:.2f} s, host entry with copies {t2 - t1:.3f} s')
        assert len(want) > 1000
        assert np.array_equal(got, want), (kind, len(got), len(want))


def test_plane_distance_within_the_float64_bound():
    """|computed - exact| <= refinement_ref.plane_distance_bound (derived there from the float64 model); exact = the same expression
    in extended precision (x87 long double: 64-bit significand, its own error 2^-11 of the bound's unit)."""
    import torch
    from Fusion3DSeg.segUtils import refinement as M
    rng = np.random.default_rng(5)
    n = 1_000_000
    pts = rng.normal(0, 5, (n, 3))
    nr = np.array([0.3, -0.5, 0.81])
    nr /= np.linalg.norm(nr)
    pp = np.array([1.25, -0.75, 2.5])
    pts[:10] = 0.0
    pts[10] = pp                                                                        # on the plane, exactly
    pts[11:1000] -= ((pts[11:1000] - pp) @ nr)[:, None] * nr                            # on the plane, to rounding
    assert np.finfo(np.longdouble).nmant >= 63
    L = np.longdouble
    d = pts.astype(L) - pp.astype(L)
    exact = np.abs(d[:, 0] * L(nr[0]) + d[:, 1] * L(nr[1]) + d[:, 2] * L(nr[2]))
    bound = R.plane_distance_bound(pts, pp, nr)
    for got in (M.plane_distance(pts, pp, nr), M.plane_distance(torch.as_tensor(pts, device='cuda'), pp, nr).cpu().numpy()):
        assert got.dtype == np.float64 and got.shape == (n,) and (got >= 0).all()
        err = np.abs(got.astype(L) - exact).astype(np.float64)
        print(f'plane_distance: max error / bound = {float((err / np.maximum(bound, 1e-300)).max()):.3f}, on-plane max {got[10:1000].max():.3e}')
        assert (err <= bound).all()
        assert got[10] == 0.0
    einsum = np.abs(np.einsum('nmc, mc -> mn', pts[:, None, :] - pp.reshape(1, 3)[None], nr.reshape(1, 3))[0])
    assert (np.abs(einsum - got) <= 2 * bound).all()                                   # the reference's order obeys the same model


def test_out_of_range_or_repeated_seed_is_an_index_error_and_the_context_survives(golden):
    import torch
    g = golden('refinement')
    kind, (offs, nb), val, seeds, thr, ml, want = R.golden_case(g, _find(g, 'depth_points', 50, 130))
    assert kind == 'depth_points' and len(want) > 0
    n = len(val)
    ctx = f3d.default_context()
    sma0 = np.average(val[seeds])
    for bad in ([n], [-1], [3, n + 7, 5], [3, 4, 3]):
        with pytest.raises(IndexError, match='region_grow'):
            ctx.region_grow(val, offs, nb, bad, sma0, 1, thr, ml)
        assert np.array_equal(ctx.region_grow(val, offs, nb, seeds, sma0, len(seeds), thr, ml, seeds_given=True), want)
    # the device entry records the error; the next call is not blamed for it
    dval, (doffs, dnb) = torch.as_tensor(val, device='cuda'), _dev((offs, nb))
    cluster, count = torch.empty(n, dtype=torch.int64, device='cuda'), torch.full((1,), -5, dtype=torch.int64, device='cuda')
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        bad = torch.as_tensor([2, n], device='cuda')
        ctx.region_grow_dev(dval.data_ptr(), f3d.F64, 1, n, doffs.data_ptr(), dnb.data_ptr(), bad.data_ptr(), 2, sma0, 2, thr, ml,
                            cluster.data_ptr(), count.data_ptr(), False, st.cuda_stream)
        with pytest.raises(IndexError, match='region_grow'):
            ctx.take_device_error(st.cuda_stream)
        assert int(count) == 0
        ds = torch.as_tensor(seeds, device='cuda')
        ctx.region_grow_dev(dval.data_ptr(), f3d.F64, 1, n, doffs.data_ptr(), dnb.data_ptr(), ds.data_ptr(), len(ds), sma0, len(ds), thr, ml,
                            cluster.data_ptr(), count.data_ptr(), True, st.cuda_stream)
        ctx.take_device_error(st.cuda_stream)
        assert np.array_equal(cluster[:int(count)].cpu().numpy(), want)
    with pytest.raises(ValueError):
        ctx.region_grow(val.astype(np.float32), offs, nb, seeds, sma0, 1, thr, ml)       # a scalar field must be float64
    # the tensor route leaves both checks to the kernel and names the cause afterwards
    from Fusion3DSeg.segUtils import refinement as M
    for bad, exc in (([3, n], IndexError), (torch.as_tensor([-1], device='cuda'), IndexError), ([3, 4, 3], ValueError)):
        with pytest.raises(exc):
            M.grow_depth(dval, (doffs, dnb), bad, thr, ml)
        got = M.grow_depth(dval, (doffs, dnb), seeds, thr, ml, given=True)
        assert np.array_equal(got.cpu().numpy(), want) and got.untyped_storage().nbytes() == 8 * len(want)


def test_strict_context_does_not_allocate_after_reserve(golden):
    import torch
    g = golden('refinement')
    kind, adj, val, seeds, thr, ml, want = R.golden_case(g, _find(g, 'color_point', 50, 1))
    assert kind == 'color_point'
    n = len(val)
    ctx = f3d.Context(0)
    ctx.reserve_refine(n)
    dval, (doffs, dnb) = torch.as_tensor(val, device='cuda'), _dev(adj)
    ds = torch.as_tensor(seeds.reshape(-1), device='cuda')
    cluster, count = torch.empty(n, dtype=torch.int64, device='cuda'), torch.zeros(1, dtype=torch.int64, device='cuda')
    torch.cuda.synchronize()
    ctx.set_strict(True)
    before = ctx.alloc_count
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        ctx.region_grow_dev(dval.data_ptr(), f3d.F64, 3, n, doffs.data_ptr(), dnb.data_ptr(), ds.data_ptr(), 1, val[int(seeds)], 0, thr, ml,
                            cluster.data_ptr(), count.data_ptr(), False, st.cuda_stream)
        ctx.take_device_error(st.cuda_stream)
    assert ctx.alloc_count == before
    assert np.array_equal(cluster[:int(count)].cpu().numpy(), want)
    ctx.close()
