"""No result depends on memory that the call did not write: every case of tests/family_cases.py (one per kernel source) returns its
reference result after f3d_debug_poison has filled the context's scratch, staging and kept buffers with a byte pattern and while
tests/poison.py fills what numpy.empty / torch.empty and their kin hand out with the same byte.  A fresh hipMalloc and fresh pages
behind np.empty are zero in practice, which is what a forgotten initialisation usually wanted; here the start is 0xFF (-1, NaN, the
empty value of a min-key), 0x5A (large, positive, finite) or 0x00 (the start most inits want, yet not the stale data of the warm run).

Per case, on the default context: run another seed (stale values), run the real input (sizes every buffer), poison, run
again under poisoned_empty, and require that the context allocated nothing in between -- a regrown buffer would be fresh memory --
and that the family's own comparison with its reference holds.  A HIP error ends the module: nothing more is started on the device."""
import ctypes as C

import numpy as np
import pytest

import f3d
import fused_families
import tsdf_ref
from family_cases import CASES, N, OTHER_SEED, SEED, check_extremes, cloud, grouping, prepared, radius_rows, rows_that_differ, same
from oracle import np_ref as O
from poison import poisoned_empty

pytestmark = pytest.mark.gpu

PATTERNS = [0x00, 0xFF, 0x5A]


def stop_on_hip_error(what, e):
    """A HIP call failed (the library's or torch's): the device may have faulted, so the module ends here."""
    if isinstance(e, f3d.F3DUnavailable) or 'hip error' in str(e).lower():
        pytest.exit(f'{what}: {e!r}; nothing more is started on this device', returncode=3)


@pytest.fixture
def ctx():
    return f3d.default_context()


@pytest.mark.parametrize('pattern', PATTERNS, ids=lambda p: f'0x{p:02X}')
@pytest.mark.parametrize('name', sorted(CASES))
def test_results_do_not_depend_on_unwritten_memory(ctx, name, pattern):
    import torch
    run, want, check, rows = prepared(name, SEED)
    other_run, _, _, other_rows = prepared(name, OTHER_SEED)
    assert len(rows) > 0 and 2 * rows_that_differ(rows, other_rows) >= len(rows)   # a stale right answer would be a wrong one
    try:
        other_run(ctx)                                                          # stale values of another seed in every recycled buffer
        run(ctx)                                                                # sizes every buffer for the real input
        torch.cuda.synchronize()
        ctx.synchronize()
        a0 = ctx.alloc_count
        buffers, nbytes = ctx.debug_poison(pattern)
        print(f'{name} 0x{pattern:02X}: {buffers} buffers, {nbytes} bytes filled')
        assert buffers > 0 and nbytes > 0
        with poisoned_empty(pattern):
            got = run(ctx)
    except RuntimeError as e:
        stop_on_hip_error(f'{name} at 0x{pattern:02X}', e)
        raise                                                                   # any other error status is an ordinary failure
    assert ctx.alloc_count == a0                                                # the run met the poisoned buffers, not fresh ones
    check(got, want)


# ---- the hook itself --------------------------------------------------------------------------------------------------------------------
R = 0.08


def test_out_of_range_bytes_are_refused(ctx):
    for bad in (-1, 256, 1 << 20):
        with pytest.raises(ValueError, match='debug_poison'):
            ctx.debug_poison(bad)
    assert ctx._lib.f3d_debug_poison(ctx._h, 0, None) == f3d.ERR_INVALID         # and a NULL out
    buffers, nbytes = ctx.debug_poison(255)
    assert buffers >= 4 and nbytes > 0                                           # at least the four small members every context owns


def test_radius_graph_fill_after_a_poison_asks_for_its_count_pass(ctx):
    pts = cloud(np.random.default_rng(SEED))
    p, dt = f3d._xyz(pts)
    offs, nnz = np.zeros(N + 1, np.int64), C.c_int64(0)
    assert ctx._lib.f3d_radius_graph_count(ctx._h, f3d._ptr(p), dt, N, R, f3d._ptr(offs), C.byref(nnz)) == 0
    ctx.debug_poison(0x5A)
    nb = np.full(nnz.value, -7, np.int32)
    assert ctx._lib.f3d_radius_graph_fill(ctx._h, N, f3d._ptr(nb)) == f3d.ERR_INVALID
    assert b'call f3d_radius_graph_count for this cloud first' in ctx._lib.f3d_last_error(ctx._h)
    assert (nb == -7).all()                                                      # nothing written
    goffs, gnb = ctx.radius_graph(pts, R)                                        # from its count pass it works again
    woffs, wnb = radius_rows(pts, pts, R)
    same(goffs, woffs); same(offs, woffs)
    same(np.concatenate([np.sort(gnb[goffs[i]:goffs[i + 1]]) for i in range(N)]), wnb)


def test_radius_query_fill_after_a_poison_asks_for_its_count_pass(ctx):
    rng = np.random.default_rng(SEED)
    data, queries = cloud(rng), cloud(rng)
    d, ddt = f3d._xyz(data)
    q, qdt = f3d._xyz(queries)
    offs, nnz = np.zeros(N + 1, np.int64), C.c_int64(0)
    assert ctx._lib.f3d_radius_query_count(ctx._h, f3d._ptr(d), ddt, N, f3d._ptr(q), qdt, N, R, f3d._ptr(offs), C.byref(nnz)) == 0
    ctx.debug_poison(0xFF)
    nb = np.full(nnz.value, -7, np.int32)
    assert ctx._lib.f3d_radius_query_fill(ctx._h, N, f3d._ptr(nb)) == f3d.ERR_INVALID
    assert b'radius_query_fill: call f3d_radius_query_count' in ctx._lib.f3d_last_error(ctx._h)
    assert (nb == -7).all()
    woffs, wnb = radius_rows(data, queries, R)
    goffs, gnb = ctx.radius_query(data, queries, R)
    same(goffs, woffs); same(gnb, wnb); same(offs, woffs)


def test_the_grouping_sequence_after_a_poison_asks_for_group_by_id(ctx):
    rng = np.random.default_rng(SEED)
    nids = 6
    ids = rng.integers(-1, nids + 1, N).astype(np.int64)
    pts = cloud(rng)
    want = grouping(ids, nids)
    ctx.group_by_id(ids, nids)
    ctx.debug_poison(0x00)
    with pytest.raises(ValueError, match='obb_extremes: call f3d_group_by_id for this cloud first'):
        ctx.obb_extremes(pts)
    ctx.group_by_id(ids, nids)
    ext = ctx.obb_extremes(pts)
    ctx.debug_poison(0xFF)
    fstart, facets, margin = np.zeros(nids + 1, np.int32), np.zeros((0, 4)), np.zeros(nids)
    with pytest.raises(ValueError, match='obb_hull_filter: call f3d_group_by_id and f3d_obb_extremes'):
        ctx.obb_hull_filter(fstart, facets, margin)
    order, starts = ctx.group_by_id(ids, nids)                                   # from its first call the sequence works again
    same(order, want[0]); same(starts, want[1])
    again = ctx.obb_extremes(pts)
    check_extremes(ids, pts, again, nids)
    same(again, ext)
    from scipy.spatial import ConvexHull
    eqs = []
    for k in range(nids):                                                        # the facets of every id's extremes, as case_obb builds them
        eqs.append(ConvexHull(pts[np.unique(again[k])]).equations)
        fstart[k + 1] = fstart[k] + len(eqs[-1])
        margin[k] = 1e-9 * 2.0
    cand, cnt = ctx.obb_hull_filter(fstart, np.concatenate(eqs), margin)
    for k in range(nids):
        mem, c = np.flatnonzero(ids == k), cand[starts[k]:starts[k] + cnt[k]]
        assert len(mem) > 100 and set(c.tolist()) <= set(mem.tolist()) and len(c) < len(mem), k      # members only, and some were dropped
        assert set(mem[ConvexHull(pts[mem]).vertices].tolist()) <= set(c.tolist()), k                 # every hull vertex survives


def test_tsdf_extract_fill_after_a_poison_asks_for_its_count_pass(ctx):
    _, want, _, _ = prepared('f3d_tsdf.hip', SEED)
    tsdf, weight = want[0].copy(), want[1].copy()
    nz, ny, nx = tsdf.shape
    lo, vs = np.array([-0.9, -0.7, 0.55]), 0.05                                  # case_tsdf's volume
    nv, nt = C.c_int64(0), C.c_int64(0)
    assert ctx._lib.f3d_tsdf_extract_count(ctx._h, f3d._ptr(tsdf), f3d._ptr(weight), nx, ny, nz, 1.0, C.byref(nv), C.byref(nt)) == 0
    assert (nv.value, nt.value) == (len(want[2]), len(want[3]))
    ctx.debug_poison(0x5A)
    verts, tris = np.full((nv.value, 3), -7.0), np.full((nt.value, 3), -7, np.int32)
    assert ctx._lib.f3d_tsdf_extract_fill(ctx._h, nx, ny, nz, f3d._ptr(lo), vs, f3d._ptr(verts), f3d._ptr(tris)) == f3d.ERR_INVALID
    assert b'tsdf_extract_fill' in ctx._lib.f3d_last_error(ctx._h)
    assert (verts == -7.0).all() and (tris == -7).all()
    gv, gt = ctx.tsdf_extract(tsdf, weight, lo, vs, 1.0)
    assert gv.tobytes() == want[2].tobytes() and np.array_equal(gt, want[3])
    want_v, want_t = tsdf_ref.extract(tsdf, weight, lo, vs, 1.0)
    assert gv.tobytes() == want_v.tobytes() and np.array_equal(gt, want_t)


def fused_scene():
    """case_fuse's scene: the base cameras of fused_families on 2500 points -> (points, views, masks, votes and labels of the oracle)."""
    from f3d import synth
    _, K, q, t, max_depth, w, h, _ = fused_families.family('base')
    pts = synth.cloud(N, seed=SEED)
    masks = synth.masks(len(t), h, w, 'iid', seed=SEED)
    with np.errstate(all='ignore'):
        votes = O.forward_votes(pts, K, q, t, masks, max_depth, ncols=134)
    return pts, f3d.views_build(K, w, h, q, t, max_depth), masks, votes, O.segment(votes, 133, 0.5, None)


def test_the_hook_is_refused_during_a_view_chunked_fused_call(ctx):
    import torch
    dev = torch.device('cuda', 0)
    pts, views, masks, _, want = fused_scene()
    V, H, W = masks.shape
    assert V >= 2
    x, vd, md = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (pts, views, masks))
    cls = torch.full((N,), -7, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    args = (x.data_ptr(), f3d.F64, N, vd.data_ptr(), V)
    tail = (md.data_ptr(), H, W, 133, 0.5, None, cls.data_ptr(), None)
    try:
        ctx.fuse_chunked_begin_dev(None, N, V, H, W, 133, None, None)
        ctx.fuse_chunk_dev(*args, 0, V // 2, *tail)
        with pytest.raises(ValueError, match='debug_poison: a view-chunked fused call is in progress'):
            ctx.debug_poison(0xFF)
        ctx.fuse_chunk_dev(*args, V // 2, V, *tail)                              # the call still completes
        ctx.take_device_error()
        ctx.synchronize()
    except RuntimeError as e:
        stop_on_hip_error('the chunked fused call', e)
        raise
    same(cls.cpu().numpy(), want)
    assert ctx.debug_poison(0xFF)[0] > 0                                         # complete: the hook works again


def test_a_reserved_context_reports_at_least_what_was_reserved():
    own = f3d.Context(0)
    try:
        n, V, H, W = 5000, 3, 48, 56
        assert own.debug_poison(0x5A) == (4, 4 * 512 + 8 + 4 + 16)               # a young context: the four small members alone (F3D_MAX_FILTER ints, 8, 4, 16)
        own.reserve(n, V, H, W)
        allocs = own.alloc_count
        buffers, nbytes = own.debug_poison(0x5A)
        slots = 1024
        while slots < 2 * H * W:
            slots *= 2
        assert buffers == 4 + allocs                                             # every buffer that reserve allocated, and the vote set among them
        assert nbytes >= n * 4 + V * own.coded_plane_bytes(H, W) + slots * 8      # the permutation, the coded planes, the vote set, ...
        assert own.alloc_count == allocs                                         # the hook allocates nothing
    finally:
        own.close()


def test_the_fused_path_in_a_strict_reserved_context_poisoned_between_two_steps():
    import torch
    dev = torch.device('cuda', 0)
    pts, views, masks, want_votes, want_labels = fused_scene()
    V, H, W = masks.shape
    x, vd, md = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (pts, views, masks))
    s = torch.cuda.Stream(dev)
    own = f3d.Context(0)
    try:
        own.reserve(N, V, H, W)
        own.set_strict(True)
        a0 = own.alloc_count
        for step, pattern in enumerate([None, 0xFF, 0x5A, 0x00]):
            if pattern is not None:
                buffers, nbytes = own.debug_poison(pattern)
                assert buffers > 4 and nbytes > N * 4
            cls = torch.full((N,), -7, dtype=torch.int64, device=dev)
            votes = torch.full((N, 134), 0x7B7B, dtype=torch.int16, device=dev)  # uint16 rows, sentinel-filled
            s.wait_stream(torch.cuda.current_stream(dev))
            try:
                own.project_vote_argmax_dev(x.data_ptr(), f3d.F64, N, vd.data_ptr(), V, md.data_ptr(), H, W, 133, 0.5, None, cls.data_ptr(),
                                            votes.data_ptr(), s.cuda_stream, flags=f3d.FUSE_SORT)
                own.take_device_error(s.cuda_stream)
                s.synchronize()
            except RuntimeError as e:
                stop_on_hip_error(f'fused step {step}', e)
                raise
            same(cls.cpu().numpy(), want_labels)
            got_votes = votes.cpu().numpy().view(np.uint16)
            assert np.array_equal(got_votes, want_votes), step
            assert own.alloc_count == a0
    finally:
        own.close()
