"""Mask lifting on the GPU (f3d_lift_overlaps, f3d_lift_instances, segUtils.lifting): every output array_equal to the restatement
tests/lift_ref.py -- the contract is integer arithmetic, so nothing is approximate."""
import functools

import numpy as np
import pytest

import f3d
import lift_ref as R

pytestmark = pytest.mark.gpu
FILL = 77


def L():
    from Fusion3DSeg.segUtils import lifting
    return lifting


def _np(x):
    return x.cpu().numpy() if hasattr(x, 'cpu') else x


def _same(got, want, what=''):
    got, want = _np(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), (what, got.dtype, got.shape, want.dtype, want.shape)


def _same_result(got, want):
    for name in ('ids', 'support', 'seen', 'seg2inst', 'inst_points'):
        _same(getattr(got, name), getattr(want, name), name)


def _same_overlaps(got, want):
    for g, w, name in zip(got, want, ('sizes', 'pairs', 'counts')):
        _same(g, w, name)


def _check(luts, inst, n, k, **kw):
    """Both entries on the NumPy route against the restatement -> the restatement's overlaps."""
    want = R.segment_overlaps(luts, inst, n, k)
    _same_overlaps(L().segment_overlaps(luts, inst, n, k), want)
    _same_result(L().lift_instances(luts, inst, n, k, **kw), R.lift_instances(luts, inst, n, k, **kw))
    return want


@functools.lru_cache(maxsize=None)
def scene(name):
    """-> (luts, inst, npoints, max_ids), read-only."""
    if name == 'A':
        out = (*R.random_scene(1, 20000, 32, 48 * 64, 64, skew=2.0), 20000, 64)
    elif name == 'B':                                               # one id per frame
        out = (*R.random_scene(2, 3000, 24, 40 * 30, 1), 3000, 1)
    elif name == 'C':                                               # ids up to 300: past uint8
        out = (*R.random_scene(3, 4000, 6, 64 * 48, 300, skew=2.0), 4000, 300)
    elif name == 'D':                                               # 5 x 333 pixels: no multiple of a block, frame boundaries inside blocks
        out = (*R.random_scene(4, 500, 5, 333, 7), 500, 7)
    elif name == 'E':                                               # 7 x 100: three frames share the first block
        out = (*R.random_scene(5, 90, 7, 100, 3, skew=1.0), 90, 3)
    for a in out[:2]:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def scene_ref(name, **kw):
    luts, inst, n, k = scene(name)
    return R.lift_instances(luts, inst, n, k, **dict(kw))


# ------------------------------------------------------------------------------------------------ hand-built scenes
def test_two_boxes():
    points, luts, inst, k, box = R.two_boxes()
    _check(luts, inst, len(points), k)
    r = L().lift_instances(luts, inst, len(points), k)
    assert r.inst_points.tolist() == [0, 64, 64] and len(set(r.ids[box == 0])) == 1 and len(set(r.ids[box == 1])) == 1
    _same_result(L().lift_instances(luts, inst, len(points)), R.lift_instances(luts, inst, len(points)))       # max_ids = max(inst)


def test_chain_and_classes():
    n, luts, inst = R.chain()
    for cls in (None, np.array([7, 7, 9], np.int32), np.array([7, 8, 7], np.int32)):
        _check(luts, inst, n, 1, ratio=0.5, min_overlap=5, seg_classes=cls)
    assert L().lift_instances(luts, inst, n, 1, min_overlap=5).seg2inst.tolist() == [1, 1, 1]
    assert L().lift_instances(luts, inst, n, 1, min_overlap=5, seg_classes=[7, 7, 9]).seg2inst.tolist() == [1, 1, 2]


def test_threshold_at_equality():
    for overlap, min_overlap, want in ((4, 1, [1, 1]), (4, 4, [1, 1]), (4, 5, [1, 2]), (3, 1, [1, 2])):
        n, luts, inst = R.threshold_pair(overlap)
        _check(luts, inst, n, 1, ratio=0.5, min_overlap=min_overlap)
        assert L().lift_instances(luts, inst, n, 1, ratio=0.5, min_overlap=min_overlap).seg2inst.tolist() == want
    n, luts, inst = R.threshold_pair(4)
    for ratio in (0.5000000000000001, 0.0, -1.0, float('nan'), float('inf')):
        _check(luts, inst, n, 1, ratio=ratio, min_overlap=1)


def test_tie_min_points_repeats_and_two_segments_in_a_frame():
    frames = [{1: range(0, 10)}, {1: list(range(0, 10)) + [20]}, {1: list(range(10, 20)) + [20]}, {1: range(10, 20)}]
    luts, inst = R.frames_from_sets(21, frames)
    _check(luts, inst, 21, 1, min_overlap=5)
    assert L().lift_instances(luts, inst, 21, 1, min_overlap=5).ids[20] == 1
    luts, inst = R.frames_from_sets(26, [{1: range(0, 10), 2: range(10, 13), 3: range(13, 25)}])
    for mp in (0, 1, 3, 4, 11, 13, 100):
        _check(luts, inst, 26, 3, min_points=mp)
    assert L().lift_instances(luts, inst, 26, 3, min_points=4).inst_points.tolist() == [4, 10, 12]
    luts = np.array([[0, 0, 0, 1, 1, 2, -1, 5]], np.int32)
    inst = np.array([[1, 1, 2, 1, 1, 2, 2, 0]], np.uint16)
    for mo in (1, 2):
        _check(luts, inst, 6, 2, min_overlap=mo)


def test_empty_and_smallest_inputs():
    luts, inst = np.full((3, 50), -1, np.int32), np.ones((3, 50), np.uint16)
    sizes, pairs, counts = _check(luts, inst, 10, 2)
    assert len(pairs) == 0 and not sizes.any()
    r = L().lift_instances(luts, inst, 10, 2)
    assert not r.ids.any() and r.inst_points.tolist() == [10]
    for lut, i in ((0, 1), (0, 0), (-1, 1)):                        # N = 1, F = 1, one pixel
        _check(np.array([[lut]], np.int32), np.array([[i]], np.uint16), 1, 1, min_overlap=1)
    _check(np.zeros((1, 9), np.int32), np.arange(9, dtype=np.uint16).reshape(1, 9), 1, 8, min_overlap=1)      # one point in 8 segments of a frame


def test_rows_across_wave_widths():
    """Points 0..3 of a 5 000-point cloud are seen by 63, 64, 65 and 129 frames (one segment per frame and point at least): rows at,
    below and above a wave's 64 lanes, the last one alone yielding 129 * 128 / 2 = 8 256 pairs."""
    rng = np.random.default_rng(11)
    n, nf, hw = 5000, 129, 96
    luts = rng.integers(4, n, (nf, hw)).astype(np.int32)
    luts[rng.random((nf, hw)) < 0.3] = -1
    inst = rng.integers(1, 3, (nf, hw)).astype(np.uint16)
    for p, frames in enumerate((63, 64, 65, 129)):
        luts[:frames, p], inst[:frames, p] = p, 1
    want = _check(luts, inst, n, 2, min_overlap=3, ratio=0.05)
    seen = R.lift_instances(luts, inst, n, 2).seen
    assert seen[:4].tolist() == [63, 64, 65, 129] and len(want[1]) >= 8256
    _check(luts, inst, n, 2, min_overlap=1, ratio=0.0)              # everything merges: the long rows vote on one instance


# ------------------------------------------------------------------------------------------------ random scenes
def test_scene_a_needs_a_grown_table():
    luts, inst, n, k = scene('A')
    want = R.segment_overlaps(luts, inst, n, k)
    assert len(want[1]) >= 100_000                                   # not a thin case
    _same_overlaps(L().segment_overlaps(luts, inst, n, k), want)
    ctx = f3d.Context(0)                                             # a fresh arena: the first table has 65 536 slots
    *out, stats = ctx.lift_instances(luts, inst, n, k, 0.2, 2, None, 1)
    assert stats[0] == len(want[1]) and stats[5] >= 2 and stats[4] >= stats[0]          # the table stage ran again, no pair was lost
    ref = scene_ref('A', min_overlap=2, ratio=0.2)
    for g, name in zip(out, ('ids', 'support', 'seen', 'seg2inst')):
        _same(g, getattr(ref, name), name)
    _same(out[4][:stats[1] + 1], ref.inst_points)
    ctx.close()
    ctx = f3d.Context(0)
    sizes, pairs, counts, stats = ctx.lift_overlaps(luts, inst, n, k, len(want[1]))
    assert stats[0] == len(want[1]) and stats[5] >= 2
    _same_overlaps((sizes, pairs, counts), want)
    _, pairs, counts, stats = ctx.lift_overlaps(luts, inst, n, k, 100)          # too little room: the count comes, the pairs do not
    assert stats[0] == len(want[1]) and stats[5] == 1 and not pairs.any() and not counts.any()
    ctx.close()


@pytest.mark.parametrize('kw', [(), (('min_overlap', 2), ('ratio', 0.2)), (('min_overlap', 2), ('ratio', 0.1), ('min_points', 40))])
def test_scene_a_instances(kw):
    luts, inst, n, k = scene('A')
    _same_result(L().lift_instances(luts, inst, n, k, **dict(kw)), scene_ref('A', **dict(kw)))


@pytest.mark.parametrize('name', ['B', 'C', 'D', 'E'])
def test_random_scenes(name):
    luts, inst, n, k = scene(name)
    if name == 'C':
        assert inst.max() > 255
    for kw in ({}, {'min_overlap': 2, 'ratio': 0.2}, {'min_overlap': 1, 'ratio': 0.0, 'min_points': 5}):
        _check(luts, inst, n, k, **kw)
    rng = np.random.default_rng(8)
    cls = rng.integers(0, 3, luts.shape[0] * k).astype(np.int32)
    _check(luts, inst, n, k, min_overlap=1, ratio=0.1, seg_classes=cls)


# ------------------------------------------------------------------------------------------------ errors, tensors, arena
def _device_call(ctx, luts, inst, n, k, **kw):
    """f3d_lift_instances_dev and f3d_lift_overlaps_dev on FILL-filled outputs -> the outputs as NumPy arrays."""
    import torch
    nf, hw = luts.shape
    dl, di = torch.tensor(luts, device='cuda'), torch.tensor(inst.view(np.int16), device='cuda')
    out = {'ids': torch.full((n,), FILL, dtype=torch.int32, device='cuda'), 'support': torch.full((n,), FILL, dtype=torch.int16, device='cuda'),
           'seen': torch.full((n,), FILL, dtype=torch.int16, device='cuda'), 'seg2inst': torch.full((nf * k,), FILL, dtype=torch.int32, device='cuda'),
           'inst_points': torch.full((nf * k + 1,), FILL, dtype=torch.int64, device='cuda'),
           'sizes': torch.full((nf * k,), FILL, dtype=torch.int32, device='cuda'), 'pairs': torch.full((64, 2), FILL, dtype=torch.int32, device='cuda'),
           'counts': torch.full((64,), FILL, dtype=torch.int32, device='cuda')}
    st = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    errors = []
    for call in (lambda: ctx.lift_instances_dev(dl.data_ptr(), di.data_ptr(), nf, hw, n, k, kw.get('ratio', 0.5), kw.get('min_overlap', 10), None,
                                                kw.get('min_points', 1), out['ids'].data_ptr(), out['support'].data_ptr(), out['seen'].data_ptr(),
                                                out['seg2inst'].data_ptr(), out['inst_points'].data_ptr(), st),
                 lambda: ctx.lift_overlaps_dev(dl.data_ptr(), di.data_ptr(), nf, hw, n, k, out['sizes'].data_ptr(), out['pairs'].data_ptr(),
                                               out['counts'].data_ptr(), 64, st)):
        try:
            call()
        except IndexError as exc:
            errors.append(exc)
    torch.cuda.synchronize()
    return {name: t.cpu().numpy() for name, t in out.items()}, errors


def test_bad_input_raises_and_writes_nothing():
    ctx = f3d.default_context(0)
    luts, inst, n, k = scene('E')
    for which in ('inst', 'lut', 'lut_without_id', 'inst_without_lut'):
        bl, bi = luts.copy(), inst.copy()
        if which == 'inst':
            bl[3, 50], bi[3, 50] = 5, k + 1
        elif which == 'lut':
            bl[6, 99], bi[6, 99] = n, 1
        elif which == 'lut_without_id':
            bl[0, 0], bi[0, 0] = n + 4, 0
        else:
            bl[2, 7], bi[2, 7] = -1, k + 1
        with pytest.raises(IndexError):
            R.lift_instances(bl, bi, n, k)
        with pytest.raises(IndexError, match='lift'):
            L().lift_instances(bl, bi, n, k)
        with pytest.raises(IndexError, match='lift'):
            L().segment_overlaps(bl, bi, n, k)
        out, errors = _device_call(ctx, bl, bi, n, k)
        assert len(errors) == 2 and all((a == FILL).all() for a in out.values()), which
    out, errors = _device_call(ctx, luts, inst, n, k)               # the error is not sticky
    assert not errors and (out['ids'] != FILL).all()
    _check(luts, inst, n, k)


def test_tensor_route_equals_the_numpy_route():
    import torch
    for name, kw in (('D', {'min_overlap': 2, 'ratio': 0.2}), ('C', {'min_overlap': 1, 'ratio': 0.1, 'min_points': 3})):
        luts, inst, n, k = scene(name)
        dl = torch.tensor(luts, device='cuda')
        for di in (torch.tensor(inst.view(np.int16), device='cuda'), torch.tensor(inst.view(np.int16), device='cuda').view(torch.uint16)):
            got = L().lift_instances(dl, di, n, k, **kw)
            assert all(getattr(got, f).is_cuda for f in ('ids', 'support', 'seen', 'seg2inst', 'inst_points'))
            _same_result(got, L().lift_instances(luts, inst, n, k, **kw))
            ov = L().segment_overlaps(dl, di, n, k)
            assert all(t.is_cuda for t in ov)
            _same_overlaps(ov, L().segment_overlaps(luts, inst, n, k))
        _same_result(L().lift_instances(dl, di, n, **kw), R.lift_instances(luts, inst, n, **kw))                # max_ids read from the tensor
        cls = torch.arange(luts.shape[0] * k, device='cuda') % 2
        _same_result(L().lift_instances(dl, di, n, k, seg_classes=cls, **kw), R.lift_instances(luts, inst, n, k, seg_classes=_np(cls), **kw))
    small = torch.as_tensor(np.minimum(scene('D')[1], 255).astype(np.uint8), device='cuda')
    _same_result(L().lift_instances(torch.tensor(scene('D')[0], device='cuda'), small, 500, 7),
                 R.lift_instances(scene('D')[0], _np(small), 500, 7))
    ids, lifted = torch.as_tensor([0, 0, 2, 2, 2, 2, 5, 5], device='cuda'), torch.as_tensor([0, 0, 3, 1, 0, 3, 7, 7], device='cuda')
    new, parent = L().split_by_lift(ids, lifted, return_parent=True)
    assert new.is_cuda and new.tolist() == [0, 0, 3, 2, 1, 3, 4, 4] and parent.tolist() == [0, 2, 2, 2, 5]


def test_reserved_arena_does_not_grow():
    luts, inst, n, k = scene('D')
    ctx = f3d.Context(0)
    ctx.reserve_lift(luts.shape[0], luts.shape[1], n, k, 1000)
    count = ctx.alloc_count
    ctx.set_strict(True)                                            # a scratch buffer that had to grow would now be a MemoryError
    first, errors = _device_call(ctx, luts, inst, n, k, min_overlap=2, ratio=0.2)
    second, _ = _device_call(ctx, luts, inst, n, k, min_overlap=2, ratio=0.2)
    assert not errors and ctx.alloc_count == count
    want = R.lift_instances(luts, inst, n, k, min_overlap=2, ratio=0.2)
    for out in (first, second):
        _same(out['ids'], want.ids); _same(out['seg2inst'], want.seg2inst); _same(out['seen'].view(np.uint16), want.seen)
        _same(out['support'].view(np.uint16), want.support); _same(out['inst_points'][:len(want.inst_points)], want.inst_points)
        assert (out['inst_points'][len(want.inst_points):] == FILL).all()
    ctx.set_strict(False)
    ctx.lift_instances(luts, inst, n, k, 0.5, 10, None, 1)          # the host route stages once ...
    count = ctx.alloc_count
    ctx.lift_instances(luts, inst, n, k, 0.5, 10, None, 1)          # ... and not again
    assert ctx.alloc_count == count
    ctx.close()


# ------------------------------------------------------------------------------------------------ end to end
def test_two_slabs_through_render_lookups():
    """A wall of 2 cm grid points cut into a left and a right slab that touch; six cameras render it with the project's own z-buffer
    (fusion.render_lookups) and a perfect 2D network names the slabs per frame, in shuffled ids.  The flood of the radius graph
    sees one object; the lift sees two."""
    from f3d import synth
    from Fusion3DSeg import fusion
    y, z = np.meshgrid(np.arange(-0.5, 0.5001, 0.02), np.arange(-0.4, 0.4001, 0.02))
    points = np.stack([np.ones(y.size), y.reshape(-1), z.reshape(-1)], axis=1)
    slab = (points[:, 1] >= 0).astype(np.int64)
    hw = (96, 128)
    eyes = np.array([[-1.0, dy, dz] for dy in (-0.2, 0.0, 0.2) for dz in (-0.1, 0.1)])
    quats = np.stack([synth._look_at_quat(e, e + [1.0, 0.0, 0.0]) for e in eyes])
    K = np.array([[0.8 * hw[1], 0.0, hw[1] / 2.0], [0.0, 0.8 * hw[1], hw[0] / 2.0], [0.0, 0.0, 1.0]])
    _, uv2pt = fusion.render_lookups(points, K, quats, eyes, hw, 10.0, 0)
    rng = np.random.default_rng(3)
    inst = np.zeros(uv2pt.shape, np.uint16)
    for f in range(len(eyes)):
        local = rng.permutation(4)[:2] + 1                           # this frame's ids of the two slabs
        hit = uv2pt[f] >= 0
        inst[f, hit] = local[slab[uv2pt[f, hit]]]
    assert R.flood_components(points[::2], 0.045) == 1               # (every second point: the flood is quadratic)
    want = R.lift_instances(uv2pt, inst, len(points), 4)
    got = L().lift_instances(uv2pt, inst, len(points), 4)
    _same_result(got, want)
    seen = got.seen > 0
    assert seen.sum() > 0.5 * len(points) and len(got.inst_points) == 3
    assert len(set(got.ids[seen & (slab == 0)])) == 1 and len(set(got.ids[seen & (slab == 1)])) == 1
    assert got.ids[seen & (slab == 0)][0] != got.ids[seen & (slab == 1)][0]
    flood_ids = np.zeros(len(points), np.int64)                      # what split_into_instances gives: one instance
    assert len(np.unique(L().split_by_lift(flood_ids, got.ids)[seen])) == 2


def test_lift_from_dirs(tmp_path):
    """Frames as files: 16-bit and 8-bit id PNGs (one at twice the size, to be resized) and .npy lookups, paired by stem."""
    from PIL import Image
    luts, inst, n, k = scene('D')
    h, w = 9, 37
    (tmp_path / 'inst').mkdir(); (tmp_path / 'uv2pt').mkdir()
    for f in range(len(luts)):
        ids = inst[f].reshape(h, w)
        if f == 1:
            ids = np.repeat(np.repeat(ids, 2, axis=0), 2, axis=1)
        Image.fromarray(ids.astype(np.uint8 if f == 2 else np.uint16)).save(tmp_path / 'inst' / f'frame{f:02d}.png')
        np.save(tmp_path / 'uv2pt' / f'frame{f:02d}.npy', luts[f].reshape(h, w))
    np.save(tmp_path / 'uv2pt' / 'frame99.npy', luts[0])             # no id map: not a frame
    kw = {'min_overlap': 2, 'ratio': 0.2}
    got = L().lift_from_dirs(tmp_path / 'inst', tmp_path / 'uv2pt', n, (h, w), max_ids=k, batch_pixels=2 * h * w, **kw)
    assert got.frames == [f'frame{f:02d}' for f in range(len(luts))]
    _same_result(got, R.lift_instances(luts, inst, n, k, **kw))
