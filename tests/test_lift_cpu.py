"""Mask lifting without a device: the C-ABI bindings, the NumPy restatement (tests/lift_ref.py) on hand-built scenes whose right
answer is written out here, and the small host-side helpers."""
import ctypes as C
import inspect

import numpy as np
import pytest

import f3d
import lift_ref as R


def test_symbols_are_bound():
    lib = f3d.library()
    vp, i32, i64, dbl = C.c_void_p, C.c_int, C.c_int64, C.c_double
    want = {'f3d_lift_overlaps': [vp, vp, vp, i32, i64, i64, i32, vp, vp, vp, i64, vp],
            'f3d_lift_overlaps_dev': [vp, vp, vp, i32, i64, i64, i32, vp, vp, vp, i64, vp, vp],
            'f3d_lift_instances': [vp, vp, vp, i32, i64, i64, i32, dbl, i64, vp, i64, vp, vp, vp, vp, vp, vp],
            'f3d_lift_instances_dev': [vp, vp, vp, i32, i64, i64, i32, dbl, i64, vp, i64, vp, vp, vp, vp, vp, vp, vp],
            'f3d_ctx_reserve_lift': [vp, i32, i64, i64, i32, i64]}
    for name, args in want.items():
        fn = getattr(lib, name)
        assert name in lib._f3d_symbols and list(fn.argtypes) == args and fn.restype is i32, name
    assert lib.f3d_version() == 100
    for m in ('lift_overlaps', 'lift_instances', 'reserve_lift', 'lift_overlaps_dev', 'lift_instances_dev'):
        assert callable(getattr(f3d.Context, m)), m


def test_module_surface():
    from Fusion3DSeg.segUtils import lifting
    assert set(lifting.__all__) >= {'segment_overlaps', 'lift_instances', 'split_by_lift', 'lift_from_dirs'}
    sig = inspect.signature(lifting.lift_instances).parameters
    assert list(sig) == ['luts', 'inst', 'npoints', 'max_ids', 'ratio', 'min_overlap', 'seg_classes', 'min_points']
    assert (sig['max_ids'].default, sig['ratio'].default, sig['min_overlap'].default, sig['seg_classes'].default,
            sig['min_points'].default) == (None, 0.5, 10, None, 1)


def test_argument_errors_come_before_any_device_call():
    from Fusion3DSeg.segUtils.lifting import lift_instances, segment_overlaps
    luts, inst = np.zeros((2, 4), np.int32), np.zeros((2, 4), np.uint16)
    with pytest.raises(ValueError, match='must both be'):
        lift_instances(luts, inst[:1], 4)
    with pytest.raises(ValueError, match='max_ids must be'):
        segment_overlaps(luts, inst, 4, 0)
    with pytest.raises(ValueError, match='max_ids must be'):
        lift_instances(luts, inst, 4, max_ids=70000)
    with pytest.raises(TypeError, match='integer'):
        lift_instances(luts.astype(np.float64), inst, 4)
    with pytest.raises(ValueError, match=r'\[0, 65535\]'):
        lift_instances(luts, np.full((2, 4), 70000, np.int32), 4)
    with pytest.raises(ValueError, match='seg_classes'):
        lift_instances(luts, inst, 4, max_ids=3, seg_classes=np.zeros(5, np.int32))
    with pytest.raises(IndexError):                                   # no point: every lookup >= 0 is out of bounds
        lift_instances(luts, inst, 0)
    r = lift_instances(np.full((2, 4), -1, np.int32), inst, 0)
    assert len(r.ids) == 0 and r.inst_points.tolist() == [0] and r.seg2inst.tolist() == [0, 0]


# ------------------------------------------------------------------------------------------------ the restatement
def test_two_touching_boxes_are_two_instances_where_the_flood_gives_one():
    points, luts, inst, k, box = R.two_boxes()
    assert R.flood_components(points, 1.0) == 1                       # the boxes touch: one flood instance
    r = R.lift_instances(luts, inst, len(points), k, ratio=0.5, min_overlap=10)
    assert r.inst_points.tolist() == [0, 64, 64]
    # a component's root is its smallest segment: the box with the smaller local id in frame 0 is instance 1
    first = {int(box[p]): int(i) for p, i in zip(luts[0], inst[0]) if p >= 0}
    assert np.array_equal(r.ids, np.where(box == 0, 1, 2) if first[0] < first[1] else np.where(box == 0, 2, 1))
    for f in range(6):                                                # every frame shuffles the ids, yet each box is one instance
        assert all(len(set(r.ids[luts[f][inst[f] == i]])) == 1 for i in np.unique(inst[f]) if i)
    assert (r.support == 6).all() and (r.seen == 6).all()
    assert sorted(np.unique(r.seg2inst).tolist()) == [0, 1, 2] and (r.seg2inst > 0).sum() == 12
    sizes, pairs, counts = R.segment_overlaps(luts, inst, len(points), k)
    assert sorted(sizes.tolist()) == [0] * 6 + [64] * 12 and len(pairs) == 2 * 15 and (counts == 64).all()


def test_chain_merges_through_the_middle_and_classes_cut_it():
    n, luts, inst = R.chain()
    sizes, pairs, counts = R.segment_overlaps(luts, inst, n, 1)
    assert sizes.tolist() == [12, 12, 12] and pairs.tolist() == [[0, 1], [1, 2]] and counts.tolist() == [6, 6]
    r = R.lift_instances(luts, inst, n, 1, ratio=0.5, min_overlap=5)
    assert r.seg2inst.tolist() == [1, 1, 1] and r.inst_points.tolist() == [0, n] and (r.ids == 1).all()
    r = R.lift_instances(luts, inst, n, 1, ratio=0.5, min_overlap=5, seg_classes=np.array([7, 7, 9], np.int32))
    assert r.seg2inst.tolist() == [1, 1, 2]
    # a = 0..11, b = 6..17, c = 12..23; the points 12..17 that b and c share see one segment of each instance: the tie goes to 1
    assert n == 24 and r.ids.tolist() == [1] * 18 + [2] * 6 and r.inst_points.tolist() == [0, 18, 6]
    assert r.support.tolist() == [1] * 6 + [2] * 6 + [1] * 12 and r.seen.tolist() == [1] * 6 + [2] * 12 + [1] * 6
    r = R.lift_instances(luts, inst, n, 1, ratio=0.5, min_overlap=5, seg_classes=np.array([7, 8, 7], np.int32))
    assert r.seg2inst.tolist() == [1, 2, 3]


def test_threshold_at_equality():
    n, luts, inst = R.threshold_pair(4)                               # min size 8, ratio 0.5: 4 >= 0.5 * 8
    assert R.lift_instances(luts, inst, n, 1, ratio=0.5, min_overlap=1).seg2inst.tolist() == [1, 1]
    assert R.lift_instances(luts, inst, n, 1, ratio=0.5, min_overlap=4).seg2inst.tolist() == [1, 1]
    assert R.lift_instances(luts, inst, n, 1, ratio=0.5, min_overlap=5).seg2inst.tolist() == [1, 2]
    n, luts, inst = R.threshold_pair(3)
    assert R.lift_instances(luts, inst, n, 1, ratio=0.5, min_overlap=1).seg2inst.tolist() == [1, 2]


def test_vote_tie_goes_to_the_smaller_id():
    # four frames, one segment each; 0-1 and 2-3 merge over points 0..9 / 10..19; point 20 lies in segments 1 and 2: a 1-1 tie
    frames = [{1: range(0, 10)}, {1: list(range(0, 10)) + [20]}, {1: list(range(10, 20)) + [20]}, {1: range(10, 20)}]
    luts, inst = R.frames_from_sets(21, frames)
    r = R.lift_instances(luts, inst, 21, 1, ratio=0.5, min_overlap=5)
    assert r.seg2inst.tolist() == [1, 1, 2, 2]
    assert r.ids[20] == 1 and r.support[20] == 1 and r.seen[20] == 2
    assert r.inst_points.tolist() == [0, 11, 10]


def test_min_points_drops_and_renumbers():
    frames = [{1: range(0, 10), 2: range(10, 13), 3: range(13, 25)}]
    luts, inst = R.frames_from_sets(26, frames)
    r = R.lift_instances(luts, inst, 26, 3, min_points=4)
    assert r.seg2inst.tolist() == [1, 0, 2]
    assert r.ids.tolist() == [1] * 10 + [0] * 3 + [2] * 12 + [0]
    assert r.support.tolist() == [1] * 10 + [0] * 3 + [1] * 12 + [0] and r.seen.tolist() == [1] * 25 + [0]
    assert r.inst_points.tolist() == [4, 10, 12]


def test_repeated_pixels_count_once_and_a_point_may_be_in_two_segments_of_a_frame():
    luts = np.array([[0, 0, 0, 1, 1, 2, -1, 5]], np.int32)
    inst = np.array([[1, 1, 2, 1, 1, 2, 2, 0]], np.uint16)
    sizes, pairs, counts = R.segment_overlaps(luts, inst, 6, 2)
    assert sizes.tolist() == [2, 2] and pairs.tolist() == [[0, 1]] and counts.tolist() == [1]
    r = R.lift_instances(luts, inst, 6, 2, ratio=0.5, min_overlap=1)
    assert r.seg2inst.tolist() == [1, 1] and r.seen.tolist() == [2, 1, 1, 0, 0, 0] and r.support.tolist() == [2, 1, 1, 0, 0, 0]
    r = R.lift_instances(luts, inst, 6, 2, ratio=0.5, min_overlap=2)
    assert r.seg2inst.tolist() == [1, 2] and r.ids.tolist() == [1, 1, 2, 0, 0, 0]          # point 0: a tie, the smaller id
    with pytest.raises(IndexError):
        R.lift_instances(luts, inst, 5, 2)                                                # lookup 5 on a pixel without an id
    with pytest.raises(IndexError):
        R.lift_instances(luts, inst, 6, 1)


# ------------------------------------------------------------------------------------------------ host helpers
def test_split_by_lift():
    from Fusion3DSeg.segUtils.lifting import split_by_lift
    ids = np.array([0, 0, 2, 2, 2, 2, 5, 5], np.int64)
    lifted = np.array([0, 0, 3, 1, 0, 3, 7, 7], np.int32)
    new, parent = split_by_lift(ids, lifted, return_parent=True)
    assert new.tolist() == [0, 0, 3, 2, 1, 3, 4, 4] and new.dtype == np.int64 and parent.tolist() == [0, 2, 2, 2, 5]
    assert np.array_equal(split_by_lift(ids, lifted), R.split_by_lift(ids, lifted))
    rng = np.random.default_rng(5)
    a, b = rng.integers(0, 9, 500), rng.integers(0, 4, 500)
    assert np.array_equal(split_by_lift(a, b), R.split_by_lift(a, b))
    assert np.array_equal(split_by_lift(a, np.zeros_like(b)), np.unique(a, return_inverse=True)[1])
    with pytest.raises(ValueError):
        split_by_lift(a, b[:-1])


def test_panoptic_to_instances():
    import get2DSeg
    pan = np.array([[1, 1, 2, 2], [3, 3, 2, 0], [4, 4, 4, 0]])
    info = [{'id': 1, 'isthing': False, 'category_id': 100}, {'id': 4, 'isthing': True, 'category_id': 56},
            {'id': 2, 'isthing': True, 'category_id': 60}, {'id': 3, 'isthing': False, 'category_id': 120}]
    inst, cats = get2DSeg.panoptic_to_instances({'sem_seg': None, 'panoptic_seg': (pan, info)})
    assert inst.dtype == np.uint16 and inst.tolist() == [[0, 0, 2, 2], [0, 0, 2, 0], [1, 1, 1, 0]] and cats == [56, 60]
    inst2, _ = get2DSeg.panoptic_to_instances((pan, info))
    assert np.array_equal(inst, inst2)


def test_get3dseg_without_instance_dir_makes_the_same_calls(monkeypatch, tmp_path):
    import get3DSeg
    sig = inspect.signature(get3DSeg.segment).parameters
    assert list(sig)[-1] == 'instance_dir' and sig['instance_dir'].default is None
    calls = []
    pts = np.zeros((4, 3))

    class Voter:
        def __init__(self, *a, **k):
            pass

        def vote(self, **k):
            calls.append('vote')
            return np.ones((4, 134))

        def segment(self, threshold, filter_classes):
            calls.append('voter.segment')
            return np.zeros(4, np.int64)

    ids = np.array([0, 1, 1, 1])
    info = [{'id': 0, 'isthing': False, 'category_id': 133, 'area': 1}, {'id': 1, 'isthing': True, 'category_id': 56, 'area': 3}]
    monkeypatch.setattr(get3DSeg.Fusion, 'load_data', staticmethod(lambda d: (pts, pts, None, None, None, 1, (2, 2), [np.array([0])] * 4)))
    monkeypatch.setattr(get3DSeg, 'VotingSegmentation', Voter)
    monkeypatch.setattr(get3DSeg, 'split_into_instances', lambda *a, **k: (calls.append('split'), (None, ids, info, None))[1])
    monkeypatch.setattr(get3DSeg, 'refine_instances', lambda *a, **k: (calls.append('refine'), (ids, info))[1])
    monkeypatch.setattr(get3DSeg, 'panoptic_viz', lambda points, ids_, info_, *a, **k: calls.append(('panoptic_viz', ids_.tolist(), len(info_))))
    for name in ('semantic_viz', 'master_classes', '_coco_meta'):
        monkeypatch.setattr(get3DSeg, name, lambda *a, **k: None)
    get3DSeg.segment(tmp_path, tmp_path, verbose=False)
    assert calls == ['vote', 'voter.segment', 'split', ('panoptic_viz', [0, 1, 1, 1], 2)]
    del calls[:]
    get3DSeg.segment(tmp_path, tmp_path, verbose=False, instance_dir=tmp_path)
    assert calls == ['vote', 'voter.segment', 'split', 'refine', ('panoptic_viz', [0, 1, 1, 1], 2)]


def test_refine_instances_splits_things_only(monkeypatch):
    import get3DSeg
    from Fusion3DSeg.segUtils import lifting
    ids = np.array([0, 0, 1, 1, 1, 1])
    info = [{'id': 0, 'isthing': False, 'category_id': 133, 'area': 2}, {'id': 1, 'isthing': True, 'category_id': 56, 'area': 4}]
    lifted = np.array([1, 2, 1, 1, 2, 0], np.int32)
    monkeypatch.setattr(lifting, 'lift_from_dirs', lambda *a, **k: type('R', (), {'ids': lifted})())
    new, new_info = get3DSeg.refine_instances(ids, info, 'a', 'b', (1, 6))
    assert new.tolist() == [0, 0, 2, 2, 3, 1]
    assert [(i['id'], i['category_id'], i['area'], i['isthing']) for i in new_info] == [(0, 133, 2, False), (1, 56, 1, True), (2, 56, 2, True),
                                                                                       (3, 56, 1, True)]
