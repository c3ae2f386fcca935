"""CVSegmentation host side (no GPU): the golden file, the restatement against it, the static helpers, no CPU fallback."""
import numpy as np
import pytest

import f3d
import cvseg_ref as R


def _graph(g, gi):
    offs, nb = g[f'g{gi}_offsets'], g[f'g{gi}_neighbours']
    return g[f'g{gi}_classes'], [nb[offs[i]:offs[i + 1]] for i in range(len(offs) - 1)]


def test_golden_loads_and_covers_the_contract(golden):
    g = golden('cvseg')
    assert int(g['nicases']) >= 10 and int(g['nccases']) >= 8
    ics = [g[f'i{k}_instance_classes'].tolist() for k in range(int(g['nicases'])) if g[f'i{k}_has_instance_classes']]
    assert any(ic and ic[-1] == 0 for ic in ics) and any(len(set(ic)) < len(ic) for ic in ics)
    assert {int(g[f'c{k}_max_level']) for k in range(int(g['nccases']))} >= {1, 2, 10}
    assert {str(g[f'c{k}_colors'].dtype) for k in range(int(g['nccases']))} == {'float32', 'float64'}
    assert any(int(g[f'c{k}_changed']) > 0 for k in range(int(g['nccases'])))
    assert any(g[f'i{k}_boundary_kinds'].any() for k in range(int(g['nicases'])))        # an object-array boundary


def test_restatement_matches_reference_golden(golden):
    g = golden('cvseg')
    for k in range(int(g['nicases'])):
        cls, rows = _graph(g, int(g[f'i{k}_graph']))
        cls = cls.copy()
        ic = g[f'i{k}_instance_classes'].tolist() if g[f'i{k}_has_instance_classes'] else None
        out = R.instance_seperate(cls, rows, ic, int(g[f'i{k}_minimum_points']))
        n, ids, info, clusters, bnds = R.decode_instances(g, f'i{k}_')
        assert len(out[0]) == n and np.array_equal(out[1], ids) and out[2] == info, k
        assert np.array_equal(cls, g[f'i{k}_classes_after']), k
        assert len(out[3]) == len(clusters) and all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(out[3], clusters)), k
        assert all(R.same_boundary(a, b) for a, b in zip(out[4], bnds)), k
    for k in range(int(g['nccases'])):
        cls, rows = _graph(g, int(g[f'c{k}_graph']))
        thr = float(g[f'c{k}_threshold']) if g[f'c{k}_threshold_is_scalar'] else tuple(g[f'c{k}_threshold'])
        got = R.color_segment(None, rows, g[f'c{k}_colors'], g[f'c{k}_ids_in'].copy(), g[f'c{k}_seeds'], thr,
                              tuple(g[f'c{k}_neutral_ids'].tolist()), int(g[f'c{k}_max_level']))
        assert np.array_equal(got, g[f'c{k}_ids_out']), k


def test_static_helpers(golden):
    from Fusion3DSeg.segUtils.cv import CVSegmentation as S
    g = golden('cvseg')
    n, ids, info, clusters, bnds = R.decode_instances(g, 'i3_')
    sem, obj = S.get_semantic_object_ids(info)
    assert sem == [d['id'] for d in info if not d['isthing']] and obj == [d['id'] for d in info if d['isthing']] and sem
    assert np.array_equal(S.get_objects(ids, obj), np.isin(ids, obj))
    want = np.zeros_like(ids)
    for d in info:
        want[ids == d['id']] = d['category_id']
    assert np.array_equal(S.get_classes(ids, info), want)
    dup = info + [{'id': info[0]['id'], 'isthing': True, 'category_id': 99, 'area': 1}]          # the last matching record wins
    assert (S.get_classes(ids, dup)[ids == info[0]['id']] == 99).all()
    cats = sorted({d['category_id'] for d in info})
    assert S.get_ids_by_classes(info, cats) == [[d['id'] for d in info if d['category_id'] == c] for c in cats]
    c = np.array([1, 2, 3, 1, 2])
    assert np.array_equal(S.merge_classes(c, (1, 2), (2, 3)), [3, 3, 3, 3, 3])                      # sequential: chains apply
    # merge_instances_by_classes against the restatement's fold, on records that carry several category-0 entries
    cls, rows = _graph(g, 0)
    recs = [{'id': i, 'isthing': i > 1, 'category_id': [5, 0, 7, 0, 9, 0][i], 'area': i + 1} for i in range(6)]
    rid = np.random.default_rng(3).integers(0, 6, len(cls)).astype(np.int64)
    cl = [np.nonzero(rid == i)[0] for i in range(6)]
    bd = [None, None] + [rid == i for i in range(2, 6)]
    import copy
    got = S.merge_instances_by_classes(rid, copy.deepcopy(recs), (0,), cl, bd)
    want = R.merge_zero(rid, copy.deepcopy(recs), cl, bd)
    assert got[0] == want[0] and np.array_equal(got[1], want[1]) and got[2] == want[2]
    assert all(np.array_equal(a, b) for a, b in zip(got[3], want[3]))
    assert all(R.same_boundary(a, b) for a, b in zip(got[4], want[4]))


def test_no_cpu_fallback_for_cvsegmentation():
    import torch
    if torch.cuda.is_available():
        pytest.skip('a HIP device is present')
    from Fusion3DSeg.segUtils.cv import CVSegmentation
    cls = np.array([1, 1, 2], np.int64)
    adj = [np.array([0, 1]), np.array([0, 1]), np.array([2])]
    with pytest.raises(f3d.F3DUnavailable):
        CVSegmentation(cls, adj).instance_seperate()
    with pytest.raises(f3d.F3DUnavailable):
        CVSegmentation(cls, adj).color_segment(np.zeros((3, 3)), np.zeros(3, np.int64), [0], 0.1)


def test_color_segment_rejects_other_colour_dtypes():
    from Fusion3DSeg.segUtils.cv import CVSegmentation
    cls = np.array([1, 1, 2], np.int64)
    adj = [np.array([0, 1]), np.array([0, 1]), np.array([2])]
    with pytest.raises(TypeError):
        CVSegmentation(cls, adj).color_segment(np.zeros((3, 3), np.uint8), np.zeros(3, np.int64), [0], 1)
