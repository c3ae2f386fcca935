"""f3d_door_window_quads where its wave paths, ballots and switches change sides, bit for bit against the restatement
tests/door_window_ref.py: instances below, at and above a wave, triangle counts around 64 and 256, a band of more than 64
candidates with a shared best count, triangles facing down and nearly down, negative vertex indices, degenerate triangles, and
more instances than one block.  The scenes are tests/quad_scenes.py; what they reach is asserted in test_flood_edges_cpu.py."""
import numpy as np
import pytest

import f3d
import door_window_ref as R
import quad_scenes as Q

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 513]


def _check(scene, inst=None):
    pts, ids, scene_inst, verts, tris = scene
    inst = scene_inst if inst is None else inst
    q, st, tri, nrm = f3d.default_context().door_window_quads(pts, ids, inst, verts, tris)
    wq, wst, wtri, wnrm = R.quads(pts, ids, inst, verts, tris)
    assert np.array_equal(nrm, wnrm, equal_nan=True)
    assert np.array_equal(st, wst), (st.tolist(), wst.tolist())
    assert np.array_equal(tri, wtri), (tri.tolist(), wtri.tolist())
    assert q.shape == wq.shape and np.array_equal(q, wq, equal_nan=True), np.nonzero((q != wq).any(axis=(1, 2)) & (st == R.QUAD_OK))[0]
    return q, st, tri


@pytest.fixture(scope='module')
def size_scene():
    return Q.rect_scene(20, SIZES, seed=3, nother=3000)


@pytest.mark.parametrize('layout', ['shuffled', 'sorted', 'descending'])
def test_instance_sizes_around_a_wave(size_scene, layout):
    """The kernels walk the members grouped by instance, so sizes 1 ... 513 give waves inside one instance and waves across two or
    more; the cloud's order (shuffled, sorted by id) decides the order of the members' point indices, and with it every sequential
    sum.  Descending wanted ids (a negative one, one above 2^40, one without points) move every slot."""
    scene = {'shuffled': Q.shuffled(size_scene, 1), 'sorted': Q.sorted_by_id(size_scene), 'descending': Q.shuffled(size_scene, 2)}[layout]
    inst = scene[2] + [999]                                                     # a wanted id without points, last
    if layout == 'descending':
        inst = sorted(inst, reverse=True)
    q, st, tri = _check(scene, inst)
    assert st[inst.index(999)] == R.QUAD_NO_CANDIDATE and (st == R.QUAD_NO_CANDIDATE).sum() == 1
    assert (st == R.QUAD_OK).sum() >= 8


@pytest.mark.parametrize('nt', [1, 2, 63, 64, 65, 128, 129, 256, 257, 600])
def test_triangle_counts_around_a_wave_and_a_block(nt):
    scene = Q.shuffled(Q.rect_scene((nt + 1) // 2, [70, 300, 1100], seed=nt, ntri=nt), nt)
    assert len(scene[4]) == nt
    q, st, tri = _check(scene)
    assert (st != R.QUAD_NO_CANDIDATE).all()


def test_wide_band_with_a_shared_best_count():
    scene = Q.fan_scene()
    q, st, tri = _check(scene)
    assert tri.tolist()[:2] == [70, 5] and (st == R.QUAD_OK).all()              # the first maximum in triangle order
    _check(Q.shuffled(scene, 4))


def test_downward_and_nearly_vertical_normals():
    scene = Q.facing_scene()
    q, st, tri = _check(scene)
    names = [f[0] for f in Q.FACINGS]
    assert [names[k] for k in np.nonzero(st == R.QUAD_HORIZONTAL)[0]] == ['up', 'up_9.9deg']
    assert (st != R.QUAD_NO_CANDIDATE).all()
    _check(Q.shuffled(scene, 6))


@pytest.mark.parametrize('which', ['sizes', 'facing', 'fan'])
def test_negative_vertex_indices(size_scene, which):
    scene = {'sizes': size_scene, 'facing': Q.facing_scene(), 'fan': Q.fan_scene()}[which]
    neg = Q.with_negative_indices(scene)
    assert (neg[4] < 0).sum() > len(neg[4]) and (neg[4] >= 0).sum() > len(neg[4])
    ctx = f3d.default_context()
    a = ctx.door_window_quads(*scene)
    b = ctx.door_window_quads(*neg)
    for x, y in zip(a, b):
        assert np.array_equal(x, y, equal_nan=True)
    _check(neg)


@pytest.mark.parametrize('spoil', [Q.with_zero_area_triangle, Q.with_nan_vertex])
def test_one_degenerate_triangle_leaves_no_candidate(size_scene, spoil):
    q, st, tri = _check(spoil(size_scene))
    assert (st == R.QUAD_NO_CANDIDATE).all() and (tri == -1).all() and np.isnan(q).all()


def test_more_instances_than_a_block():
    pts, ids, inst, verts, tris = Q.rect_scene(20, [3] * 257, seed=8, nother=500)
    assert len(inst) == 257 and len(tris) == 40
    order = np.random.default_rng(8).permutation(257)
    q, st, tri = _check(Q.shuffled((pts, ids, inst, verts, tris), 8), [inst[k] for k in order])
    assert (st != R.QUAD_NO_CANDIDATE).all()
