"""The input recipes of tests/flood_graphs.py and tests/quad_scenes.py do what the GPU edge tests rely on: the graphs meet the
kernels' preconditions and have the level sizes they are named for, the restatements return the closed form on them, the reject
recipes put accepted and rejected entries on both sides of the 1024-entry chunk boundaries and children behind expanders past
1024, and the quad scenes reach every branch of door_window_ref.  No GPU."""
import numpy as np
import pytest

import cvseg_ref as C
import door_window_ref as D
import flood_graphs as G
import quad_scenes as Q
import refinement_ref as R

SMALL = {'CHUNK_EDGES': G.CHUNK_EDGES, 'CARRY_EDGES': G.CARRY_EDGES, 'SHARE_EDGES': G.SHARE_EDGES, 'STAR': G.STAR,
         **{f'PATH{d}': G.PATH(d) for d in G.PATH_DEPTHS}}


@pytest.fixture(scope='module')
def batch():
    return G.layered(G.BATCH_EDGE)


def _check_layered(widths, csr):
    for name, g, perm in G.variants(csr, 11):
        G.check_rows(g)
        assert G.bfs_levels(g, int(perm[0])) == list(widths), name
    offs, nb = csr
    assert np.array_equal(nb[offs[:-1]], np.arange(len(offs) - 1))              # as built: the row's own node first


@pytest.mark.parametrize('name', sorted(SMALL))
def test_layered_graphs_meet_the_preconditions_and_have_their_level_sizes(name):
    _check_layered(SMALL[name], G.layered(SMALL[name]))


def test_batch_edge_has_a_level_above_1024_times_256(batch):
    _check_layered(G.BATCH_EDGE, batch)
    assert max(G.BATCH_EDGE) > 1024 * 256 and len(batch[0]) - 1 < 270_000
    cls = G.batch_classes(True)
    assert G.bfs_levels(batch, 0, cls == 4) == [1, 150, 150 * 875] and (cls == 6).sum() == len(cls) - 151 - 150 * 875
    assert G.bfs_levels(batch, 151, cls == 6) == [1, 875] and G.bfs_levels(batch, 300, cls == 6) == [1, 820]


def test_tailed_batch_edge_has_children_in_second_batches():
    """layered(BATCH_EDGE)'s widest frontier is its last level: nothing it computes in a second batch can be seen.  With the tails the
    same frontier has a child at every 64th entry, so k_fo_count / k_fo_apply add up counts of entries past the 256th of a block's
    share, and k_fo_place puts their children behind those of the first batch."""
    csr = G.tailed(G.BATCH_EDGE, G.BATCH_TAIL_EVERY)
    nf = G.BATCH_EDGE[-1]
    ntails = -(-nf // G.BATCH_TAIL_EVERY)
    for name, g, perm in G.variants(csr, 9, keep_first=True):
        G.check_rows(g)
        assert perm[0] == 0 and G.bfs_levels(g, 0) == G.BATCH_EDGE + [ntails]
    n = len(csr[0]) - 1
    clusters = C.instance_seperate(np.full(n, 4, np.int64), csr, None, 1)[3]
    assert np.array_equal(clusters[0], np.arange(n))                              # frontier position = index inside the level
    per = -(-nf // 1024)                                                          # a block's share of the frontier (fo_range)
    has_child = np.arange(0, nf, G.BATCH_TAIL_EVERY)
    assert per > 256 and ((has_child % per) >= 256).sum() > 10
    cls = G.batch_classes(True, tails=True)
    assert len(cls) == n and np.array_equal(cls[n - ntails:], cls[301:301 + nf:G.BATCH_TAIL_EVERY]) and (cls[-5:] == 6).all()


def test_relabel_is_the_same_graph():
    for csr in (G.layered(G.SHARE_EDGES), G.class_union()[0]):
        n = len(csr[0]) - 1
        rng = np.random.default_rng(3)
        perm = rng.permutation(n)
        offs, nb = G.relabel(csr, perm, rng)
        inv = np.argsort(perm)
        rows = {(int(inv[i]), int(inv[j])) for i in range(n) for j in nb[offs[i]:offs[i + 1]]}
        assert rows == {(i, int(j)) for i in range(n) for j in csr[1][csr[0][i]:csr[0][i + 1]]}
        assert not np.array_equal(nb[offs[:-1]], np.arange(n))                    # the row's own node is no longer first


def test_class_union_joins_components_of_different_class_only():
    csr, cls = G.class_union()
    for name, g, perm in G.variants(csr, 5):
        G.check_rows(g)
    offs, nb = csr
    row = np.repeat(np.arange(len(cls)), np.diff(offs))
    starts = np.concatenate([[0], np.cumsum([sum(w) for w in G.UNION_WIDTHS])])
    comp = np.searchsorted(starts, np.arange(len(cls)), side='right') - 1
    cross = comp[row] != comp[nb]
    assert cross.sum() == 12 and (cls[row[cross]] != cls[nb[cross]]).all()
    for k, w in enumerate(G.UNION_WIDTHS):
        assert G.bfs_levels(csr, int(starts[k]), comp == k) == list(w)
    want = C.instance_seperate(cls.copy(), csr, None, 1)
    assert len(want[3]) == 5 and any(b.any() for b in want[4])                   # five clusters, boundary flags set
    assert sum(d['category_id'] == 0 for d in C.instance_seperate(cls.copy(), csr, None, 4)[2]) == 1
    assert len(C.instance_seperate(cls.copy(), csr, None, 4)[3]) == 4            # two small clusters folded into one record


@pytest.mark.parametrize('name', ['CHUNK_EDGES', 'SHARE_EDGES', 'PATH9', 'PATH17'])
def test_restatements_return_the_closed_form_on_a_graph_as_built(name):
    widths = SMALL[name]
    csr = G.layered(widths)
    n = sum(widths)
    _, ids, info, clusters, bnds = C.instance_seperate(np.full(n, 4, np.int64), csr, None, 1)
    assert len(clusters) == 1 and np.array_equal(clusters[0], np.arange(n)) and not bnds[0].any()
    assert info == [{'id': 0, 'isthing': True, 'category_id': 4, 'area': n}] and not ids.any()
    assert np.array_equal(R.grow(np.ones(n), csr, [0], 1.0, 0, 0.1, 0, False), np.arange(n))
    ids = np.zeros(n, np.int64)
    ids[0] = 8
    counts = []
    C.color_segment(None, csr, np.full((n, 3), 0.5), ids, [0], 0.1, (0,), 0, counts)
    assert (ids == 8).all() and counts == [n]
    for ml in (1, 2, 3, 4):                                                      # nothing, the seed, one ring, two rings
        assert np.array_equal(R.grow(np.ones(n), csr, [0], 1.0, 0, 0.1, ml, False), np.arange(sum(widths[:ml - 1])))


def test_batch_edge_closed_form(batch):
    n = sum(G.BATCH_EDGE)
    clusters = C.instance_seperate(np.full(n, 4, np.int64), batch, None, 1)[3]
    assert len(clusters) == 1 and np.array_equal(clusters[0], np.arange(n))


REJECT = [(w, v, dt, thr) for w in ('CHUNK_EDGES', 'CARRY_EDGES') for v in (0, 1) for dt in (np.float64, np.float32)
          for thr in (0.07, (0.07, 0.06, 0.08))]


@pytest.mark.parametrize('wname, variant, dtype, thr', REJECT)
def test_reject_recipe_mixes_every_chunk_and_places_children_past_1024(wname, variant, dtype, thr):
    widths = SMALL[wname]
    val, far = G.reject_colors(widths, 1, dtype)
    name, csr, perm = G.variants(G.layered(widths), 7)[variant]
    val, n = G.moved(val, perm), len(val)
    seed = int(perm[0])
    got = R.grow(val, csr, [seed], val[seed], 0, thr, 0, False)
    ids = np.zeros(n, np.int64)
    ids[seed] = 8
    C.color_segment(None, csr, val, ids, [seed], thr, (0,), 0)
    assert np.array_equal(np.nonzero(ids == 8)[0], np.sort(got))                 # the two restatements agree on the accepted set
    accepted = np.zeros(n, bool)
    accepted[got] = True
    trace = G.flood_trace(csr, [seed], accepted)
    assert np.array_equal(np.concatenate([q[ok] for q, ok, _ in trace]), got)    # the replay is the restatement's flood
    assert [len(q) for q, _, _ in trace] == list(widths) or wname == 'CARRY_EDGES'
    assert len(trace) == len(widths) and len(trace[-1][1]) > 0                   # the flood reaches and accepts in the last level
    assert not accepted[G.moved(far, perm)].any() and (~accepted & ~G.moved(far, perm)).sum() > 100   # near entries rejected too
    mixed, carried = G.carry_coverage(trace)
    assert mixed
    # CHUNK_EDGES: only the first three nodes of its widest level have children, so no expander past 1024 can (as built, the pop
    # order is the index order); CARRY_EDGES is the recipe for the placement's carry
    assert carried == (wname == 'CARRY_EDGES')
    if wname == 'CARRY_EDGES':
        assert max(len(ok) for _, ok, _ in trace) > 2048                          # three placement rounds


def test_float32_rounding_decides_an_entry():
    """the same colours in float32 and float64 accept different sets: the running mean's rounding reaches a decision"""
    val, _ = G.reject_colors(G.CHUNK_EDGES, 1)
    name, csr, perm = G.variants(G.layered(G.CHUNK_EDGES), 7)[1]
    val = G.moved(val, perm)
    seed = int(perm[0])
    a = R.grow(val, csr, [seed], val[seed], 0, 0.07, 0, False)
    b = R.grow(val.astype(np.float32), csr, [seed], val.astype(np.float32)[seed], 0, 0.07, 0, False)
    assert not np.array_equal(a, b)


def test_several_seeds_case_uses_the_epoch_and_the_neutral_seed_id():
    csr, colors, ids, seeds, neutral, (a, b) = G.seeded_colors()
    G.check_rows(csr)
    na = sum(G.CHUNK_EDGES)
    assert ids[seeds[[0, 1, 3]]].tolist() == [5, 9, 7] and all(ids[v] in neutral for v in (a, b, seeds[2]))
    first = C.color_segment(None, csr, colors, ids.copy(), seeds[:1], 0.07, neutral, 0)
    assert first[b] == 5 and first[a] == ids[a] and not (first[:na] != ids[:na]).any()      # B's flood meets a and rejects it
    counts = []
    out = C.color_segment(None, csr, colors, ids.copy(), seeds, 0.07, neutral, 0, counts)
    assert out[a] == 9 and out[seeds[2]] == 9                                     # the second seed takes a, and the third seed's node
    assert all(c > 0 for c in counts) and counts[2] > 1                           # the third seed accepts what the second rejected
    nine_c = np.nonzero(ids[2 * na:] == 9)[0] + 2 * na
    assert len(nine_c) >= 2 and (out[nine_c] == 9).all() and counts[3] < 15 - len(nine_c) + 1   # C's flood cannot pass its nines


def test_star_seeds_fail_about_a_third():
    val, far = G.star_values(2)
    for count in G.SEED_COUNTS:
        sd = G.star_seeds(count, far, np.arange(len(far)), 4)
        assert len(np.unique(sd)) == count and 0 not in sd and not far[sd[0]]
        if count > 1000:
            assert 0.25 < far[sd].mean() < 0.42
            sma0 = np.average(val[sd])
            assert (np.abs(val[sd][far[sd]] - sma0) > 0.25).all() and (np.abs(val[sd][~far[sd]] - sma0) < 0.25).all()


# ------------------------------------------------------------------------------------------------ quad scenes
def _switch(nrm):
    """the np.allclose switch of door_window_ref.basis"""
    a = nrm / np.sqrt(D.blas_dot(nrm, nrm))
    return abs(abs(D.blas_dot(a, np.array([0.0, 0.0, 1.0]))) - 1.0) <= 1e-08 + 1e-05 * 1.0


def test_facing_scene_reaches_every_status_and_both_sides_of_the_switch():
    pts, ids, inst, verts, tris = Q.facing_scene()
    q, st, tri, nrm = D.quads(pts, ids, inst, verts, tris)
    names = [f[0] for f in Q.FACINGS]
    assert all(t // 2 == k for k, t in enumerate(tri))                           # every instance chooses its own rectangle
    status = dict(zip(names, st))
    assert np.array_equal(nrm[0], [0.0, 0.0, 1.0]) and np.array_equal(nrm[2], [0.0, 0.0, -1.0])
    assert status['up'] == status['up_9.9deg'] == D.QUAD_HORIZONTAL
    assert status['down'] == status['down_4e-3'] == status['down_5e-3'] == status['up_10.1deg'] == status['wall'] == D.QUAD_OK
    sw = {n: bool(_switch(nrm[t])) for n, t in zip(names, tri)}
    assert sw['down'] and sw['down_4e-3'] and not sw['down_5e-3'] and not sw['wall'] and not sw['up_10.1deg']
    for s in (Q.with_zero_area_triangle, Q.with_nan_vertex):
        assert (D.quads(*s((pts, ids, inst, verts, tris)))[1] == D.QUAD_NO_CANDIDATE).all()


def test_fan_scene_has_a_wide_band_with_a_shared_maximum():
    pts, ids, inst, verts, tris = Q.fan_scene()
    nrm = D.normals(verts, tris)
    tv = verts[tris]
    for s, heavy in enumerate(((70, 100), (5, 69))):
        p = pts[ids == inst[s]]
        td = D.tri_dist(p, tv[:, 0], nrm)
        cand = np.nonzero(td < td.min() + 0.05 * td.min())[0]
        assert len(cand) == 136 > 64 and np.array_equal(cand, np.arange(136))
        counts = np.array([D.inside_count(p - nrm[t][None, :] * D._perp(p, tv[t, 0], nrm[t])[:, None], tv[t]) for t in cand])
        assert counts.max() == 4 and np.nonzero(counts == 4)[0].tolist() == list(heavy)
        st, t, quad = D.quad_of(pts, ids, inst[s], verts, tris, nrm)
        assert st == D.QUAD_OK and t == heavy[0]


def test_size_scene_statuses():
    sizes = [1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 513]
    pts, ids, inst, verts, tris = Q.rect_scene(20, sizes, seed=3, nother=3000)
    assert inst[0] < 0 and inst[-1] > 2 ** 40 and len(tris) == 40
    assert [(ids == i).sum() for i in inst] == sizes
    q, st, tri, _ = D.quads(pts, ids, inst + [999], verts, tris)
    assert st[-1] == D.QUAD_NO_CANDIDATE and (st[:-1] != D.QUAD_NO_CANDIDATE).all() and (st == D.QUAD_OK).sum() >= 8
