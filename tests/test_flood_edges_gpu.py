"""The ordered floods at the sizes where their machinery changes behaviour, against the restatements, exactly:
f3d_flood_order (1024 block shares, batches of 256 above a frontier of 262 144, a readback every 8 levels), f3d_color_segment and
f3d_region_grow (queues staged and children placed 1024 entries at a time).  The inputs are the recipes of tests/flood_graphs.py
(what they cover is asserted in test_flood_edges_cpu.py); every graph runs as built, where a flood pops in index order, and
relabelled by a seeded permutation with shuffled rows, where only the right order passes."""
import numpy as np
import pytest

import f3d
import cvseg_ref as C
import flood_graphs as G
import refinement_ref as R

pytestmark = pytest.mark.gpu

WIDTHS = {'CHUNK_EDGES': G.CHUNK_EDGES, 'CARRY_EDGES': G.CARRY_EDGES, 'SHARE_EDGES': G.SHARE_EDGES}
VARIANTS = ('built', 'relabelled')
THRESHOLDS = (0.07, (0.07, 0.06, 0.08))


@pytest.fixture(scope='module')
def batch():
    return {False: G.layered(G.BATCH_EDGE), True: G.tailed(G.BATCH_EDGE, G.BATCH_TAIL_EVERY)}


def _variant(csr, which, seed=7):
    return G.variants(csr, seed)[VARIANTS.index(which)]


# ------------------------------------------------------------------------------------------------ f3d_flood_order
def _same_instances(got, want):
    n, ids, info, clusters, bnds = len(want[0]), want[1], want[2], want[3], list(want[4])
    assert len(got[0]) == n and np.array_equal(got[0], np.arange(n))
    assert got[1].dtype == ids.dtype and np.array_equal(got[1], ids)
    assert got[2] == info
    assert len(got[3]) == len(clusters) and len(got[4]) == len(bnds)
    for k, (a, b) in enumerate(zip(got[3], clusters)):
        assert a.dtype == b.dtype and np.array_equal(a, b), k                  # flood (pop) order
    for k in range(len(bnds)):
        assert C.same_boundary(got[4][k], bnds[k]), k


def _separate(cls, csr, ic, mp):
    """CVSegmentation.instance_seperate against the restatement -> the segmentation (its floods carry the stats)"""
    from Fusion3DSeg.segUtils.cv import CVSegmentation
    want_cls, mine = cls.copy(), cls.copy()
    want = C.instance_seperate(want_cls, csr, ic, mp)
    seg = CVSegmentation(mine, csr)
    _same_instances(seg.instance_seperate(ic, mp), want)
    assert np.array_equal(mine, want_cls)                                        # the caller's classes, rewritten in place
    return seg


def _readbacks(levels):
    """f3d_launch_flood_order enqueues FO_CHUNK = 8 rounds, reads the frontier length back and stops when it is 0.  Round r (from
    1) consumes BFS level r and leaves level r + 1 as the frontier, so after 8 q rounds the frontier is empty exactly when
    levels <= 8 q: ceil(levels / 8) readbacks, and one when there is nothing to flood."""
    return max(1, -(-levels // 8))


def _depth(seg, csr, cls):
    """BFS levels of the deepest cluster, each from its seed (the clusters themselves are checked against the restatement)"""
    fl = seg.floods[0]
    return max(len(G.bfs_levels(csr, int(s), cls == cls[s])) for s in fl.order[fl.coffs[:-1]])


@pytest.mark.parametrize('which', VARIANTS)
@pytest.mark.parametrize('depth', G.PATH_DEPTHS)
def test_path_depths_around_the_readback_chunk(depth, which):
    csr = G.layered(G.PATH(depth))
    if which == 'relabelled':                                  # the path's end keeps index 0, so the seed and the depth stay
        rng = np.random.default_rng(depth)
        csr = G.relabel(csr, np.concatenate([[0], 1 + rng.permutation(depth - 1)]).astype(np.int64), rng)
    assert len(G.bfs_levels(csr, 0)) == depth
    seg = _separate(np.full(depth, 4, np.int64), csr, None, 1)
    assert len(seg.floods) == 1
    assert seg.floods[0].stats == {'clusters': 1, 'points': depth, 'levels': depth, 'readbacks': _readbacks(depth)}
    assert _readbacks(depth) == {1: 1, 7: 1, 8: 1, 9: 2, 16: 2, 17: 3}[depth]


@pytest.mark.parametrize('which', VARIANTS)
@pytest.mark.parametrize('name', ['SHARE_EDGES', 'CHUNK_EDGES', 'CARRY_EDGES'])
def test_one_cluster_across_block_shares(name, which):
    _, csr, perm = _variant(G.layered(WIDTHS[name]), which)
    n = len(perm)
    levels = len(G.bfs_levels(csr, 0))                          # the seed is the smallest index
    for ic in (None, [4]):
        seg = _separate(np.full(n, 4, np.int64), csr, ic, 1)
        assert seg.floods[0].stats == {'clusters': 1, 'points': n, 'levels': levels, 'readbacks': _readbacks(levels)}


@pytest.mark.parametrize('which', VARIANTS)
@pytest.mark.parametrize('ic', [[2, 1], None])
def test_five_components_flooded_together(ic, which):
    csr, cls = G.class_union()
    _, csr, perm = _variant(csr, which, seed=5)
    cls = G.moved(cls, perm)
    for mp in (1, 3, 4):                                        # 3 folds the one-point cluster, 4 the three-point one too
        seg = _separate(cls, csr, ic, mp)
        assert len(seg.floods) == 1
        levels = _depth(seg, csr, cls)
        assert levels == 9 or which == 'relabelled'
        assert seg.floods[0].stats == {'clusters': 4 if ic else 5, 'points': int((cls != 3).sum()) + (0 if ic else 1),
                                       'levels': levels, 'readbacks': _readbacks(levels)}


@pytest.mark.parametrize('which', VARIANTS)
@pytest.mark.parametrize('split', [False, True])
@pytest.mark.parametrize('tails', [False, True])
def test_frontier_above_262144_entries(batch, tails, split, which):
    """The only inputs whose frontier gives a block a share above 256 entries (a second batch in k_fo_count / k_fo_apply): one
    cluster, then 151 clusters in flight together whose frontiers straddle the shares.  Without tails that frontier is the last
    level; with them every 64th of its entries has a child, so the second batch's counts and carry decide where children go.
    Relabelled, the first node keeps its index: it stays the seed, and the frontier its size."""
    _, csr, perm = G.variants(batch[tails], 9, keep_first=True)[VARIANTS.index(which)]
    cls = G.moved(G.batch_classes(split, tails), perm)
    seg = _separate(cls, csr, None, 1)
    levels = _depth(seg, csr, cls)                              # relabelled, a small cluster's seed may be a leaf: deeper
    assert levels == 3 + tails or (split and which == 'relabelled')
    assert seg.floods[0].stats == {'clusters': 151 if split else 1, 'points': len(cls), 'levels': levels, 'readbacks': 1}


@pytest.mark.parametrize('self_entry', [True, False])
def test_one_point(self_entry):
    csr = (np.array([0, 1 if self_entry else 0], np.int64), np.zeros(1 if self_entry else 0, np.int32))
    for ic in (None, [4], [5]):
        seg = _separate(np.array([4], np.int64), csr, ic, 1)
        assert seg.floods[0].stats['clusters'] == (0 if ic == [5] else 1)
    _separate(np.array([4], np.int64), csr, None, 2)                             # folded into category 0


def test_no_listed_class():
    csr, cls = G.class_union()
    assert not _separate(cls, csr, [], 1).floods                                # an empty list: every class is semantic, nothing floods
    seg = _separate(cls, csr, [77, 78], 1)                                       # no point carries a listed class
    assert seg.floods[0].stats == {'clusters': 0, 'points': 0, 'levels': 0, 'readbacks': 1}
    ctx = f3d.default_context()
    root, order, coffs, flags, stats = ctx.flood_order(cls, csr[0], csr[1], [])
    assert np.array_equal(root, ctx.components_same_class(cls, csr[0], csr[1]))
    assert len(order) == 0 and coffs.tolist() == [0] and not flags.any() and stats['clusters'] == 0 and stats['readbacks'] == 1


# ------------------------------------------------------------------------------------------------ f3d_color_segment
def _color(csr, colors, ids_in, seeds, thr, neutral, ml):
    """ctx.color_segment against the restatement: ids, and the accepted count as the restatement counts it"""
    counts = []
    want = C.color_segment(None, csr, colors, ids_in.copy(), seeds, thr, neutral, ml, counts)
    got, accepted = f3d.default_context().color_segment(colors, csr[0], csr[1], ids_in.copy(), seeds, thr, neutral, ml)
    assert np.array_equal(got, want), (int((got != want).sum()), int((want != ids_in).sum()))
    assert accepted == sum(counts)
    return want, counts


def _one_seed(n, seed):
    ids = np.zeros(n, np.int64)
    ids[seed] = 8
    return ids


@pytest.mark.parametrize('which', VARIANTS)
@pytest.mark.parametrize('name', ['CHUNK_EDGES', 'CARRY_EDGES'])
def test_color_segment_reject_pattern(name, which):
    widths = WIDTHS[name]
    _, csr, perm = _variant(G.layered(widths), which)
    seed, n = int(perm[0]), len(perm)
    for dt in (np.float64, np.float32):
        colors = G.moved(G.reject_colors(widths, 1, dt)[0], perm)
        for thr in THRESHOLDS:
            want, counts = _color(csr, colors, _one_seed(n, seed), [seed], thr, (0,), 0)
            assert counts[0] == (want != _one_seed(n, seed)).sum() + 1 > 3000     # the changed ids plus the accepted seed
    colors = G.moved(G.reject_colors(widths, 1)[0], perm)
    for ml in (1, 2, 3, 4, len(widths) + 5):                                     # nothing; the seed only; one ring; ...
        want, counts = _color(csr, colors, _one_seed(n, seed), [seed], 0.07, (0,), ml)
        assert counts[0] == (want != _one_seed(n, seed)).sum() + (ml > 1)
        assert ml > 2 or counts[0] == ml - 1


@pytest.mark.parametrize('which', VARIANTS)
def test_color_segment_accepts_everything(which):
    _, csr, perm = _variant(G.layered(G.CHUNK_EDGES), which)
    seed, n = int(perm[0]), len(perm)
    for dt in (np.float64, np.float32):
        for ml in (0, -1):
            want, counts = _color(csr, np.full((n, 3), 0.5, dt), _one_seed(n, seed), [seed], 0.1, (0,), ml)
            assert (want == 8).all() and counts == [n]


@pytest.mark.parametrize('which', VARIANTS)
def test_color_segment_several_seeds(which):
    """Two neutral ids, one of them a seed's own id (the whole-cloud pass, needed the first time only); a node rejected by the first
    seed's flood and taken by the second's (the enqueue epoch); a seed that an earlier seed took."""
    from Fusion3DSeg.segUtils.cv import CVSegmentation
    csr, colors, ids, seeds, neutral, _ = G.seeded_colors()
    _, csr, perm = _variant(csr, which, seed=3)
    colors, ids, seeds = G.moved(colors, perm), G.moved(ids, perm), perm[seeds]
    for dt in (np.float64, np.float32):
        for thr in THRESHOLDS:
            for ml in (0, 10):
                want, counts = _color(csr, colors.astype(dt), ids, seeds, thr, neutral, ml)
                assert len(counts) == 4 and all(counts)
    mine = ids.copy()
    out = CVSegmentation(np.zeros(len(ids), np.int64), csr).color_segment(colors, mine, seeds, 0.07, neutral, 0)
    assert out is mine and np.array_equal(mine, C.color_segment(None, csr, colors, ids.copy(), seeds, 0.07, neutral, 0))


# ------------------------------------------------------------------------------------------------ f3d_region_grow
def _values(widths, perm, kind, accept_all):
    dt, nchan = {'f64x1': (np.float64, 1), 'f64x3': (np.float64, 3), 'f32x3': (np.float32, 3)}[kind]
    if accept_all:
        return np.full(len(perm) if nchan == 1 else (len(perm), 3), 0.53125, dt)
    return G.moved(G.reject_colors(widths, 1, dt, nchan)[0], perm)


@pytest.mark.parametrize('which', VARIANTS)
@pytest.mark.parametrize('kind', ['f64x1', 'f64x3', 'f32x3'])
@pytest.mark.parametrize('name', ['CHUNK_EDGES', 'CARRY_EDGES'])
def test_region_grow_from_one_seed(name, kind, which):
    widths = WIDTHS[name]
    _, csr, perm = _variant(G.layered(widths), which)
    seed = int(perm[0])
    ctx = f3d.default_context()
    for accept_all in (False, True):
        val = _values(widths, perm, kind, accept_all)
        thr = 0.07 if kind == 'f64x1' or accept_all else np.array(THRESHOLDS[1])
        for ml in (1, 2, 3, 0):
            for npts0, sma0 in ((0, val[seed]), (5, np.full_like(val[seed], 0.53125))):     # 0.53125 = 17 / 32: exact in float32
                want = R.grow(val, csr, [seed], sma0, npts0, thr, ml, False)
                got = ctx.region_grow(val, csr[0], csr[1], [seed], sma0, npts0, thr, ml)
                assert got.dtype == np.int64 and np.array_equal(got, want), (accept_all, ml, npts0, len(got), len(want))
                if accept_all:
                    assert len(want) == (len(perm) if ml == 0 else sum(widths[:ml - 1]))
                elif ml == 0:
                    assert 2000 < len(want) < len(perm) - 1000


@pytest.mark.parametrize('given', [False, True])
@pytest.mark.parametrize('count', G.SEED_COUNTS)
def test_region_grow_seed_lists_around_the_chunk(count, given):
    """The first queue is the caller's seed list: 1, 1023, 1024, 1025 and 3000 seeds in seeded random order on a relabelled star of
    3100 nodes, about a third of them failing the test (they expand nothing), with the four start rules of the reference."""
    from Fusion3DSeg.segUtils import refinement as M
    _, csr, perm = _variant(G.layered(G.STAR), 'relabelled', seed=13)
    for kind, (dt, nchan) in (('depth', (np.float64, 1)), ('color', (np.float64, 3)), ('color', (np.float32, 3))):
        val, far = G.star_values(2, dt, nchan)
        seeds = G.star_seeds(count, far, perm, 4)
        val = G.moved(val, perm)
        thr = 0.25 if nchan == 1 else np.array([0.25, 0.3, 0.25])
        grow = M.grow_depth if kind == 'depth' else M.grow_color
        want = (R.depth_points if given else R.depth_point)(val, csr, seeds, thr, 50)       # the start rule of a list is the same for
        got = grow(val, csr, seeds, thr, 50, given=given)                                   # depths and colours
        assert np.array_equal(got, want), (kind, dt.__name__, len(got), len(want))
        passing = int((~far[np.argsort(perm)[seeds]]).sum())                                # every near node is reached and accepted,
        assert len(want) == (~far).sum() - (passing if given else 0)                       # but for the given seeds among them
        if count == 1 and nchan == 3 and not given:                                        # one picked index: the colour-point rule
            assert np.array_equal(M.grow_color(val, csr, int(seeds[0]), thr, 50), R.color_point(val, csr, int(seeds[0]), thr, 50))
