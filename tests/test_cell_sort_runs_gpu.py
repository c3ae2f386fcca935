"""The scatter passes of the cell sort (rs_scatter_tile, csrc/f3d_sort.hip) keep a wave's digit counts and tile positions as 16-bit
halves of shared 32-bit words, and pass 1 finds the run of an output position from a bitmap of run starts, a count of the starts in
front of each 64-bit word and gdelta compacted by the rank of the non-empty run.  Every cloud here is built for one way those pieces
can go wrong: a count of 1024 in one half, both halves of a word in use, a tile that is one run, run starts every 32 positions, 64
run starts inside one word, runs of one key across word boundaries, a last run cut by a ragged tile, tiles that hold non-finite points
only.  Each cloud is asked the same things: perm is the stable argsort of the keys restated in tests/sort_ref.py and the sorted copy
is x[perm] bit for bit (f3d_cloud_sort_cells_dev), and the one-shot fused call that sorts (F3D_FUSE_SORT: the route whose sort
launches carry rider blocks) labels every point as oracle/np_ref.py does.

The clouds are cell centres of a 64 x 64 x 16 lattice over the synthetic room, one per key, picked by their restated keys.  Four anchor
points with a NaN coordinate (key 0xFFFF, but their finite coordinates count for the bounding box) pin the box, and so the grid,
whatever is picked; they are the last four points.  Pass 1 ranks the keys' low bytes in index order; with one low byte for the whole
cloud its output keeps index order, so pass 2 ranks the high bytes in index order: `byte` = 'low' / 'high' aims a pattern at pass 1 /
pass 2.  A size is the whole cloud, anchors included."""
import functools

import numpy as np
import pytest

import f3d
import sort_ref as S
from f3d import synth
from oracle import np_ref as O

pytestmark = pytest.mark.gpu

TILE, WAVE_KEYS, WORD = 8192, 1024, 64                    # RS_TILE; keys of a wave (16 rounds); positions of a bitmap word = keys of a round
SIZES = [513, 8191, 8192, 8193, 16385, 24577]             # one ragged tile; a tile less one, exactly, plus one; two and three tiles plus one
SMALL = [1, 63, 64, 65]                                   # sort only (the fused call sorts beyond 512 points)
NAN = np.float32(np.nan)
CELL = np.float32(0.15625)                                # 10 m / 64 cells, exact in float32; the room is [-5, 5] x [-5, 5] x [0, 2.5]
LO = np.array([-5, -5, 0], np.float32)
HI = LO + CELL * np.array([64, 64, 16], np.float32)
ANCHORS = np.array([[NAN, LO[1], LO[2]], [NAN, HI[1], HI[2]], [LO[0], NAN, NAN], [HI[0], NAN, NAN]], np.float32)
V, H, W, MAX_DEPTH, NCLASSES = 4, 64, 64, 10.0, 133


@pytest.fixture(scope='module')
def ctx():
    return f3d.default_context()


@functools.lru_cache(maxsize=None)
def _lattice():
    """(cell centres float32 [65536, 3], index of the centre with key k [65536]) under the grid the anchors pin."""
    g = S.grid(ANCHORS)
    assert g['bits'] == [6, 6, 4] and g['tables'] and np.array_equal(g['lo'], LO.astype(np.float64))
    ix, iy, iz = np.meshgrid(np.arange(64), np.arange(64), np.arange(16), indexing='ij')
    pts = LO + CELL * (np.stack([ix.ravel(), iy.ravel(), iz.ravel()], axis=1).astype(np.float32) + np.float32(0.5))
    assert pts.dtype == np.float32
    keys = S.keys(pts, g)
    assert (np.bincount(keys, minlength=1 << 16) == 1).all()             # one centre per key
    of_key = np.empty(1 << 16, np.int64)
    of_key[keys] = np.arange(len(pts))
    pts.setflags(write=False)
    return pts, of_key


def _cloud(keys, nonfinite=()):
    """The lattice points with these keys, in this order, the points at `nonfinite` made NaN, and the anchors behind them; checks that
    the final cloud has these keys (0xFFFF at the NaN points)."""
    pts, of_key = _lattice()
    want = np.asarray(keys, np.int64).copy()
    x = np.concatenate([pts[of_key[want]], ANCHORS])
    bad = np.asarray(nonfinite, np.int64)
    x[bad] = NAN
    want[bad] = S.LAST_KEY
    got = S.keys(x)
    assert np.array_equal(got[:-4], want.astype(np.uint16)) and (got[-4:] == S.LAST_KEY).all()
    return x, got


def _with_byte(digits, byte, other=0xFF):
    """Keys with `digits` as the low byte (pass 1 ranks them) or the high byte (pass 2 does), the other byte `other` throughout."""
    d = np.asarray(digits, np.int64)
    return ((other << 8) | d) if byte == 'low' else ((d << 8) | other)


def _digits(keys, byte):
    return (keys & 0xFF) if byte == 'low' else (keys >> 8)


def _tiles(d):
    return [d[a:a + TILE] for a in range(0, len(d), TILE)]


def _bits(t):
    import torch
    return t.view(torch.int32)


def _check_sort(ctx, x, keys=None):
    """perm == stable argsort of the restated keys, sorted copy == x[perm] bit for bit; returns perm (device)."""
    import torch
    keys = S.keys(x) if keys is None else keys
    want = S.expected_perm(x)
    assert np.array_equal(want, np.argsort(keys, kind='stable'))
    dev = torch.device('cuda', 0)
    xd = torch.tensor(x).to(dev)
    perm = torch.full((len(x),), -1, dtype=torch.int32, device=dev)
    xs = torch.full_like(xd, float('nan'))
    torch.cuda.synchronize(dev)
    ctx.cloud_sort_cells_dev(xd.data_ptr(), f3d.F32, len(x), xs.data_ptr(), perm.data_ptr())
    ctx.synchronize()
    wd = torch.from_numpy(want).to(dev)
    if not torch.equal(perm, wd):
        got = perm.cpu().numpy()
        j = int(np.flatnonzero(got != want)[0])
        pytest.fail(f'n = {len(x)}: {int((got != want).sum())} positions differ, the first at {j}: got index {int(got[j])}, want {int(want[j])} '
                    f'(key {int(keys[want[j]])}); a permutation: {bool((np.bincount(got.clip(0, len(x) - 1), minlength=len(x)) == 1).all())}')
    assert torch.equal(_bits(xs), _bits(xd)[wd.long()]), 'sorted copy != x[perm] bit for bit'
    return perm


@functools.lru_cache(maxsize=None)
def _scene():
    """(K, wxyz, t, packed views, masks uint8 [V, H, W] of 8x8 blocks of 12 labels)"""
    K = np.array([[0.78 * W, 0, W / 2], [0, 0.78 * W, H / 2], [0, 0, 1]])
    q, t = synth.ring_views(V)
    b = np.random.default_rng(7).integers(0, 12, (V, H // 8, W // 8)).astype(np.uint8)
    m = np.ascontiguousarray(np.repeat(np.repeat(b, 8, axis=1), 8, axis=2))
    for a in (K, q, t, m):
        a.setflags(write=False)
    return K, q, t, f3d.views_build(K, W, H, q, t, MAX_DEPTH), m


def _check_fused(ctx, x):
    """The one-shot call with F3D_FUSE_SORT against the oracle's labels; returns the labels."""
    import torch
    K, q, t, views, m = _scene()
    with np.errstate(all='ignore'):
        want = O.project_vote_argmax(np.asarray(x, np.float64), K, q, t, m, MAX_DEPTH, NCLASSES, 0.0, None)
    dev = torch.device('cuda', 0)
    n = len(x)
    xd = torch.tensor(x).to(dev)
    vd = torch.from_numpy(np.array(views)).to(dev)
    md = torch.from_numpy(np.array(m)).to(dev)
    cls = torch.full((n,), -7, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    ctx.project_vote_argmax_dev(xd.data_ptr(), f3d.F32, n, vd.data_ptr(), V, md.data_ptr(), H, W, NCLASSES, 0.0, None, cls.data_ptr(), None, None,
                                flags=f3d.FUSE_SORT)
    ctx.take_device_error(None)
    torch.cuda.synchronize(dev)
    got = cls.cpu().numpy()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f'n = {n}: {bad.size} labels differ, the first at point {int(bad[0])}: got {int(got[bad[0]])}, want {int(want[bad[0]])}'
    return got


def _check(ctx, x, keys):
    _check_sort(ctx, x, keys)
    return _check_fused(ctx, x)


# ---------------------------------------------------------------------------------------------------- the patterns, as digit values per key
def _one_value(m, value):
    return np.full(m, value)


def _every_value_32_each(m, rng):
    """Per tile a shuffle of 32 keys of each of the 256 values: a run starts every 32 positions, two per bitmap word."""
    out = []
    for a in range(0, m, TILE):
        d = np.repeat(np.arange(256), TILE // 256)
        rng.shuffle(d)
        out.append(d[:m - a])
    return np.concatenate(out)


def _singles_and_one_big(m, rng, big):
    """Per tile one key of every value but `big`, scattered, and `big` everywhere else: 255 runs of one key side by side (64 run starts
    in one word, across word boundaries), in front of the big run (big = 255) or behind it (big = 0)."""
    d = np.full(m, big)
    singles = np.array([v for v in range(256) if v != big])
    for a in range(0, m, TILE):
        size = min(TILE, m - a)
        if size >= 255:
            d[a + rng.choice(size, 255, replace=False)] = singles
    return d


def _pattern(name, m, rng):
    if name == 'one_even':
        return _one_value(m, 0x5A)
    if name == 'one_odd':
        return _one_value(m, 0xA5)
    if name == 'two_values':
        return rng.choice([0x12, 0x92], m)
    if name == 'every_value_32_each':
        return _every_value_32_each(m, rng)
    if name == 'singles_big_lowest':
        return _singles_and_one_big(m, rng, 0)
    if name == 'singles_big_highest':
        return _singles_and_one_big(m, rng, 255)
    if name == 'neighbours':
        return rng.choice([0x40, 0x41], m)                    # the two halves of one count word, ~512 keys of each per wave
    raise KeyError(name)


PATTERNS = ['one_even', 'one_odd', 'two_values', 'every_value_32_each', 'singles_big_lowest', 'singles_big_highest', 'neighbours']


def _assert_pattern(name, d):
    """The intended shape, on the digit values of the final cloud (anchors excluded)."""
    for t in _tiles(d):
        c = np.bincount(t, minlength=256)
        if name in ('one_even', 'one_odd'):
            assert (c > 0).sum() == 1 and (len(t) < WAVE_KEYS or c.max() >= WAVE_KEYS)
        elif name == 'two_values':
            assert (c > 0).sum() <= 2
        elif name == 'every_value_32_each' and len(t) == TILE:
            assert (c == 32).all()
        elif name.startswith('singles') and len(t) >= 255:
            assert (c == 1).sum() == 255 and (c > 0).sum() == (256 if len(t) > 255 else 255)
        elif name == 'neighbours' and len(t) == TILE:
            w = np.stack([np.bincount(v, minlength=256) for v in t.reshape(8, WAVE_KEYS)])
            assert (w[:, 0x40] > 400).all() and (w[:, 0x41] > 400).all() and (w[:, 0x40] + w[:, 0x41] == WAVE_KEYS).all()


@pytest.mark.parametrize('byte', ['low', 'high'])
@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('name', PATTERNS)
def test_pattern(ctx, name, n, byte):
    """513 and 8191 points: a ragged tile whose count is no multiple of 64, its last run cut; 8193 and beyond: a last tile that holds one
    anchor -- a non-finite point -- and nothing else."""
    rng = np.random.default_rng(41)
    d = _pattern(name, n - 4, rng)
    x, keys = _cloud(_with_byte(d, byte))
    assert len(x) == n and np.array_equal(_digits(keys, byte)[:-4], d)
    assert (_digits(keys, 'high' if byte == 'low' else 'low') == 0xFF).all()       # so pass 2 meets the high bytes in index order
    _assert_pattern(name, d)
    _check(ctx, x, keys)


@pytest.mark.parametrize('n', SIZES)
def test_two_cells_that_differ_in_one_byte(ctx, n):
    rng = np.random.default_rng(42)
    for a, b in ((0x1234, 0x9234), (0x1234, 0x12B4)):                  # the high byte only; the low byte only
        x, keys = _cloud(rng.choice([a, b], n - 4))
        assert set(keys[:-4].tolist()) == {a, b}
        _check(ctx, x, keys)


@pytest.mark.parametrize('n', SIZES)
def test_nonfinite_points_mixed_in_and_alone_in_a_tile(ctx, n):
    """Random keys with one point in 16 non-finite; from 16385 points on the second tile holds non-finite points only."""
    rng = np.random.default_rng(43)
    m = n - 4
    want = rng.integers(0, 1 << 16, m)
    bad = np.flatnonzero(rng.random(m) < 1 / 16)
    if m > 2 * TILE:
        bad = np.union1d(bad, np.arange(TILE, 2 * TILE))
    x, keys = _cloud(want, bad)
    assert (keys == S.LAST_KEY).sum() >= 4 + len(bad) and (m <= 2 * TILE or (keys[TILE:2 * TILE] == S.LAST_KEY).all())
    got = _check(ctx, x, keys)
    assert (got[bad] == NCLASSES).all() and (got[:-4] != NCLASSES).any()          # a non-finite point has no label; the room is seen


@pytest.mark.parametrize('n', SMALL)
def test_small_clouds_sort_only(ctx, n):
    pts, _ = _lattice()
    x = pts[np.random.default_rng(44).integers(0, len(pts), n)]
    _check_sort(ctx, x)
    one = np.repeat(pts[12345:12346], n, axis=0)
    assert np.array_equal(_check_sort(ctx, one).cpu().numpy(), np.arange(n))


def test_largest_case_then_smallest_on_one_context(ctx):
    """Scratch reuse: what the three-tile cloud left in the sort's scratch (keys, records, histograms) must not show in the next sorts."""
    rng = np.random.default_rng(45)
    big, kb = _cloud(_with_byte(_singles_and_one_big(SIZES[-1] - 4, rng, 0), 'low'))
    small, ks = _cloud(_with_byte(_every_value_32_each(SIZES[0] - 4, rng), 'low'))
    _check(ctx, big, kb)
    _check(ctx, small, ks)
    _check_sort(ctx, small[:1])
    _check(ctx, big, kb)
