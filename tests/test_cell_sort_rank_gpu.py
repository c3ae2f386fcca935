"""The ranking rounds of the cell sort's scatter passes (k_rs_scatter, csrc/f3d_sort.hip): a wave ranks 64 keys through one 64-bit lane
mask per digit value in LDS.  Every cloud here is built for one way that protocol can go wrong -- a digit value shared by a whole round
(lane 63, the full mask), a mask word left over from an earlier round, lanes without a key, eight waves with the same digit values (the
per-wave tables, which lie on the record array), digit values 0 and 255 -- and every case asks the same two things: perm is the stable
argsort of the keys restated in tests/sort_ref.py, and the sorted copy is x[perm] bit for bit.

The clouds are cell centres of a 64 x 64 x 16 lattice, one per key, picked by their restated keys.  Four anchor points with a NaN
coordinate (key 0xFFFF, but their finite coordinates count for the bounding box) pin the box, and so the grid, whatever is picked; they sit
at the end of the cloud, behind the rounds a case is about.  Pass 1 ranks the keys' low bytes in index order; with one low byte for the
whole cloud its output keeps index order, so pass 2 ranks the high bytes in index order: `byte` = 'low' / 'high' aims a pattern at pass 1 /
pass 2.  The intended pattern is asserted on the final cloud's keys before the sort runs."""
import functools

import numpy as np
import pytest

import f3d
import sort_ref as S

pytestmark = pytest.mark.gpu

TILE, WAVE_KEYS, ROUND = 8192, 1024, 64                   # RS_TILE; keys of a wave (16 rounds); keys of a round
NAN = np.float32(np.nan)
ANCHORS = np.array([[NAN, 0, 0], [NAN, 64, 16], [0, NAN, NAN], [64, NAN, NAN]], np.float32)


@pytest.fixture(scope='module')
def ctx():
    return f3d.default_context()


@functools.lru_cache(maxsize=None)
def _lattice():
    """(cell centres float32 [65536, 3], index of the centre with key k [65536]) under the grid the anchors pin."""
    g = S.grid(ANCHORS)
    assert g['bits'] == [6, 6, 4] and g['tables'] and (g['lo'] == 0).all()
    ix, iy, iz = np.meshgrid(np.arange(64), np.arange(64), np.arange(16), indexing='ij')
    pts = (np.stack([ix.ravel(), iy.ravel(), iz.ravel()], axis=1) + 0.5).astype(np.float32)
    keys = S.keys(pts, g)
    assert (np.bincount(keys, minlength=1 << 16) == 1).all()             # one centre per key
    of_key = np.empty(1 << 16, np.int64)
    of_key[keys] = np.arange(len(pts))
    pts.setflags(write=False)
    return pts, of_key


def _cloud(keys):
    """The lattice points with these keys, in this order, and the anchors behind them; checks that the final cloud has these keys."""
    pts, of_key = _lattice()
    x = np.concatenate([pts[of_key[np.asarray(keys, np.int64)]], ANCHORS])
    got = S.keys(x)
    assert np.array_equal(got[:-4], np.asarray(keys, np.uint16)) and (got[-4:] == S.LAST_KEY).all()
    return x, got


def _with_byte(digits, byte):
    """Keys with `digits` as the low byte (pass 1 ranks them) or the high byte (pass 2 does), the other byte 0xFF throughout."""
    d = np.asarray(digits, np.int64)
    return (0xFF00 | d) if byte == 'low' else ((d << 8) | 0xFF)


def _digits(keys, byte):
    return (keys & 0xFF) if byte == 'low' else (keys >> 8)


def _bits(t):
    import torch
    return t.view(torch.int32)


def _sort(ctx, x):
    import torch
    dev = torch.device('cuda', 0)
    xd = torch.tensor(x).to(dev)
    perm = torch.full((len(x),), -1, dtype=torch.int32, device=dev)
    xs = torch.full_like(xd, float('nan'))
    torch.cuda.synchronize(dev)
    ctx.cloud_sort_cells_dev(xd.data_ptr(), f3d.F32, len(x), xs.data_ptr(), perm.data_ptr())
    ctx.synchronize()
    return xd, perm, xs


def _check(ctx, x, keys=None):
    """perm == stable argsort of the restated keys, sorted copy == x[perm] bit for bit; returns perm (device)."""
    import torch
    keys = S.keys(x) if keys is None else keys
    want = S.expected_perm(x)
    assert np.array_equal(want, np.argsort(keys, kind='stable'))
    xd, perm, xs = _sort(ctx, x)
    wd = torch.from_numpy(want).to(perm.device)
    if not torch.equal(perm, wd):
        got = perm.cpu().numpy()
        j = int(np.flatnonzero(got != want)[0])
        pytest.fail(f'n = {len(x)}: {int((got != want).sum())} positions differ, the first at {j}: got index {int(got[j])}, want {int(want[j])} '
                    f'(key {int(keys[want[j]])}); a permutation: {bool((np.bincount(got.clip(0, len(x) - 1), minlength=len(x)) == 1).all())}')
    assert torch.equal(_bits(xs), _bits(xd)[wd.long()]), 'sorted copy != x[perm] bit for bit'
    return perm


# ---------------------------------------------------------------------------------------------------- one digit value for a whole round
@pytest.mark.parametrize('n', [64, 65, 128, 8192, 8193])
def test_all_points_in_one_cell(ctx, n):
    """Both passes: every round has one digit value, its mask is full (lane 63 included) and its leader is lane 0."""
    x = np.repeat(_lattice()[0][12345:12346], n, axis=0)
    keys = S.keys(x)
    assert len(x) == n and (keys == keys[0]).all()
    perm = _check(ctx, x, keys)
    assert np.array_equal(perm.cpu().numpy(), np.arange(n))


@pytest.mark.parametrize('byte', ['low', 'high'])
def test_one_byte_shared_the_other_spread_over_256_values(ctx, byte):
    """byte = 'high': the keys share their high byte and spread over 256 low bytes -- pass 1 sees the spread, pass 2 one digit value in every
    round.  byte = 'low': the other way round."""
    rng = np.random.default_rng(31)
    d = np.concatenate([np.arange(256), rng.integers(0, 256, 9000 - 256)])
    rng.shuffle(d)
    x, keys = _cloud(_with_byte(d, 'high' if byte == 'low' else 'low'))
    shared, spread = _digits(keys, byte), _digits(keys, 'high' if byte == 'low' else 'low')
    assert (shared == 0xFF).all() and len(np.unique(spread)) == 256 and len(x) > TILE
    _check(ctx, x, keys)


# ---------------------------------------------------------------------------------------------------- stale mask words
A, B, C, D = 0x5A, 0xA5, 0x00, 0xFF


def _stale_rounds():
    """The first 8 rounds of wave 0 (digit values per lane)."""
    lanes = np.arange(ROUND)
    even = lanes % 2 == 0
    return [np.where(even, A, B),                         # 0: A on the even lanes
            np.where(even, B, A),                         # 1: A on the odd lanes: a mask word of round 0 that was not cleared shows here
            np.where(even, C, D),                         # 2: no A
            np.where(even, A, C),                         # 3: A again after a round without it
            np.full(ROUND, A),                            # 4: A on all 64 lanes
            np.where(lanes < 32, A, B),                   # 5: the low half of the mask only
            np.where(lanes == 63, A, B),                  # 6: lane 63 alone: the leader of A is the last lane
            np.where(lanes == 0, A, B)]                   # 7: lane 0 alone


@pytest.mark.parametrize('byte', ['low', 'high'])
def test_a_digit_value_on_disjoint_lane_sets_of_consecutive_rounds(ctx, byte):
    rng = np.random.default_rng(32)
    head = np.concatenate(_stale_rounds())
    d = np.concatenate([head, rng.choice([A, B, C, D], TILE + 100 - len(head))])
    x, keys = _cloud(_with_byte(d, byte))
    got = _digits(keys, byte)[:8 * ROUND].reshape(8, ROUND)
    assert (got[0, 0::2] == A).all() and (got[0, 1::2] != A).all()
    assert (got[1, 1::2] == A).all() and (got[1, 0::2] != A).all()
    assert (got[2] != A).all() and (got[3, 0::2] == A).all() and (got[3, 1::2] != A).all()
    assert (got[4] == A).all() and (got[6] == A).sum() == 1 and got[6, 63] == A and (got[7] == A).sum() == 1 and got[7, 0] == A
    assert (_digits(keys, 'high' if byte == 'low' else 'low') == 0xFF).all()       # so pass 2 meets the high bytes in index order
    _check(ctx, x, keys)


# ---------------------------------------------------------------------------------------------------- lanes without a key
@pytest.mark.parametrize('n', [1, 63, 65, 8191, 8193, 2 * 8192 + 1])
def test_ragged_last_round_and_last_tile(ctx, n):
    """The lanes past n neither OR nor read: the last round of the last wave with a key is ragged, and so is the last tile."""
    pts, _ = _lattice()
    x = pts[np.random.default_rng(33).integers(0, len(pts), n)]
    keys = S.keys(x)
    assert len(x) == n and n % ROUND != 0 and len(np.unique(keys)) >= min(n, 50)
    _check(ctx, x, keys)


# ---------------------------------------------------------------------------------------------------- the per-wave tables
@pytest.mark.parametrize('byte', ['low', 'high'])
def test_all_eight_waves_of_a_block_hold_the_same_digit_values(ctx, byte):
    """Every wave of the first tile walks the same 1024 digit values: a wave that touched another wave's masks or counts, or records placed
    over masks still in use, would show."""
    rng = np.random.default_rng(34)
    one = np.concatenate([np.arange(256), rng.integers(0, 256, WAVE_KEYS - 256)])
    rng.shuffle(one)
    x, keys = _cloud(_with_byte(np.tile(one, 8), byte))
    rows = _digits(keys, byte)[:TILE].reshape(8, WAVE_KEYS)
    assert (rows == rows[0]).all() and len(np.unique(rows[0])) == 256 and len(x) == TILE + 4
    _check(ctx, x, keys)


# ---------------------------------------------------------------------------------------------------- digit values 0 and 255, non-finite points
def test_digit_values_0_and_255_with_nonfinite_points_mixed_in(ctx):
    rng = np.random.default_rng(35)
    n = 10_000
    want = rng.integers(0, 1 << 16, n)
    want[rng.integers(0, n, 400)] &= 0xFF00               # low byte 0
    want[rng.integers(0, n, 400)] |= 0x00FF               # low byte 255
    want[rng.integers(0, n, 400)] &= 0x00FF               # high byte 0
    want[rng.integers(0, n, 400)] |= 0xFF00               # high byte 255
    want[[7, 5000]] = [0x0000, 0xFFFF]                    # (0xFFFF: the finite points of the last cell)
    x, _ = _cloud(want)
    bad = rng.choice(n, 300, replace=False)
    x[bad[:100]] = np.nan
    x[bad[100:200], 0] = np.inf
    x[bad[200:], 2] = -np.inf
    want[bad] = S.LAST_KEY
    keys = S.keys(x)
    assert np.array_equal(keys[:-4], want) and S.grid(x)['bits'] == [6, 6, 4]
    for byte in ('low', 'high'):
        d = _digits(keys, byte)
        assert (d == 0).sum() >= 100 and (d == 255).sum() >= 300
    assert (keys == S.LAST_KEY).sum() >= 305 and keys[5000] == S.LAST_KEY and np.isfinite(x[5000]).all()
    _check(ctx, x, keys)


# ---------------------------------------------------------------------------------------------------- random clouds, scratch and mask state
@pytest.mark.parametrize('seed', [36, 37])
def test_random_cloud_twice_on_one_context(ctx, seed):
    import torch
    pts, _ = _lattice()
    x = pts[np.random.default_rng(seed).integers(0, len(pts), 20_000)]
    keys = S.keys(x)
    assert len(np.unique(keys)) >= 10_000
    first = _check(ctx, x, keys)
    second = _check(ctx, x, keys)
    assert torch.equal(first, second)
