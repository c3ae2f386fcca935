"""The deal of k_fuse's tiles to its blocks (csrc/f3d_fuse_deal.h): blocks walk one position per layer, the low block indices through
the most layers.  What can go wrong is a position nobody walks or two blocks walk, a block that runs past its last layer, a skipped
position (its tile lies beyond the cloud) in the middle of a walk, and the ragged last tile.  Labels depend on the point alone, so the
yardstick is oracle/np_ref.py on subsets of the first 3.2M points of the cloud of test_fuse_tile_rotation_gpu.py (shared with it,
read-only), bit for bit: three ways of calling, float64 and float32 storage, the view-chunked call, and tiny clouds on every point."""
import functools

import numpy as np
import pytest

from test_fuse_tile_rotation_gpu import (N_MULTI, NCLASSES, TILE, WAYS, _at, _cloud, _frozen, _fuse, _oracle, _upload,
                                         ctx)  # noqa: F401  (ctx: the module's context fixture)

pytestmark = pytest.mark.gpu

SLOTS, CAP, LAYERS, FACTOR, MOST = 128, 1024, 16, 2, 3    # blocks an XCD holds of the headline's instance; F3D_FUSE_GRID / 8; f3d_fuse_deal.h
N = 6168 * TILE + 131                                     # 3 158 147 points: 6169 tiles, the last one of 131 points
assert N < N_MULTI


def _list_of(ntiles):
    """f3d_xcd_list_of: (xlog, positions per XCD)."""
    xlog = 6
    while xlog > 0 and ntiles < (64 << xlog):
        xlog -= 1
    return xlog, ((ntiles + (8 << xlog) - 1) >> (xlog + 3)) << xlog


def _deal(positions, slots=SLOTS, cap=CAP):
    """f3d_deal_make restated for a list the factoring deal holds within the cap: tiles per block, in block order."""
    assert positions > slots
    tail = slots if positions > 2 * slots else 0
    sizes, left = [1] * tail, positions - tail
    while left > 0:
        each = min(max(-(-left // (FACTOR * slots)), 1), MOST)
        for _ in range(slots):
            if left <= 0:
                break
            t = min(each, left)
            sizes.append(t)
            left -= t
    assert len(sizes) <= cap
    return sorted(sizes, reverse=True)


def _tile(xcd, j, xlog):
    return ((j >> xlog) << (xlog + 3)) + (xcd << xlog) + (j & ((1 << xlog) - 1))


def test_shape_has_three_block_sizes_skipped_positions_and_a_ragged_tile():
    """What N is chosen for, restated from the deal arithmetic with 128 slots per XCD."""
    ntiles = (N + TILE - 1) // TILE
    xlog, positions = _list_of(ntiles)
    assert (ntiles, xlog, positions) == (6169, 6, 832) and N % TILE == 131           # the last tile is ragged
    sizes = _deal(positions)
    assert sizes == [3] * 128 + [2] * 128 + [1] * 192                                # three block sizes, a one-tile tail
    skipped = [(x, j) for x in range(8) for j in range(positions) if _tile(x, j, xlog) >= ntiles]
    assert len(skipped) == 7 * 64 + 39 and {x for x, _ in skipped} == set(range(8))  # positions without a tile, on every XCD


@functools.lru_cache(maxsize=None)
def _subset():
    """Caller-order indices worth checking (sorted, unique): the last tile of every XCD, the tiles of the deepest layer, both ends of
    the cloud and 50k random points."""
    ntiles = (N + TILE - 1) // TILE
    xlog, positions = _list_of(ntiles)
    sizes = _deal(positions)
    width = [sum(1 for s in sizes if s > k) for k in range(max(sizes))]
    start = [sum(width[:k]) for k in range(len(width))]
    t = np.arange(ntiles)
    tiles = [int(t[((t >> xlog) & 7) == x].max()) for x in range(8)]
    tiles += [_tile(x, start[-1] + bx, xlog) for x in range(8) for bx in range(width[-1])]
    parts = [np.arange(1536), np.arange(N - 1536, N)]
    parts += [np.arange(tt * TILE, min((tt + 1) * TILE, N)) for tt in tiles if tt < ntiles]
    parts.append(np.random.default_rng(20250311).integers(0, N, 50_000))
    return _frozen(np.unique(np.concatenate(parts)))


@functools.lru_cache(maxsize=None)
def _want(V, thr):
    want = _oracle(_cloud(N_MULTI)[:N][_subset()], V, thr)
    assert (want != NCLASSES).mean() > (0.05 if thr > 0 else 0.2)                    # the subset sees the cameras
    return _frozen(want)


@pytest.mark.parametrize('thr', [0.5, 0.0])
@pytest.mark.parametrize('f32', [False, True], ids=['f64', 'f32'])
@pytest.mark.parametrize('way', WAYS)
def test_layered_blocks_match_the_oracle(ctx, way, f32, thr):
    import torch
    sel, want = _subset(), _want(3, thr)
    x = _upload(_cloud(N_MULTI)[:N], f32)
    cls, deferred = _fuse(ctx, x, 3, thr, way)                                       # (labels pre-set to the sentinel -7)
    got = _at(cls, sel)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f'{bad.size} of {sel.size} labels differ, the first at point {int(sel[bad[0]])}: got {int(got[bad[0]])}, want {int(want[bad[0]])}'
    assert int((cls == -7).sum()) == 0                                               # every point was written
    cls2, deferred2 = _fuse(ctx, x, 3, thr, way)
    assert deferred2 == deferred and torch.equal(cls2, cls)                          # the same inputs: the same labels, the same points deferred


@pytest.mark.parametrize('f32', [False, True], ids=['f64', 'f32'])
@pytest.mark.parametrize('way', ['sort', 'gather'])
def test_view_chunked_call_on_layered_blocks(ctx, way, f32):
    """4 views in 2 chunks (a decoy perm for the second): equal to the one-shot call everywhere, to the oracle on the subset."""
    import torch
    sel, want = _subset(), _want(4, 0.0)
    x = _upload(_cloud(N_MULTI)[:N], f32)
    one, _ = _fuse(ctx, x, 4, 0.0, way)
    two, _ = _fuse(ctx, x, 4, 0.0, way, bounds=[0, 2, 4])
    assert np.array_equal(_at(one, sel), want)
    assert np.array_equal(_at(two, sel), want)
    assert torch.equal(one, two)


@pytest.mark.parametrize('n', [1, 64, 513, 4097])
def test_small_clouds_every_point(ctx, n):
    pts = _cloud(4097)[:n]
    for thr in (0.5, 0.0):
        want = _oracle(pts, 2, thr)
        for way in WAYS:
            for f32 in (False, True):
                cls, _ = _fuse(ctx, _upload(pts, f32), 2, thr, way)
                assert np.array_equal(cls.cpu().numpy(), want), (n, thr, way, f32)
