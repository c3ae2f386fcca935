"""The cell sort (f3d_cloud_sort_cells_dev, csrc/f3d_sort.hip) as a sort: its permutation equals the stable argsort of the keys restated
in tests/sort_ref.py, exactly, and the sorted copy is x[perm] bit for bit -- over the wave, tile, partial-box and sample-stride boundaries,
both block shapes of the key kernel, both record widths at 2^24 points, the float64 key path, degenerate clouds, non-finite points, outliers
inside and outside the sampled box, both launcher forms, scratch reuse and a side stream."""
import functools

import numpy as np
import pytest

import f3d
import sort_ref as S
from f3d import synth

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
WIDE = (1 << 24) + 1                                      # the first n with 64-bit records


@pytest.fixture(scope='module')
def ctx():
    return f3d.default_context()


def _frozen(a):
    a.setflags(write=False)
    return a


def _explain(perm, keys, want):
    """Why perm != want: what tells a kernel bug from a slip of the restatement."""
    n = len(want)
    inside = (perm >= 0) & (perm < n)
    is_perm = bool(inside.all()) and bool((np.bincount(perm, minlength=n) == 1).all())
    msg = [f'n = {n}: perm is {"a" if is_perm else "NOT a"} permutation']
    if is_perm:
        ks = keys[perm].astype(np.int64)
        dk, dp = np.diff(ks), np.diff(perm.astype(np.int64))
        msg.append(f'keys[perm] is {"" if (dk >= 0).all() else "NOT "}non-decreasing ({int((dk < 0).sum())} descents)')
        msg.append(f'ties are {"" if (dp[dk == 0] > 0).all() else "NOT "}in ascending index ({int((dp[dk == 0] <= 0).sum())} out of order)')
    j = int(np.flatnonzero(perm != want)[0])
    key_of = lambda i: int(keys[i]) if 0 <= i < n else None
    msg.append(f'{int((perm != want).sum())} positions differ, the first at {j}: got index {int(perm[j])} (key {key_of(int(perm[j]))}), '
               f'want index {int(want[j])} (key {key_of(int(want[j]))})')
    return '; '.join(msg)


def _bits(t):
    import torch
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _sort(ctx, x, copy=True, side_stream=False):
    """perm int32 [n] on the device (and the sorted copy) of one f3d_cloud_sort_cells_dev call on the context's stream, or on a side stream
    right behind the torch kernel that writes the cloud."""
    import torch
    dev = torch.device('cuda', 0)
    n = len(x)
    xd = torch.tensor(x).to(dev)                          # (a copy: the shared clouds are read-only)
    perm = torch.full((n,), -1, dtype=torch.int32, device=dev)
    xs = torch.full_like(xd, float('nan')) if copy else None
    dt = f3d.F32 if x.dtype == F32 else f3d.F64
    if side_stream:
        late = torch.zeros_like(xd)
        s = torch.cuda.Stream(dev)
        torch.cuda.synchronize(dev)
        late.copy_(xd)                                    # still in flight on the current stream when the sort is enqueued
        s.wait_stream(torch.cuda.current_stream(dev))     # torch streams do not wait for it by themselves
        with torch.cuda.stream(s):
            ctx.cloud_sort_cells_dev(late.data_ptr(), dt, n, xs.data_ptr() if copy else None, perm.data_ptr(), s.cuda_stream)
            s.synchronize()
    else:
        torch.cuda.synchronize(dev)
        ctx.cloud_sort_cells_dev(xd.data_ptr(), dt, n, xs.data_ptr() if copy else None, perm.data_ptr())
        ctx.synchronize()
    return xd, perm, xs


def _check(ctx, x, copy=True, side_stream=False, keys=None):
    """The core assertion; returns (expected permutation on the host, perm and sorted copy on the device)."""
    import torch
    keys = S.keys(x) if keys is None else keys
    want = np.argsort(keys, kind='stable').astype(np.int32)
    xd, perm, xs = _sort(ctx, x, copy, side_stream)
    wd = torch.from_numpy(want).to(perm.device)
    if not torch.equal(perm, wd):
        pytest.fail(_explain(perm.cpu().numpy(), keys, want))
    if copy:
        assert torch.equal(_bits(xs), _bits(xd)[wd.long()]), 'sorted copy != x[perm] bit for bit'
    return want, perm, xs


def _distinct(keys):
    return int(np.count_nonzero(np.bincount(keys, minlength=1 << 16)))


# ---------------------------------------------------------------------------------------------------- the room cloud, small sizes
SMALL = [1, 2, 63, 64, 65, 511, 512, 513, 8191, 8192, 8193, 16128, 16129, 65536, 65537, 131071, 131072, 131073]


@pytest.mark.parametrize('dtype', [F64, F32], ids=['f64', 'f32'])
@pytest.mark.parametrize('n', SMALL)
def test_room_cloud_across_wave_tile_box_and_stride_boundaries(ctx, n, dtype):
    """64: a wave; 8192: a tile (and a partial last one); 16128 = 63 * 256 sampled points: 63 / 64 partial boxes; 65536 / 131072: the
    sample stride 1 -> 2 (n >> 16) and its first odd tail."""
    x = synth.cloud(n, dtype=dtype)
    keys = S.keys(x)
    assert _distinct(keys) >= (1000 if n >= 8191 else n // 2 + 1)
    assert S.sample_stride(n) == (2 if n >= 131072 else 1)
    _check(ctx, x, keys=keys)


# ---------------------------------------------------------------------------------------------------- block shapes and record widths
@functools.lru_cache(maxsize=None)
def _big_room():
    return _frozen(synth.cloud(WIDE, dtype=F32))


@functools.lru_cache(maxsize=None)
def _big_lattice():
    return _frozen(S.lattice_cloud(WIDE))


@pytest.mark.parametrize('n', [4_186_112, 4_186_113])
def test_key_kernel_block_shapes(ctx, n):
    """511 tiles: the 512-thread k_rs_keys; 512 tiles: the 256-thread one (ntiles < 512)."""
    assert (n + 8191) // 8192 == (511 if n == 4_186_112 else 512)
    x = _big_room()[:n]
    keys = S.keys(x)
    assert _distinct(keys) >= 1000
    _check(ctx, x, keys=keys)


@pytest.mark.parametrize('cloud', ['room', 'lattice'])
@pytest.mark.parametrize('n', [1 << 24, WIDE])
def test_record_widths_at_2_pow_24(ctx, n, cloud):
    """n = 2^24: 32-bit records with the largest 24-bit index; 2^24 + 1: run_passes<uint64_t> (64-bit records, 72 KB of dynamic LDS).  The room
    cloud uses every key; on the lattice each key holds ~32 768 points spread over all 2048 tiles: stability across waves, rounds and tiles."""
    x = (_big_room() if cloud == 'room' else _big_lattice())[:n]
    keys = S.keys(x)
    if cloud == 'room':
        assert _distinct(keys) == 65536
    else:
        assert _distinct(keys) <= 512 and np.bincount(keys).max() > 4 * 8192
    _check(ctx, x, keys=keys)


# ---------------------------------------------------------------------------------------------------- degenerate clouds
@pytest.mark.parametrize('n', [70_001, 9_000])
@pytest.mark.parametrize('kind', ['identical', 'plane', 'thin-f64', 'thin-f32'])
def test_degenerate_clouds(ctx, n, kind):
    if kind == 'identical':
        x = np.repeat(synth.cloud(1), n, axis=0)
    elif kind == 'plane':
        x = synth.cloud(n)
        x[:, 2] = 1.25
    else:
        x = S.thin_cloud(n, dtype=F64 if kind == 'thin-f64' else F32)
    g = S.grid(x)
    assert g['bits'] == {'identical': [6, 5, 5], 'plane': [8, 8, 0]}.get(kind, [12, 2, 2])
    assert g['tables'] == (not kind.startswith('thin'))                # the thin cloud: cell_of, float64
    want = _check(ctx, x)[0]
    if kind == 'identical':
        assert np.array_equal(want, np.arange(n))
    else:
        assert _distinct(S.keys(x, g)) >= 1000


@pytest.mark.parametrize('dtype', [F64, F32], ids=['f64', 'f32'])
def test_nonfinite_points_come_last_in_index_order(ctx, dtype):
    n = 70_000
    pts, base, flagged = S.nonfinite_cloud(n, dtype)
    pts[40_500] = base[np.setdiff1d(np.arange(n), flagged)].max(axis=0)         # a finite point of the last cell, among the flagged ones
    g = S.grid(pts)
    assert g['bits'] == [6, 6, 4] and g['tables']
    keys = S.keys(pts, g)
    assert keys[40_500] == 65535 and (keys[flagged] == 65535).all() and _distinct(keys) >= 1000
    want = _check(ctx, pts, keys=keys)[0]
    tail = want[-int((keys == 65535).sum()):]
    assert (np.diff(tail) > 0).all() and set(tail.tolist()) == set(flagged.tolist()) | set(np.flatnonzero(keys == 65535).tolist())
    assert 40_500 in tail[1:-1]


@pytest.mark.parametrize('dtype', [F64, F32], ids=['f64', 'f32'])
@pytest.mark.parametrize('at', [99_999, 100_000], ids=['sampled', 'unsampled'])
def test_finite_outlier(ctx, at, dtype):
    """n = 200 001: every third point is sampled for the box.  A sampled (1e6, 0, 0) stretches the grid to 65536 x 1 x 1 (float64 path); an
    unsampled one leaves the grid alone and is clamped into a border cell."""
    x = S.outlier_cloud(200_001, at, dtype)
    g = S.grid(x)
    assert S.sample_stride(len(x)) == 3 and (at % 3 == 0) == (g['bits'] == [16, 0, 0]) and g['tables'] == (at % 3 != 0)
    keys = S.keys(x, g)
    if at % 3:
        assert _distinct(keys) >= 1000
    _check(ctx, x, keys=keys)


# ---------------------------------------------------------------------------------------------------- launcher forms, reuse, streams
@pytest.mark.parametrize('n', [65, 131_073])
def test_perm_without_a_sorted_copy(ctx, n):
    """sorted_xyz = NULL (what F3D_FUSE_SORT passes) gives the same permutation."""
    x = synth.cloud(n, dtype=F32)
    assert np.array_equal(_check(ctx, x, copy=False)[0], _check(ctx, x, copy=True)[0])


def test_scratch_reuse_gives_the_same_perm(ctx):
    import torch
    a, b = synth.cloud(131_073), synth.cloud(65)
    keys = S.keys(a)
    assert _distinct(keys) >= 1000
    _, first, first_xs = _check(ctx, a, keys=keys)
    _check(ctx, b)
    _, third, third_xs = _check(ctx, a, keys=keys)
    assert torch.equal(first, third) and torch.equal(_bits(first_xs), _bits(third_xs))


@pytest.mark.parametrize('dtype', [F64, F32], ids=['f64', 'f32'])
def test_sort_on_a_side_stream_behind_the_writer(ctx, dtype):
    x = synth.cloud(1_000_003, dtype=dtype)
    keys = S.keys(x)
    assert _distinct(keys) >= 1000
    _check(ctx, x, side_stream=True, keys=keys)
