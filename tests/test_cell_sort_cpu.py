"""Known answers of tests/sort_ref.py, the NumPy restatement of the cell sort's key (csrc/f3d_sort.hip) that
tests/test_cell_sort_gpu.py holds the kernels to.  No GPU: these keep the restatement itself honest -- grids, keys and permutations worked out
by hand from the kernel source, the table / float64 path choice, non-finite points, sampled and unsampled outliers -- and check that the
clouds of the gpu file are not trivial inputs."""
import numpy as np
import pytest

import sort_ref as S
from f3d import synth
from sort_ref import lattice_cloud, nonfinite_cloud, outlier_cloud, thin_cloud


def test_cube_corners():
    corners = np.array([[x, y, z] for x in (0., 1.) for y in (0., 1.) for z in (0., 1.)])
    g = S.grid(corners)
    assert g['bits'] == [6, 5, 5] and g['dim'] == [64, 32, 32] and g['tables']
    assert S.keys(corners).tolist() == [0, 4681, 9362, 14043, 51492, 56173, 60854, 65535]
    assert np.array_equal(S.expected_perm(corners), np.arange(8))
    assert S.keys(corners.astype(np.float32)).tolist() == S.keys(corners).tolist()


def test_spread_tables_partition_the_key_bits():
    for bits in ([6, 5, 5], [6, 6, 4], [12, 2, 2], [16, 0, 0], [8, 8, 0], [0, 0, 16]):
        full = [int(S.spread_table(c, bits)[-1]) for c in range(3)]                   # every bit of the axis set
        assert full[0] | full[1] | full[2] == 0xFFFF and full[0] + full[1] + full[2] == 0xFFFF
        for c in range(3):
            t = S.spread_table(c, bits)
            assert len(t) == 1 << bits[c] and len(np.unique(t)) == len(t) and (np.diff(t.astype(np.int64)) > 0).all()
    # the bit-by-bit loop of cell_of on one cell
    bits, idx = [6, 6, 4], (0b101101, 0b010011, 0b1001)
    key = 0
    for level in range(15, -1, -1):
        for c in range(3):
            if bits[c] > level:
                key = (key << 1) | ((idx[c] >> level) & 1)
    assert key == sum(int(S.spread_table(c, bits)[idx[c]]) for c in range(3))


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_room_cloud_takes_the_table_path(dtype):
    x = synth.cloud(100_000, dtype=dtype)
    g = S.grid(x)
    assert g['bits'] == [6, 6, 4] and g['tables'] and S.sample_stride(len(x)) == 1
    k = S.keys(x)
    assert k.dtype == np.uint16 and len(np.unique(k)) > 50_000
    assert np.array_equal(k, S.keys(synth.cloud(100_000, dtype=np.float64)))          # the storage type changes nothing
    p = S.expected_perm(x)
    assert p.dtype == np.int32 and np.array_equal(np.sort(p), np.arange(len(x)))
    ks = k[p].astype(np.int64)
    assert (np.diff(ks) >= 0).all() and (np.diff(p)[np.diff(ks) == 0] > 0).all()      # sorted, ties in index order


def test_thin_cloud_takes_the_float64_path():
    x = thin_cloud(70_001)
    g = S.grid(x)
    assert g['bits'] == [12, 2, 2] and not g['tables'] and S.sample_stride(len(x)) == 1
    assert len(np.unique(S.keys(x))) > 30_000
    # the cell of a point by plain Python floats
    i = 12345
    cell = [min(max(int((float(x[i, c]) - float(g['lo'][c])) * float(g['inv_cell'][c])), 0), g['dim'][c] - 1) for c in range(3)]
    assert int(S.keys(x)[i]) == sum(int(S.spread_table(c, g['bits'])[cell[c]]) for c in range(3))


@pytest.mark.parametrize('n', [1, 9_000, 70_001])
def test_identical_points(n):
    x = np.repeat(synth.cloud(1), n, axis=0)
    g = S.grid(x)
    assert g['bits'] == [6, 5, 5]                                                     # three extents of 1e-12: ties go to the first axis
    assert np.unique(S.keys(x)).tolist() == [0]
    assert np.array_equal(S.expected_perm(x), np.arange(n))


def test_plane_cloud():
    x = synth.cloud(70_001)
    x[:, 2] = 1.25
    g = S.grid(x)
    assert g['bits'] == [8, 8, 0] and g['tables']
    assert len(np.unique(S.keys(x))) > 30_000


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_nonfinite_points_get_the_last_key_and_leave_the_grid_alone(dtype):
    pts, base, flagged = nonfinite_cloud(70_000, dtype)
    g, g0 = S.grid(pts), S.grid(base)
    assert g['bits'] == g0['bits'] == [6, 6, 4] and np.array_equal(g['lo'], g0['lo']) and np.array_equal(g['inv_cell'], g0['inv_cell'])
    # (and not by luck: the flagged points may have held the box's extreme values: the box of the unflagged rest is the same too)
    rest = np.delete(base, flagged, axis=0)
    assert np.array_equal(g['lo'], S.grid(rest)['lo']) and np.array_equal(g['inv_cell'], S.grid(rest)['inv_cell'])
    k, k0 = S.keys(pts), S.keys(base, g)
    assert (k[flagged] == 65535).all()
    keep = np.ones(len(pts), bool); keep[flagged] = False
    assert np.array_equal(k[keep], k0[keep])
    assert np.array_equal(np.flatnonzero(k != k0), flagged[k0[flagged] != 65535])     # exactly those points changed
    p = S.expected_perm(pts)
    tail = p[k[p] == 65535]
    assert set(flagged) <= set(tail.tolist()) and (np.diff(tail) > 0).all()           # last, in index order


def test_finite_outlier_sampled_and_unsampled():
    n = 200_001
    assert S.sample_stride(n) == 3
    base = synth.cloud(n)
    g0, k0 = S.grid(base), S.keys(base)
    assert g0['bits'] == [6, 6, 4]
    off = outlier_cloud(n, 100_000)                                                   # 100000 % 3 == 1: the box never sees it
    assert 100_000 % 3 == 1
    g = S.grid(off)
    assert g['bits'] == g0['bits'] and np.array_equal(g['lo'], g0['lo']) and np.array_equal(g['inv_cell'], g0['inv_cell'])
    assert np.flatnonzero(S.keys(off) != k0).tolist() == [100_000]
    x_last = int(S.spread_table(0, g['bits'])[-1])
    assert int(S.keys(off)[100_000]) & x_last == x_last                               # clamped into the border cells of x
    on = outlier_cloud(n, 99_999)
    g = S.grid(on)
    assert g['bits'] == [16, 0, 0] and not g['tables']
    k = S.keys(on)
    assert int(k[99_999]) == 65535 and k[np.arange(n) != 99_999].max() < 65535 and len(np.unique(k)) <= 3


def test_saturating_conversion_is_restated():
    """Values the device's float -> int conversion saturates (and NumPy's does not) land in the border cells."""
    x = synth.cloud(9_000)
    g = S.grid(x)
    x[7] = (1e20, -1e20, 1.5)
    x[8] = (-1e20, 1e20, 1.5)
    k = S.keys(x, g)
    last = [int(S.spread_table(c, g['bits'])[-1]) for c in range(3)]
    zmid = int(S.spread_table(2, g['bits'])[8])                                       # trunc(1.5 * 16 / 3.0000003) = 7 or 8
    assert int(k[7]) & ~last[2] == last[0] and int(k[8]) & ~last[2] == last[1]
    assert int(k[7]) & last[2] in (zmid, int(S.spread_table(2, g['bits'])[7]))


def test_the_gpu_inputs_are_not_trivial():
    """The gpu file asserts the same next to each use: a 'room' input has >= 1000 distinct keys wherever it has that many points, a 'lattice'
    input at most 512 -- and several 8192-key tiles per key at the sizes that test stability."""
    for n in (8191, 16129, 65537, 131073, 200_001):
        for dtype in (np.float64, np.float32):
            assert len(np.unique(S.keys(synth.cloud(n, dtype=dtype)))) >= 1000
    x = lattice_cloud(300_000)
    k = S.keys(x)
    assert S.grid(x)['bits'] == [6, 6, 4] and 400 <= len(np.unique(k)) <= 512
