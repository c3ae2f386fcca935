"""Restatement of the cell sort's key (csrc/f3d_sort.hip: f3d_launch_cell_sort, k_bbox_partial, grid_from_partials, k_rs_keys), the
oracle of tests/test_cell_sort_*.py.  NumPy only, operation for operation: the library is built with -ffp-contract=off, so every
product and sum below rounds on its own, in the kernel's type.  The two radix passes are stable, so the keys are the whole
specification of the permutation: expected_perm(x) = argsort(keys(x), kind='stable')."""
import numpy as np

KEY_BITS = 16                                             # F3D_SORT_KEY_BITS
LUT_CELLS = 1024                                          # RS_LUT: the float32 table path while no axis has more cells
LAST_KEY = (1 << KEY_BITS) - 1                            # also the key of every point that is not `ok`


def sample_stride(n):
    """f3d_launch_cell_sort: the bounding box looks at x[::stride]."""
    return n >> 16 if n > (1 << 16) else 1


def sample_box(x):
    """-> (lo [3], ext [3]) float64 of the strided sample: per coordinate only |v| < 1e300 counts (k_bbox_partial), an axis without
    such a value gets lo = 0, ext = 0, and ext is floored to 1e-12 by `!(ext > 1e-12)` (grid_from_partials)."""
    x = np.asarray(x)
    s = x[::sample_stride(len(x))].astype(np.float64)
    lo, ext = np.zeros(3), np.zeros(3)
    for c in range(3):
        v = s[:, c]
        v = v[np.abs(v) < 1e300]
        if v.size:
            lo[c] = v.min()
            ext[c] = v.max() - lo[c]
        if not ext[c] > 1e-12:
            ext[c] = 1e-12
    return lo, ext


def deal_bits(ext):
    """The key bits dealt one at a time to the axis whose cell, ext / 2^bits, is currently the longest; strict `>`, so the first
    axis wins ties."""
    bits = [0, 0, 0]
    for _ in range(KEY_BITS):
        best, bl = 0, -1.0
        for c in range(3):
            length = float(ext[c]) / float(1 << bits[c])
            if length > bl:
                bl, best = length, c
        bits[best] += 1
    return bits


def grid(x):
    """-> dict(lo, inv_cell float64 [3]; bits, dim int [3]; tables bool): the f3d_cellgrid of grid_from_partials."""
    lo, ext = sample_box(x)
    bits = deal_bits(ext)
    dim = [1 << b for b in bits]
    inv_cell = np.array([np.float64(dim[c]) / (ext[c] * np.float64(1.0000001)) for c in range(3)])
    return dict(lo=lo, inv_cell=inv_cell, bits=bits, dim=dim, tables=all(d <= LUT_CELLS for d in dim))


def spread_table(c, bits):
    """uint32 [2^bits[c]]: spread_axis(i, c, bits) for every cell index of axis c -- a Morton code with per-axis bit counts: from the
    most significant level down, the axes that still have a bit at that level contribute it, in the order x, y, z."""
    i = np.arange(1 << bits[c], dtype=np.uint32)
    key = np.zeros_like(i)
    pos = KEY_BITS
    for level in range(KEY_BITS - 1, -1, -1):
        for a in range(3):
            if bits[a] > level:
                pos -= 1
                if a == c:
                    key |= ((i >> np.uint32(level)) & np.uint32(1)) << np.uint32(pos)
    return key


def _cells(v, lo, inv, dim):
    """trunc((v - lo) * inv) clamped to [0, dim - 1], in v's type.  The clamp comes before the conversion and NaN maps to cell 0: the
    device's float -> int conversion saturates and turns NaN into 0, NumPy's does neither."""
    with np.errstate(all='ignore'):
        f = (v - lo) * inv
        f = np.where(f == f, f, 0)
        return np.clip(f, 0, dim - 1).astype(np.int64)


def keys(x, g=None):
    """uint16 [n]: k_rs_keys.  Table path (every dim <= 1024): lo, inv_cell and the coordinate converted to float32, ok = |x| < 1e30f on
    all three coordinates (cell_index).  Otherwise the same arithmetic in float64 with the threshold 1e300 (cell_of)."""
    x = np.asarray(x)
    g = grid(x) if g is None else g
    ft, big = (np.float32, np.float32(1e30)) if g['tables'] else (np.float64, np.float64(1e300))
    key = np.zeros(len(x), np.uint32)
    ok = np.ones(len(x), bool)
    for c in range(3):
        with np.errstate(all='ignore'):
            v = x[:, c].astype(ft)
        ok &= np.abs(v) < big
        key |= spread_table(c, g['bits'])[_cells(v, ft(g['lo'][c]), ft(g['inv_cell'][c]), g['dim'][c])]
    return np.where(ok, key, np.uint32(LAST_KEY)).astype(np.uint16)


def expected_perm(x, g=None):
    """int32 [n]: the permutation f3d_cloud_sort_cells_dev must return (both LSD passes are stable: equal keys keep index order)."""
    return np.argsort(keys(x, g), kind='stable').astype(np.int32)


# ---- the clouds both test files sort -------------------------------------------------------------------------------------------
def _room(n, dtype=np.float64):
    from f3d import synth
    return synth.cloud(n, dtype=dtype)


def thin_cloud(n, dtype=np.float64, seed=21):
    """Uniform in [0, 1000] x [0, 1] x [0, 1], drawn as float32: 12 + 2 + 2 bits, 4096 cells along x (beyond the tables)."""
    rng = np.random.default_rng(seed)
    return (rng.random((n, 3), dtype=np.float32) * np.array([1000, 1, 1], np.float32)).astype(dtype)


def lattice_cloud(n, dtype=np.float32, seed=22):
    """Every coordinate one of 8 values per axis of the room's box: at most 512 distinct keys, so a key's run spans many tiles."""
    rng = np.random.default_rng(seed)
    axes = np.stack([np.linspace(-5, 5, 8), np.linspace(-5, 5, 8), np.linspace(0, 3, 8)]).astype(np.float32)
    pick = rng.integers(0, 8, (n, 3), dtype=np.uint8)
    return np.stack([axes[c][pick[:, c]] for c in range(3)], axis=1).astype(dtype)


def nonfinite_cloud(n, dtype=np.float64):
    """(cloud with the flagged points, the same cloud without, the flagged indices)."""
    base = _room(n, dtype=dtype)
    pts = base.copy()
    with np.errstate(over='ignore'):
        pts[::1000] = np.nan
        pts[1::1000, 0] = np.inf
        pts[5] = 1e308                                    # float32 storage: +inf
    flagged = np.unique(np.concatenate([np.arange(0, n, 1000), np.arange(1, n, 1000), [5]]))
    return pts, base, flagged


def outlier_cloud(n, at, dtype=np.float64):
    pts = _room(n, dtype=dtype)
    pts[at] = (1e6, 0, 0)
    return pts
