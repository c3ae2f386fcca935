"""The rotated tile loop of k_fuse (csrc/f3d_fuse.hip): a block requests its next tile's points while the current tile finishes, so
what can go wrong is a block that walks more than one tile (above 8192 x 512 points), the positions a block skips, the ragged last tile,
a tile requested past the end, and a point that leaks from one tile into the next.  Labels depend on the point alone, so the yardstick
is oracle/np_ref.py on subsets of a 4.2M-point cloud, bit for bit, three ways of calling (the call sorts; caller's perm + gather; no
perm), float64 and float32 storage, the view-chunked call, unusable points at tile seams, tiny clouds and an exact-size last point."""
import functools

import numpy as np
import pytest

import f3d
from f3d import synth
from oracle import np_ref as O

pytestmark = pytest.mark.gpu

TILE, GRID = 512, 8192                                    # points per tile (256 threads x 2) and blocks per launch of k_fuse
N_MULTI = GRID * TILE + 8 * TILE * 3 + 131                # 4 206 723: 8217 tiles; 25 blocks of XCD 0 walk two, every other block one
H = W = 256
K = np.array([[200., 0, 128], [0, 200., 128], [0, 0, 1]])
MAX_DEPTH, NCLASSES = 10.0, 133
WAYS = ['sort', 'gather', 'plain']


@pytest.fixture(scope='module')
def ctx():
    return f3d.default_context()


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _cloud(n):
    return _frozen(synth.cloud(n, dtype=np.float32))      # drawn as float32: both storages hold the same points


@functools.lru_cache(maxsize=None)
def _scene(V):
    q, t = synth.ring_views(V)
    return dict(q=q, t=t, masks=_frozen(synth.masks(V, H, W, 'block64')), views=_frozen(f3d.views_build(K, W, H, q, t, MAX_DEPTH)))


def _oracle(pts, V, thr):
    sc = _scene(V)
    with np.errstate(all='ignore'):
        return O.project_vote_argmax(np.asarray(pts, np.float64), K, sc['q'], sc['t'], sc['masks'], MAX_DEPTH, NCLASSES, thr, None)


@functools.lru_cache(maxsize=None)
def _subset(n):
    """Caller-order indices worth checking in a cloud of n points (sorted, unique)."""
    ntiles = (n + TILE - 1) // TILE
    t = np.arange(ntiles)
    assert ntiles >= 64 * 64                              # chunks of 64 tiles, dealt to the 8 XCDs in turn
    last_of_xcd = [int(t[((t >> 6) & 7) == x].max()) for x in range(8)]
    second = [tt for tt in range(GRID, ntiles)]           # the tiles a block reaches at its second position
    parts = [np.arange(1536), np.arange(n - 2048, n)]
    parts += [np.arange(tt * TILE, min((tt + 1) * TILE, n)) for tt in last_of_xcd + second]
    parts.append(np.random.default_rng(20240607).integers(0, n, 50_000))
    return _frozen(np.unique(np.concatenate(parts)))


@functools.lru_cache(maxsize=None)
def _want_multi(V, thr):
    """The oracle's labels on the subset of the multi-tile cloud: computed once, shared, read-only."""
    want = _oracle(_cloud(N_MULTI)[_subset(N_MULTI)], V, thr)
    assert (want != NCLASSES).mean() > (0.05 if thr > 0 else 0.2)          # the subset sees the cameras
    return _frozen(want)


def _upload(pts, f32):
    """Exact-size device tensor of the cloud in the asked storage."""
    import torch
    return torch.from_numpy(np.array(pts, dtype=np.float32 if f32 else np.float64)).to(torch.device('cuda', 0))   # (a copy: the shared clouds are read-only)


def _fuse(ctx, x, V, thr, way, bounds=None):
    """One fused call on a device-resident cloud -> (labels on the device, deferred counts).  way: 'sort' = F3D_FUSE_SORT, 'gather' = the
    cell sort's perm handed over with F3D_FUSE_GATHER, 'plain' = no perm.  bounds: view-chunk boundaries for the view-chunked entry."""
    import torch
    dev = x.device
    sc = _scene(V)
    n = x.shape[0]
    dt = f3d.F32 if x.dtype == torch.float32 else f3d.F64
    vd, md = torch.from_numpy(np.array(sc['views'])).to(dev), torch.from_numpy(np.array(sc['masks'])).to(dev)
    cls = torch.full((n,), -7, dtype=torch.int64, device=dev)
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        flags, perm, decoy = 0, None, None
        if way == 'sort':
            flags = f3d.FUSE_SORT
        elif way == 'gather':
            flags = f3d.FUSE_GATHER
            perm = torch.full((n,), -1, dtype=torch.int32, device=dev)          # exact size
            ctx.cloud_sort_cells_dev(x.data_ptr(), dt, n, None, perm.data_ptr(), s.cuda_stream)
            decoy = torch.zeros(n, dtype=torch.int32, device=dev)               # later chunks: in bounds, wrong, and not to be read
        if bounds is None:
            ctx.project_vote_argmax_dev(x.data_ptr(), dt, n, vd.data_ptr(), V, md.data_ptr(), H, W, NCLASSES, thr, None, cls.data_ptr(), None,
                                        s.cuda_stream, flags=flags, perm_ptr=None if perm is None else perm.data_ptr())
        else:
            present = torch.empty(256, dtype=torch.uint8, device=dev)
            ctx.mask_presence_dev(md.data_ptr(), V, H, W, present.data_ptr(), s.cuda_stream)
            ctx.fuse_chunked_begin_dev(present.data_ptr(), n, V, H, W, NCLASSES, None, s.cuda_stream)
            for a, b in zip(bounds[:-1], bounds[1:]):
                pp = None if perm is None else (perm if a == 0 else decoy).data_ptr()
                ctx.fuse_chunk_dev(x.data_ptr(), dt, n, vd.data_ptr(), V, a, b, md.data_ptr(), H, W, NCLASSES, thr, None, cls.data_ptr(),
                                   s.cuda_stream, flags=flags, perm_ptr=pp)
        ctx.take_device_error(s.cuda_stream)                                   # clean: raises otherwise
        s.synchronize()
    return cls, ctx.fuse_deferred()


def _at(cls, idx):
    import torch
    return cls[torch.from_numpy(np.asarray(idx, np.int64)).to(cls.device)].cpu().numpy()


# ---------------------------------------------------------------------------------------------------- blocks that walk two tiles
def test_shape_has_one_and_two_tile_blocks_and_skipped_positions():
    """What N_MULTI is chosen for, restated from the tile mapping: 17 chunk rows of 64 tiles per XCD, 1024 blocks per XCD."""
    ntiles = (N_MULTI + TILE - 1) // TILE
    assert ntiles == 8217 and N_MULTI % TILE == 131
    rows = (ntiles + 511) // 512
    per_xcd, gx = rows * 64, GRID // 8
    tile = lambda xcd, j: ((j >> 6) << 9) + (xcd << 6) + (j & 63)
    walks = {(xcd, bx): [j for j in range(bx, per_xcd, gx) if tile(xcd, j) < ntiles] for xcd in range(8) for bx in range(gx)}
    counts = np.bincount([len(v) for v in walks.values()])
    assert counts.tolist() == [0, GRID - 25, 25]                               # 25 blocks with a second tile, all of XCD 0
    assert all(len(walks[(0, bx)]) == 2 for bx in range(25))
    assert sum(1 for xcd in range(1, 8) for bx in range(per_xcd - gx) if tile(xcd, gx + bx) >= ntiles) == 7 * 64   # positions skipped


@pytest.mark.parametrize('thr', [0.5, 0.0])
@pytest.mark.parametrize('f32', [False, True], ids=['f64', 'f32'])
@pytest.mark.parametrize('way', WAYS)
def test_multi_tile_blocks_match_the_oracle(ctx, way, f32, thr):
    sel = _subset(N_MULTI)
    want = _want_multi(3, thr)
    x = _upload(_cloud(N_MULTI), f32)
    cls, deferred = _fuse(ctx, x, 3, thr, way)
    got = _at(cls, sel)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f'{bad.size} of {sel.size} labels differ, the first at point {int(sel[bad[0]])}: got {int(got[bad[0]])}, want {int(want[bad[0]])}'
    cls2, deferred2 = _fuse(ctx, x, 3, thr, way)
    assert deferred2 == deferred                                               # the same inputs defer the same points
    import torch
    assert torch.equal(cls2, cls)
    assert int((cls == -7).sum()) == 0                                         # every point was written


# ---------------------------------------------------------------------------------------------------- the view-chunked call
@pytest.mark.parametrize('f32', [False, True], ids=['f64', 'f32'])
@pytest.mark.parametrize('way', ['sort', 'gather'])
def test_view_chunked_call_on_multi_tile_blocks(ctx, way, f32):
    """4 views in 2 chunks: the first chunk reads the cloud through perm and leaves the cell-order copy, the second streams that copy
    (it is handed a decoy perm it must not read).  Equal to the one-shot call everywhere and to the oracle on the subset."""
    import torch
    sel = _subset(N_MULTI)
    want = _want_multi(4, 0.0)
    x = _upload(_cloud(N_MULTI), f32)
    one, _ = _fuse(ctx, x, 4, 0.0, way)
    two, _ = _fuse(ctx, x, 4, 0.0, way, bounds=[0, 2, 4])
    assert np.array_equal(_at(one, sel), want)
    assert np.array_equal(_at(two, sel), want)
    assert torch.equal(one, two)


# ---------------------------------------------------------------------------------------------------- unusable points at tile seams
@pytest.mark.parametrize('f32', [False, True], ids=['f64', 'f32'])
@pytest.mark.parametrize('way', ['plain', 'sort'])
def test_unusable_points_at_tile_seams_leave_their_neighbours_alone(ctx, way, f32):
    n = N_MULTI
    second = GRID * TILE                                                       # first lane of block 0's second tile ('plain': caller order is tile order)
    at = [511, 512, 513, n - 1, second, second + TILE - 1]
    values = [np.nan, np.inf, -np.inf, 1e300 if not f32 else 3e38, np.nan, -np.inf]
    pts = _cloud(n).astype(np.float32 if f32 else np.float64)
    for k, (i, v) in enumerate(zip(at, values)):
        pts[i, k % 3] = v
    near = np.unique(np.concatenate([np.arange(max(i - 64, 0), min(i + 65, n)) for i in at]))
    want = _oracle(pts[near], 3, 0.0)
    clean = _oracle(_cloud(n)[near], 3, 0.0)
    untouched = ~np.isin(near, at)
    assert np.array_equal(want[untouched], clean[untouched])                    # (labels depend on the point alone)
    cls, deferred = _fuse(ctx, _upload(pts, f32), 3, 0.0, way)
    assert np.array_equal(_at(cls, near), want)
    assert deferred[0] >= len(at)                                              # the unusable points went to the later tiers
    sel = _subset(n)
    keep = ~np.isin(sel, at)
    assert np.array_equal(_at(cls, sel[keep]), _want_multi(3, 0.0)[keep])


# ---------------------------------------------------------------------------------------------------- blocks without a next tile
@pytest.mark.parametrize('n', [1, 63, 64, 65, 511, 512, 513, 4097])
def test_small_clouds_every_point(ctx, n):
    pts = _cloud(4097)[:n]
    for thr in (0.5, 0.0):
        want = _oracle(pts, 2, thr)
        for way in WAYS:
            for f32 in (False, True):
                cls, _ = _fuse(ctx, _upload(pts, f32), 2, thr, way)
                assert np.array_equal(cls.cpu().numpy(), want), (n, thr, way, f32)


# ---------------------------------------------------------------------------------------------------- the last point
@pytest.mark.parametrize('f32', [False, True], ids=['f64', 'f32'])
@pytest.mark.parametrize('way', ['gather', 'plain'])
def test_last_point_of_an_exact_size_cloud(ctx, way, f32):
    """n = 8192 * 512 + 1: one block walks a second tile that holds a single point; xyz and perm are exact-size allocations."""
    n = GRID * TILE + 1
    pts = _cloud(N_MULTI)[:n]
    tail = np.arange(n - 600, n)
    want = _oracle(pts[tail], 3, 0.0)
    x = _upload(pts, f32)
    assert x.shape == (n, 3) and x.is_contiguous()
    cls, _ = _fuse(ctx, x, 3, 0.0, way)
    assert np.array_equal(_at(cls, tail), want)
    assert int((cls == -7).sum()) == 0
