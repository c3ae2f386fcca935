"""The one-shot fused call that sorts (F3D_FUSE_SORT) runs label presence, k_fuse_setup with the code book, mask coding and the label fill
as rider blocks inside the cell sort's launches (csrc/f3d_fuse_blocks.h, csrc/f3d_sort.hip).  What can go wrong is a rider slice that
misses a piece of its work (the last bytes of the masks, an odd width, an unaligned pointer), a role mapping that drops a sort tile, a
book built before presence is complete, and the 64-bit record instantiation of the sort with its large LDS.  Labels depend on the point
alone, so the yardstick is oracle/np_ref.py, bit for bit (and the uint16 vote rows where votes are asked for); the call without
F3D_FUSE_SORT has no riders and serves as a second yardstick for the cloud too large for the oracle."""
import functools

import numpy as np
import pytest

import f3d
from f3d import synth
from oracle import np_ref as O

pytestmark = pytest.mark.gpu

MAX_DEPTH, NCLASSES = 10.0, 133
ODD = (37, 53)                                            # H x W: neither a multiple of 8, 37 * 53 * V odd for odd V


@pytest.fixture(scope='module')
def ctx():
    return f3d.default_context()


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _cloud(n):
    return _frozen(synth.cloud(n, dtype=np.float32))


def _K(h, w):
    return np.array([[0.78 * w, 0, w / 2], [0, 0.78 * w, h / 2], [0, 0, 1]])


@functools.lru_cache(maxsize=None)
def _views(V, h, w):
    q, t = synth.ring_views(V)
    return q, t, _frozen(f3d.views_build(_K(h, w), w, h, q, t, MAX_DEPTH))


@functools.lru_cache(maxsize=None)
def _masks(V, h, w, lo, k, seed=7):
    """uint8 [V, h, w]: 8x8 blocks of the k labels lo..lo+k-1, every one of which occurs (written at k places spread from the first byte
    to the last)."""
    rng = np.random.default_rng(seed)
    b = rng.integers(lo, lo + k, (V, (h + 7) // 8, (w + 7) // 8)).astype(np.uint8)
    m = np.ascontiguousarray(np.repeat(np.repeat(b, 8, axis=1), 8, axis=2)[:, :h, :w])
    flat = m.reshape(-1)
    flat[np.linspace(0, flat.size - 1, k).astype(np.int64)] = np.arange(lo, lo + k, dtype=np.uint8)
    return _frozen(m)


def _oracle(pts, V, h, w, masks, thr, flt=None, votes=False):
    q, t, _ = _views(V, h, w)
    with np.errstate(all='ignore'):
        return O.project_vote_argmax(np.asarray(pts, np.float64), _K(h, w), q, t, masks, MAX_DEPTH, NCLASSES, thr, flt, return_votes=votes)


def _call(ctx, pts, V, h, w, masks, thr, flt=None, votes=False, sort=True, offset=0, stream='side', f32=True, perm=False, bounds=None):
    """One fused call on device tensors -> labels (numpy) or (labels, votes).  offset: the mask pointer is that many bytes past an
    aligned allocation.  stream: 'side' = a stream of the caller's, 'ctx' = the context's own."""
    import torch
    dev = torch.device('cuda', 0)
    n = len(pts)
    x = torch.from_numpy(np.array(pts, dtype=np.float32 if f32 else np.float64)).to(dev)
    dt = f3d.F32 if f32 else f3d.F64
    vd = torch.from_numpy(np.array(_views(V, h, w)[2])).to(dev)
    buf = torch.zeros(masks.size + 16, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 16 == 0
    md = buf[offset:offset + masks.size]
    md.copy_(torch.from_numpy(np.array(masks)).reshape(-1))
    cls = torch.full((n,), -7, dtype=torch.int64, device=dev)
    vo = torch.full((n, NCLASSES + 1), -1, dtype=torch.int16, device=dev) if votes else None
    s = torch.cuda.Stream(dev) if stream == 'side' else None
    if s is not None:
        s.wait_stream(torch.cuda.current_stream(dev))
    else:
        torch.cuda.synchronize(dev)
    sp = None if s is None else s.cuda_stream
    flags, pp = (f3d.FUSE_SORT if sort else 0), None
    if perm:                                                                   # the prepared-layout route: the caller's perm, no sort in the call
        flags = f3d.FUSE_GATHER
        pm = torch.full((n,), -1, dtype=torch.int32, device=dev)
        ctx.cloud_sort_cells_dev(x.data_ptr(), dt, n, None, pm.data_ptr(), sp)
        pp = pm.data_ptr()
    if bounds is None:
        ctx.project_vote_argmax_dev(x.data_ptr(), dt, n, vd.data_ptr(), V, md.data_ptr(), h, w, NCLASSES, thr, flt, cls.data_ptr(),
                                    None if vo is None else vo.data_ptr(), sp, flags=flags, perm_ptr=pp)
    else:
        present = torch.empty(256, dtype=torch.uint8, device=dev)
        ctx.mask_presence_dev(md.data_ptr(), V, h, w, present.data_ptr(), sp)
        ctx.fuse_chunked_begin_dev(present.data_ptr(), n, V, h, w, NCLASSES, flt, sp)
        for a, b in zip(bounds[:-1], bounds[1:]):
            ctx.fuse_chunk_dev(x.data_ptr(), dt, n, vd.data_ptr(), V, a, b, md.data_ptr(), h, w, NCLASSES, thr, flt, cls.data_ptr(), sp, flags=flags)
    ctx.take_device_error(sp)
    if s is not None:
        s.synchronize()
    else:
        torch.cuda.synchronize(dev)
    assert int(buf[:offset].sum()) == 0 and int(buf[offset + masks.size:].sum()) == 0      # the masks' surroundings were not written
    got = cls.cpu().numpy()
    return (got, vo.cpu().numpy().view(np.uint16)) if votes else got


def _check(got, want, what):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f'{what}: {bad.size} of {want.size} labels differ, the first at point {int(bad[0])}: got {int(got[bad[0]])}, want {int(want[bad[0]])}'


# ---------------------------------------------------------------------------------------------------- cloud sizes
@pytest.mark.parametrize('thr', [0.5, 0.0])
@pytest.mark.parametrize('n', [513, 8192, 8193, 20011])
def test_cloud_sizes_match_the_oracle(ctx, n, thr):
    """513 points: one sort tile beside hundreds of rider blocks; 8192 / 8193: one tile exactly / a second tile of one key."""
    h, w = ODD
    m = _masks(3, h, w, 0, 8)
    pts = _cloud(20011)[:n]
    want = _oracle(pts, 3, h, w, m, thr)
    assert (want != NCLASSES).mean() > (0.05 if thr > 0 else 0.5)
    _check(_call(ctx, pts, 3, h, w, m, thr), want, f'n={n} thr={thr}')


def test_wide_records_beyond_2_pow_24_points(ctx):
    """2^24 + 5000 points: the sort's 64-bit records (83 / 75 KB of LDS per block, which a rider block holds too).  The whole vector
    against the same call without the sort (no riders), a seeded 50 000-point sample against the oracle."""
    n = (1 << 24) + 5000
    h, w = ODD
    m = _masks(2, h, w, 0, 8)
    pts = _cloud(n)
    got = _call(ctx, pts, 2, h, w, m, 0.0)
    plain = _call(ctx, pts, 2, h, w, m, 0.0, sort=False)
    assert int((got == -7).sum()) == 0
    _check(got, plain, 'sorting call against the plain call')
    sel = np.random.default_rng(20250101).integers(0, n, 50_000)
    _check(got[sel], _oracle(pts[sel], 2, h, w, m, 0.0), 'sample against the oracle')


# ---------------------------------------------------------------------------------------------------- mask shapes
@pytest.mark.parametrize('offset', [0, 1, 4, 8])
@pytest.mark.parametrize('V', [1, 3, 64, 70])
def test_odd_masks_unaligned_pointers_and_view_counts(ctx, V, offset):
    """37 x 53 masks (the byte-wise forms of presence and coding), 37 * 53 * V bytes (odd for odd V: a tail beyond the last 8-byte word
    when the pointer is aligned), the pointer 1 and 4 bytes off an 8-byte boundary and 8 bytes off a 16-byte one (the presence rider's
    16-byte pairs then start at the second word); 70 views are two view groups."""
    h, w = ODD
    m = _masks(V, h, w, 0, 40)
    pts = _cloud(8193)
    _check(_call(ctx, pts, V, h, w, m, 0.0, offset=offset), _oracle(pts, V, h, w, m, 0.0), f'V={V} offset={offset}')


@pytest.mark.parametrize('offset', [0, 4])
def test_width_multiple_of_8_odd_height(ctx, offset):
    """41 x 24 masks: the 8-byte forms of coding and of presence (W % 8 == 0) with a last tile row of one pixel row, the pointer aligned
    (16-byte pairs from the first byte) and 4 bytes off (byte-wise)."""
    h, w = 41, 24
    m = _masks(3, h, w, 0, 8)
    pts = _cloud(8193)
    _check(_call(ctx, pts, 3, h, w, m, 0.0, offset=offset), _oracle(pts, 3, h, w, m, 0.0), f'offset={offset}')


# ---------------------------------------------------------------------------------------------------- label coverage
@pytest.mark.parametrize('V', [1, 3])
def test_labels_only_in_the_first_and_the_last_mask_byte(ctx, V):
    """Label 0 occurs only in the first byte of the first mask, label 1 only in the last byte of the last; points that see those pixels
    are labelled 0 and 1 at threshold 0.  A presence slice that misses either byte gives the label no bin; a coding slice that misses it
    leaves the pixel without a sample."""
    h, w = ODD
    rng = np.random.default_rng(7)
    m = rng.integers(10, 21, (V, h, w)).astype(np.uint8)
    m.reshape(-1)[0] = 0
    m.reshape(-1)[-1] = 1
    pts = _cloud(50000)
    want = _oracle(pts, V, h, w, m, 0.0)
    assert (want == 0).any() and (want == 1).any()
    for offset in (0, 1, 8):
        _check(_call(ctx, pts, V, h, w, m, 0.0, offset=offset), want, f'V={V} offset={offset}')


# ---------------------------------------------------------------------------------------------------- books
@pytest.mark.parametrize('thr', [0.5, 0.0])
@pytest.mark.parametrize('k', [8, 40, 100, 134])
def test_presence_books_of_every_k_fuse_instance(ctx, k, thr):
    h, w = 64, 72                                                              # W % 8 == 0: the vector forms
    m = _masks(4, h, w, 0, k)
    assert np.unique(m).size == k
    pts = _cloud(20011)
    _check(_call(ctx, pts, 4, h, w, m, thr), _oracle(pts, 4, h, w, m, thr), f'k={k} thr={thr}')


@pytest.mark.parametrize('thr', [0.5, 0.0])
@pytest.mark.parametrize('flt', [[3, 5, 7], [0, 1, 2, 3, 4, 5, 6, 7], [0, 1, 2, 3, 4, 5, 6, 7, 8, 9], [86, 114, 115]], ids=['3', '8', '10', 'absent'])
def test_filter_lists(ctx, flt, thr):
    """Up to 8 filter classes: the filter book, no presence rider.  10: the presence book with the filter applied at the end."""
    h, w = ODD
    m = _masks(3, h, w, 0, 12)
    pts = _cloud(20011)
    _check(_call(ctx, pts, 3, h, w, m, thr, flt=flt), _oracle(pts, 3, h, w, m, thr, flt), f'filter={flt} thr={thr}')


@pytest.mark.parametrize('flt', [None, [3, 5, 7]], ids=['nofilter', 'filter3'])
def test_vote_rows(ctx, flt):
    """Votes requested: a short filter list no longer picks the filter book (every label needs its bin)."""
    h, w = ODD
    m = _masks(3, h, w, 0, 12)
    pts = _cloud(8193)
    want, wv = _oracle(pts, 3, h, w, m, 0.0, flt, votes=True)
    got, gv = _call(ctx, pts, 3, h, w, m, 0.0, flt=flt, votes=True)
    _check(got, want, 'labels')
    assert np.array_equal(gv.astype(np.int64), np.asarray(wv, np.int64))


# ---------------------------------------------------------------------------------------------------- sequences
def test_two_alphabets_on_one_context_and_both_streams(ctx):
    """Presence is consumed by the book and left zero: the second call's alphabet is disjoint from the first's.  Then the same two calls
    on the context's own stream."""
    h, w = ODD
    a, b = _masks(3, h, w, 0, 40), _masks(3, h, w, 50, 8, seed=11)
    pts = _cloud(20011)
    wa, wb = _oracle(pts, 3, h, w, a, 0.0), _oracle(pts, 3, h, w, b, 0.0)
    for stream in ('side', 'ctx'):
        _check(_call(ctx, pts, 3, h, w, a, 0.0, stream=stream), wa, f'first alphabet, {stream}')
        _check(_call(ctx, pts, 3, h, w, b, 0.0, stream=stream), wb, f'second alphabet, {stream}')
        _check(_call(ctx, pts, 3, h, w, b, 0.5, stream=stream, f32=False), _oracle(pts, 3, h, w, b, 0.5), f'float64 cloud, {stream}')


# ---------------------------------------------------------------------------------------------------- routes without riders
def test_caller_perm_and_chunked_routes_still_match(ctx):
    h, w = ODD
    m = _masks(4, h, w, 0, 12)
    pts = _cloud(20011)
    want = _oracle(pts, 4, h, w, m, 0.0)
    _check(_call(ctx, pts, 4, h, w, m, 0.0, perm=True), want, "caller's perm")
    _check(_call(ctx, pts, 4, h, w, m, 0.0, bounds=[0, 2, 4]), want, 'view-chunked entry')
    _check(_call(ctx, pts, 4, h, w, m, 0.0), want, 'one-shot call afterwards')
