"""PointVotingSegmentation on the GPU: the fused radius search + frame vote (f3d_point_vote_frames*) and the last-column segment
against the reference's fixture and against the test-only restatement.  Everything here is bit-exact: the votes are integer counts."""
import numpy as np
import pytest

import f3d
import point_voting_ref as ref
from Fusion3DSeg.segUtils.voting import PointVotingSegmentation

pytestmark = pytest.mark.gpu
PREFIX, EXT, ZFILL = 'm_', 'png', 3


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def _object(g, dirname, masks, present=None, frames=None):
    from PIL import Image
    h, w = (int(x) for x in g['hw'])
    frames = g['frames'] if frames is None else frames
    for j, n in enumerate(g['frame_numbers']):
        if present is None or present[j]:
            Image.fromarray(masks[j].reshape(h, w)).save(dirname / f'{PREFIX}{str(n).zfill(ZFILL)}.{EXT}')
    tof = [{'modPoints': frames[j], 'frameNumber': str(n)} for j, n in enumerate(g['frame_numbers'])]
    return PointVotingSegmentation(tof, g['cloud'], (h, w), str(dirname), int(g['nclasses']), prefix=PREFIX, extension=EXT, zfill=ZFILL)


def test_fixture_scenes_through_the_file_api(golden, tmp_path):
    g = golden('point_voting')
    r = float(g['radius'])
    pv = _object(g, tmp_path, g['a_masks'], g['a_present'])
    out = pv.vote(radius=r, resize=False, filename=str(tmp_path / 'out' / 'votes.npy'))
    assert out is pv.votes and _same(out, g['a_votes_all']) and _same(np.load(tmp_path / 'out' / 'votes.npy'), g['a_votes_all'])
    assert _same(pv.vote(radius=r, resize=False), g['a_votes_twice'])                 # a second call accumulates
    pv.zero()
    assert pv.votes.shape == g['a_votes_all'].shape and not pv.votes.any()
    assert _same(pv.vote(skip=2, radius=r, resize=False), g['a_votes_skip2'])
    pv.zero()
    assert _same(pv.vote(frame_numbers=g['a_subset'], radius=r, resize=False), g['a_votes_subset'])
    pv.zero()
    assert _same(pv.vote(radius=r, resize=True), g['a_votes_all'])                    # the masks already have the depth size
    nns, freq = pv.get_nns(g['frames'][0], r)
    assert nns.dtype == np.int32 and _same(freq, g['e_frequency'])
    offs = np.concatenate([[0], np.cumsum(freq)])
    want = np.concatenate([np.sort(g['e_nns'][offs[i]:offs[i + 1]]) for i in range(len(freq))])
    assert _same(nns, want)


def test_out_of_range_labels_raise_only_where_a_pixel_has_a_neighbour(golden, tmp_path):
    g = golden('point_voting')
    r = float(g['radius'])
    (tmp_path / 'b').mkdir(); (tmp_path / 'c').mkdir(); (tmp_path / 'v').mkdir()
    pv = _object(g, tmp_path / 'b', g['b_masks'])
    assert _same(pv.vote(radius=r, resize=False), g['b_votes'])                       # label 200 on pixels that see nothing
    pv = _object(g, tmp_path / 'c', g['c_masks'])
    with pytest.raises(IndexError, match='point_vote_frames'):
        pv.vote(radius=r, resize=False)
    assert _same(pv.votes, g['c_votes'])                                              # frames 0 and 1 applied, 2 and 3 not
    pv.zero()
    pv.maskdir = str(tmp_path / 'b')
    assert _same(pv.vote(radius=r, resize=False), g['b_votes'])                       # the error was consumed
    # non-finite depth points: sklearn's ValueError at that frame; with both offences the first offending frame decides
    bad = g['frames'].copy()
    bad[3, 5, 2] = np.inf
    pv = _object(g, tmp_path / 'v', g['c_masks'], frames=bad)
    with pytest.raises(IndexError):
        pv.vote(radius=r, resize=False)
    assert _same(pv.votes, g['c_votes'])
    bad = g['frames'].copy()
    bad[1, 7, 0] = np.nan
    pv = _object(g, tmp_path / 'v', g['c_masks'], frames=bad)
    want = np.zeros_like(g['c_votes'])
    ref.vote(want, g['cloud'], g['frames'][:1], g['c_masks'][:1], r)
    for frame_numbers in (None, [0, 1, 2, 3]):
        pv.zero()
        with pytest.raises(ValueError, match='NaN or infinity'):
            pv.vote(frame_numbers=frame_numbers, radius=r, resize=False)
        assert _same(pv.votes, want)
    with pytest.raises(ValueError):
        PointVotingSegmentation([], np.array([[0.0, np.nan, 0.0]]), (2, 2), '.', 3)


def test_host_pointer_entry_matches_and_keeps_partial_votes(golden):
    g = golden('point_voting')
    ctx = f3d.default_context()
    r, F = float(g['radius']), len(g['frames'])
    votes = np.zeros_like(g['b_votes'])
    ctx.point_vote_frames(votes, g['cloud'].astype(np.float32), g['frames'].astype(np.float32), g['b_masks'], r)   # (lattice: exact in float32)
    assert _same(votes, g['b_votes'])
    votes = np.zeros_like(g['c_votes'])
    with pytest.raises(IndexError, match='point_vote_frames'):
        ctx.point_vote_frames(votes, g['cloud'], g['frames'], g['c_masks'], r)
    assert _same(votes, g['c_votes'])
    bad = g['frames'].copy()
    bad[2, 0, 1] = -np.inf
    votes = np.zeros_like(g['c_votes'])
    with pytest.raises(ValueError, match='frame 2'):
        ctx.point_vote_frames(votes, g['cloud'], bad, g['c_masks'], r)                # frame 2 has both offences: the search comes first
    assert _same(votes, g['c_votes'])
    votes = np.zeros_like(g['c_votes'])
    ctx.point_vote_frames(votes, g['cloud'], g['frames'], g['a_masks'], -1.0)         # a negative radius pairs nothing
    ctx.point_vote_frames(votes, g['cloud'], g['frames'][:0], g['a_masks'][:0], r)
    assert not votes.any()
    with pytest.raises(ValueError):
        ctx.point_vote_frames(np.zeros((0, 6)), np.zeros((0, 3)), g['frames'], g['a_masks'], r)
    assert F == 4


@pytest.mark.parametrize('batch', [1, 3, 4])
def test_vote_frames_on_device_tensors_equals_the_file_path(golden, tmp_path, batch):
    import torch
    g = golden('point_voting')
    r, F = float(g['radius']), len(g['frames'])
    pv = _object(g, tmp_path, g['a_masks'])
    want = pv.vote(radius=r, resize=False).copy()
    pv.zero()
    dev = torch.device('cuda', f3d.default_context().device)
    pts = torch.from_numpy(g['frames']).to(dev)
    masks = torch.from_numpy(g['a_masks']).to(dev)
    for f0 in range(0, F, batch):
        out = pv.vote_frames(pts[f0:f0 + batch], masks[f0:f0 + batch].reshape(-1, int(g['hw'][0]), int(g['hw'][1])), r)
    assert out.is_cuda and tuple(out.shape) == want.shape
    assert _same(pv.votes, want)
    pv.vote_frames(pts.float(), masks, r)                                             # accumulates; float32 points (lattice: exact)
    assert _same(pv.votes, 2 * want)
    pv.zero()
    assert not pv.votes.any()


# ---- capture size: 8 frames of 256 x 192 pixels against 200k points, against the restatement ---------------------------------
CF, CH, CW, CM, CN = 8, 192, 256, 200_000, 40


@pytest.fixture(scope='module')
def capture():
    """A wall about 8 m away seen by 8 cameras; float32-representable coordinates, so the float32 and the float64 cloud are the same
    points.  2 % dropout pixels sit at their camera centre, where a clump of cloud points waits.  One restatement run per radius."""
    rng = np.random.default_rng(77)
    frames = np.empty((CF, CH * CW, 3))
    u, v = np.meshgrid(np.arange(CW), np.arange(CH))
    for j in range(CF):
        z = 8.0 + 0.5 * np.sin(u / 40.0 + j) + rng.uniform(0, 0.02, u.shape)
        p = np.stack([(u - CW / 2) / 128.0 * z + 0.3 * j, (v - CH / 2) / 128.0 * z, z], -1).reshape(-1, 3)
        p[rng.random(len(p)) < 0.02] = [0.3 * j, 0.0, 0.0]
        frames[j] = p
    frames = frames.astype(np.float32).astype(np.float64)
    flat = frames.reshape(-1, 3)
    cloud = flat[rng.choice(len(flat), CM - 64, replace=False)] + rng.normal(0, 0.02, (CM - 64, 3))
    cloud = np.concatenate([cloud, np.array([0.3, 0.0, 0.0]) + rng.normal(0, 0.02, (64, 3))]).astype(np.float32)
    masks = rng.integers(0, CN + 1, (CF, CH * CW)).astype(np.uint8)
    masks[:, ::7] = 3                                                                 # a common label: many duplicates per point
    tree = ref.make_tree(cloud.astype(np.float64))
    want = {}
    for r in (0.01, 0.05):
        votes = np.zeros((CM, CN + 1))
        ref.vote(votes, None, frames, masks, r, tree=tree)
        want[r] = votes
    return frames, cloud, masks, want


@pytest.mark.parametrize('radius', [0.01, 0.05])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_capture_size_votes_equal_the_restatement(capture, dtype, radius):
    import torch
    frames, cloud, masks, want = capture
    ctx = f3d.default_context()
    dev = torch.device('cuda', ctx.device)
    pv = PointVotingSegmentation([], cloud.astype(dtype), (CH, CW), '.', CN)
    pts = torch.from_numpy(frames if dtype == np.float64 else frames.astype(np.float32)).to(dev)
    pv.vote_frames(pts, torch.from_numpy(masks).to(dev), radius)
    got = pv.votes
    print(f'capture {np.dtype(dtype).name} r={radius}: votes {want[radius][:, :-1].sum():.0f}, points seen {(want[radius][:, -1] > 0).sum()}, '
          f'differing cells {(got != want[radius]).sum()}')
    assert want[radius][:, -1].max() >= 2 and _same(got, want[radius])


def test_reserved_strict_context_allocates_nothing(golden):
    import torch
    g = golden('point_voting')
    ctx = f3d.Context(0)
    dev = torch.device('cuda', 0)
    cloud, pts, masks = (torch.from_numpy(g[k]).to(dev) for k in ('cloud', 'frames', 'a_masks'))
    M, ncols, F, hw = len(cloud), int(g['nclasses']) + 1, pts.shape[0], pts.shape[1]
    votes = torch.zeros((M, ncols), dtype=torch.float64, device=dev)
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    ctx.reserve_point_vote(M, ncols)
    ctx.set_strict(True)
    before = ctx.alloc_count
    for radius in (float(g['radius']), 0.001):                                        # another radius = another grid, same scratch
        ctx.point_vote_frames_dev(cloud.data_ptr(), f3d.F64, M, pts.data_ptr(), f3d.F64, masks.data_ptr(), F, hw, radius, votes.data_ptr(),
                                  ncols, s.cuda_stream)
        assert ctx.alloc_count == before
    s.synchronize()
    ctx.take_device_error(s.cuda_stream)
    small = np.zeros_like(g['a_votes_all'])
    ref.vote(small, g['cloud'], g['frames'], g['a_masks'], 0.001)
    assert _same(votes.cpu().numpy(), _full(g) + small)
    with pytest.raises(MemoryError):                                                  # a larger cloud than reserved: strict says so
        big = torch.zeros((1 << 16, 3), dtype=torch.float64, device=dev)
        bv = torch.zeros((1 << 16, 300), dtype=torch.float64, device=dev)
        ctx.point_vote_frames_dev(big.data_ptr(), f3d.F64, 1 << 16, pts.data_ptr(), f3d.F64, masks.data_ptr(), F, hw, 0.5, bv.data_ptr(), 300,
                                  s.cuda_stream)
    ctx.close()


def _full(g):
    votes = np.zeros_like(g['a_votes_all'])
    return ref.vote(votes, g['cloud'], g['frames'], g['a_masks'], float(g['radius']))


def test_device_error_bit_belongs_to_the_point_vote(golden):
    import torch
    g = golden('point_voting')
    ctx = f3d.Context(0)
    dev = torch.device('cuda', 0)
    cloud, pts, bad = (torch.from_numpy(g[k]).to(dev) for k in ('cloud', 'frames', 'c_masks'))
    M, ncols, F, hw, r = len(cloud), int(g['nclasses']) + 1, pts.shape[0], pts.shape[1], float(g['radius'])
    votes = torch.zeros((M, ncols), dtype=torch.float64, device=dev)
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    ctx.point_vote_frames_dev(cloud.data_ptr(), f3d.F64, M, pts.data_ptr(), f3d.F64, bad.data_ptr(), F, hw, r, votes.data_ptr(), ncols, s.cuda_stream)
    s.synchronize()                                              # the IndexError is pending, nobody has taken it
    assert _same(votes.cpu().numpy(), g['c_votes'])
    uv = np.zeros((6, 3))
    ctx.vote_uv2pt(uv, np.array([0, 1, 5, 5], np.int32), np.array([0, 2, 1, 1], np.uint8))
    assert uv.sum() == 3 and uv[5, 1] == 1                       # the other voter ran and was not blamed
    with pytest.raises(IndexError, match='vote_uv2pt'):
        ctx.vote_uv2pt(uv, np.array([0, 9], np.int32), np.array([0, 0], np.uint8))
    ctx.point_vote_frames_dev(cloud.data_ptr(), f3d.F64, M, pts.data_ptr(), f3d.F64, bad.data_ptr(), F, hw, r, votes.data_ptr(), ncols, s.cuda_stream)
    s.synchronize()
    assert _same(votes.cpu().numpy(), g['c_votes'])              # while its error is pending, the point vote writes nothing
    with pytest.raises(IndexError, match='point_vote_frames'):
        ctx.take_device_error(s.cuda_stream)
    ctx.take_device_error(s.cuda_stream)                         # consumed
    # and the other way round: a pending uv2pt error neither skips nor is blamed on the point vote
    lut = torch.tensor([0, 99], dtype=torch.int32, device=dev)
    lm = torch.zeros(2, dtype=torch.uint8, device=dev)
    uvd = torch.zeros((6, 3), dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    ctx.vote_uv2pt_dev(lut.data_ptr(), lm.data_ptr(), 2, uvd.data_ptr(), 6, 3, s.cuda_stream)
    s.synchronize()
    host = np.zeros_like(g['b_votes'])
    ctx.point_vote_frames(host, g['cloud'], g['frames'], g['b_masks'], r)
    assert _same(host, g['b_votes'])
    with pytest.raises(IndexError, match='point_vote_frames'):
        ctx.point_vote_frames(np.zeros_like(host), g['cloud'], g['frames'], g['c_masks'], r)
    with pytest.raises(IndexError, match='vote_uv2pt'):
        ctx.take_device_error(s.cuda_stream)
    ctx.take_device_error(s.cuda_stream)
    ctx.close()


def test_segment_reproduces_the_fixture(golden, tmp_path):
    """Thresholds 0.0, 0.5 and an exact tie, no filter and four filter lists (aliasing, negative and total-column entries), and a
    votes_file object: the classes the reference returned."""
    g = golden('point_voting')
    np.save(tmp_path / 'v.npy', g['d_votes'])
    pf = PointVotingSegmentation(None, None, None, None, None, votes_file=str(tmp_path / 'v.npy'))
    assert _same(pf.segment(0.5), g['d_file_classes'])
    for k in range(5):
        flt = None if k == 0 else tuple(int(x) for x in g[f'd_filter_{k}'])
        for t, thr in enumerate(g['d_thresholds']):
            assert _same(pf.segment(float(thr), filter_classes=flt), g[f'd_classes_{k}_{t}']), (k, t)
            assert _same(pf.segment(float(thr), filter_classes=flt, votes=g['d_votes'][:50]), g[f'd_classes_{k}_{t}'][:50])


@pytest.mark.parametrize('ncols', [2, 7, 134])
def test_segment_equals_the_restatement_on_random_votes(ncols):
    rng = np.random.default_rng(ncols)
    n = 5000
    votes = rng.integers(0, 4, (n, ncols)).astype(np.float64) * (rng.random((n, ncols)) < 0.3)
    votes[:, -1] = rng.integers(0, 9, n)
    votes[::11, -1] = 0                                          # votes without a total
    votes[::13, :-1] = 0                                         # a total without votes
    votes[::17] = 0
    pv = PointVotingSegmentation.__new__(PointVotingSegmentation)
    pv.votes, pv.nclasses = votes, ncols - 1
    filters = [None, (ncols - 1,), (1, 0), (-1, 0, 1), tuple(rng.permutation(ncols)[: min(ncols, 12)])]
    for flt in filters:
        for thr in (0.0, 0.5, 1 / 3, 1.0, 2.0):
            got = pv.segment(thr, filter_classes=flt)
            assert got.dtype == np.int64 and _same(got, ref.segment(votes, ncols - 1, thr, flt).astype(np.int64)), (flt, thr)
    assert _same(pv.segment(0.5, votes=votes[:100]), ref.segment(votes[:100], ncols - 1, 0.5).astype(np.int64))
    with pytest.raises(ValueError):
        pv.segment(0.5, votes=votes[:, :1])                      # votes[:, :-1] is empty: argmax of an empty sequence
    with pytest.raises(IndexError):
        pv.segment(0.5, filter_classes=(ncols,))
