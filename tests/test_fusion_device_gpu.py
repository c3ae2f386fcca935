"""Fusion.fuse and Fusion.fuse_device (one frame loop: NumPy in and out, or the cloud left on the device) against the literal oracle
O.fuse bit for bit -- cloud, lookups in order, the state of the global NumPy generator and, for fuse, the consumed masks -- on the
reference golden and on synthetic sequences that walk every quirk of the reference's loop.  The oracle is pinned to the reference's
own runs by tests/test_fusion_oracle_cpu.py."""
import numpy as np
import pytest

import f3d
from f3d import synth
from Fusion3DSeg import fusion
from Fusion3DSeg.fusion import Fusion
from fusion_scenes import assert_same_fuse as _assert_same, copy_frames as _copy, run_fuse as _run

pytestmark = pytest.mark.gpu


def _assert_masks(got, want):
    for (name, *_, a), (_, *_, b) in zip(got, want):
        assert a.dtype == b.dtype and np.array_equal(a, b), name


def test_fuse_device_matches_the_golden(golden, tmp_path):
    g = golden('fuse')
    h, w = (int(x) for x in g['hw'])
    F = len(g['points'])
    frames = [(f'{100 + j}', g['points'][j], g['normals'][j], g['colors'][j], g['valid'][j]) for j in range(F)]
    for ci in range(int(g['ncases'])):
        radius, angle, stride, max_depth, skip, seed = g[f'c{ci}_params']
        params = (float(radius), float(angle), None if stride < 0 else int(stride), float(max_depth), int(skip))
        if ci == 0:
            for how in ('host', 'device'):
                (tmp_path / how).mkdir()
        _, _, oracle_after, _ = _run(g['K'], w, h, g['wxyz'], g['t'], _copy(frames), params, int(seed), 'oracle')
        for how in ('host', 'device'):
            (pts, nrm, clr, nmerges, occ), lookups, after, _ = _run(g['K'], w, h, g['wxyz'], g['t'], _copy(frames), params, int(seed), how,
                                                                    tmp_path / how if ci == 0 else None)
            assert pts.dtype == nrm.dtype == clr.dtype == np.float64 and nmerges.dtype == np.int64 and occ.dtype == np.uint32
            assert np.array_equal(nmerges, g[f'c{ci}_nmerges']) and np.array_equal(occ, g[f'c{ci}_occurences']), (ci, how)
            for got, key in ((pts, 'ds_pts'), (nrm, 'ds_norms'), (clr, 'ds_clrs')):
                assert np.array_equal(got, g[f'c{ci}_{key}']), (ci, how, key)
            assert sorted(int(k) for k, _ in lookups) == g[f'c{ci}_uv2pt_names'].tolist()
            lookups = dict(lookups)
            for name, want in zip(g[f'c{ci}_uv2pt_names'], g[f'c{ci}_uv2pt']):
                assert np.array_equal(lookups[str(name)], want), (ci, how, name)
            assert after == oracle_after, (ci, how)
            if ci == 0:
                for name, want in zip(g['c0_uv2pt_names'], g['c0_uv2pt']):
                    got = np.load(tmp_path / how / f'{int(name)}.npy')
                    assert got.dtype == np.int32 and np.array_equal(got, want)


def _sequence(h=96, w=128, F=24):
    """A sequence that walks the quirks: a frame whose camera sees none of the cloud (no hits: the previous frame's free mask is
    used, already consumed -> no shuffle drawn), an all-invalid frame, a zero normal and a NaN point (sequential fallback, and
    a pixel left free for the no-hit frame after it)."""
    K, q, t, frames = synth.depth_sequence(h, w, F, step=0.02, seed=3)
    frames = _copy(frames)
    t = t.copy()
    t[6] = [0.0, 0.0, 60.0]                         # looks away from the wall: no hits
    t[11] = [0.0, 0.0, 60.0]
    t[17] = [0.0, 0.0, 60.0]
    frames[8][4][:] = False                         # all invalid: skipped
    frames[10][2][5 * w + 7] = 0.0                  # zero normal at a valid pixel: sequential
    frames[10][4][5 * w + 7] = True
    frames[15][1][40 * w + 60] = np.nan             # NaN point at a valid pixel: sequential
    frames[15][4][40 * w + 60] = True
    return K, q, t, frames


PARAMS = [(0.05, 10, None, 10, 1), (0.05, 10, 6, 10, 2), (0.03, 15, 4, 2.8, 1), (0.08, 20, 8, 10, 3), (0.02, 10, 2, 10, 1)]


@pytest.mark.parametrize('params', PARAMS)
def test_fuse_device_equals_fuse_on_a_synthetic_sequence(params):
    K, q, t, frames = _sequence()
    h, w = 96, 128
    oracle_frames, host_frames, device_frames = _copy(frames), _copy(frames), _copy(frames)
    want = _run(K, w, h, q, t, oracle_frames, params, 5, 'oracle')
    _assert_same(_run(K, w, h, q, t, host_frames, params, 5, 'host'), want)
    _assert_masks(host_frames, oracle_frames)       # fuse consumes the masks as the reference does
    assert any(not np.array_equal(a[4], b[4]) for a, b in zip(host_frames, frames))
    got = _run(K, w, h, q, t, device_frames, params, 5, 'device')
    _assert_same(got, want)
    _assert_masks(device_frames, frames)            # fuse_device leaves them as they are
    stats = got[3].fuse_device_stats
    if params[2] == 2:                              # a dense cloud: the resident storage doubles on the way
        assert stats['capacity_growths'] >= 1
    if params[4] == 1:                              # frames 10 and 15 are fused: both go down the sequential path
        assert stats['sequential_frames'] >= 2
        assert stats['draws_undone'] >= 1          # a no-hit frame after a fully consumed free mask draws nothing


def _split_normal(min_cosine, seed=7):
    """A normal whose squared length lies above min_cosine added as (x*x + y*y) + z*z and not above it in np.einsum's order."""
    rng = np.random.default_rng(seed)
    for _ in range(100000):
        u = rng.normal(size=3)
        n = u / np.linalg.norm(u) * np.sqrt(min_cosine) * (1 + rng.integers(-4, 5) * np.finfo(float).eps)
        if (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2] > min_cosine >= np.einsum('ij,ij->i', n[None], n[None])[0]:
            return n
    raise AssertionError('np.einsum adds a squared length as (x*x + y*y) + z*z here')


def test_numpy_frames_take_the_sequential_path_on_the_host_test():
    """The sequential fallback of a NumPy frame is decided as patch_downsample decides it, with np.einsum's dot: a free pixel whose
    normal accepts itself in one summation order and not in the other sends the frame down the reference's own order of events."""
    h, w, p = 48, 64, 20 * 64 + 30
    params = (0.05, 10, None, 10, 1)
    K, q, t, frames = synth.depth_sequence(h, w, 4, step=0.02, seed=5)
    plain = _run(K, w, h, q, t, _copy(frames), params, 3, 'device')
    assert plain[3].fuse_device_stats['sequential_frames'] == 0
    frames = _copy(frames)
    frames[0][4].reshape(h, w)[20 - 8:20 + 9, 30 - 8:30 + 9] = False     # alone in its window: the pixel seeds
    frames[0][4][p] = True
    frames[0][2][p] = _split_normal(np.cos(np.deg2rad(params[1])))
    want = _run(K, w, h, q, t, _copy(frames), params, 3, 'oracle')
    for how in ('host', 'device'):
        got = _run(K, w, h, q, t, _copy(frames), params, 3, how)
        _assert_same(got, want)
        assert got[3].fuse_device_stats['sequential_frames'] == 1, how


def test_fuse_device_with_device_tensor_frames():
    import torch
    dev = torch.device('cuda', 0)
    ctx = f3d.default_context()
    K, q, t, frames = _sequence()
    h, w = 96, 128
    params = PARAMS[0]
    want = _run(K, w, h, q, t, _copy(frames), params, 9, 'oracle')
    as_tensors = [(n, torch.from_numpy(p).to(dev), torch.from_numpy(nn).to(dev), torch.from_numpy(c).to(dev), torch.from_numpy(v).to(dev))
                  for n, p, nn, c, v in _copy(frames)]
    _assert_same(_run(K, w, h, q, t, as_tensors, params, 9, 'device'), want)
    assert all(np.array_equal(v.cpu().numpy(), f[4]) for (_, _, _, _, v), f in zip(as_tensors, frames))    # masks not consumed
    # points unprojected on the device from depth frames (uint16 millimetres), valid as uint8
    F = 10
    rng = np.random.default_rng(4)
    depth = (2500 + rng.integers(-3, 4, (F, h, w))).astype(np.uint16)
    depth[:, :, :3] = 0
    qd = np.tile([1.0, 0.0, 0.0, 0.0], (F, 1))
    td = np.stack([[0.02 * j, 0.0, 0.0] for j in range(F)])
    dd = torch.from_numpy(depth.view(np.int16)).to(dev)
    pts = torch.empty((F, h * w, 3), dtype=torch.float64, device=dev)
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    ctx.unproject_depth_batch_dev(dd.data_ptr(), 2, F, h, w, K, qd, td, pts.data_ptr(), 1000.0, s.cuda_stream)
    torch.cuda.current_stream(dev).wait_stream(s)
    nrm = torch.tensor([0.0, 0.0, -1.0], dtype=torch.float64, device=dev).expand(h * w, 3).contiguous()
    clr = torch.from_numpy(rng.uniform(0, 1, (F, h * w, 3))).to(dev)
    valid = torch.from_numpy((depth > 0).reshape(F, -1).astype(np.uint8)).to(dev)
    dev_frames = [(str(j), pts[j], nrm, clr[j], valid[j]) for j in range(F)]
    host_frames = [(str(j), pts[j].cpu().numpy(), nrm.cpu().numpy(), clr[j].cpu().numpy(), valid[j].cpu().numpy().astype(bool))
                   for j in range(F)]
    want = _run(K, w, h, qd, td, _copy(host_frames), params, 2, 'oracle')
    _assert_same(_run(K, w, h, qd, td, dev_frames, params, 2, 'device'), want)
    _assert_same(_run(K, w, h, qd, td, _copy(host_frames), params, 2, 'device'), want)


def test_fused_cloud_to_votes_on_the_device():
    import torch
    from Fusion3DSeg.segUtils.voting import _DeviceVotes
    dev = torch.device('cuda', 0)
    ctx = f3d.default_context()
    K, q, t, frames = _sequence()
    h, w = 96, 128
    host_out, host_luts, _, _ = _run(K, w, h, q, t, _copy(frames), PARAMS[0], 13, 'host')
    host_luts = dict(host_luts)
    dev_luts = {}
    fu = Fusion.from_frames(K, w, h, q, t, _copy(frames), lookup_sink=lambda name, lut: dev_luts.__setitem__(name, lut))
    np.random.seed(13)
    out = fu.fuse_device(*PARAMS[0])
    npts, ncls = len(host_out[0]), 20
    assert out[0].shape[0] == npts
    names = sorted(host_luts, key=int)
    masks = np.random.default_rng(6).integers(0, ncls, (len(names), h * w), dtype=np.uint8)
    a = _DeviceVotes(ctx, np.zeros((npts, ncls + 1)))
    a.add_frames([dev_luts[n] for n in names], [torch.from_numpy(m).to(dev) for m in masks], h, w)
    b = _DeviceVotes(ctx, np.zeros((npts, ncls + 1)))
    b.add_frames([host_luts[n] for n in names], list(masks), h, w)
    va, vb = a.download(), b.download()
    assert va.sum() > 0 and np.array_equal(va, vb)
    assert np.array_equal(ctx.segment_votes(va, ncls, 0.5, None), ctx.segment_votes(vb, ncls, 0.5, None))


def test_kernel_normalisation_matches_row_norms_on_adversarial_vectors():
    import torch
    dev = torch.device('cuda', 0)
    ctx = f3d.default_context()
    v = fusion._norm_probe_vectors(512, seed=99)
    m, half = len(v), v / 2                                # (sum + 0) / (1 + 1): the seed row is zero, one pixel taken
    dd_fma = np.array([fusion._fma(z, z, fusion._fma(y, y, x * x)) for x, y, z in half])
    dd_plain = (half[:, 0] * half[:, 0] + half[:, 1] * half[:, 1]) + half[:, 2] * half[:, 2]
    assert not np.array_equal(dd_fma, dd_plain)            # the vectors tell the two orders apart
    cases = [(f3d.NORM_FMA, half / np.sqrt(dd_fma)[:, None]), (f3d.NORM_PLAIN, half / np.sqrt(dd_plain)[:, None])]
    if fusion._norm_mode() != f3d.NORM_HOST:
        cases.append((fusion._norm_mode(), half / fusion._row_norms(half)[:, None]))
    for mode, want in cases:
        sums = np.zeros((m, 9))
        sums[:, 3:6] = v
        cloud = [torch.zeros((m, 3), dtype=torch.float64, device=dev) for _ in range(3)]
        nm, occ = torch.zeros(m, dtype=torch.int64, device=dev), torch.zeros(m, dtype=torch.int32, device=dev)
        ids = torch.arange(m, dtype=torch.int32, device=dev)
        ds, dc = torch.from_numpy(sums).to(dev), torch.ones(m, dtype=torch.int32, device=dev)
        s = torch.cuda.Stream(dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        ctx.fusion_seed_update_dev(ids.data_ptr(), m, ds.data_ptr(), dc.data_ptr(), mode, *(c.data_ptr() for c in cloud), nm.data_ptr(),
                                   occ.data_ptr(), s.cuda_stream)
        s.synchronize()
        assert np.array_equal(cloud[1].cpu().numpy(), want), mode
        assert np.array_equal(nm.cpu().numpy(), np.ones(m)) and np.array_equal(occ.cpu().numpy(), np.ones(m))


def test_fuse_device_without_a_matching_dot_order_normalises_on_the_host(golden, monkeypatch):
    g = golden('fuse')
    h, w = (int(x) for x in g['hw'])
    frames = [(f'{100 + j}', g['points'][j], g['normals'][j], g['colors'][j], g['valid'][j]) for j in range(len(g['points']))]
    radius, angle, stride, max_depth, skip, seed = g['c0_params']
    params = (float(radius), float(angle), None if stride < 0 else int(stride), float(max_depth), int(skip))
    monkeypatch.setattr(fusion, '_norm_mode', lambda: f3d.NORM_HOST)
    for how in ('host', 'device'):
        (pts, nrm, clr, nmerges, occ), _, _, fu = _run(g['K'], w, h, g['wxyz'], g['t'], _copy(frames), params, int(seed), how)
        assert np.array_equal(pts, g['c0_ds_pts']) and np.array_equal(nrm, g['c0_ds_norms']) and np.array_equal(clr, g['c0_ds_clrs'])
        assert np.array_equal(nmerges, g['c0_nmerges']) and np.array_equal(occ, g['c0_occurences'])
        assert fu.fuse_device_stats['host_normalised'] > 0, how


def test_first_fused_frame_without_hits_raises_like_fuse():
    K, q, t, frames = synth.depth_sequence(48, 64, 4, step=0.02)
    params = (0.05, 10, None, 1.0, 1)                      # the far plane before the wall: no frame sees the cloud
    oracle_frames, host_frames = _copy(frames), _copy(frames)
    with pytest.raises(UnboundLocalError):
        _run(K, 64, 48, q, t, oracle_frames, params, 1, 'oracle')
    for how, used in (('host', host_frames), ('device', _copy(frames))):
        with pytest.raises(UnboundLocalError):
            _run(K, 64, 48, q, t, used, params, 1, how)
    _assert_masks(host_frames, oracle_frames)             # the first frame's mask is consumed before the error
    assert not np.array_equal(host_frames[0][4], frames[0][4])


def test_fuse_device_on_the_default_and_on_a_side_stream():
    import torch
    dev = torch.device('cuda', 0)
    K, q, t, frames = _sequence()
    params = PARAMS[0]
    want = _run(K, 128, 96, q, t, _copy(frames), params, 21, 'oracle')
    assert torch.cuda.current_stream(dev).cuda_stream == 0
    _assert_same(_run(K, 128, 96, q, t, _copy(frames), params, 21, 'device'), want)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        got = [_run(K, 128, 96, q, t, _copy(frames), params, 21, how) for how in ('device', 'host')]
    for g in got:
        _assert_same(g, want)
