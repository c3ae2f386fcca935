"""The literal oracle of Fusion.fuse / patch_downsample (oracle/np_ref.py) pinned to the reference's own runs: it must reproduce
tests/golden/fuse.npz and tests/golden/fuse_curved.npz bit for bit (cloud, lookups, the global generator's state), so that the GPU
tests may use it as the reference at sizes no golden file can hold.  No GPU needed."""
import contextlib
import warnings

import numpy as np
import pytest

from fusion_scenes import capture_digest, copy_frames, curved_capture
from oracle import np_ref as O

KEYS = ('ds_pts', 'ds_norms', 'ds_clrs', 'nmerges', 'occurences')


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


@contextlib.contextmanager
def _quiet():
    with warnings.catch_warnings(), np.errstate(all='ignore'):
        warnings.simplefilter('ignore', RuntimeWarning)              # means of empty sets (zero normal / NaN point), as the reference
        yield


def _params(g, ci):
    radius, angle, stride, max_depth, skip, seed = g[f'c{ci}_params']
    return (float(radius), float(angle), None if stride < 0 else int(stride), float(max_depth), int(skip)), int(seed)


def _check_case(g, ci, out, names_as_int):
    for got, key in zip(out[:5], KEYS):
        want = g[f'c{ci}_{key}']
        assert _same(got, want), (ci, key)
    assert out[4].dtype == np.uint32
    names = [int(n) if names_as_int else str(n) for n, _ in out[5]]
    assert names == g[f'c{ci}_uv2pt_names'].tolist(), ci
    for (_, got), want in zip(out[5], g[f'c{ci}_uv2pt']):
        assert got.dtype == np.int32 and np.array_equal(got, want), ci


def test_oracle_fuse_reproduces_the_reference_golden(golden):
    g = golden('fuse')
    h, w = (int(x) for x in g['hw'])
    F = len(g['points'])
    for ci in range(int(g['ncases'])):
        params, seed = _params(g, ci)
        frames = [(f'{100 + j}', g['points'][j].copy(), g['normals'][j].copy(), g['colors'][j].copy(), g['valid'][j].copy())
                  for j in range(F)]
        np.random.seed(seed)
        _check_case(g, ci, O.fuse(g['K'], w, h, g['wxyz'], g['t'], frames, *params), True)


def test_oracle_fuse_reproduces_the_curved_golden(golden):
    g = golden('fuse_curved')
    h, w = (int(x) for x in g['hw'])
    K, q, t, frames = curved_capture(h, w, int(g['nframes']), int(g['capture_seed']))
    assert capture_digest(K, q, t, frames) == str(g['capture_sha256'])      # the capture the reference fused
    for ci in range(int(g['ncases'])):
        params, seed = _params(g, ci)
        np.random.seed(seed)
        with _quiet():
            out = O.fuse(K, w, h, q, t, copy_frames(frames), *params)
        assert np.random.random() == float(g[f'c{ci}_next_draw']), ci
        _check_case(g, ci, out, False)


def test_curved_capture_walks_the_quirks():
    """What the golden relies on: fusion starts at frame 1, frame 3 leaves two pixels free (zero normal, NaN point), frame 4 sees
    none of the cloud and down-samples its points on frame 3's left-over mask (two new rows), frame 2's pose is un-normalised."""
    K, q, t, frames = curved_capture(24, 32, 6, 9)
    assert not frames[0][4].any() and all(f[4].any() for f in frames[1:])
    assert abs(np.dot(q[2], q[2]) - 1.69) < 1e-9 and all(abs(np.dot(q[j], q[j]) - 1) < 1e-12 for j in (0, 1, 3, 4, 5))
    assert (~np.isfinite(frames[3][1])).any(axis=1).sum() == 1 and (np.abs(frames[3][2]).sum(axis=1) == 0).sum() == 1
    for j in (0, 1, 2, 4, 5):
        assert np.isfinite(frames[j][1]).all() and (np.abs(frames[j][2]).sum(axis=1) > 0).all()
    np.random.seed(3)
    with _quiet():
        out = O.fuse(K, 32, 24, q, t, copy_frames(frames))
    names = [n for n, _ in out[5]]
    assert names == ['201', '202', '203', '204', '205']
    lut4 = dict(out[5])['204']
    assert (lut4 != -1).sum() == 2
    planes = O.frustum_planes(K, 32, 24, q, t, 10)
    assert not O.point_inside_polyhedra(out[0][np.isfinite(out[0]).all(axis=1)], planes[0][4], planes[1][4]).any()


def test_oracle_fuse_without_hits_in_the_first_fused_frame_raises_like_the_reference():
    K, q, t, frames = curved_capture(24, 32, 6, 9)
    t = t.copy()
    t[2] = [0.0, 0.0, 60.0]
    np.random.seed(1)
    with pytest.raises(UnboundLocalError):
        O.fuse(K, 32, 24, q, t, copy_frames(frames))


@pytest.mark.parametrize('h,w,stride', [(24, 32, 10), (17, 29, 4), (40, 40, 20), (9, 9, 1), (30, 23, 2)])
def test_oracle_patch_downsample_equals_the_sequential_fallback(h, w, stride):
    """O.patch_downsample (literal) against Fusion._patch_downsample_sequential (the product's host path for frames the kernels do
    not take) on random frames: partly consumed masks, normals near the angle threshold, a zero normal and a NaN point."""
    from Fusion3DSeg.fusion import Fusion
    rng = np.random.default_rng(h * 1000 + w + stride)
    n = h * w
    pts = np.stack(np.meshgrid(np.arange(w) * 0.02, np.arange(h) * 0.02), -1).reshape(-1, 2)
    pts = np.concatenate([pts, rng.uniform(-0.01, 0.01, (n, 1)) + (np.arange(n)[:, None] % 5 == 0) * 0.15], 1)
    nrm = rng.uniform(-0.2, 0.2, (n, 3)) + [0, 0, 1]
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    clr = rng.integers(0, 256, (n, 3)) / 255.0
    free0 = rng.random((h, w)) < 0.8
    if n > 40:
        nrm[7] = 0.0
        pts[n // 2, 2] = np.nan
        free0.reshape(-1)[[7, n // 2]] = True
    pcdimg = np.arange(n).reshape(h, w)
    pt2u, pt2v = (np.arange(n) % w).astype(np.int32), (np.arange(n) // w).astype(np.int32)
    radius, min_cos = 0.05, np.cos(np.deg2rad(12))
    with _quiet():
        np.random.seed(h + w)
        fa = free0.copy()
        got = O.patch_downsample(pts, nrm, clr, h, w, stride, radius, min_cos, pcdimg, pt2u, pt2v, fa)
        after = np.random.random()
        np.random.seed(h + w)
        order = np.arange(n)
        np.random.shuffle(order)
        fb = free0.copy()
        want = Fusion._patch_downsample_sequential(order, pts, nrm, clr, h, w, stride // 2, radius, min_cos, pcdimg, pt2u, pt2v, fb)
    assert np.random.random() == after
    for a, b in zip(got, want):
        assert _same(a, b)
    assert np.array_equal(fa, fb) and len(got[0]) > 3
    taken = got[4].sum()
    assert 0 < taken < free0.sum() or stride == 1
