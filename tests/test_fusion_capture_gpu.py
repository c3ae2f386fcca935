"""Fusion.fuse / fuse_device and the patch kernels under them, checked against the reference at capture size and at the thresholds.

* the curved golden (tests/golden/fuse_curved.npz, the reference's own run): both fusion paths bit for bit;
* capture size (192x256 and 480x640 frames): both paths against the literal oracle O.fuse, pinned to the goldens by
  tests/test_fusion_oracle_cpu.py;
* patch_match / patch_match_dev at 480x640 against O.fuse_match_frame on pairs built so that the three summation orders of the
  normal dot product, and of the squared distance, fall on different sides of the thresholds (or exactly on the radius);
* patch_seeds_sums / _dev, through Fusion.patch_downsample, against O.patch_downsample at 480x640.
The oracle takes the criterion with this host's NumPy (np.einsum, np.linalg.norm), exactly as the reference does."""
import contextlib
import warnings

import numpy as np
import pytest

import f3d
from fusion_scenes import capture_digest, copy_frames, curved_capture
from Fusion3DSeg.fusion import Fusion
from oracle import np_ref as O

pytestmark = pytest.mark.gpu


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


def _fuse(K, w, h, q, t, frames, params, seed, how):
    """-> (five outputs as NumPy, [(name, lookup)] in the order they were handed out, the generator's next draw, Fusion object)."""
    lookups = []
    if how == 'oracle':
        np.random.seed(seed)
        with _quiet():
            *out, lookups = O.fuse(K, w, h, q, t, copy_frames(frames), *params)
        return out, lookups, np.random.random(), None
    fu = Fusion.from_frames(K, w, h, q, t, copy_frames(frames), lookup_sink=lambda name, lut: lookups.append((name, lut)))
    np.random.seed(seed)
    with _quiet():
        out = fu.fuse_device(*params) if how == 'device' else fu.fuse(*params)
    after = np.random.random()
    if how == 'device':
        out = [o.cpu().numpy() for o in out]
        lookups = [(n, lut.cpu().numpy()) for n, lut in lookups]
    else:
        lookups = [(n, np.array(lut, copy=True)) for n, lut in lookups]
    return out, lookups, after, fu


def _assert_same(got, want, tag):
    (go, gl, ga, _), (wo, wl, wa, _) = got, want
    for k, (a, b) in enumerate(zip(go, wo)):
        assert _same(a, b), (tag, k, a.dtype, b.dtype, a.shape, b.shape)
    assert [n for n, _ in gl] == [n for n, _ in wl], tag
    for (name, a), (_, b) in zip(gl, wl):
        assert _same(a, b), (tag, name)
    assert ga == wa, tag


# ---------------------------------------------------------------------------------------------------------------- the golden
def test_fuse_and_fuse_device_match_the_curved_golden(golden):
    g = golden('fuse_curved')
    h, w = (int(x) for x in g['hw'])
    K, q, t, frames = curved_capture(h, w, int(g['nframes']), int(g['capture_seed']))
    assert capture_digest(K, q, t, frames) == str(g['capture_sha256'])
    for ci in range(int(g['ncases'])):
        radius, angle, stride, max_depth, skip, seed = g[f'c{ci}_params']
        params = (float(radius), float(angle), None if stride < 0 else int(stride), float(max_depth), int(skip))
        want = ([g[f'c{ci}_{k}'] for k in ('ds_pts', 'ds_norms', 'ds_clrs', 'nmerges', 'occurences')],
                list(zip(g[f'c{ci}_uv2pt_names'].tolist(), g[f'c{ci}_uv2pt'])), float(g[f'c{ci}_next_draw']), None)
        for how in ('host', 'device'):
            got = _fuse(K, w, h, q, t, frames, params, int(seed), how)
            _assert_same(got, want, (ci, how))
            if how == 'device' and int(skip) == 1:
                assert got[3].fuse_device_stats['sequential_frames'] >= 1      # frame 3: zero normal and NaN point


# ---------------------------------------------------------------------------------------------------------------- capture size
CAPTURES = [(192, 256, 6), (480, 640, 3)]
SIZE_PARAMS = {'dense': (0.02, 10, 2, 10, 1), 'wide': (0.05, 10, 40, 10, 1)}


@pytest.mark.parametrize('shape', CAPTURES, ids=lambda s: f'{s[0]}x{s[1]}x{s[2]}')
@pytest.mark.parametrize('kind', sorted(SIZE_PARAMS))
def test_fuse_at_capture_size_matches_the_oracle(shape, kind):
    h, w, F = shape
    params = SIZE_PARAMS[kind]
    K, q, t, frames = curved_capture(h, w, F, 17 + F)
    want = _fuse(K, w, h, q, t, frames, params, 31, 'oracle')
    _assert_same(_fuse(K, w, h, q, t, frames, params, 31, 'host'), want, 'fuse')
    dev = _fuse(K, w, h, q, t, frames, params, 31, 'device')
    _assert_same(dev, want, 'fuse_device')
    stats = dev[3].fuse_device_stats
    assert stats['frames'] == len(want[1])
    nmerges, occ = want[0][3], want[0][4]
    assert occ.max() >= 2                                               # later frames really merge into the cloud
    if kind == 'dense':
        assert stats['capacity_growths'] >= 1 and len(want[0][0]) > h * w // 20
    if kind == 'wide' and h == 480:
        assert nmerges.max() >= 1000                                    # 41- and 81-pixel windows: seeds with thousands of members


# ---------------------------------------------------------------------------------------------------------------- patch_match
H, W = 480, 640
RADIUS, MIN_COS = 3e-4, float(np.cos(np.deg2rad(10)))


def _dot(order, n, s):
    p0, p1, p2 = n[..., 0] * s[..., 0], n[..., 1] * s[..., 1], n[..., 2] * s[..., 2]
    return {'A': (p0 + p1) + p2, 'B': (p0 + p2) + p1, 'C': p0 + (p1 + p2)}[order]


def _dist(order, d):
    s0, s1, s2 = d[..., 0] * d[..., 0], d[..., 1] * d[..., 1], d[..., 2] * d[..., 2]
    return np.sqrt({'A': (s0 + s1) + s2, 'B': (s0 + s2) + s1, 'C': s0 + (s1 + s2)}[order])


def _unit(v):
    return v / np.sqrt((v[..., 0:1] ** 2 + v[..., 1:2] ** 2) + v[..., 2:3] ** 2)


def _adversarial_normals(rng, n, want):
    """n (seed normal, pixel normal) pairs whose dot products in the orders A, B, C do not all fall on the same side of MIN_COS;
    `want` picks the pairs where order `want` and the kernel's order B disagree."""
    out_s, out_n = [], []
    while sum(len(x) for x in out_s) < n:
        s = _unit(rng.uniform(-0.3, 0.3, (200000, 3)) + [0, 0, -1])
        perp = _unit(np.cross(s, rng.uniform(-1, 1, (len(s), 3))))
        pn = MIN_COS * s + np.sqrt(1 - MIN_COS * MIN_COS) * perp
        pn = pn * (1 + rng.integers(-6, 7, pn.shape) * np.finfo(float).eps)
        d = {o: _dot(o, pn, s) > MIN_COS for o in 'ABC'}
        keep = d[want] != d['B']
        out_s.append(s[keep])
        out_n.append(pn[keep])
    return np.concatenate(out_s)[:n], np.concatenate(out_n)[:n]


def _adversarial_offsets(rng, base, goal):
    """Pixel points q = base + t with the squared distance's orders straddling RADIUS (goal 'B' / 'C': that order and the kernel's
    order A disagree) or the kernel's order landing exactly on RADIUS (goal 'eq')."""
    n = len(base)
    q = np.empty_like(base)
    done = np.zeros(n, bool)
    while not done.all():
        todo = np.nonzero(~done)[0]
        d = _unit(rng.uniform(-1, 1, (len(todo), 3)))
        t = RADIUS * d * (1 + rng.integers(-8, 9, (len(todo), 1)) * np.finfo(float).eps)
        cand = base[todo] + t
        diff = cand - base[todo]                                        # what the criterion sees: fl(q - x)
        da = _dist('A', diff)
        ok = (da == RADIUS) if goal == 'eq' else ((da < RADIUS) != (_dist(goal, diff) < RADIUS))
        q[todo[ok]] = cand[ok]
        done[todo[ok]] = True
    return q


def _owners(uv, x_pts, x_nrm, q_pts, q_nrm, free, half, dot='np', dist='np', strict=True):
    """The matching loop's owners with the criterion taken in a given order (only to count what the test can tell apart)."""
    free = free.reshape(H, W).copy()
    owner = np.full(H * W, -1, np.int32)
    pcd = np.arange(H * W).reshape(H, W)
    for k, (u_, v_) in enumerate(uv.T):
        r0, r1, c0, c1 = max(0, v_ - half), v_ + half + 1, max(0, u_ - half), u_ + half + 1
        patch = pcd[r0:r1, c0:c1].reshape(-1)
        patch = patch[free[r0:r1, c0:c1].reshape(-1)]
        if not len(patch):
            continue
        diff = q_pts[patch] - x_pts[k][None, :]
        dd = np.linalg.norm(diff, axis=-1) if dist == 'np' else _dist(dist, diff)
        cs = np.einsum('ij, j -> i', q_nrm[patch], x_nrm[k]) if dot == 'np' else _dot(dot, q_nrm[patch], x_nrm[k])
        take = patch[((dd < RADIUS) if strict else (dd <= RADIUS)) & (cs > MIN_COS)]
        owner[take] = k
        free.reshape(-1)[take] = False
    return owner


@pytest.fixture(scope='module')
def match_frame():
    """A 480x640 frame of a slightly rough plane (0.1 mm pixels) with random seeds (several per bucket, some far off the image)
    and, first in index order, seeds sitting on the pixels of adversarial pairs."""
    rng = np.random.default_rng(2024)
    n = H * W
    uu, vv = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    q_pts = np.stack([(uu - W / 2) * 1e-4, (vv - H / 2) * 1e-4, 1e-3 + rng.uniform(-2e-5, 2e-5, (H, W))], -1).reshape(n, 3)
    q_nrm = _unit(rng.uniform(-0.12, 0.12, (n, 3)) + [0, 0, -1])
    q_clr = rng.integers(0, 256, (n, 3)) / 255.0
    free = rng.random(n) < 0.85
    # adversarial pixels on a 6-pixel lattice (farther apart than the radius): the seed on a pixel is its pixel's plane point
    lat = np.stack(np.meshgrid(np.arange(3, W - 3, 6), np.arange(3, H - 3, 6)), -1).reshape(-1, 2)
    lat = lat[rng.permutation(len(lat))[:4000]]
    adv_pix = lat[:, 1] * W + lat[:, 0]
    free[adv_pix] = True
    groups = {'dotA': 700, 'dotC': 700, 'eq': 600, 'distB': 600, 'distC': 600}
    x_pts, x_nrm, at = [], [], 0
    for kind, cnt in groups.items():
        pix = adv_pix[at:at + cnt]
        at += cnt
        base = q_pts[pix].copy()
        if kind.startswith('dot'):
            s, pn = _adversarial_normals(rng, cnt, kind[-1])
            q_pts[pix] = base + _unit(rng.uniform(-1, 1, (cnt, 3))) * RADIUS * 0.3
            q_nrm[pix] = pn
        else:
            s = _unit(rng.uniform(-0.1, 0.1, (cnt, 3)) + [0, 0, -1])
            q_pts[pix] = _adversarial_offsets(rng, base, 'eq' if kind == 'eq' else kind[-1])
            q_nrm[pix] = s
        x_pts.append(base)
        x_nrm.append(s)
    adv = adv_pix[:at]
    uv_adv = np.stack([adv % W, adv // W])
    # random seeds: 7000 on 3000 pixels (several per bucket) and 300 on adversarial pixels; 300 of them moved up to 2 * max(h, w)
    # off the image, in both directions
    pool = rng.integers(0, n, 3000)
    pix = np.concatenate([pool[rng.integers(0, len(pool), 7000)], adv[rng.integers(0, len(adv), 300)]])
    r_pts = q_pts[pix] + rng.uniform(-1.5e-4, 1.5e-4, (len(pix), 3))
    r_nrm = _unit(q_nrm[pix] + rng.uniform(-0.08, 0.08, (len(pix), 3)))
    uv_r = np.stack([pix % W, pix // W])
    off = rng.permutation(len(pix))[:300]
    uv_r[:, off] += rng.integers(-2 * max(H, W), 2 * max(H, W) + 1, (2, 300))
    perm = rng.permutation(len(pix))                                    # random seeds in a random order after the adversarial ones
    uv = np.concatenate([uv_adv, uv_r[:, perm]], 1).astype(np.int32)
    x_pts = np.concatenate(x_pts + [r_pts[perm]])
    x_nrm = np.concatenate(x_nrm + [r_nrm[perm]])
    return dict(uv=uv, x_pts=x_pts, x_nrm=x_nrm, q_pts=q_pts, q_nrm=q_nrm, q_clr=q_clr, free=free)


@pytest.mark.parametrize('half', [0, 1, 5, 20])
def test_patch_match_at_capture_size_and_at_the_thresholds(match_frame, half):
    import torch
    fr = match_frame
    uv, x_pts, x_nrm, q_pts, q_nrm, q_clr, free = (fr[k] for k in ('uv', 'x_pts', 'x_nrm', 'q_pts', 'q_nrm', 'q_clr', 'free'))
    m = len(x_pts)
    inside = (uv[0] >= 0) & (uv[0] < W) & (uv[1] >= 0) & (uv[1] < H)
    assert np.bincount((uv[1] * W + uv[0])[inside]).max() >= 4 and (~inside).sum() >= 250
    assert (uv[:, ~inside] < -W).any() and (uv[:, ~inside] > H + W).any()
    ctx = f3d.default_context()
    owner, sums, counts = ctx.patch_match(uv, x_pts, x_nrm, q_pts, q_nrm, q_clr, free, H, W, half, RADIUS, MIN_COS)

    xp, xn, xc = x_pts.copy(), x_nrm.copy(), np.zeros((m, 3))
    xm, xo = np.zeros(m, np.int64), np.zeros(m, np.uint32)
    want = O.fuse_match_frame(uv, xp, xn, xc, xm, xo, np.arange(m), q_pts, q_nrm, q_clr, free.reshape(H, W).copy(), H, W, half,
                              RADIUS, MIN_COS)
    assert np.array_equal(owner, want)
    assert np.array_equal(counts.astype(np.int64), xm) and np.array_equal(counts > 0, xo == 1)
    took = counts > 0
    denom = (counts[took].astype(np.int64) + 1)[:, None]                 # the seed is the last row of the reference's vstack
    assert _same((sums[took, 0:3] + x_pts[took]) / denom, xp[took])
    assert _same(sums[took, 6:9] / denom, xc[took])
    nsum = (sums[took, 3:6] + x_nrm[took]) / denom
    assert _same(nsum / np.array([np.linalg.norm(v) for v in nsum])[:, None], xn[took])
    assert took.sum() > 1000 and (owner >= 0).sum() > 3000

    # the _dev entry on device buffers: bit for bit the host entry
    dev = torch.device('cuda', ctx.device)
    T = lambda a, dt=torch.float64: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)
    d_uv, d_sp, d_sn, d_qp, d_qn, d_qc = T(uv.reshape(-1), torch.int32), T(x_pts), T(x_nrm), T(q_pts), T(q_nrm), T(q_clr)
    d_free = T(free.astype(np.uint8), torch.uint8)
    d_owner = torch.full((H * W,), -7, dtype=torch.int32, device=dev)
    d_sums, d_counts = torch.zeros((m, 9), dtype=torch.float64, device=dev), torch.full((m,), -7, dtype=torch.int32, device=dev)
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    ctx.patch_match_dev(d_uv.data_ptr(), m, H, W, half, RADIUS, MIN_COS, d_sp.data_ptr(), d_sn.data_ptr(), d_qp.data_ptr(),
                        d_qn.data_ptr(), d_qc.data_ptr(), d_free.data_ptr(), d_owner.data_ptr(), d_sums.data_ptr(), d_counts.data_ptr(),
                        s.cuda_stream)
    s.synchronize()
    assert np.array_equal(d_owner.cpu().numpy(), owner) and np.array_equal(d_counts.cpu().numpy(), counts)
    assert _same(d_sums.cpu().numpy()[took], sums[took])                # rows of seeds that take nothing are left unwritten

    # what the adversarial pairs prove: each other order / a non-strict radius would own hundreds of pixels differently
    if half in (0, 20):
        for variant, kw in (('dot A', dict(dot='A')), ('dot C', dict(dot='C')), ('dist <=', dict(strict=False)),
                            ('dist B', dict(dist='B')), ('dist C', dict(dist='C'))):
            alt = _owners(uv, x_pts, x_nrm, q_pts, q_nrm, free, half, **kw)
            differ = int((alt != want).sum())
            assert differ >= 300, (variant, differ)


# ---------------------------------------------------------------------------------------------------------------- patch_seeds_sums
@pytest.fixture(scope='module')
def capture_frame():
    K, q, t, frames = curved_capture(H, W, 1, 77, quirks=False)
    _, pts, nrm, clr, valid = frames[0]
    rng = np.random.default_rng(78)
    free = valid.reshape(H, W).copy()
    for _ in range(40):                                                  # partly consumed: blocks already taken by the cloud
        r, c = rng.integers(0, H - 30), rng.integers(0, W - 30)
        free[r:r + rng.integers(3, 30), c:c + rng.integers(3, 30)] = False
    free &= rng.random((H, W)) > 0.1
    return pts, nrm, clr, free


@pytest.mark.parametrize('stride,radius,angle', [(2, 0.004, 10), (10, 0.01, 5), (40, 0.05, 30)])
def test_patch_seeds_sums_at_capture_size_matches_the_oracle(capture_frame, stride, radius, angle):
    import torch
    pts, nrm, clr, free0 = capture_frame
    n = H * W
    pcdimg = np.arange(n).reshape(H, W)
    pt2u, pt2v = (np.arange(n) % W).astype(np.int32), (np.arange(n) // W).astype(np.int32)
    min_cos = np.cos(np.deg2rad(angle))
    np.random.seed(stride)
    fa = free0.copy()
    got = Fusion.patch_downsample(pts, nrm, clr, H, W, stride, radius, min_cos, pcdimg, pt2u, pt2v, fa)
    after = np.random.random()
    np.random.seed(stride)
    fb = free0.copy()
    want = O.patch_downsample(pts, nrm, clr, H, W, stride, radius, min_cos, pcdimg, pt2u, pt2v, fb)
    assert np.random.random() == after
    for a, b in zip(got, want):
        assert _same(a, b)
    assert np.array_equal(fa, fb)
    assert len(want[0]) > 100 and want[4].max() >= {2: 5, 10: 20, 40: 1000}[stride]

    # the _dev entry: same owners, sums and counts as the host entry on the same visiting order
    ctx = f3d.default_context()
    np.random.seed(stride)
    order = np.arange(n)
    np.random.shuffle(order)
    prio = np.empty(n, np.int32)
    prio[order] = np.arange(n, dtype=np.int32)
    owner, sums, counts, _ = ctx.patch_seeds_sums(pts, nrm, clr, prio, free0.reshape(-1), H, W, stride // 2, radius, min_cos)
    dev = torch.device('cuda', ctx.device)
    T = lambda a, dt=torch.float64: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)
    d_owner = torch.full((n,), -7, dtype=torch.int32, device=dev)
    d_sums, d_counts = torch.zeros((n, 9), dtype=torch.float64, device=dev), torch.full((n,), -7, dtype=torch.int32, device=dev)
    d_p, d_n, d_c, d_prio, d_free = T(pts), T(nrm), T(clr), T(prio, torch.int32), T(free0.reshape(-1).astype(np.uint8), torch.uint8)
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    ctx.patch_seeds_sums_dev(d_p.data_ptr(), d_n.data_ptr(), d_c.data_ptr(), d_prio.data_ptr(), d_free.data_ptr(), H, W, stride // 2,
                             radius, min_cos, d_owner.data_ptr(), d_sums.data_ptr(), d_counts.data_ptr(), s.cuda_stream)
    s.synchronize()
    assert np.array_equal(d_owner.cpu().numpy(), owner) and np.array_equal(d_counts.cpu().numpy(), counts)
    seeds = counts > 0                                                  # only the seeds' rows carry sums
    assert _same(d_sums.cpu().numpy()[seeds], sums[seeds]) and np.array_equal(seeds, owner == np.arange(n))
    assert np.array_equal(owner >= 0, ~fa.reshape(-1) & free0.reshape(-1))
