"""Surface normals on the device (f3d_estimate_normals*): exact neighbour selection, normals against the oracle
(tests/normals_ref.py), the reference's orientation, bit-for-bit consistency of every entry point, and depth -> points ->
normals -> Fusion.fuse_device end to end."""
import numpy as np
import pytest

import f3d
import normals_ref as R
from Fusion3DSeg import fusion
from RTAB_utils import ios_rtab
from test_fusion_device_gpu import PARAMS, _assert_same, _copy, _run

pytestmark = pytest.mark.gpu

H, W = 96, 128
KD = np.array([[105.0, 0.0, 64.0], [0.0, 105.0, 48.0], [0.0, 0.0, 1.0]])     # 256x192 at f = 210, halved


def _depth(F, dropout=0.0, seed=0, floor_at=1.2):
    """uint16 millimetres: a wall at 2.5 m, a floor `floor_at` m below the camera (at 0.8 m it meets the wall in view, at row 82),
    a box in front; optional zero-depth pixels."""
    rng = np.random.default_rng(seed)
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    wall = np.full((H, W), 2.5)
    with np.errstate(divide='ignore'):
        floor = np.where(v > 48.5, 105.0 * floor_at / (v - 48.0), np.inf)
    d = np.minimum(wall, floor)
    d[30:60, 20:50] = np.minimum(d[30:60, 20:50], 1.6 + 0.004 * (u[30:60, 20:50] - 20))   # a slanted box face
    out = []
    for f in range(F):
        mm = np.round(d * 1000 + rng.normal(0, 1.0, d.shape) + 3 * f).astype(np.uint16)
        if dropout:
            mm[rng.random(mm.shape) < dropout] = 0
        out.append(mm)
    return np.stack(out)


def _frames(F, dropout=0.0, seed=0):
    """-> (depth [F,H,W], points [F,H*W,3] unprojected on the device, poses (q_wxyz [F,4], t [F,3]))."""
    ctx = f3d.default_context()
    depth = _depth(F, dropout, seed)
    q = np.tile([1.0, 0.0, 0.0, 0.0], (F, 1))
    t = np.stack([[0.03 * f, -0.01 * f, 0.02 * f] for f in range(F)])
    pts = np.stack([ctx.unproject_depth(depth[f], KD, q[f], t[f]) for f in range(F)])
    return depth, pts, q, t


def _lattice_cloud():
    """Exact lattice (spacing 0.25; radius 0.5 lands exactly on lattice distances), isolated points, a 1000-point coincident
    cluster and one far outlier."""
    g = np.stack(np.meshgrid(np.arange(7), np.arange(6), np.arange(3), indexing='ij'), -1).reshape(-1, 3) * 0.25
    iso = np.array([[10.0, 0.0, 0.0], [10.4, 0.0, 0.0], [20.0, 0.0, 0.0], [30.0, 0.0, 0.0], [30.0, 0.25, 0.0]])
    cluster = np.tile([[-5.0, 2.0, 1.0]], (1000, 1))
    far = np.array([[1e4, -3e3, 7e2]])
    pts = np.concatenate([g, iso, cluster, g[:20] + [0.0, 0.0, 0.125], far])
    return pts[np.random.default_rng(1).permutation(len(pts))]


@pytest.mark.parametrize('max_nn', [1, 3, 30, 64])
def test_selection_is_exact(max_nn):
    ctx = f3d.default_context()
    pts = _lattice_cloud()
    nrm, counts, nb = ctx.estimate_normals(pts, np.zeros(3), 0.5, max_nn, orient=False, want_neighbours=True)
    want = R.neighbours(pts, 0.5, max_nn)
    assert np.array_equal(counts, [len(k) for k in want])
    pad = np.full((len(pts), max_nn), -1, np.int32)
    for i, k in enumerate(want):
        pad[i, :len(k)] = k
    assert np.array_equal(nb, pad)
    assert (counts < 3).any() and (counts == max_nn).any()
    wn, gap, degenerate, _ = R.normals(pts, 0.5, max_nn)
    assert degenerate.any()
    assert np.array_equal(R.bits(nrm[degenerate]), R.bits(np.tile([0.0, 0.0, 1.0], (int(degenerate.sum()), 1))))


@pytest.mark.parametrize('max_nn', [8, 30, 64])
def test_normals_agree_with_the_oracle_on_depth_scenes(max_nn):
    ctx = f3d.default_context()
    _, pts, _, t = _frames(2)
    for f in range(2):
        got = ctx.estimate_normals(pts[f], t[f], 0.05, max_nn, orient=False)
        excluded, compared, degenerate = R.check_against_oracle(pts[f], 0.05, max_nn, got)
        print(f'frame {f} max_nn {max_nn}: {compared} rows compared, {excluded} excluded (small eigen-gap), {degenerate} degenerate')
        assert excluded <= 0.001 * len(got)
        assert compared >= 0.99 * len(got)


def test_normals_agree_with_the_oracle_on_analytic_clouds():
    ctx = f3d.default_context()
    k = np.arange(20000) + 0.5
    phi, theta = np.arccos(1 - 2 * k / len(k)), np.pi * (1 + 5 ** 0.5) * k
    sphere = np.stack([np.cos(theta) * np.sin(phi), np.sin(theta) * np.sin(phi), np.cos(phi)], 1) + [1.0, 2.0, 3.0]
    u, v = np.meshgrid(np.arange(40) * 0.01, np.arange(30) * 0.01)
    plane = np.stack([u.ravel(), v.ravel()], 1) @ np.array([[1.0, 0.2, -0.3], [0.1, 1.0, 0.4]]) + [0.3, -0.2, 2.0]
    for pts in (sphere, plane):
        got = ctx.estimate_normals(pts, np.zeros(3), 0.05, 30, orient=False)
        excluded, compared, _ = R.check_against_oracle(pts, 0.05, 30, got)
        assert excluded == 0 and compared == len(pts)


def test_orientation_is_the_reference_flip_of_the_unoriented_output():
    ctx = f3d.default_context()
    _, pts, _, t = _frames(2, dropout=0.1, seed=5)
    for f in range(2):
        raw = ctx.estimate_normals(pts[f], t[f], 0.05, 30, orient=False)
        got = ctx.estimate_normals(pts[f], t[f], 0.05, 30, orient=True)
        dots = R.orient_dots(pts[f], raw, t[f])
        close = np.abs(dots) < 1e-12
        assert int(close.sum()) == 0
        want = R.orient(pts[f], raw, t[f])
        assert np.array_equal(R.bits(got), R.bits(want))
        at_centre = (pts[f] == t[f]).all(axis=1)
        assert at_centre.sum() > 0 and (got[at_centre] == [0.0, 0.0, 1.0]).all()        # NaN direction: not flipped


def _side_stream(torch, dev):
    """A stream ordered after torch's current one (a null-stream handle would select the context's own stream)."""
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    return s


def test_entry_points_agree_bit_for_bit():
    import torch
    dev = torch.device('cuda', 0)
    ctx = f3d.default_context()
    F, n, max_nn = 3, H * W, 30
    _, pts, _, t = _frames(F, dropout=0.1, seed=7)
    single = [ctx.estimate_normals(pts[f], t[f], 0.05, max_nn, want_neighbours=True) for f in range(F)]
    x = torch.from_numpy(pts).to(dev)
    out = torch.full((F, n, 3), 7.0, dtype=torch.float64, device=dev)
    cnt = torch.full((F * n,), -7, dtype=torch.int32, device=dev)
    nb = torch.full((F * n, max_nn), -7, dtype=torch.int32, device=dev)
    s = _side_stream(torch, dev).cuda_stream
    ctx.estimate_normals_batch_dev(x.data_ptr(), F, n, t, out.data_ptr(), 0.05, max_nn, True, cnt.data_ptr(), nb.data_ptr(), s)
    torch.cuda.synchronize(dev)
    batch = out.cpu().numpy()
    bc, bn = cnt.cpu().numpy().reshape(F, n), nb.cpu().numpy().reshape(F, n, max_nn)
    for f in range(F):
        assert np.array_equal(R.bits(batch[f]), R.bits(single[f][0]))                      # batch == single-frame calls
        assert np.array_equal(bc[f], single[f][1]) and np.array_equal(bn[f], single[f][2])
    # device call of one frame == host-pointer call; the drop-in == the Context method; a repeat gives the same bits
    one = torch.empty((n, 3), dtype=torch.float64, device=dev)
    ctx.estimate_normals_batch_dev(x[1].data_ptr(), 1, n, t[1:2], one.data_ptr(), 0.05, max_nn, True, stream=s)
    torch.cuda.synchronize(dev)
    assert np.array_equal(R.bits(one.cpu().numpy()), R.bits(single[1][0]))
    drop_in = ios_rtab.surface_normal_estimation(pts[2], t[2])
    assert drop_in.dtype == np.float64 and drop_in.shape == (n, 3)
    assert np.array_equal(R.bits(drop_in), R.bits(ctx.estimate_normals(pts[2], t[2])))
    assert np.array_equal(R.bits(drop_in), R.bits(single[2][0]))
    assert np.array_equal(R.bits(ios_rtab.surface_normal_estimation(pts[2], t[2])), R.bits(drop_in))
    ctx.estimate_normals_batch_dev(x.data_ptr(), F, n, t, out.data_ptr(), 0.05, max_nn, True, cnt.data_ptr(), nb.data_ptr(), s)
    torch.cuda.synchronize(dev)
    assert np.array_equal(R.bits(out.cpu().numpy()), R.bits(batch)) and np.array_equal(nb.cpu().numpy().reshape(F, n, max_nn), bn)


def test_errors_write_nothing():
    import torch
    dev = torch.device('cuda', 0)
    ctx = f3d.default_context()
    pts = np.random.default_rng(2).uniform(0, 1, (500, 3))
    x = torch.from_numpy(pts).to(dev)
    out = torch.full((500, 3), 7.0, dtype=torch.float64, device=dev)
    cnt = torch.full((500,), -7, dtype=torch.int32, device=dev)
    s = _side_stream(torch, dev).cuda_stream
    bad_pts = pts.copy()
    bad_pts[17, 1] = np.nan
    xb = torch.from_numpy(bad_pts).to(dev)
    cases = [(xb, 0.05, 30), (x, 0.0, 30), (x, -1.0, 30), (x, float('nan'), 30), (x, 0.05, 0), (x, 0.05, f3d.NORMALS_MAX_NN + 1)]
    for src, radius, max_nn in cases:
        with pytest.raises(ValueError):
            ctx.estimate_normals_batch_dev(src.data_ptr(), 1, 500, np.zeros((1, 3)), out.data_ptr(), radius, max_nn, True, cnt.data_ptr(),
                                           None, s)
        torch.cuda.synchronize(dev)
        assert bool((out == 7.0).all()) and bool((cnt == -7).all())
    inf_pts = pts.copy()
    inf_pts[3, 0] = np.inf
    for p, radius, max_nn in [(inf_pts, 0.05, 30), (pts, 0.0, 30), (pts, 0.05, 0), (pts, 0.05, 65)]:
        with pytest.raises(ValueError):
            ctx.estimate_normals(p, np.zeros(3), radius, max_nn)
    # n = 0 and F = 0 do nothing
    ctx.estimate_normals_batch_dev(x.data_ptr(), 0, 500, np.zeros((0, 3)), out.data_ptr(), 0.05, 30, True, stream=s)
    ctx.estimate_normals_batch_dev(x.data_ptr(), 1, 0, np.zeros((1, 3)), out.data_ptr(), 0.05, 30, True, stream=s)
    torch.cuda.synchronize(dev)
    assert bool((out == 7.0).all())
    assert ctx.estimate_normals(np.zeros((0, 3)), np.zeros(3)).shape == (0, 3)


def test_depth_to_fused_cloud_end_to_end():
    """uint16 depth (with dropouts) -> frames_world_dev -> Fusion.from_frames(...).fuse_device == Fusion.fuse on the downloaded
    arrays, bit for bit with the lookups; the normals now make the angle test reject candidates."""
    import torch
    dev = torch.device('cuda', 0)
    F = 8
    depth = _depth(F, dropout=0.1, seed=11, floor_at=0.8)              # a wall / floor crease: normals at 90 degrees
    odo_xyzw = np.tile([0.0, 0.0, 0.0, 1.0], (F, 1))
    odo_xyz = np.stack([[0.02 * j, 0.0, 0.0] for j in range(F)])
    pts, nrm = ios_rtab.frames_world_dev(depth, KD, odo_xyzw, odo_xyz)
    assert pts.shape == (F, H * W, 3) and nrm.shape == (F, H * W, 3) and pts.is_cuda and nrm.dtype == torch.float64
    host_pts = pts.cpu().numpy()
    for j in range(F):                                                 # the same as the one-frame host paths
        assert np.array_equal(R.bits(host_pts[j]), R.bits(ios_rtab.frame_points_world(depth[j], KD, odo_xyzw[j], odo_xyz[j])))
    assert np.array_equal(R.bits(nrm[2].cpu().numpy()), R.bits(ios_rtab.surface_normal_estimation(host_pts[2], odo_xyz[2])))
    rng = np.random.default_rng(4)
    clr = torch.from_numpy(rng.uniform(0, 1, (F, H * W, 3))).to(dev)
    valid = torch.from_numpy((depth > 0).reshape(F, -1).astype(np.uint8)).to(dev)
    q_wxyz = odo_xyzw[:, [3, 0, 1, 2]]
    dev_frames = [(str(j), pts[j], nrm[j], clr[j], valid[j]) for j in range(F)]
    host_frames = [(str(j), pts[j].cpu().numpy(), nrm[j].cpu().numpy(), clr[j].cpu().numpy(), valid[j].cpu().numpy().astype(bool))
                   for j in range(F)]
    params = PARAMS[0]
    want = _run(KD, W, H, q_wxyz, odo_xyz, _copy(host_frames), params, 2, False)
    _assert_same(_run(KD, W, H, q_wxyz, odo_xyz, dev_frames, params, 2, True), want)
    # the angle test of the patch criterion now rejects candidates that the distance test alone would take
    radius, min_cosine = params[0], np.cos(np.deg2rad(params[1]))
    p, n, ok = host_frames[0][1], host_frames[0][2], host_frames[0][4]
    rejected = 0
    for i in np.flatnonzero(ok)[::7]:
        cand = np.array([c for c in (i + 1, i + W, i + W + 1) if c < H * W and ok[c]])
        if len(cand):
            near = np.linalg.norm(p[cand] - p[i], axis=-1) < radius
            take = fusion._mergeable(p[i], n[i], p[cand], n[cand], radius, min_cosine)
            rejected += int((near & ~take).sum())
    assert rejected > 0
