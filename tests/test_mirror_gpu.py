"""The reference's call surface (Fusion3DSeg.*, RTAB_utils.*, get3DSeg, get2DSeg) running on the HIP library,
checked against the golden vectors / the oracle.  Needs a GPU."""
import copy
import json
import pickle
from pathlib import Path

import numpy as np
import pytest

import f3d
from f3d import synth
from oracle import np_ref as O

pytestmark = pytest.mark.gpu


def test_camera_utils_and_intersections_drop_in(golden):
    from Fusion3DSeg.camera_utils import points2pixel
    from Fusion3DSeg.intersections import point_inside_polyhedra
    g = golden('points2pixel')
    uv = points2pixel(g['points'], g['K'][0], g['q_wxyz'][0], g['t'][0])
    assert uv.dtype == np.int32 and uv.shape == (2, len(g['points']))
    assert np.array_equal(uv, O.points2pixel(g['points'], g['K'][0], g['q_wxyz'][0], g['t'][0]))
    gi = golden('inside_polyhedra')
    got = point_inside_polyhedra(gi['adv_points'], gi['plane_points'][2], gi['plane_normals'][2])
    assert got.dtype == np.bool_ and np.array_equal(got, gi['inside_adv'][2])


def test_spatquad_drop_in(golden):
    from RTAB_utils.spatQuad import SpatQuadranion, get_quaternion_from_euler, multiplyQuadernion
    g = golden('rotate')
    for q, want in zip(g['q_wxyz'], g['rotated']):
        got = SpatQuadranion(q).rotate(g['points'])
        assert np.array_equal(got, O.rotate(q, g['points']))
        assert np.abs(got - want).max() <= 8 * np.finfo(float).eps * np.dot(q, q) * np.abs(g['points']).max()
    q = SpatQuadranion([2.0, 0, 0, 0])
    assert np.array_equal(q.inverse.elements, [0.5, 0, 0, 0])                  # Q4: un-normalised inverse
    with pytest.raises(ZeroDivisionError):
        SpatQuadranion([0, 0, 0, 0]).inverse
    e = get_quaternion_from_euler(0.1, -0.2, 0.3)
    assert abs(np.linalg.norm(e.elements) - 1) < 1e-12
    prod = multiplyQuadernion(e, e.inverse)
    assert np.allclose(prod.elements, [1, 0, 0, 0], atol=1e-12)


def test_frustum_data_drop_in(golden):
    from Fusion3DSeg.fusion import Fusion
    g = golden('frustum')
    w, h = g['calib_wh']
    e, l, so, fn = Fusion._get_frustum_data(g['calib_K'], int(w), int(h), g['q_wxyz'], g['t'])
    for got, key in ((e, 'eyes'), (l, 'lookats'), (so, 'spoke_origins'), (fn, 'face_normals')):
        assert got.shape == g[f'calib_{key}'].shape and np.abs(got - g[f'calib_{key}']).max() <= 1e-12
    e, l, so, fn = Fusion._get_frustum_data(g['calib_K'], int(w), int(h), g['q_wxyz'], g['t'], g['perm_ids'])
    assert np.abs(so - g['perm_spoke_origins']).max() <= 1e-12              # eyes[ids][ids], like the reference


def _write_frames(tmp_path, masks, luts):
    from PIL import Image
    md, ud = tmp_path / 'masks', tmp_path / 'fusion' / 'uv2pt'
    md.mkdir(parents=True); ud.mkdir(parents=True)
    for i, (m, u) in enumerate(zip(masks, luts)):
        Image.fromarray(m).save(md / f'{i:04d}.png')
        np.save(ud / f'{i:04d}.npy', u)
    return md, ud


def test_voting_segmentation_drop_in_from_files(golden, tmp_path):
    from Fusion3DSeg.segUtils.voting import VotingSegmentation
    g = golden('voting')
    md, ud = _write_frames(tmp_path, g['masks'], g['uv2pt'])
    h, w = g['masks'].shape[1:]
    voter = VotingSegmentation(len(g['votes']), (h, w), md, ud, int(g['nclasses']))
    votes = voter.vote(resize=True, filename=tmp_path / 'seg' / 'votes.npy')
    assert votes.dtype == np.float64 and np.array_equal(votes, g['votes'])
    assert np.array_equal(np.load(tmp_path / 'seg' / 'votes.npy'), g['votes'])
    for i in range(int(g['nseg'])):
        flt = g[f'seg{i}_filter'].tolist() if g[f'seg{i}_has_filter'] else None
        assert np.array_equal(voter.segment(float(g[f'seg{i}_threshold']), flt), g[f'seg{i}_classes'])
    voter.vote(resize=True)                                                   # votes accumulate across calls (:98)
    assert np.array_equal(voter.votes, 2 * g['votes'])
    voter.zero()
    assert voter.votes.sum() == 0
    again = VotingSegmentation(0, None, None, None, 0, votes_file=tmp_path / 'seg' / 'votes.npy')
    assert np.array_equal(again.segment(0.75, None), g['segq2_classes'])      # Q2 after reload


def test_voting_raises_indexerror_for_bad_label(tmp_path):
    from Fusion3DSeg.segUtils.voting import VotingSegmentation
    masks = np.full((1, 4, 4), 200, np.uint8)
    md, ud = _write_frames(tmp_path, masks, [np.zeros(16, np.int32)])
    voter = VotingSegmentation(5, (4, 4), md, ud, 133)
    with pytest.raises(IndexError):
        voter.vote()


def test_fusion_project_vote_argmax_drop_in():
    from Fusion3DSeg.fusion import project_vote_argmax
    sc = synth.scene('C1', n=20000)
    got = project_vote_argmax(sc['points'], sc['K'], sc['wxyzs'], sc['translations'], sc['masks'], sc['max_depth'], 133, 0.5, [86, 114, 115])
    want = O.project_vote_argmax(sc['points'], sc['K'], sc['wxyzs'], sc['translations'], sc['masks'], sc['max_depth'], 133, 0.5, [86, 114, 115])
    assert np.array_equal(got, want)


def _blobs(rng, nblobs, per, spread=6.0):
    centres = rng.uniform(0, spread, (nblobs, 3))
    pts = np.vstack([c + rng.normal(size=(per, 3)) * [0.5, 0.3, 0.1] for c in centres])
    ids = np.repeat(np.arange(nblobs), per).astype(np.int64)
    return pts, ids


def test_points_in_obb_and_relabel_kernels():
    rng = np.random.default_rng(4)
    ctx = f3d.default_context()
    pts, ids = _blobs(rng, 70, 300)
    boxes = [O.obb_from_points(pts[ids == k]) for k in range(70)]
    packed = np.array([np.concatenate([c, R.reshape(-1), e]) for c, R, e in boxes])
    inside, cooc = ctx.points_in_obb(pts, packed)
    want = np.stack([O.points_in_obb(pts, *b) for b in boxes], axis=1)
    assert np.array_equal(inside, want)
    assert np.array_equal(cooc, (want.astype(np.int64).T @ want.astype(np.int64)) > 0)
    _, cooc2 = ctx.points_in_obb(pts.astype(np.float32), packed, want_bits=False)
    want32 = np.stack([O.points_in_obb(pts.astype(np.float32).astype(np.float64), *b) for b in boxes], axis=1)
    assert np.array_equal(cooc2, (want32.astype(np.int64).T @ want32.astype(np.int64)) > 0)
    moved = ids.copy()
    n = ctx.relabel(moved, 3, 1)
    assert n == 300 and (moved == 3).sum() == 0 and (moved == 1).sum() == 600
    assert ctx.relabel(moved, 999, 0) == 0


def test_merge_bb_control_flow_with_the_oracles_fit_injected(tmp_path):
    """Control flow, quirks (Q6/Q7), scans and files -- with a GIVEN fit: the oracle's obb_from_points is injected as box_fn (called
    on pcd_points[ids == id] like the reference's), so this test says nothing about the product's own fit (see
    test_merge_bb_own_gpu_fit_end_to_end_against_the_oracle)."""
    from Fusion3DSeg.merge_intersecting_bb import merge_bb
    rng = np.random.default_rng(9)
    pts, ids = _blobs(rng, 14, 250, spread=3.0)
    ids[ids == 13] = 12                                            # one instance with no points at all
    ids[:3] = 11                                                   # a few stray points of another instance
    info = [{'id': k, 'category_id': 86 + (k % 3), 'parent_id': k % 2, 'area': int((ids == k).sum())} for k in range(14)]
    want_info, want_ids = O.merge_bb(copy.deepcopy(info), ids.copy(), pts)
    got_info, got_ids = merge_bb(tmp_path, copy.deepcopy(info), ids.copy(), pts, box_fn=O.obb_from_points)
    assert np.array_equal(got_ids, want_ids)
    assert [d['id'] for d in got_info] == [d['id'] for d in want_info]
    assert [d['area'] for d in got_info] == [d['area'] for d in want_info]
    assert len(got_info) < len(info)                               # something merged
    assert np.array_equal(np.load(tmp_path / 'panoptic_segmentation' / 'ids.npy'), want_ids)
    saved = json.loads((tmp_path / 'panoptic_segmentation' / 'final_info.json').read_text())
    assert [d['id'] for d in saved] == [d['id'] for d in want_info]


def test_sem_to_mask_kernel(golden):
    """a9: k_sem_to_mask against the reference's own post-processing run with CPU torch (tests/golden/sem_mask.npz):
    equal labels outside a 1e-5 relative band around the threshold (stated in test_oracle_golden.sem_compare),
    first-maximum ties, conf_threshold = 0, C = 8 and C = 133, widths that are not multiples of 4."""
    import get2DSeg
    import torch
    from test_oracle_golden import SEM_CASES, sem_compare
    g = golden('sem_mask')
    for name in SEM_CASES:
        sem, thr = g[f'{name}_sem'], float(g[f'{name}_conf'])
        got = get2DSeg.sem_to_mask(sem, thr)
        assert got.dtype == np.uint8 and got.shape == sem.shape[1:]
        sem_compare(got, g, name)
        assert np.array_equal(get2DSeg.sem_to_mask(torch.from_numpy(sem).cuda(), thr), got)        # device-tensor entry
    # a larger random image against torch run here (CPU torch travels with the image; the reference's six ops inline)
    rng = np.random.default_rng(5)
    sem = (rng.normal(size=(133, 37, 53)) * 3).astype(np.float32)
    sem[:, :4, :] *= 0.01                                            # flat logits -> max prob ~ 1/133 < 0.017 -> label 133
    ts = torch.from_numpy(sem)
    want = ts.argmax(dim=0)
    pmax = torch.amax(torch.nn.Softmax(dim=0)(ts), dim=0)
    want[pmax < 0.017] = 133
    got = get2DSeg.sem_to_mask(sem, 0.017)
    clear = (pmax.numpy().astype(np.float64) - 0.017).__abs__() > 1e-5 * 0.017
    assert clear.mean() > 0.999 and np.array_equal(got[clear], want.numpy().astype(np.uint8)[clear])
    assert (got[:4] == 133).all() and (got[4:] != 133).mean() > 0.9
    assert np.array_equal(get2DSeg.sem_to_mask(sem, 0), ts.argmax(dim=0).numpy().astype(np.uint8))    # no thresholding


def test_device_resident_2d_to_3d_hand_off(tmp_path):
    """Row g1 (BASELINE config 3 "end-to-end incl. the 2D backbone on PyTorch-ROCm"; get2DSeg.py:106-126): network logits on the
    GPU -> f3d_sem_logits_to_masks_dev -> plane j of ONE uint8 [V,H,W] device tensor -> f3d_project_vote_argmax_dev, with torch's
    sync debug mode armed ('error') over the whole hand-off: no .cpu(), no synchronisation, no PNG.  The network is the
    stand-in with OneFormer's contract (f3d/standin.py; OneFormer is absent).  Checked: the masks against the reference's own
    statements in torch (outside sem_mask.npz's band around the threshold), the labels against the oracle fed those masks, and
    the PNG way out of SegmentImage against the device way."""
    import torch
    from PIL import Image
    import get2DSeg
    from f3d.standin import StandInSegNet, synthetic_frames
    from test_oracle_golden import SEM_BAND
    dev = torch.device('cuda', 0)
    V, S, n = 6, 256, 40_000
    K = np.array([[200., 0, S / 2], [0, 200., S / 2], [0, 0, 1]])
    q, t = synth.ring_views(V)
    pts = synth.cloud(n)
    views = f3d.views_build(K, S, S, q, t, 10.0)
    net = StandInSegNet().to(dev).eval()
    frames = synthetic_frames(V, S, S, dev)
    x, vd = torch.from_numpy(pts).to(dev), torch.from_numpy(views).to(dev)
    masks = torch.empty((V, S, S), dtype=torch.uint8, device=dev)
    cls = torch.empty(n, dtype=torch.int64, device=dev)
    ctx = f3d.default_context()
    stream = torch.cuda.Stream(dev)
    net(frames[:2]); torch.cuda.synchronize()                                   # GEMM selection etc. happen outside the armed region
    batches = [frames[0:2], frames[2:4], frames[4], frames[5]]                  # batched and single-frame predictor answers
    with torch.cuda.stream(stream):
        torch.cuda.set_sync_debug_mode('error')
        try:
            out = get2DSeg.masks_to_device(batches, lambda im: {'sem_seg': net(im)}, 0.017, out=masks)
            ctx.project_vote_argmax_dev(x.data_ptr(), f3d.F64, n, vd.data_ptr(), V, out.data_ptr(), S, S, 133, 0.0, None,
                                        cls.data_ptr(), None, stream.cuda_stream, flags=f3d.FUSE_SORT)
        finally:
            torch.cuda.set_sync_debug_mode('default')
        stream.synchronize()
    assert out.data_ptr() == masks.data_ptr()
    # (1) the masks: the reference's statements (:110-118) on the same logits
    def reference_statements(sem):                                              # on [B,C,H,W]; the same GEMM shapes as the run above
        want = sem.argmax(dim=1)
        pmax = torch.amax(torch.nn.Softmax(dim=1)(sem), dim=1)
        want[pmax < 0.017] = 133
        return want.cpu().numpy().astype(np.uint8), ((pmax.double() - 0.017).abs() > SEM_BAND * 0.017).cpu().numpy()
    parts = [reference_statements(net(b) if b.dim() == 4 else net(b)[None]) for b in batches]
    want, clear = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    got_masks = masks.cpu().numpy()
    assert clear.mean() > 0.999 and np.array_equal(got_masks[clear], want[clear])
    assert 0.005 < (got_masks == 133).mean() < 0.6 and len(np.unique(got_masks)) > 10      # both branches of the threshold, many labels
    # (2) the labels: the oracle fed the masks the device produced
    want_cls = O.project_vote_argmax(pts, K, q, t, got_masks, 10.0, 133, 0.0, None)
    assert np.array_equal(cls.cpu().numpy(), want_cls) and (want_cls != 133).mean() > 0.3
    # (3) SegmentImage: the reference's PNG way and the device way give the same masks; the filter skip (:123-124) is reported, not lost
    rgb = tmp_path / 'rgb'; rgb.mkdir()
    host_frames = frames.cpu().numpy()
    for j in range(V):
        Image.fromarray(host_frames[j][:, :, ::-1]).save(rgb / f'{j:03d}.png')          # lossless, so both runs see the same pixels
    written = get2DSeg.SegmentImage(str(rgb), str(tmp_path / 'm1'), extension='png', predictor=net.predict)
    res = get2DSeg.SegmentImage(str(rgb), str(tmp_path / 'm2'), extension='png', predictor=net.predict, out_device=True)
    assert [Path(w).name for w in written] == [f'{j:03d}.png' for j in range(V)] == [Path(w).name for w in res.written]
    assert (tmp_path / 'm1' / 'viz').is_dir()
    for j in range(V):
        a = np.asarray(Image.open(tmp_path / 'm1' / f'{j:03d}.png'))
        assert np.array_equal(a, res.masks[j].cpu().numpy()) and np.array_equal(a, np.asarray(Image.open(tmp_path / 'm2' / f'{j:03d}.png')))
        w1, c1 = reference_statements(net(frames[j])[None])
        assert np.array_equal(a[c1[0]], w1[0][c1[0]])
    absent = sorted(set(range(133)) - set(np.unique(got_masks).tolist()))[:2]
    res2 = get2DSeg.SegmentImage(str(rgb), str(tmp_path / 'm3'), extension='png', predictor=net.predict, filter_classes=absent, out_device=True)
    assert res2.written == [] and not res2.kept.any().item() and res2.masks.shape == (V, S, S)
    assert get2DSeg.SegmentImage(str(rgb), str(tmp_path / 'm4'), extension='png', predictor=net.predict, filter_classes=absent) == []
    with pytest.raises(ValueError):
        get2DSeg.sem_to_mask_device(net(frames[:2]), torch.empty((2, S, S + 1), dtype=torch.uint8, device=dev))


def test_get3dseg_segment_end_to_end(tmp_path, monkeypatch):
    """segment(): votes -> classes -> instances -> files -> parent classes -> merge_bb, on a synthetic fusion directory."""
    import get3DSeg
    rng = np.random.default_rng(21)
    pts, truth = _blobs(rng, 6, 400, spread=4.0)
    n, h, w, nframes = len(pts), 24, 32, 5
    labels = np.array([86, 114, 115, 86, 114, 3])[truth]
    masks, luts = [], []
    for f in range(nframes):
        lut = np.full(h * w, -1, np.int32)
        sel = rng.choice(n, h * w // 2, replace=False)
        pix = rng.choice(h * w, len(sel), replace=False)
        lut[pix] = sel
        mask = np.full(h * w, 133, np.uint8)
        mask[pix] = labels[sel]
        masks.append(mask.reshape(h, w)); luts.append(lut)
    md, ud = _write_frames(tmp_path, masks, luts)
    d2 = ((pts[:, None, :] - pts[None, :, :]) ** 2).sum(-1)
    adj = np.array([np.nonzero(d2[i] < 0.35 ** 2)[0] for i in range(n)], dtype=object)
    with open(tmp_path / 'fusion' / 'fusion_data.pkl', 'wb') as fp:
        pickle.dump({'points': pts, 'normals': np.zeros_like(pts), 'colors': np.zeros_like(pts), 'nmerges': np.ones(n),
                     'occurences': np.ones(n), 'nframes': nframes, 'depth_hw': (h, w)}, fp)
    with open(tmp_path / 'fusion' / 'adj.pkl', 'wb') as fp:
        pickle.dump(adj, fp)
    (tmp_path / 'classes.csv').write_text('Class_ID,Parent,Parent_ID,flag_infojson,flag_objremoval\n'
                                          '86,wall,1,1,0\n114,floor,2,1,0\n115,ceiling,3,1,0\n133,unclassified,0,1,1\n')
    (tmp_path / 'classes_meta.json').write_text(json.dumps({'classes': ['unclassified', 'wall', 'floor', 'ceiling'],
                                                            'colors': [[0, 0, 0], [255, 0, 0], [0, 255, 0], [0, 0, 255]]}))
    monkeypatch.setattr(get3DSeg, '_CLASSES_CSV', tmp_path / 'classes.csv')
    monkeypatch.setattr(get3DSeg, '_CLASSES_META', tmp_path / 'classes_meta.json')
    get3DSeg.segment(tmp_path, md, threshold=0.5, nclasses=133, filter_classes=[86, 114, 115], min_pts_per_inst=50, verbose=False)
    # oracle for the arithmetic parts
    votes = np.zeros((n, 134))
    for m, u in zip(masks, luts):
        O.vote_frame(votes, u, m.reshape(-1))
    classes = O.segment(votes, 133, 0.5, [86, 114, 115])
    assert np.array_equal(np.load(tmp_path / 'segmentation' / 'votes.npy'), votes)
    assert np.array_equal(np.load(tmp_path / 'segmentation' / 'classes.npy'), classes)
    assert (classes != 133).mean() > 0.3
    info = json.loads((tmp_path / 'panoptic_segmentation' / 'final_info.json').read_text())
    ids = np.load(tmp_path / 'panoptic_segmentation' / 'ids.npy')
    assert len(info) >= 2 and ids.shape == (n,)
    assert (tmp_path / 'segmentation' / 'final_pcd.ply').is_file() and (tmp_path / 'panoptic_segmentation' / 'pcd.ply').is_file()
    # remove_classes reuses votes.npy (Q2 path) and keeps the wall/floor/ceiling points
    remaining = get3DSeg.remove_classes(tmp_path, md, None, threshold=0.5, verbose=False)
    cls2 = O.segment(votes, 134, 0.5, None)
    assert np.array_equal(remaining, np.isin(cls2, [86, 114, 115]))


@pytest.mark.parametrize('seed,nblobs,spread', [(31, 40, 4.0), (32, 60, 9.0)])
def test_merge_bb_randomised_control_flow_with_the_oracles_fit_injected(seed, nblobs, spread):
    """Control flow with a given fit (the oracle's, injected), random scenes incl. instances with fewer than 4 points (:83-84)."""
    from Fusion3DSeg.merge_intersecting_bb import merge_bb
    rng = np.random.default_rng(seed)
    pts, ids = _blobs(rng, nblobs, 120, spread=spread)
    small = rng.choice(np.arange(5, nblobs), 4, replace=False)           # instances with < 4 points: early return (:83-84)
    for s_ in small:
        idx = np.nonzero(ids == s_)[0]
        ids[idx[2:]] = int(rng.integers(1, 5))
    info = [{'id': k, 'category_id': 86, 'parent_id': int(rng.integers(0, 3)), 'area': int((ids == k).sum())} for k in range(nblobs)]
    want_info, want_ids = O.merge_bb(copy.deepcopy(info), ids.copy(), pts)
    got_info, got_ids = merge_bb(None, copy.deepcopy(info), ids.copy(), pts, box_fn=O.obb_from_points)
    assert np.array_equal(got_ids, want_ids)
    assert [(d['id'], d['area']) for d in got_info] == [(d['id'], d['area']) for d in want_info]
    for g, w in zip(got_info, want_info):
        assert ('bbox' in g) == ('bbox' in w)
        if 'bbox' in g:
            assert np.allclose(g['bbox'], w['bbox'])


def _c5_blobs(B, n, seed=3456):
    """The C5 merge recipe of SURVEY 8(d): n points in B Gaussian blobs (sigma 0.15 m, centres uniform in the cloud box), parent = id mod 8."""
    rng = np.random.default_rng(seed)
    centres = rng.uniform([-5, -5, 0], [5, 5, 3], (B, 3))
    ids = rng.integers(1, B, n).astype(np.int64)
    pts = centres[ids] + rng.normal(size=(n, 3)) * 0.15
    info = [{'id': k, 'category_id': 86, 'parent_id': k % 8, 'area': int((ids == k).sum())} for k in range(B)]
    return pts, ids, info


def test_group_by_id_extremes_and_hull_filter_kernels():
    """The GPU grouping equals np.nonzero(ids == k) for every id; the reported extremes are members with the maximal dot product;
    the survivors of the hull filter contain every vertex of the full hull, so the box fitted on them is the box of all members."""
    from scipy.spatial import ConvexHull
    import f3d
    ctx = f3d.default_context()
    rng = np.random.default_rng(17)
    nids = 37
    n = 60_000
    ids = rng.integers(-2, nids + 3, n).astype(np.int64)               # some ids outside [0, nids)
    ids[ids == 5] = 6                                                  # an id without members
    centres = rng.uniform(-4, 4, (nids + 3, 3))
    pts = centres[np.clip(ids, 0, nids + 2)] + rng.normal(size=(n, 3)) * [0.4, 0.2, 0.1]
    order, starts = ctx.group_by_id(ids, nids)
    assert starts[0] == 0 and starts[nids + 1] == n and starts[5] == starts[6]
    for k in range(nids):
        assert np.array_equal(order[starts[k]:starts[k + 1]], np.nonzero(ids == k)[0]), k
    assert set(order[starts[nids]:].tolist()) == set(np.nonzero((ids < 0) | (ids >= nids))[0].tolist())
    ext = ctx.obb_extremes(pts)
    assert (ext[5] == -1).all()
    p32 = pts.astype(np.float32)
    x, y, z = p32[:, 0], p32[:, 1], p32[:, 2]
    dots = np.stack([x, y, z, x + y, x - y, x + z, x - z, y + z, y - z, (x + y) + z, (x + y) - z, (x - y) + z, (x - y) - z])
    for k in (0, 7, 36):
        mem = np.nonzero(ids == k)[0]
        for d in range(13):
            assert ids[ext[k, 2 * d]] == k and dots[d, ext[k, 2 * d]] == dots[d, mem].max()
            assert ids[ext[k, 2 * d + 1]] == k and dots[d, ext[k, 2 * d + 1]] == dots[d, mem].min()
    fstart, eqs, margin = np.zeros(nids + 1, np.int32), [], np.zeros(nids)
    nf = np.zeros(nids, np.int64)
    for k in range(nids):
        e = np.unique(ext[k][ext[k] >= 0])
        if len(e) >= 4 and k % 5:                                      # every fifth id gets no facets: nothing may be dropped there
            eq = ConvexHull(pts[e]).equations
            eqs.append(eq); nf[k] = len(eq); margin[k] = 1e-9 * (np.abs(pts[e]).max() + 1)
    fstart[1:] = np.cumsum(nf)
    cand, cnt = ctx.obb_hull_filter(fstart, np.concatenate(eqs), margin)
    dropped = 0
    for k in range(nids):
        mem = np.nonzero(ids == k)[0]
        c = np.sort(cand[starts[k]:starts[k] + cnt[k]])
        assert set(c.tolist()) <= set(mem.tolist())
        if nf[k] == 0:
            assert np.array_equal(c, mem)
            continue
        hull_vertices = mem[ConvexHull(pts[mem]).vertices]
        assert set(hull_vertices.tolist()) <= set(c.tolist()), k
        for a, b in zip(O.obb_from_points(pts[c]), O.obb_from_points(pts[mem])):
            assert np.array_equal(a, b)                                # bit for bit the same box
        dropped += len(mem) - len(c)
    assert dropped > 0.8 * (ids >= 0).sum() * 0.7                      # the filter really removes most members


GROUPINGS = {'all_out': (np.array([7, -1, 9, 4, 4, -3, 1 << 40], np.int64), 4),           # every id outside [0, nids)
             'none_out': (np.array([2, 0, 2, 1, 0, 2, 2], np.int64), 3),
             'nids_1': (np.array([0, 5, 0, -1, 0], np.int64), 1),
             'one_point': (np.array([3], np.int64), 6),
             'descending_257': (np.arange(256, -1, -1, dtype=np.int64), 257)}             # more than one block of keys, reversed


@pytest.mark.parametrize('on_device', [False, True], ids=['host', 'device'])
@pytest.mark.parametrize('case', list(GROUPINGS))
def test_group_by_id_equals_a_stable_argsort(case, on_device):
    ids, nids = GROUPINGS[case]
    n = len(ids)
    keys = np.where((ids >= 0) & (ids < nids), ids, nids)
    want_order = np.argsort(keys, kind='stable').astype(np.int32)
    want_starts = np.searchsorted(keys[want_order], np.arange(nids + 2), side='left').astype(np.int64)
    ctx = f3d.default_context()
    if on_device:
        import torch
        st = torch.cuda.current_stream().cuda_stream
        di = torch.from_numpy(ids).cuda()
        order, skeys = torch.full((n,), -7, dtype=torch.int32, device='cuda'), torch.full((n,), -7, dtype=torch.int32, device='cuda')
        starts = torch.full((nids + 2,), -7, dtype=torch.int64, device='cuda')
        torch.cuda.synchronize()
        ctx.group_by_id_dev(di.data_ptr(), n, nids, order.data_ptr(), skeys.data_ptr(), starts.data_ptr(), st)
        torch.cuda.synchronize()
        assert np.array_equal(skeys.cpu().numpy(), keys[want_order])
        order, starts = order.cpu().numpy(), starts.cpu().numpy()
    else:
        order, starts = ctx.group_by_id(ids, nids)
    assert order.dtype == np.int32 and starts.dtype == np.int64
    assert np.array_equal(order, want_order), (order, want_order)
    assert np.array_equal(starts, want_starts), (starts, want_starts)


def _same_boxes(got_info, want_info, tol=1e-8):
    """'bbox' entries as corner SETS (the eigenvector signs, hence the corner order, are a convention: f3d.h)."""
    for g, w in zip(got_info, want_info):
        assert ('bbox' in g) == ('bbox' in w), (g.get('id'), w.get('id'))
        if 'bbox' in g:
            a, b = np.array(g['bbox']), np.array(w['bbox'])
            d = np.abs(a[:, None, :] - b[None, :, :]).max(-1)
            assert (d.min(1) < tol).all() and (d.min(0) < tol).all(), (g['id'], d.min(1).max())


def test_merge_bb_own_gpu_fit_end_to_end_against_the_oracle():
    """The product's OWN fit (f3d_obb_candidates_dev + f3d_obb_fit_dev in one batch, no box_fn) end to end against the oracle's literal
    restatement of merge_bb.  Two comparisons:
    (1) exact: the oracle's control flow calling the SAME GPU fit per instance on ALL members (host-pointer f3d_obb_fit) -- ids, areas,
        entries and boxes bit for bit.  This pins the candidate pipeline (a box fitted on the hull candidates has the bits of a box fitted on
        all members), the batched launch, the scans and the control flow.
    (2) against the oracle with ITS fit (scipy Qhull + LAPACK): boxes equal as corner sets within 1e-8, and the merge decisions equal on
        these seeded scenes.  (2) cannot be demanded of every scene: "the boxes share a cloud point" hangs on points ON a box face -- the
        vertices that define a box's extents are in or out by the last bit of whoever computed the box (scripts/aux_fuzz.py: ~5 % of small
        dense scenes differ, every flipped point within 3 ulp of a face; Open3D's own rounding would be a third opinion)."""
    import Fusion3DSeg.merge_intersecting_bb as M
    ctx = f3d.default_context()

    def gpu_fit(p):
        boxes, status = ctx.obb_fit([p])
        assert status[0] == f3d.OBB_OK
        return boxes[0, 0:3].copy(), boxes[0, 3:12].reshape(3, 3).copy(), boxes[0, 12:15].copy()
    for B, n, seed in [(160, 40_000, 3456), (96, 150_000, 99)]:
        pts, ids, info = _c5_blobs(B, n, seed)
        prof = {}
        keep = M._MergeState.__init__

        def spy(self, *a, **k):
            keep(self, *a, **k)
            prof['st'] = self
        M._MergeState.__init__ = spy
        try:
            got_info, got_ids = M.merge_bb(None, copy.deepcopy(info), ids.copy(), pts)
        finally:
            M._MergeState.__init__ = keep
        st = prof['st'].prof
        assert st['nfit_gpu'] >= B - 2 and st['nfit_deferred'] == 0, st          # the fits really ran on the GPU
        same_info, same_ids = O.merge_bb(copy.deepcopy(info), ids.copy(), pts, box_fn=gpu_fit)          # (1)
        assert np.array_equal(got_ids, same_ids) and len(got_info) < len(info)
        assert json.dumps(got_info) == json.dumps(same_info)
        want_info, want_ids = O.merge_bb(copy.deepcopy(info), ids.copy(), pts)                          # (2)
        assert np.array_equal(got_ids, want_ids)
        assert [(d['id'], d['area']) for d in got_info] == [(d['id'], d['area']) for d in want_info]
        _same_boxes(got_info, want_info)


def test_merge_bb_c5_recipe_with_the_oracles_fit_and_prefilter_off():
    """merge_bb on the C5 recipe (Gaussian blobs, parent = id mod 8): control flow with the oracle's fit injected (on all members and
    on the hull candidates: the same boxes bit for bit), and -- 2M points, 512 instances, the product's own GPU fit -- the same
    result with the hull prefilter switched off (the vertex set, hence the box, does not depend on which candidates came along)."""
    import Fusion3DSeg.merge_intersecting_bb as M
    pts, ids, info = _c5_blobs(160, 40_000)
    want_info, want_ids = O.merge_bb(copy.deepcopy(info), ids.copy(), pts)
    for pf in (False, True):
        got_info, got_ids = M.merge_bb(None, copy.deepcopy(info), ids.copy(), pts, box_fn=O.obb_from_points, prefilter=pf)
        assert np.array_equal(got_ids, want_ids) and len(got_info) < len(info)
        assert [(d['id'], d['area']) for d in got_info] == [(d['id'], d['area']) for d in want_info]
        for g, w in zip(got_info, want_info):
            assert ('bbox' in g) == ('bbox' in w) and ('bbox' not in g or np.array_equal(np.array(g['bbox']), np.array(w['bbox'])))
    pts, ids, info = _c5_blobs(512, 2_000_000)
    a_info, a_ids = M.merge_bb(None, copy.deepcopy(info), ids.copy(), pts)
    keep = M._MergeState.PREFILTER_MIN
    try:
        M._MergeState.PREFILTER_MIN = 1 << 30
        b_info, b_ids = M.merge_bb(None, copy.deepcopy(info), ids.copy(), pts)
    finally:
        M._MergeState.PREFILTER_MIN = keep
    assert np.array_equal(a_ids, b_ids) and json.dumps(a_info) == json.dumps(b_info) and len(a_info) < len(info)


def test_merge_bb_dev_on_a_resident_cloud_equals_merge_bb():
    """merge_bb_dev: cloud and ids are device tensors; ids are relabelled in place on the device (f3d_relabel_dev), the refits gather
    their candidates on the device.  Same entries, same ids as merge_bb on the host copies; the host copy of the cloud is never made."""
    import torch
    import Fusion3DSeg.merge_intersecting_bb as M
    dev = torch.device('cuda', 0)
    pts, ids, info = _c5_blobs(200, 120_000, seed=5)
    want_info, want_ids = M.merge_bb(None, copy.deepcopy(info), ids.copy(), pts)
    dp, di = torch.from_numpy(pts).to(dev), torch.from_numpy(ids).to(dev)
    prof = {}
    keep = M._MergeState.__init__

    def spy(self, *a, **k):
        keep(self, *a, **k)
        prof['st'] = self
    M._MergeState.__init__ = spy
    try:
        got_info, got_ids = M.merge_bb_dev(copy.deepcopy(info), di, dp)
    finally:
        M._MergeState.__init__ = keep
    assert got_ids.data_ptr() == di.data_ptr() and np.array_equal(di.cpu().numpy(), want_ids)
    assert json.dumps(got_info) == json.dumps(want_info) and len(got_info) < len(info)
    assert prof['st'].cloud._host is None and prof['st'].members is None           # nothing of the cloud came to the host
    with pytest.raises(ValueError):
        M.merge_bb_dev(copy.deepcopy(info), di.to(torch.int32), dp)


def test_obb_fit_kernel_hull_vertices_and_boxes():
    """f3d_obb_fit: the hull vertex set equals scipy's Qhull (ConvexHull(...).vertices) on every set the kernel certifies; the box
    equals the oracle's recipe (hull -> PCA -> extents; LAPACK eigh) up to the axis signs: centre / extent within 1e-9 relative,
    axes within 1e-7 (|cos| of the angle; eigenvectors of close eigenvalues are ill-conditioned), corners as sets.  Sets it must
    not certify (fewer than 4 points, coplanar, duplicates, NaN) come back FEW / DEFERRED -- never a guessed box."""
    from scipy.spatial import ConvexHull
    ctx = f3d.default_context()
    rng = np.random.default_rng(12)
    sets = []
    for k in range(400):
        m = int(rng.choice([4, 5, 6, 9, 26, 60, 150, 700, 3000]))
        kind = k % 4
        if kind == 0:
            p = rng.normal(size=(m, 3)) * rng.uniform(0.05, 2.0, 3)
        elif kind == 1:
            p = rng.uniform(-1, 1, (m, 3)) * rng.uniform(0.1, 3.0, 3)
        elif kind == 2:                                              # points ON a sphere: every point is a vertex
            p = rng.normal(size=(m, 3)); p /= np.linalg.norm(p, axis=1)[:, None]
        else:                                                        # float32-representable coordinates far from the origin
            p = (rng.normal(size=(m, 3)) * 0.15 + rng.uniform(-50, 50, 3)).astype(np.float32).astype(np.float64)
        q = np.linalg.qr(rng.normal(size=(3, 3)))[0]
        sets.append(p @ q.T + rng.uniform(-5, 5, 3))
    boxes, status, verts = ctx.obb_fit(sets, want_vertices=True)
    ok = 0
    for k, p in enumerate(sets):
        if status[k] != f3d.OBB_OK:
            # the only deferrals of this seeded run: 3000 points ON a sphere -- a hull of 3000 vertices / 5996 facets, whose frontier
            # outgrows the 1024-edge LDS table (a capacity deferral, not a guess: the host fits those)
            assert status[k] == f3d.OBB_DEFERRED and k % 4 == 2 and len(p) == 3000, k
            continue
        ok += 1
        assert np.array_equal(np.flatnonzero(verts[k]), np.sort(ConvexHull(p).vertices)), k
        c, R, e = O.obb_from_points(p)
        gc, gR, ge = boxes[k, 0:3], boxes[k, 3:12].reshape(3, 3), boxes[k, 12:15]
        scale = np.abs(p).max()
        gap = np.diff(np.sort(np.linalg.eigvalsh(np.cov((p[verts[k]] - p[verts[k]].mean(0)).T, bias=True)))).min() / scale ** 2
        tol = 1e-9 * scale / max(gap, 1e-6)
        assert np.allclose(np.abs(np.sum(gR * R, axis=0)), 1.0, atol=1e-7 / max(gap, 1e-6)), (k, gap)
        assert np.abs(gc - c).max() < tol and np.abs(ge - e).max() < tol, (k, gap)
        assert abs(np.linalg.det(gR) - 1.0) < 1e-12 and np.allclose(gR.T @ gR, np.eye(3), atol=1e-12)
        assert (gR[np.abs(gR[:, 0]).argmax(), 0] > 0) and (gR[np.abs(gR[:, 1]).argmax(), 1] > 0)      # the sign convention of f3d.h
    assert ok >= 390                                                 # random data is in general position: everything else is certified
    # what must not be certified
    flat = rng.normal(size=(50, 3)); flat[:, 2] = 0.25
    dup = rng.normal(size=(40, 3)); dup[7] = dup[3]
    cube = np.array([[x, y, z] for x in (0., 1) for y in (0., 1) for z in (0., 1)])      # four coplanar points per face
    nan = rng.normal(size=(30, 3)); nan[4, 1] = np.nan
    b2, s2 = ctx.obb_fit([flat, rng.normal(size=(3, 3)), np.zeros((0, 3)), dup, cube, nan, flat @ np.linalg.qr(rng.normal(size=(3, 3)))[0]])
    assert s2.tolist() == [f3d.OBB_DEFERRED, f3d.OBB_FEW, f3d.OBB_FEW, f3d.OBB_DEFERRED, f3d.OBB_DEFERRED, f3d.OBB_DEFERRED, f3d.OBB_DEFERRED]
    assert (b2 == 0).all()
    # the same bits in every run, and a box does not depend on which non-vertices came along
    again, _ = ctx.obb_fit(sets[:50])
    assert np.array_equal(again, boxes[:50])
    k = next(i for i, p in enumerate(sets) if status[i] == f3d.OBB_OK and len(p) >= 700)
    only_vertices, st1 = ctx.obb_fit([sets[k][verts[k]]])
    assert st1[0] == f3d.OBB_OK and np.array_equal(only_vertices[0], boxes[k])


def test_obb_candidates_pipeline_on_the_device():
    """f3d_obb_candidates_dev: per id a subset of its members in ascending point index that contains every vertex of the hull of all
    members (so the box of the candidates is the box of the instance); small instances and uncertifiable inner hulls keep every
    member; ids outside [0, nids) are ignored."""
    import torch
    from scipy.spatial import ConvexHull
    ctx = f3d.default_context()
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(23)
    nids, n = 41, 90_000
    ids = rng.integers(-2, nids + 3, n).astype(np.int64)
    ids[ids == 5] = 6                                                  # an id without members
    small = np.flatnonzero(ids == 9); ids[small[100:]] = 10            # an id below min_members
    centres = rng.uniform(-4, 4, (nids + 3, 3))
    pts = centres[np.clip(ids, 0, nids + 2)] + rng.normal(size=(n, 3)) * [0.4, 0.2, 0.1]
    flat = np.flatnonzero(ids == 11); pts[flat, 2] = 1.0               # a flat instance: its inner hull cannot be certified
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        x, di = torch.from_numpy(pts).to(dev), torch.from_numpy(ids).to(dev)
        order = torch.empty(n, dtype=torch.int32, device=dev); keys = torch.empty(n, dtype=torch.int32, device=dev)
        starts = torch.empty(nids + 2, dtype=torch.int64, device=dev)
        cand = torch.empty(n, dtype=torch.int32, device=dev); cs = torch.empty(nids + 1, dtype=torch.int64, device=dev)
        ctx.group_by_id_dev(di.data_ptr(), n, nids, order.data_ptr(), keys.data_ptr(), starts.data_ptr(), s.cuda_stream)
        ctx.obb_candidates_dev(x.data_ptr(), f3d.F64, n, order.data_ptr(), keys.data_ptr(), starts.data_ptr(), nids, 256, cand.data_ptr(), cs.data_ptr(), s.cuda_stream)
        s.synchronize()
    cs, cand = cs.cpu().numpy(), cand.cpu().numpy()
    assert cs[0] == 0 and (np.diff(cs) >= 0).all()
    dropped = 0
    for k in range(nids):
        mem = np.flatnonzero(ids == k)
        c = cand[cs[k]:cs[k + 1]]
        assert np.array_equal(c, np.sort(c)) and set(c.tolist()) <= set(mem.tolist()), k
        if k in (9, 11) or len(mem) < 256:
            assert np.array_equal(c, mem), k
            continue
        hv = mem[ConvexHull(pts[mem]).vertices]
        assert set(hv.tolist()) <= set(c.tolist()), k
        dropped += len(mem) - len(c)
    assert dropped > 0.5 * n


def test_config_c5_merge_50m_points_4096_instances():
    """C5's merge leg at full size (BASELINE.json config 5): 50M points, 4096 instances, the product's own GPU fit.  The oracle's
    O(B^2 N) control flow cannot afford this size (it is compared at 160 instances above); at full size the evidence is a second run
    of the same scene in which every box comes from ANOTHER implementation of the fit (the oracle's scipy / LAPACK recipe, injected).
    (No "same parent" property holds: the reference looks parents up by LIST INDEX after entries have been deleted -- quirk
    Q6/Q7 -- which the drop-in reproduces.)"""
    import time
    from Fusion3DSeg.merge_intersecting_bb import merge_bb
    pts, ids, info = _c5_blobs(4096, 50_000_000)
    before = ids.copy()
    t0 = time.perf_counter()
    out_info, out_ids = merge_bb(None, copy.deepcopy(info), ids, pts)
    dt = time.perf_counter() - t0
    # independent evidence at full size: the same scene with the ORACLE's fit (scipy Qhull + LAPACK, on the host) injected
    # on the hull candidates -- another implementation of every box the control flow asks for -- must merge the same instances
    ref_info, ref_ids = merge_bb(None, copy.deepcopy(info), before.copy(), pts, box_fn=O.obb_from_points, prefilter=True)
    assert np.array_equal(out_ids, ref_ids) and [(d['id'], d['area']) for d in out_info] == [(d['id'], d['area']) for d in ref_info]
    _same_boxes(out_info, ref_info, tol=1e-7)
    assert len(out_info) < len(info) - 50
    moved = out_ids != before
    assert moved.any() and len(np.unique(out_ids)) < len(np.unique(before))
    boxed = [d for d in out_info[1:] if 'bbox' in d]
    assert len(boxed) > 3800 and all(np.asarray(d['bbox']).shape == (8, 3) for d in boxed[:64])
    print(f'C5 merge_bb: {dt:.2f} s')


def _info_rows(info):
    return np.array([[d['id'], int(d['isthing']), d['category_id'], d['area']] for d in info], np.int64).reshape(-1, 4)


def test_split_into_instances_gpu_matches_reference_golden(golden):
    from Fusion3DSeg.segUtils.cv import split_into_instances
    g = golden('split_instances')
    offs, flat = g['adj_offsets'], g['adj_flat']
    adj = [flat[offs[i]:offs[i + 1]] for i in range(len(offs) - 1)]
    for i in range(int(g['ncases'])):
        ic = g[f'case{i}_instance_classes'].tolist() if g[f'case{i}_has_instance_classes'] else None
        insts, ids, info, newcls = split_into_instances(g['classes'], adj, 133, ic, int(g[f'case{i}_minimum_points']))
        assert len(insts) == int(g[f'case{i}_ninst']), i
        assert np.array_equal(ids, g[f'case{i}_ids']), i
        assert np.array_equal(newcls, g[f'case{i}_classes']), i
        assert np.array_equal(_info_rows(info), g[f'case{i}_info']), i


@pytest.mark.parametrize('ic,minpts', [(None, 1), (None, 6), ([86, 114], 4), ([3, 133, 86], 5), ([133], 1)])
def test_split_into_instances_gpu_matches_oracle_random(ic, minpts):
    from Fusion3DSeg.segUtils.cv import split_into_instances
    rng = np.random.default_rng(17)
    n = 6000
    xy = rng.uniform(0, 30, (n, 3)) * [1, 1, 0.05]
    from scipy.spatial import cKDTree
    adj = cKDTree(xy).query_ball_point(xy, r=0.55)                       # symmetric radius graph, self included
    classes = rng.choice([86, 114, 115, 133, 3], n, p=[0.3, 0.25, 0.2, 0.15, 0.1]).astype(np.int64)
    want = O.split_into_instances(classes, adj, 133, ic, minpts)
    got = split_into_instances(classes, adj, 133, ic, minpts)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[3], want[3])
    assert np.array_equal(_info_rows(got[2]), _info_rows(want[2]))
    assert len(want[0]) > 10


def test_components_kernel_long_chains_and_bad_index():
    ctx = f3d.default_context()
    n = 200_000                                                          # one long path: worst case for label propagation
    offs = np.arange(0, 2 * n + 1, 2, dtype=np.int64)
    nb = np.stack([np.maximum(np.arange(n) - 1, 0), np.minimum(np.arange(n) + 1, n - 1)], axis=1).reshape(-1).astype(np.int32)
    cls = np.zeros(n, np.int64); cls[n // 2] = 7                         # cut the path in the middle
    root = ctx.components_same_class(cls, offs, nb)
    assert (root[:n // 2] == 0).all() and root[n // 2] == n // 2 and (root[n // 2 + 1:] == n // 2 + 1).all()
    nb[5] = n + 3
    with pytest.raises(IndexError):
        ctx.components_same_class(cls, offs, nb)


def _rows(offs, nbrs):
    return [np.sort(nbrs[offs[i]:offs[i + 1]]) for i in range(len(offs) - 1)]


def test_radius_graph_matches_sklearn_kdtree():
    """(f)#1 adjacency build (fusion.py:374-375) against the library the reference calls, ties at the radius included."""
    from sklearn.neighbors import KDTree
    ctx = f3d.default_context()
    rng = np.random.default_rng(21)
    lattice = np.stack(np.meshgrid(np.arange(9.), np.arange(7.), np.arange(5.), indexing='ij'), -1).reshape(-1, 3)
    far = rng.uniform(0, 2, (3000, 3)) + np.array([1.0e6, -2.0e6, 3.0e5])           # cell indices from large coordinates
    cases = [(synth.cloud(30_000), 0.1), (rng.uniform(-1, 1, (5000, 3)), 0.3), (lattice, 1.0), (lattice, np.sqrt(2.0)),
             (lattice * 0.05, 2 * 0.05), (far, 0.08), (np.repeat(rng.uniform(0, 1, (300, 3)), 4, axis=0), 0.0),
             (np.zeros((70, 3)), 0.5), (rng.uniform(0, 1, (1, 3)), 0.2), (rng.uniform(0, 1, (2, 3)), 5.0),
             (rng.uniform(0, 100, (4000, 3)) * [1, 1, 0], 2.5)]
    for P, r in cases:
        offs, nbrs = ctx.radius_graph(P, r)
        want = KDTree(P).query_radius(P, r=r)
        assert offs[0] == 0 and offs[-1] == len(nbrs) == sum(len(w) for w in want), (len(P), r)
        assert all(np.array_equal(np.sort(w), g) for w, g in zip(want, _rows(offs, nbrs))), (len(P), r)
        brute = O.radius_adjacency(P[:400], r)                                        # the oracle agrees on what it can afford
        if len(P) <= 400:
            assert all(np.array_equal(b, g) for b, g in zip(brute, _rows(offs, nbrs)))
    # float32 storage is widened exactly, as KDTree does
    P32 = synth.cloud(8000, dtype=np.float32)
    offs, nbrs = ctx.radius_graph(P32, 0.2)
    want = KDTree(P32.astype(np.float64)).query_radius(P32.astype(np.float64), r=0.2)
    assert all(np.array_equal(np.sort(w), g) for w, g in zip(want, _rows(offs, nbrs)))
    offs, nbrs = ctx.radius_graph(np.zeros((0, 3)), 0.3)
    assert offs.tolist() == [0] and len(nbrs) == 0
    bad = synth.cloud(100); bad[7, 1] = np.nan
    with pytest.raises(ValueError):                                                   # as sklearn: ValueError("Input contains NaN")
        ctx.radius_graph(bad, 0.1)


def test_radius_adjacency_feeds_split_into_instances():
    """adj.pkl's content and the CSR short cut give the same instances as the reference's KDTree adjacency."""
    from sklearn.neighbors import KDTree
    from Fusion3DSeg.fusion import radius_adjacency
    from Fusion3DSeg.segUtils.cv import split_into_instances
    rng = np.random.default_rng(22)
    P = rng.uniform(0, 6, (8000, 3)) * [1, 1, 0.1]
    classes = rng.choice([86, 114, 115, 133], len(P), p=[0.35, 0.3, 0.2, 0.15]).astype(np.int64)
    ds_radius = 0.06
    adj_ref = KDTree(P).query_radius(P, r=2 * ds_radius)
    adj = radius_adjacency(P, ds_radius)
    assert adj.dtype == object and all(a.dtype == np.int64 for a in adj[:5])
    assert all(np.array_equal(np.sort(a), np.sort(b)) for a, b in zip(adj, adj_ref))
    assert radius_adjacency(P, None) is None
    want = O.split_into_instances(classes, adj_ref, 133, [86, 114, 115], 5)
    for a in (adj, radius_adjacency(P, ds_radius, as_csr=True)):
        got = split_into_instances(classes, a, 133, [86, 114, 115], 5)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[3], want[3])
        assert np.array_equal(_info_rows(got[2]), _info_rows(want[2]))


def test_unproject_depth_matches_oracle_bit_for_bit():
    """(f)#3: ios_rtab.py:171-173,187-192 -- every depth storage type, an odd-sized frame, an un-normalised pose quaternion."""
    from RTAB_utils.ios_rtab import frame_points_world, resize_camera_matrix
    rng = np.random.default_rng(31)
    K = resize_camera_matrix(synth.CALIB_K, 256 / 1440, 192 / 1920)
    for (h, w) in [(192, 256), (37, 53), (1, 1)]:
        d16 = rng.integers(0, 6000, (h, w)).astype(np.uint16)
        d16[0, 0] = 0                                                       # holes stay at the camera centre
        for depth in (d16, d16.astype(np.float32) * np.float32(1.1), d16.astype(np.float64) * 0.93, d16.astype(np.int32)):
            q_xyzw = rng.normal(size=4) * 1.3
            t = rng.normal(size=3)
            want = O.unproject_depth(depth, K, q_xyzw[[3, 0, 1, 2]], t)
            got = frame_points_world(depth, K, q_xyzw, t)
            assert got.shape == (h * w, 3) and np.array_equal(got, want), (h, w, depth.dtype)
    assert f3d.default_context().unproject_depth(np.zeros((0, 5), np.uint16), K, [1, 0, 0, 0], [0, 0, 0]).shape == (0, 3)


def test_unproject_depth_batch_equals_frame_by_frame():
    """f3d_unproject_depth_batch_dev: F frames in one launch = F single-frame calls = the oracle, bit for bit (every depth type)."""
    import torch
    dev = torch.device('cuda', 0)
    ctx = f3d.default_context()
    rng = np.random.default_rng(41)
    F, h, w = 5, 48, 67
    K = np.array([[210.0, 0, w / 2], [0, 205.0, h / 2], [0, 0, 1]])
    q, t = rng.normal(size=(F, 4)) * 1.2, rng.normal(size=(F, 3))
    for code, d in [(2, rng.integers(0, 6000, (F, h, w)).astype(np.uint16)), (1, rng.uniform(0, 6, (F, h, w)).astype(np.float32)),
                    (0, rng.uniform(0, 6, (F, h, w)))]:
        want = np.stack([O.unproject_depth(d[f], K, q[f], t[f]) for f in range(F)])
        dd = torch.from_numpy(d.view(np.int16) if code == 2 else d).to(dev)
        out = torch.empty((F, h * w, 3), dtype=torch.float64, device=dev)
        s = torch.cuda.Stream(dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        ctx.unproject_depth_batch_dev(dd.data_ptr(), code, F, h, w, K, q, t, out.data_ptr(), 1000.0, s.cuda_stream)
        s.synchronize()
        assert np.array_equal(out.cpu().numpy(), want), code
        assert np.array_equal(want[2], ctx.unproject_depth(d[2], K, q[2], t[2]))
    # more frames than one launch carries in its argument block (64): the call splits itself
    F2, h2, w2 = 70, 5, 7
    q2, t2 = rng.normal(size=(F2, 4)), rng.normal(size=(F2, 3))
    d2 = rng.integers(0, 6000, (F2, h2, w2)).astype(np.uint16)
    dd = torch.from_numpy(d2.view(np.int16)).to(dev)
    out = torch.empty((F2, h2 * w2, 3), dtype=torch.float64, device=dev)
    ctx.unproject_depth_batch_dev(dd.data_ptr(), 2, F2, h2, w2, K, q2, t2, out.data_ptr(), 1000.0, None)
    ctx.synchronize()
    assert np.array_equal(out.cpu().numpy(), np.stack([O.unproject_depth(d2[f], K, q2[f], t2[f]) for f in range(F2)]))
    ctx.unproject_depth_batch_dev(None, 2, 0, h2, w2, K, np.zeros((0, 4)), np.zeros((0, 3)), None, 1000.0, None)      # no frames: nothing happens


def test_unproject_depth_matches_reference_golden(golden):
    """(f)#3 against the reference's own __getModP3d output (tests/golden/make_golden_rtab.py)."""
    from RTAB_utils.ios_rtab import frames_points_world
    g = golden('modp3d')
    got = frames_points_world(g['depths'], g['K'], g['odo_xyzw'], g['odo_xyz'])
    for q, t, orig, have, want in zip(g['odo_xyzw'], g['odo_xyz'], g['orig_ptx'], got, g['mod_ptx']):
        scale = np.dot(q, q) * np.abs(orig / 1000).max() + np.abs(t).max()
        assert np.abs(have - want).max() <= 8 * np.finfo(float).eps * scale


def test_fusion_fuse_matches_reference_golden(golden, tmp_path):
    """Rows a5 / (f)#2: Fusion.fuse + patch_downsample against the reference's own run on a synthetic sequence
    (tests/golden/make_golden_fuse.py): same shuffles from the seeded global generator, frustum cull + projection on the GPU."""
    from Fusion3DSeg.fusion import Fusion
    g = golden('fuse')
    h, w = (int(x) for x in g['hw'])
    F = len(g['points'])
    for ci in range(int(g['ncases'])):
        radius, angle, stride, max_depth, skip, seed = g[f'c{ci}_params']
        frames = [(f'{100 + j}', g['points'][j].copy(), g['normals'][j].copy(), g['colors'][j].copy(), g['valid'][j].copy())
                  for j in range(F)]
        lookups = {}
        fu = Fusion.from_frames(g['K'], w, h, g['wxyz'], g['t'], frames, lookup_dir=tmp_path if ci == 0 else None,
                                lookup_sink=lambda name, lut: lookups.__setitem__(name, np.array(lut, copy=True)))
        np.random.seed(int(seed))
        pts, nrm, clr, nmerges, occ = fu.fuse(float(radius), float(angle), None if stride < 0 else int(stride), float(max_depth), int(skip))
        assert np.array_equal(nmerges, g[f'c{ci}_nmerges']) and np.array_equal(occ, g[f'c{ci}_occurences']), ci
        assert occ.dtype == np.uint32
        assert sorted(int(k) for k in lookups) == g[f'c{ci}_uv2pt_names'].tolist()
        for name, want in zip(g[f'c{ci}_uv2pt_names'], g[f'c{ci}_uv2pt']):
            assert lookups[str(name)].dtype == np.int32 and np.array_equal(lookups[str(name)], want), (ci, name)
        for got, key in ((pts, 'ds_pts'), (nrm, 'ds_norms'), (clr, 'ds_clrs')):
            assert np.array_equal(got, g[f'c{ci}_{key}']), (ci, key)
        if ci == 0:                                                        # the .npy lookups the voting stage reads
            assert np.array_equal(np.load(tmp_path / '100.npy'), g['c0_uv2pt'][0])
            fu.dump_data(tmp_path / 'out', pts, nrm, clr, nmerges, occ)
            back = Fusion.load_data(tmp_path / 'out')
            assert np.array_equal(back[0], pts) and back[5] == F and tuple(back[6]) == (h, w)
            from sklearn.neighbors import KDTree
            ref_adj = KDTree(pts).query_radius(pts, r=2 * float(radius))
            assert all(np.array_equal(np.sort(a), np.sort(b)) for a, b in zip(back[7], ref_adj))
            assert (tmp_path / 'out' / 'fusion' / 'fusion_0_05_10.0.ply').is_file()


def test_patch_owner_kernel_matches_the_sequential_matching_loop():
    """a5: the data-parallel ownership formulation against the literal loop (oracle, pinned by fuse.npz) on random frames,
    seeds projecting outside the image (Python slice semantics of the window) included."""
    ctx = f3d.default_context()
    rng = np.random.default_rng(41)
    for trial, (h, w, half, m) in enumerate([(20, 28, 3, 900), (33, 17, 5, 400), (8, 8, 9, 60), (16, 16, 0, 300)]):
        q_pts = rng.uniform(0, 1, (h * w, 3)) * [1, 1, 0.05]
        q_nrm = rng.normal(size=(h * w, 3)); q_nrm /= np.linalg.norm(q_nrm, axis=1, keepdims=True)
        q_nrm[:, 2] = np.abs(q_nrm[:, 2]) + 1.0; q_nrm /= np.linalg.norm(q_nrm, axis=1, keepdims=True)
        free = rng.random((h, w)) < 0.85
        pix = rng.integers(0, h * w, m)
        x_pts = q_pts[pix] + rng.normal(0, 0.02, (m, 3))
        x_nrm = q_nrm[pix].copy()
        uv = np.stack([pix % w, pix // w]).astype(np.int32)
        uv[:, :12] += rng.integers(-2 * max(h, w), 2 * max(h, w), (2, 12)).astype(np.int32)     # seeds off the image, both signs
        radius, min_cos = 0.12, np.cos(np.deg2rad(35))
        owner = ctx.patch_owner(uv, x_pts, x_nrm, q_pts, q_nrm, free.reshape(-1), h, w, half, radius, min_cos)
        want = O.fuse_match_frame(uv, x_pts.copy(), x_nrm.copy(), np.zeros((m, 3)), np.zeros(m, np.int64), np.zeros(m, np.uint32),
                                  np.arange(m), q_pts, q_nrm, np.zeros((h * w, 3)), free.copy(), h, w, half, radius, min_cos)
        assert owner.dtype == np.int32 and np.array_equal(owner, want), trial
        assert (owner >= 0).sum() > 20
    assert np.array_equal(ctx.patch_owner(np.zeros((2, 0), np.int32), np.zeros((0, 3)), np.zeros((0, 3)), q_pts, q_nrm,
                                          free.reshape(-1), h, w, half, 0.1, 0.5), np.full(h * w, -1, np.int32))


def test_patch_downsample_rounds_match_the_sequential_order_of_events():
    """Fusion.patch_downsample (HIP seed resolution in rounds + ordered sums) against the literal visiting loop on random
    frames: same seeds, members, means, lookups and the same consumption of the global generator."""
    from Fusion3DSeg.fusion import Fusion
    rng = np.random.default_rng(43)
    for trial, (h, w, stride) in enumerate([(24, 32, 10), (17, 29, 4), (40, 40, 20), (9, 9, 1)]):
        n = h * w
        pts = np.stack(np.meshgrid(np.arange(w) * 0.03, np.arange(h) * 0.03), -1).reshape(-1, 2)
        pts = np.concatenate([pts, rng.normal(0, 0.01, (n, 1)) + (np.arange(n)[:, None] % 7 == 0) * 0.2], 1)
        nrm = rng.normal(0, 0.15, (n, 3)) + [0, 0, 1]; nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        clr = rng.uniform(0, 1, (n, 3))
        free0 = rng.random((h, w)) < 0.9
        pcdimg = np.arange(n).reshape(h, w)
        pt2u, pt2v = (np.arange(n) % w).astype(np.int32), (np.arange(n) // w).astype(np.int32)
        np.random.seed(100 + trial)
        fa = free0.copy()
        got = Fusion.patch_downsample(pts, nrm, clr, h, w, stride, 0.07, np.cos(np.deg2rad(20)), pcdimg, pt2u, pt2v, fa)
        after_a = np.random.random()
        np.random.seed(100 + trial)
        order = np.arange(n); np.random.shuffle(order)
        fb = free0.copy()
        want = Fusion._patch_downsample_sequential(order, pts, nrm, clr, h, w, stride // 2, 0.07, np.cos(np.deg2rad(20)), pcdimg, pt2u, pt2v, fb)
        assert np.random.random() == after_a                              # one shuffle each
        for a, b in zip(got, want):
            assert a.dtype == b.dtype and np.array_equal(a, b), trial
        assert np.array_equal(fa, fb) and len(got[0]) > 3
    # a free pixel with a zero normal does not accept itself: handled in the reference's own order of events
    nrm[5] = 0.0
    np.random.seed(7)
    with np.errstate(all='ignore'):
        z = Fusion.patch_downsample(pts, nrm, clr, h, w, 3, 0.07, 0.9, pcdimg, pt2u, pt2v, np.ones((h, w), bool))
    assert len(z[0]) == len(z[4])


def test_process3dseg_end_to_end_from_capture_files(golden, tmp_path):
    """process3D.py:14-68 on a capture written to disk: same cloud as the in-memory run, fusion directory complete."""
    from test_mirror_cpu import _write_capture
    from Fusion3DSeg.fusion import Fusion
    from Fusion3DSeg.process3D import process3DSeg
    g = golden('fuse')
    F = len(g['points'])
    _write_capture(tmp_path / 'capture', g, F)
    np.random.seed(11)
    pts, nrm, clr, nmerges, occ, nframes, hw, adj = process3DSeg(str(tmp_path / 'capture'), str(tmp_path / 'out'), radius=0.05, angle=10,
                                                                 stride=10, point_range=(0.1, 10), decimation=1, min_occ=3)
    assert np.array_equal(pts, g['c0_ds_pts']) and np.array_equal(nmerges, g['c0_nmerges']) and np.array_equal(occ, g['c0_occurences'])
    assert nframes == F and len(adj) == len(pts)
    lut_dir = tmp_path / 'capture' / 'fusion' / 'uv2pt'
    assert sorted(p.name for p in lut_dir.glob('*.npy')) == [f'{100 + j}.npy' for j in range(F)]
    assert np.array_equal(np.load(lut_dir / '102.npy'), g['c0_uv2pt'][2])
    assert (tmp_path / 'out' / 'fusion' / 'fusion_data.pkl').is_file() and (tmp_path / 'out' / 'fusion' / 'adj.pkl').is_file()


def test_other_intersections_primitives_match_reference_golden(golden):
    import Fusion3DSeg.intersections as I
    g = golden('intersections')
    tol = dict(rtol=1e-11, atol=1e-11)
    pts, within = I.ray_x_lines(g['rxl_origin'], g['rxl_direction'], g['rxl_starts'], g['rxl_ends'])
    assert np.allclose(pts, g['rxl_points'], **tol) and np.array_equal(within, g['rxl_within'])
    pts, valid = I.rays_x_plane(g['rxp_plane_point'], g['rxp_plane_normal'], g['rxp_origins'], g['rxp_directions'])
    assert np.allclose(pts, g['rxp_points'], **tol) and np.array_equal(valid, g['rxp_valid'])
    pts, valid = I.lines_x_planes(g['lxp_origins'], g['lxp_ends'], g['lxp_plane_points'], g['lxp_plane_normals'])
    assert np.allclose(pts, g['lxp_points'], **tol) and np.array_equal(valid, g['lxp_valid'])       # N == M broadcasting quirk
    assert str(g['lxp_n_ne_m_error']) == 'ValueError'
    with pytest.raises(ValueError):
        I.lines_x_planes(np.vstack([g['lxp_origins']] * 2), np.vstack([g['lxp_ends']] * 2), g['lxp_plane_points'], g['lxp_plane_normals'])
    inside, wb = I.point_inside_polygon(g['pip_points'], g['pip_vertices'])
    assert np.array_equal(inside, g['pip_inside']) and np.array_equal(wb, g['pip_within'])
    assert np.allclose(I.plane_x_plane(n1=g['pxp_n1'], n2=g['pxp_n2'], lookat=g['pxp_lookat']), g['pxp_dir_normals'], **tol)
    assert np.allclose(I.plane_x_plane(v1=g['pxp_v1'], v2=g['pxp_v2']), g['pxp_dir_vertices'], **tol)
    assert np.allclose(I.points_plane_projection(g['ppp_points'], g['ppp_plane_point'], g['ppp_normal']), g['ppp_out'], **tol)
    sp, ep, dr = I.lines_plane_projection(g['lpp_starts'], g['lpp_ends'], g['ppp_plane_point'], g['ppp_normal'])
    assert np.allclose(sp, g['lpp_out0'], **tol) and np.allclose(ep, g['lpp_out1'], **tol) and np.allclose(dr, g['lpp_out2'], **tol)
    for k in range(len(g['rrc_o1'])):
        with np.errstate(all='ignore'):
            pa, pb, dist, hit, wa, wb_ = I.ray_ray_closest(g['rrc_o1'][k], g['rrc_d1'][k], g['rrc_o2'][k], g['rrc_d2'][k])
        assert np.allclose(pa, g['rrc_pa'][k], equal_nan=True, rtol=1e-9, atol=1e-9)
        assert np.allclose(pb, g['rrc_pb'][k], equal_nan=True, rtol=1e-9, atol=1e-9)
        assert np.allclose(dist, g['rrc_distance'][k], equal_nan=True, rtol=1e-9, atol=1e-9)
        assert [bool(hit), bool(wa), bool(wb_)] == g['rrc_flags'][k].tolist()
