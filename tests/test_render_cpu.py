"""Occlusion-aware forward voting, host side: the test-only restatement of the z-buffer contract (tests/render_ref.py) agrees with
the oracle where the two must agree, separates the two-wall scene, and the product has no CPU fallback."""
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import render_ref as R
from f3d import synth
from oracle import np_ref as O

ROOT = Path(__file__).resolve().parent.parent
PKG = ROOT / '3d-point-cloud-segmentation-using-2d-img-segmentation_amd'


def _scene(n, V, H, W, seed=3):
    pts = synth.cloud(n, seed=seed)
    q, t = synth.ring_views(V)
    return pts, R.pinhole(H, W), q, t, synth.masks(V, H, W, 'iid')


@pytest.mark.parametrize('splat', [0, 1, 2])
def test_every_sample_is_visible_at_infinite_tolerance(splat):
    pts, K, q, t, masks = _scene(3000, 5, 24, 40)
    want = O.forward_votes(pts, K, q, t, masks, 10.0)
    assert want.sum() > 3000                                                 # the views do see the cloud
    got = R.visible_votes(pts, K, q, t, masks, 10.0, splat, np.inf)
    assert got.dtype == want.dtype and np.array_equal(got, want)
    near = R.visible_votes(pts, K, q, t, masks, 10.0, splat, 0.05)
    assert (near <= want).all() and 0 < near.sum() < want.sum()              # the test does remove votes, and only removes


def test_lookup_votes_are_a_subset_of_the_forward_votes():
    """splat = 0: a pixel's winner is one of the samples of that very pixel, so the reference's vote over the lookups gives every
    (point, label) cell at most what the forward path gives it."""
    pts, K, q, t, masks = _scene(3000, 5, 24, 40)
    depth, uv2pt = R.lookups(pts, K, q, t, (24, 40), 10.0, 0)
    assert depth.dtype == np.float32 and uv2pt.dtype == np.int32 and depth.shape == (5, 24, 40) and uv2pt.shape == (5, 960)
    assert np.array_equal(np.isinf(depth).reshape(5, -1), uv2pt == -1) and (uv2pt >= 0).any()
    votes = np.zeros((len(pts), 134))
    for j in range(5):
        O.vote_frame(votes, uv2pt[j], masks[j].reshape(-1))
    full = R.visible_votes(pts, K, q, t, masks, 10.0, 0, np.inf)
    assert votes.sum() == (uv2pt >= 0).sum() and (votes <= full).all()
    # and the winners are exactly the samples that pass the test with no tolerance, up to ties in float32 depth
    front = R.visible_votes(pts, K, q, t, masks, 10.0, 0, 0.0)
    assert (votes <= front).all()


def test_keys_order_by_float32_depth_then_index():
    idx = np.array([5, 2, 9, 7])
    z32 = np.array([2.0, 2.0, 1.5, 3.0], np.float32)
    u, v = np.array([1, 1, 3, 1]), np.array([1, 1, 0, 1])
    depth, uv2pt = R.unpack(R.view_keys(idx, u, v, z32, 3, 4, 0))
    assert uv2pt[1 * 4 + 1] == 2 and depth[5] == 2.0 and uv2pt[3] == 9 and (uv2pt >= 0).sum() == 2
    depth, uv2pt = R.unpack(R.view_keys(idx, u, v, z32, 3, 4, 1))             # 3 x 3 patches, clipped to 3 x 4
    assert uv2pt.reshape(3, 4).tolist() == [[2, 2, 9, 9], [2, 2, 9, 9], [2, 2, 2, -1]]


def test_two_walls_are_told_apart_by_the_restatement():
    pts, far, K, q, t, masks, hw = R.two_walls()
    plain = O.forward_votes(pts, K, q, t, masks, 10.0)
    assert (plain[:, 86] == 3).all() and (plain[:, 114] == 3).all()           # without the test both walls collect both labels
    assert (O.segment(plain, 133, 0.5) == 86).all()
    votes = R.visible_votes(pts, K, q, t, masks, 10.0, 1, 0.05)
    cls = O.segment(votes, 133, 0.5)
    assert (cls[~far] == 86).all() and (cls[far] == 114).all()
    assert (votes[~far, 86] == 3).all() and (votes[far, 114] == 3).all() and votes.sum() == 3 * len(pts)


def test_visible_voting_has_no_cpu_fallback():
    """Without a device (none visible to the child process) both functions raise F3DUnavailable."""
    code = ('import numpy as np, f3d\n'
            'from Fusion3DSeg import fusion\n'
            'P, K = np.random.default_rng(0).random((8, 3)), np.array([[4., 0, 3], [0, 4., 2], [0, 0, 1]])\n'
            'q, t = np.array([[1., 0, 0, 0]]), np.zeros((1, 3))\n'
            'for call in (lambda: fusion.render_lookups(P, K, q, t, (5, 7)),\n'
            '             lambda: fusion.project_vote_argmax_visible(P, K, q, t, np.zeros((1, 5, 7), np.uint8))):\n'
            '    try:\n'
            '        call()\n'
            '    except f3d.F3DUnavailable:\n'
            '        print("ok")\n')
    env = dict(os.environ, HIP_VISIBLE_DEVICES='-1', ROCR_VISIBLE_DEVICES='-1', CUDA_VISIBLE_DEVICES='-1',
               PYTHONPATH=os.pathsep.join([str(ROOT), str(PKG)]))
    r = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.split() == ['ok', 'ok'], r.stdout + r.stderr


def test_library_declares_the_render_entries():
    import f3d
    lib = f3d.library()
    for name in ('f3d_render_lookups', 'f3d_render_lookups_dev', 'f3d_vote_visible', 'f3d_vote_visible_dev', 'f3d_ctx_reserve_render'):
        assert name in lib._f3d_symbols and hasattr(lib, name)


def test_product_imports_neither_oracle_nor_tests():
    src = (PKG / 'Fusion3DSeg' / 'fusion.py').read_text()
    assert not re.search(r'^\s*(from|import)\s+(oracle|tests|render_ref)\b', src, re.M)
