"""Surface normals, host side: the oracle (tests/normals_ref.py) against the reference's orientation lines and analytic clouds, and
no CPU fallback for surface_normal_estimation / frames_world_dev."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np

import normals_ref as R

ROOT = Path(__file__).resolve().parent.parent
PKG = ROOT / '3d-point-cloud-segmentation-using-2d-img-segmentation_amd'


def test_oracle_orientation_reproduces_the_reference_bit_for_bit(golden):
    g = golden('normals_orient')
    got = R.orient(g['points'], g['raw'], g['cam_centre'])
    assert np.array_equal(got.view(np.uint64), g['oriented'].view(np.uint64))
    dots = R.orient_dots(g['points'], g['raw'], g['cam_centre'])
    assert np.isnan(dots).sum() >= 40 and (dots == 0).sum() >= 40        # the fixture holds both edge cases
    assert (g['oriented'] != g['raw']).any(axis=1).sum() > 0


def _angle(a, b):
    """Angle between unit vectors up to sign, per row."""
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=1), np.abs(np.einsum('ij,ij->i', a, b)))


def test_oracle_on_a_noise_free_tilted_plane():
    u, v = np.meshgrid(np.arange(40) * 0.01, np.arange(30) * 0.01)
    e1, e2 = np.array([1.0, 0.2, -0.3]), np.array([0.1, 1.0, 0.4])
    pts = np.stack([u.ravel(), v.ravel()], 1) @ np.stack([e1, e2]) + [0.3, -0.2, 2.0]
    want = np.cross(e1, e2)
    want /= np.linalg.norm(want)
    nrm, gap, degenerate, nb = R.normals(pts, 0.05, 30)
    assert not degenerate.any()
    assert all(len(k) == min(30, len(k)) for k in nb)
    assert _angle(nrm, np.tile(want, (len(pts), 1))).max() < 1e-9
    oriented = R.orient(pts, nrm, np.zeros(3))
    assert (np.einsum('ij,ij->i', oriented, pts) <= 0).all()             # facing the camera at the origin


def test_oracle_on_a_sphere():
    k = np.arange(20000) + 0.5
    phi, theta = np.arccos(1 - 2 * k / len(k)), np.pi * (1 + 5 ** 0.5) * k   # Fibonacci sphere, spacing ~1.3 cm
    pts = np.stack([np.cos(theta) * np.sin(phi), np.sin(theta) * np.sin(phi), np.cos(phi)], 1) + [1.0, 2.0, 3.0]
    nrm, gap, degenerate, _ = R.normals(pts, 0.05, 30)
    assert not degenerate.any()
    radial = pts - [1.0, 2.0, 3.0]
    assert _angle(nrm, radial).max() < 0.05
    oriented = R.orient(pts, nrm, np.array([1.0, 2.0, 3.0]))             # camera at the centre: every normal points inwards
    assert (np.einsum('ij,ij->i', oriented, radial) < 0).all()


def test_oracle_degenerate_rows():
    pts = np.array([[0.0, 0.0, 0.0]] * 5 + [[1.0, 0.0, 0.0], [1.01, 0.0, 0.0], [5.0, 5.0, 5.0]])
    nrm, gap, degenerate, nb = R.normals(pts, 0.05, 3)
    assert degenerate.all() and (nrm == [0.0, 0.0, 1.0]).all()
    assert [list(x) for x in nb[:2]] == [[0, 1, 2], [0, 1, 2]] and list(nb[5]) == [5, 6] and list(nb[7]) == [7]


def test_normals_have_no_cpu_fallback():
    """Without a device (none visible to the child process) both entry points raise F3DUnavailable."""
    code = ('import numpy as np, f3d\n'
            'from RTAB_utils import ios_rtab\n'
            'for call in (lambda: ios_rtab.surface_normal_estimation(np.zeros((4, 3)), np.zeros(3)),\n'
            '             lambda: ios_rtab.frames_world_dev(np.zeros((1, 2, 2), np.uint16), np.eye(3), [[0, 0, 0, 1]], [[0, 0, 0]])):\n'
            '    try:\n'
            '        call()\n'
            '    except f3d.F3DUnavailable:\n'
            '        continue\n'
            '    raise SystemExit("no F3DUnavailable")\n'
            'print("ok")\n')
    env = dict(os.environ, HIP_VISIBLE_DEVICES='-1', ROCR_VISIBLE_DEVICES='-1', CUDA_VISIBLE_DEVICES='-1',
               PYTHONPATH=os.pathsep.join([str(ROOT), str(PKG)]))
    r = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == 'ok', r.stdout + r.stderr
