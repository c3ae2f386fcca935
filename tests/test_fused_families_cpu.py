"""The scene families of fused_families.py are not vacuous: conditions on the INPUTS of test_fused_geometry_gpu.py, checked with the
oracle alone (f3d.views_build is host code and needs no device)."""
import numpy as np
import pytest

import f3d
import fused_families as FF
from oracle import np_ref as O


@pytest.mark.parametrize('name', FF.FAMILIES + FF.EXTRA_CAMERAS)
def test_views_build_planes_and_qinv_equal_the_oracle(name):
    _, K, q, t, max_depth, w, h, _ = FF.family(name)
    F = f3d.view_fields(f3d.views_build(K, w, h, q, t, max_depth))
    ppts, pnrm = O.frustum_planes(K, w, h, q, t, max_depth)
    assert np.array_equal(F['plane_pt'], ppts) and np.array_equal(F['plane_n'], pnrm)
    assert np.array_equal(F['qinv'], np.stack([O.quat_inverse(x) for x in q]))


@pytest.mark.parametrize('name', FF.FAMILIES)
def test_random_cloud_is_seen_and_voted_for(name):
    pts, K, q, t, max_depth, w, h, masks = FF.family(name)
    ppts, pnrm = O.frustum_planes(K, w, h, q, t, max_depth)
    share = np.array([O.point_inside_polyhedra(pts, ppts[j], pnrm[j]).mean() for j in range(len(t))])
    assert (share >= 0.01).sum() >= 3, share
    votes = O.forward_votes(pts, K, q, t, masks, max_depth, ncols=134)
    assert votes.sum() >= 0.1 * len(pts), votes.sum() / len(pts)


@pytest.mark.parametrize('name', FF.FAMILIES)
def test_on_plane_cloud_straddles_the_planes_of_its_own_view(name):
    _, K, q, t, max_depth, w, h, _ = FF.family(name)
    per = FF.PLANE_PER.get(name, 300)
    pts, owner = FF.on_plane_points(name, per), FF.on_plane_owner(name, per)
    assert len(pts) == len(t) * 5 * per <= 32_000
    ppts, pnrm = O.frustum_planes(K, w, h, q, t, max_depth)
    for j in range(len(t)):
        own = pts[owner == j]
        share = O.point_inside_polyhedra(own, ppts[j], pnrm[j]).mean()
        assert 0.3 <= share <= 0.7, (j, share)
        # ... and really on the planes: a handful of ulp of the coordinates' magnitude from the plane each was drawn on
        for m in range(5):
            d = own[m * per:(m + 1) * per] - ppts[j, m]
            scale = np.abs(own).max() + np.abs(d).max()
            assert np.abs(d @ pnrm[j, m]).max() <= 64 * np.finfo(np.float64).eps * scale, (j, m)


def _on_plane_points_as_first_written(name, per):
    """on_plane_points as it stood before its body became on_plane_points_of (a function of the scene, with chosen owner views): kept
    word for word as the record of the clouds every family test has run on."""
    _, K, q, t, max_depth, w, h, _ = FF.family(name)
    rng = np.random.default_rng(29)
    Kinv = O.inv3(K)
    eyes, lookats, _, _ = O.frustum_data(K, w, h, q, t)
    ppts, pnrm = O.frustum_planes(K, w, h, q, t, max_depth)
    out = []
    for j in range(len(t)):
        def rays(pix):                                                   # unit rays through pixels, as O.frustum_data builds them
            cam = np.stack([(Kinv[r, 0] * pix[:, 0] + Kinv[r, 1] * pix[:, 1]) + Kinv[r, 2] * pix[:, 2] for r in range(3)], axis=1)
            vec = (O.rotate(q[j], cam) + t[j][None, :]) - eyes[j][None, :]
            return vec / np.sqrt((vec[:, 0] * vec[:, 0] + vec[:, 1] * vec[:, 1]) + vec[:, 2] * vec[:, 2])[:, None]

        def snap(p, m):                                                  # one Newton step onto plane m as the oracle evaluates it
            g = p - ppts[j, m]
            return p - ((g[:, 0] * pnrm[j, m, 0] + g[:, 2] * pnrm[j, m, 2]) + g[:, 1] * pnrm[j, m, 1])[:, None] * pnrm[j, m]

        corner = rays(np.array([[0, 0, 1], [w, 0, 1], [w, h, 1], [0, h, 1]], np.float64))
        for m in range(4):
            a, b = corner[m], corner[(m + 1) % 4]
            s, r = rng.uniform(0.05, 1.0, (per, 1)), rng.uniform(0.0, max_depth, (per, 1))
            out.append(snap(eyes[j] + r * (s * a + (1 - s) * b), m))
        d = rays(np.stack([rng.uniform(-0.2 * w, 1.2 * w, per), rng.uniform(-0.2 * h, 1.2 * h, per), np.ones(per)], axis=1))
        out.append(snap(eyes[j] + max_depth * d / ((d[:, 0] * lookats[j, 0] + d[:, 1] * lookats[j, 1]) + d[:, 2] * lookats[j, 2])[:, None], 4))
    pts = np.concatenate(out)
    return FF._ulp_steps(pts, rng.integers(-3, 4, pts.shape))


@pytest.mark.parametrize('name', FF.FAMILIES)
def test_on_plane_points_are_the_same_bytes_as_before_the_split(name):
    per = FF.PLANE_PER.get(name, 300)
    _, K, q, t, max_depth, w, h, _ = FF.family(name)
    want = _on_plane_points_as_first_written(name, per).tobytes()
    assert FF.on_plane_points(name, per).tobytes() == want
    assert FF.on_plane_points_of(K, q, t, max_depth, w, h, per, owners=tuple(range(len(t)))).tobytes() == want   # every view named = None
    # a chosen owner gets points of its own planes: the draws differ (the stream starts with it), the construction does not
    last = len(t) - 1
    own = FF.on_plane_points_of(K, q, t, max_depth, w, h, 20, owners=(last,))
    ppts, pnrm = O.frustum_planes(K, w, h, q, t, max_depth)
    for m in range(5):
        d = own[m * 20:(m + 1) * 20] - ppts[last, m]
        assert np.abs(d @ pnrm[last, m]).max() <= 64 * np.finfo(np.float64).eps * (np.abs(own).max() + np.abs(d).max()), m


def test_families_are_seeded_and_change_one_thing():
    base = FF.family('base')
    assert FF.family('base') is base                                      # cached: the tests share one copy
    assert not base[0].flags.writeable and not FF.on_plane_points('base').flags.writeable
    for name, T in FF.SHIFTS.items():
        fam = FF.family(name)
        assert np.array_equal(fam[0], base[0] + np.array(T)) and np.array_equal(fam[2], base[2])
    assert np.array_equal(FF.family('q_big')[2], base[2] * 30.0) and np.array_equal(FF.family('q_big')[0], base[0])
    kinds = [FF.MASK_KIND[n] for n in FF.FAMILIES]
    assert abs(kinds.count('iid') - kinds.count('block64')) <= 1
    assert FF.family('many')[7].shape == (70, FF.H, FF.W) and len(FF.family('many')[0]) == 5_000
    # the roll is real: the cameras' x axes are not horizontal
    x_axis = np.stack([O.rotate(q, np.array([[1.0, 0, 0]]))[0] for q in base[2]])
    assert (np.abs(x_axis[:, 2]) > 0.05).sum() >= 6
