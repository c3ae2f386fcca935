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
