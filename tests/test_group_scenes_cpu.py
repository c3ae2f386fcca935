"""The scenes of tests/group_scenes.py are what tests/test_fuse_view_groups_gpu.py takes them for: conditions on the INPUTS, checked
with the oracle alone.  The compact clouds are checked against the two ways k_fuse (csrc/f3d_fuse.hip) leaves a view open for a point,
restated here with wide margins: the per-point cull (a plane of the view within the float32 margin of the point) and a view without
a centre row (the wave's box too large for its distance from the camera: centre_precompute)."""
import numpy as np
import pytest

import group_scenes as GS
from oracle import np_ref as O

CULL_MARGIN = 1e-3        # metres; k_fuse's per-point margin is ~1e-4 here: 32 * 2^-24 * (|p|_1 + |plane point|_1), both under 25 m
CHOSEN_193 = {'group0': (0, 63), 'group3': (192,), 'group1': (64, 127), 'groups0and3': (0, 63, 192), 'every': GS.group_edge_owners(193)}


def _plane_distances(V, pts):
    """[V, n, 5]: n . (p - plane point) for every view, point and plane, as the oracle orders the sum."""
    sc = GS.scene(V)
    ppts, pnrm = O.frustum_planes(sc.K, sc.w, sc.h, sc.q, sc.t, sc.max_depth)
    d = pts[None, :, None, :] - ppts[:, None, :, :]
    return (d[..., 0] * pnrm[:, None, :, 0] + d[..., 2] * pnrm[:, None, :, 2]) + d[..., 1] * pnrm[:, None, :, 1]


def test_group_edge_owners_are_the_first_and_last_view_of_their_groups():
    assert GS.group_edge_owners(63) == (0, 62) and GS.group_edge_owners(64) == (0, 63) and GS.group_edge_owners(65) == (0, 63, 64)
    assert GS.group_edge_owners(193) == (0, 63, 64, 127, 128, 191, 192)
    assert GS.group_edge_owners(1024) == (0, 63, 448, 511, 960, 1023) and GS.group_edge_owners(1025)[-1] == 1024
    pts, owner = GS.cloud(65, (0, 63, 64), 8, 200)
    assert len(pts) == 3 * 40 + 200 and list(owner[[0, 39, 40, 119, 120]]) == [0, 0, 63, 64, -1]
    assert not pts.flags.writeable and GS.cloud(65, (0, 63, 64), 8, 200)[0] is pts
    r = GS.cloud(65, (0, 63, 64), 8, 200, True)[0]
    assert np.array_equal(r, r.astype(np.float32).astype(np.float64)) and not np.array_equal(r[:120], pts[:120]) and np.array_equal(r[120:], pts[120:])


@pytest.mark.parametrize('kind,codes', [('const', 3), ('merged2', 4), ('block64', 10), ('alpha30', 32), ('alpha80', 82), ('iid', 136)])
def test_mask_kinds_select_their_instances(kind, codes):
    """Codes = labels present + "no sample" + "rejected": dword bins up to 12, the packed middle instances up to 48 and up to 100, then
    the any-alphabet instance (launch_fuse_t)."""
    for V in (65, 300):
        m = GS.masks(V, kind)
        assert m.shape == (V, GS.H, GS.W) and m.dtype == np.uint8 and not m.flags.writeable
        assert len(np.unique(m)) + 2 == codes


@pytest.mark.parametrize('where', sorted(CHOSEN_193))
@pytest.mark.parametrize('rounded', [False, True])
def test_compact_clouds_leave_open_only_views_of_the_chosen_groups(where, rounded):
    V, owners = 193, CHOSEN_193[where]
    sc = GS.scene(V)
    pts, owner = GS.compact_cloud(V, owners, rounded)
    assert len(pts) == GS.TILE * len(owners)
    dist = _plane_distances(V, pts)                                             # [V, n, 5]
    lowest = dist.min(2)
    could_be_open = np.abs(lowest) <= CULL_MARGIN                               # maybe and not sure, with ten times the margin
    assert np.all(could_be_open[owner, np.arange(len(pts))])                    # every point is that near a plane of its owner
    assert np.all(could_be_open.sum(0) == 1)                                    # ... and of no other view, of whichever group
    # every wave's box: small against its depth in every view that does not see it entirely outside (Q of centre_precompute < 0.5,
    # asked for at 0.4), in front of that camera, its centre within 1.9 image sizes of the image (2 asked for)
    eyes, lookats, _, _ = O.frustum_data(sc.K, sc.w, sc.h, sc.q, sc.t)
    _, pnrm = O.frustum_planes(sc.K, sc.w, sc.h, sc.q, sc.t, sc.max_depth)
    for k in range(len(owners)):
        tile = pts[k * GS.TILE:(k + 1) * GS.TILE]
        c, e = 0.5 * (tile.min(0) + tile.max(0)), 0.5 * (tile.max(0) - tile.min(0))
        assert e.max() <= 0.5, (where, k, e)
        base = _plane_distances(V, c[None])[:, 0, :]                            # [V, 5]
        spread = np.abs(pnrm) @ e
        seen = ~(base + spread < -CULL_MARGIN).any(1)
        assert seen[owners[k]]
        depth = np.einsum('vc,vc->v', c[None] - eyes, lookats)
        Q = (np.abs(lookats) @ e) / depth
        assert np.all(depth[seen] > 0) and np.all(Q[seen] < 0.4), (where, k, Q[seen].max())
        for v in np.flatnonzero(seen):
            uv = O.points2pixel(c[None], sc.K, sc.q[v], sc.t[v])[0]
            assert np.all(np.abs(uv) <= 1.9 * GS.W), (where, k, int(v), uv)


CLOUDS = [(V, (GS.group_edge_owners(V), 8, 200)) for V in (63, 64, 65, 127, 128, 129, 241, 242, 255, 256, 257, 1024, 1025)] + \
         [(V, (GS.group_edge_owners(V), 8, 400)) for V in (65, 129, 130, 255, 256)] + \
         [(193, (o, 40, 0)) for o in CHOSEN_193.values()] + [(193, (o, 'compact', 0)) for o in CHOSEN_193.values()] + \
         [(129, (GS.group_edge_owners(129), 40, 0)), (129, (GS.group_edge_owners(129), 'compact', 0)), (300, (tuple(range(0, 300, 13)), 12, 500))]


@pytest.mark.parametrize('V,cloud', CLOUDS, ids=lambda x: str(x) if isinstance(x, int) else f'{len(x[0])}owners-{x[1]}-{x[2]}')
def test_the_oracle_votes_for_the_on_plane_points(V, cloud):
    """At least 90 % of every cloud's on-plane points get a vote (the choice of masks does not matter: a vote is a sample)."""
    for rounded in (False, True):
        assert GS.voted_share(V, 'const', *cloud, rounded) >= 0.9, rounded


def test_bins_above_255_at_300_views():
    cloud = (tuple(range(0, 300, 13)), 12, 500)
    for rounded in (False, True):
        own = GS.points(300, *cloud, rounded)[1] >= 0
        assert (GS.votes(300, 'const', *cloud, rounded)[own].max(1) > 255).sum() >= 10
        assert (GS.votes(300, 'merged2', *cloud, rounded).max(1) > 255).sum() >= 1
        assert GS.votes(300, 'block64', *cloud, rounded).max() < 255 and GS.votes(300, 'iid', *cloud, rounded).max() < 255
