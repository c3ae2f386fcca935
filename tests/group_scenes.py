"""Scenes with any number of views for the fused call's 64-view groups (k_fuse, k_fuse_mid: csrc/f3d_fuse.hip): the rolled ring
cameras of fused_families.py on a small image, masks by kind (one per k_fuse instance), and clouds whose first points lie within a
few ulp of the frustum planes of CHOSEN views -- such a point cannot be proven by the float32 tier for its owner view, so it leaves
that view open, in group owner // 64.  The oracle's vote rows are computed once per (views, mask kind, cloud) and shared.
NumPy only, seeded, nothing here touches the GPU; no tests in this file; arrays are cached and read-only."""
import functools
from types import SimpleNamespace

import numpy as np

import f3d
from f3d import synth
from oracle import np_ref as O
import fused_families as FF

H = W = 64
K = np.array([[50., 0, 32], [0, 50., 32], [0, 0, 1]])
MAX_DEPTH, NCLASSES = 10.0, 133
MASK_KINDS = ('block64', 'const', 'iid', 'alpha30', 'alpha80', 'merged2')
# (threshold, filter list): the reference's threshold with and without a filter list, and the threshold that switches the table off
SETTINGS = ((0.0, None), (0.5, None), (0.5, (86, 114, 115)))
K.setflags(write=False)


def _frozen(a):
    a.setflags(write=False)
    return a


def group_edge_owners(V):
    """The first and last view of every 64-view group (up to 257 views); beyond, of groups 0, 7, 15 and of group 16 where it exists."""
    ngroups = (V + 63) // 64
    groups = range(ngroups) if V <= 257 else [g for g in (0, 7, 15, 16) if g < ngroups]
    return tuple(sorted({v for g in groups for v in (64 * g, min(64 * g + 63, V - 1))}))


@functools.lru_cache(maxsize=None)
def _alphabet_masks(V, nlabels):
    """8 x 8-pixel blocks, every block one label of a seeded choice of `nlabels` of the labels 0..132; every label of the choice occurs."""
    rng = np.random.default_rng([4321, nlabels])
    alphabet = np.sort(rng.choice(NCLASSES, nlabels, replace=False)).astype(np.uint8)
    blocks = alphabet[rng.integers(0, nlabels, (V, H // 8, W // 8))]
    blocks.reshape(-1)[:nlabels] = alphabet                                # (view 0 shows them all, whatever the draw)
    return np.ascontiguousarray(np.repeat(np.repeat(blocks, 8, axis=1), 8, axis=2))


@functools.lru_cache(maxsize=None)
def masks(V, kind):
    """uint8 [V, H, W].  block64: one of 8 labels per view (10 codes: the dword-bin instance); const: label 86 everywhere (3 codes, dword
    bins); merged2: block64 with its eight labels merged into two, seven to one (4 codes, dword bins); alpha30 / alpha80: 32 / 82 codes, the two packed
    middle instances; iid: every pixel uniform over 0..133 (136 codes, the any-alphabet instance)."""
    if kind == 'block64':
        m = synth.masks(V, H, W, 'block64')
    elif kind == 'const':
        m = np.full((V, H, W), 86, np.uint8)
    elif kind == 'iid':
        m = synth.masks(V, H, W, 'iid')
    elif kind == 'merged2':
        m = np.where(synth.masks(V, H, W, 'block64') == 86, 114, 86).astype(np.uint8)   # seven of the eight become 86, label 86 becomes 114
    elif kind in ('alpha30', 'alpha80'):
        m = _alphabet_masks(V, int(kind[5:])).copy()
    else:
        raise KeyError(kind)
    return _frozen(m)


@functools.lru_cache(maxsize=None)
def scene(V):
    """-> namespace: V, K, q [V,4] (wxyz, camera -> world), t [V,3], max_depth, w, h, views (the f3d_view table), masks(kind)."""
    q, t = FF._rolled_cameras(V, 4.0, (0.3, 2.7), seed=FF.CAMERA_SEED)
    views = f3d.views_build(K, W, H, q, t, MAX_DEPTH)
    return SimpleNamespace(V=V, K=K, q=_frozen(q), t=_frozen(t), max_depth=MAX_DEPTH, w=W, h=H, views=_frozen(views),
                           masks=functools.partial(masks, V))


@functools.lru_cache(maxsize=None)
def cloud(V, owners, per, n_random, rounded=False):
    """-> (points [n,3] float64, owner int64 [n]): per owner view (a tuple of view indices) 5 * per points on its frustum planes, in
    (owner, plane, draw) order, then n_random points of the synthetic room (owner -1; float32 values as drawn).
    rounded: every coordinate rounded to float32 -- what float32 storage holds.  The rounding moves an on-plane point by half a float32
    ulp at most: still far inside the float32 tier's margin (k_fuse defers it), but ~1e8 times the float64 tier's margin, so k_fuse_mid
    proves it and the reference's own arithmetic is not needed.  Only the points as built (float64 storage) reach that last tier; from
    here on only the oracle says on which side of its plane a point of either form lies."""
    sc = scene(V)
    owners = tuple(int(v) for v in owners)
    assert all(0 <= v < V for v in owners)
    parts, owner = [], []
    if owners and per:
        parts.append(FF.on_plane_points_of(sc.K, sc.q, sc.t, sc.max_depth, sc.w, sc.h, per, owners))
        owner.append(np.repeat(np.array(owners, np.int64), 5 * per))
    if n_random:
        parts.append(synth.cloud(n_random, seed=3))
        owner.append(np.full(n_random, -1, np.int64))
    pts = np.concatenate(parts)
    if rounded:
        pts = pts.astype(np.float32).astype(np.float64)
    return _frozen(pts), _frozen(np.concatenate(owner))


TILE = 128                                   # points of one wave of k_fuse: two per lane, consecutive in the order the kernel reads them
ROOM_CENTRE = np.array([0.0, 0.0, 1.5])
CLEAR = 2e-3                                 # metres: twenty times the float32 margin of k_fuse's per-point cull at these magnitudes


@functools.lru_cache(maxsize=None)
def _compact_points(V, owners, draw=16000):
    sc = scene(V)
    ppts, pnrm = O.frustum_planes(sc.K, sc.w, sc.h, sc.q, sc.t, sc.max_depth)
    parts = []
    for i, v in enumerate(owners):
        m = i % 4                                                             # the owners take the four side planes in turn (a far plane is too sparsely drawn for a patch)
        c = FF.on_plane_points_of(sc.K, sc.q, sc.t, sc.max_depth, sc.w, sc.h, draw, (v,))[m * draw:(m + 1) * draw]
        anchor = c[np.argmin(((c - ROOM_CENTRE) ** 2).sum(1))]
        c = c[np.argsort(((c - anchor) ** 2).sum(1), kind='stable')[:4 * TILE]]
        # ... without the points that ANOTHER view's frustum boundary passes within CLEAR of (193 frusta cut every patch somewhere)
        d = c[None, :, None, :] - ppts[:, None, :, :]
        lowest = ((d[..., 0] * pnrm[:, None, :, 0] + d[..., 2] * pnrm[:, None, :, 2]) + d[..., 1] * pnrm[:, None, :, 1]).min(2)   # [V, 4 TILE]
        lowest[v] = np.inf
        c = c[(np.abs(lowest) > CLEAR).all(0)][:TILE]
        assert len(c) == TILE
        parts.append(c)
    return _frozen(np.concatenate(parts))


@functools.lru_cache(maxsize=None)
def compact_cloud(V, owners, rounded=False):
    """-> (points [TILE * len(owners), 3], owner [n]): per owner view ONE wave's worth of points, all on one side plane of that view and the
    TILE closest to each other of a large draw (the patch of the plane nearest the middle of the room, a few decimetres across).  In
    caller order every wave of k_fuse then holds one such patch: its box is small against its distance from every camera that sees it,
    so every view has a centre row, and a point's open views are the views with a plane within the float32 margin of the point itself
    -- its owner and no other view: points that another frustum's boundary passes within CLEAR of are left out of the patch
    (tests/test_group_scenes_cpu.py checks both on the host).  The clouds of cloud(), spread
    over whole frustum planes, make wave boxes of metres: there most views have no usable row and leave every point open."""
    owners = tuple(int(v) for v in owners)
    pts = _compact_points(V, owners)
    if rounded:
        pts = _frozen(pts.astype(np.float32).astype(np.float64))
    return pts, _frozen(np.repeat(np.array(owners, np.int64), TILE))


def points(V, owners, per, n_random, rounded=False):
    """per == 'compact': compact_cloud(V, owners); otherwise cloud(V, owners, per, n_random)."""
    return compact_cloud(V, owners, rounded) if per == 'compact' else cloud(V, owners, per, n_random, rounded)


@functools.lru_cache(maxsize=None)
def votes(V, kind, owners, per, n_random, rounded=False):
    """The oracle's vote rows of points(V, owners, per, n_random, rounded) under masks(V, kind): float64 [n, NCLASSES + 1], computed once."""
    sc = scene(V)
    pts, _ = points(V, owners, per, n_random, rounded)
    with np.errstate(all='ignore'):
        return _frozen(O.forward_votes(pts, sc.K, sc.q, sc.t, masks(V, kind), sc.max_depth, ncols=NCLASSES + 1))


@functools.lru_cache(maxsize=None)
def labels(V, kind, owners, per, n_random, rounded, threshold, flt):
    """The oracle's labels of that cloud for one setting (flt: None or a tuple): int64 [n].  A label depends on the point's own row
    alone, so the labels of the cloud's first n points are the first n of these."""
    return _frozen(O.segment(votes(V, kind, owners, per, n_random, rounded), NCLASSES, threshold, None if flt is None else list(flt)))


def voted_share(V, kind, owners, per, n_random, rounded=False):
    """Share of the cloud's on-plane points that some view votes for (oracle)."""
    own = points(V, owners, per, n_random, rounded)[1] >= 0
    return float((votes(V, kind, owners, per, n_random, rounded)[own].sum(1) > 0).mean())


def labelled_and_unlabelled(V, kinds, owners, per, n_random, rounded, threshold):
    """True when, under at least one of the mask kinds, the on-plane points hold both labelled and unlabelled ones at this threshold."""
    own = points(V, owners, per, n_random, rounded)[1] >= 0
    for kind in kinds:
        lab = labels(V, kind, owners, per, n_random, rounded, threshold, None)[own] != NCLASSES
        if lab.any() and not lab.all():
            return True
    return False
