"""Triangle z-buffer renders on the GPU: the rasteriser (f3d_render_mesh_lookups*), the face vote (f3d_vote_faces*), the forward vote
behind a mesh occluder (f3d_vote_visible_mesh*) and their Python entry points against the test-only restatement
(tests/raster_ref.py).  The contract is deterministic, so every comparison is array_equal unless it says otherwise."""
import numpy as np
import pytest

import f3d
import raster_ref as M
import render_ref as R
from f3d import synth
from Fusion3DSeg import fusion
from Fusion3DSeg.segUtils import meshUtils
from oracle import np_ref as O

pytestmark = pytest.mark.gpu
IMAGES = ((7, 5), (24, 40))                                                    # (H, W)
MAX_DEPTH = 10.0
Q1, T1 = M.IDENTITY


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


@pytest.fixture(scope='module')
def ctx():
    return f3d.default_context(0)


def _views(K, hw, q, t, max_depth=MAX_DEPTH):
    return f3d.views_build(K, hw[1], hw[0], q, t, max_depth)


def _face_votes(ctx, verts, tris, views, masks, z_far=MAX_DEPTH, per=0, ncols=134):
    return ctx.vote_faces(np.zeros((len(tris), ncols)), verts, tris, views, masks, z_far, per)


def _dev_render(ctx, verts, tris, views, hw, z_far=np.inf, list_capacity=None):
    """render_mesh_lookups_dev (or, with a list capacity, the counting diagnostic) on device copies -> depth, uv2tri, third"""
    import torch
    dev = torch.device('cuda', ctx.device)
    s = torch.cuda.Stream(dev)
    dv, dt, dw = torch.from_numpy(verts).to(dev), torch.from_numpy(tris).to(dev), torch.from_numpy(views).to(dev)
    V = len(views)
    depth = torch.empty((V, *hw), dtype=torch.float32, device=dev)
    lut = torch.empty((V, hw[0] * hw[1]), dtype=torch.int32, device=dev)
    strad = torch.empty(V, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    args = (dv.data_ptr(), f3d.tensors.dtype_code(dv), len(dv), dt.data_ptr(), f3d.tensors.index_code(dt), len(dt), dw.data_ptr(), V, hw[0], hw[1], z_far)
    if list_capacity is None:
        ctx.render_mesh_lookups_dev(*args, depth.data_ptr(), lut.data_ptr(), strad.data_ptr(), s.cuda_stream)
        third = strad
    else:
        third = ctx.raster_counts_dev(*args, list_capacity, depth.data_ptr(), lut.data_ptr(), s.cuda_stream)
    s.synchronize()
    ctx.take_device_error(s.cuda_stream)
    return depth.cpu().numpy(), lut.cpu().numpy(), third.cpu().numpy() if list_capacity is None else third


@pytest.mark.parametrize('nt,V', [(nt, V) for V in (1, 2, 65) for nt in (1, 2, 63, 64, 65, 257, 5000) if V <= 2 or nt <= 257])
def test_lookups_and_face_votes_equal_the_restatement(ctx, nt, V):
    """Soup triangles plus (from 257 on) a grid mesh under the ring cameras; both images; float64 / float32 vertices and int64 / int32
    indices against one restatement (the vertices hold float32 values)."""
    verts, tris = M.scene_mesh(nt, 200 + nt)
    q, t = synth.ring_views(V)
    for hw in IMAGES:
        K, masks = R.pinhole(*hw), synth.masks(V, hw[0], hw[1], 'iid', seed=nt + V)
        views = _views(K, hw, q, t)
        depth, uv2tri, straddling = M.lookups(verts, tris, K, q, t, hw, MAX_DEPTH)
        votes = M.face_votes(uv2tri, masks, nt)
        for vx, tr in ((verts, tris), (verts.astype(np.float32), tris.astype(np.int32))):
            gd, gl, gs = ctx.render_mesh_lookups(vx, tr, views, hw[0], hw[1], MAX_DEPTH)
            assert _same(gd, depth) and _same(gl, uv2tri) and _same(gs, straddling), (hw, vx.dtype)
            assert _same(_face_votes(ctx, vx, tr, views, masks), votes), (hw, vx.dtype)
    if nt >= 63:
        assert (uv2tri >= 0).any() and votes.sum() > 0 and (nt < 257 or straddling.sum() > 0)


def _sized_mesh():
    """256 triangles for a 256 x 256 image of the identity camera (focal 128), right-angled with legs of s pixels, each at a depth of
    its own: wave 0 has the triangle that covers the whole image at lane 0 and a 128 px one at lane 63, wave 1 a mix of 16, 32, 64
    and 100 px, wave 2 nothing above 4 px (0.3 px ones among them: often no fragment at all), wave 3 every power of two up to 256."""
    rng = np.random.default_rng(7)
    size = rng.choice([0.3, 1.0, 2.0, 4.0], 256)
    size[64:128] = rng.choice([16.0, 32.0, 64.0, 100.0], 64)
    size[192:256] = 2.0 ** rng.integers(-1, 9, 64)
    size[63] = 128.0
    corner = np.stack([rng.uniform(-20, 250, 256), rng.uniform(-20, 250, 256)], 1)
    z = rng.permutation(256) / 256.0 + 1.0
    px = corner[:, None, :] + size[:, None, None] * np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]])
    px[0], z[0] = [[-10.0, -10.0], [600.0, -10.0], [-10.0, 600.0]], 5.0          # behind everything else
    px[63, :, :] = [[40.3, 30.7], [168.3, 30.7], [40.3, 158.7]]
    verts = np.concatenate([(px - 128.0) / 128.0 * z[:, None, None], np.broadcast_to(z[:, None, None], (256, 3, 1))], 2).reshape(-1, 3)
    tris = np.arange(768).reshape(256, 3)
    tris[1::2] = tris[1::2, ::-1]                                               # both windings
    return verts, tris.astype(np.int64), np.array([[128.0, 0.0, 128.0], [0.0, 128.0, 128.0], [0.0, 0.0, 1.0]]), (256, 256)


def test_triangle_sizes_and_work_tiers(ctx):
    verts, tris, K, hw = _sized_mesh()
    views = _views(K, hw, Q1, T1)
    depth, uv2tri, straddling = M.lookups(verts, tris, K, Q1, T1, hw, np.inf)
    assert (uv2tri >= 0).all() and len(np.unique(uv2tri)) > 40 and straddling[0] == 0       # the big one fills the image behind the rest
    gd, gl, gs = ctx.render_mesh_lookups(verts, tris, views, hw[0], hw[1])
    assert _same(gd, depth) and _same(gl, uv2tri) and _same(gs, straddling)
    cd, cl, counts = _dev_render(ctx, verts, tris, views, hw, np.inf, 0)
    assert _same(cd, depth) and _same(cl, uv2tri)
    assert counts['small'] > 0 and counts['medium'] > 0 and counts['huge'] > 1 and counts['overflow'] == 0, counts
    assert counts['fill_ms'] > 0 and counts['raster_ms'] > 0
    od, ol, over = _dev_render(ctx, verts, tris, views, hw, np.inf, 1)         # a list of one entry: the other huge pairs overflow
    assert over['huge'] == 1 and over['overflow'] == counts['huge'] - 1 and over['small'] == counts['small'], (counts, over)
    assert _same(od, depth) and _same(ol, uv2tri)


def test_exact_ties_and_shared_edges(ctx):
    """Fronto-parallel dyadic grid: pixel centres lie on vertices and shared edges; no interior pixel is empty and the winner is the
    lowest index among the triangles that touch the pixel, in either winding."""
    verts, tris = M.grid_mesh(6, 4, [-3.0, -2.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0])
    K = np.array([[2.0, 0.0, 6.5], [0.0, 2.0, 4.5], [0.0, 0.0, 1.0]])          # vertex (i, j) -> pixel centre (2 i + 0.5, 2 j + 0.5)
    hw = (10, 14)
    px = np.stack([2.0 * verts[:, 0] + 6.5, 2.0 * verts[:, 1] + 4.5], 1)
    for t in (tris, np.ascontiguousarray(tris[:, ::-1])):
        want = M.lowest_touching(px, t, *hw)
        assert (want[0:9, 0:13] >= 0).all() and (want[9] == -1).all()
        gd, gl, _ = ctx.render_mesh_lookups(verts, t, _views(K, hw, Q1, T1), hw[0], hw[1])
        assert _same(gl, want.reshape(1, -1).astype(np.int32)) and (gd[0][want >= 0] == 1.0).all()
        assert _same(gl, M.lookups(verts, t, K, Q1, T1, hw, np.inf)[1])


def test_dropped_input_reaches_no_output(ctx):
    verts, tris, K, good, nstraddle = M.dropped_scene()
    hw = (8, 8)
    views, masks = _views(K, hw, Q1, T1), synth.masks(1, 8, 8, 'iid')
    want = M.lookups(verts, tris, K, Q1, T1, hw, np.inf)
    got = ctx.render_mesh_lookups(verts, tris, views, 8, 8)
    assert all(_same(g, w) for g, w in zip(got, want))
    assert set(np.unique(got[1])) == {-1, good} and got[2][0] == nstraddle
    votes = _face_votes(ctx, verts, tris, views, masks, np.inf)
    assert not votes[:good].any() and votes[good].sum() > 0 and _same(votes, M.face_votes(want[1], masks, len(tris)))
    col = np.array([[0.0, 0.0, 2.0], [1.0, 1.0, 2.0], [2.0, 2.0, 2.0]])        # collinear
    assert (ctx.render_mesh_lookups(col, np.array([[0, 1, 2]]), views, 8, 8)[1] == -1).all()
    near = ctx.render_mesh_lookups(verts, tris, views, 8, 8, 1.5)              # every fragment lies beyond z_far
    assert (near[1] == -1).all() and np.isinf(near[0]).all() and near[2][0] == nstraddle
    assert all(_same(g, w) for g, w in zip(near, M.lookups(verts, tris, K, Q1, T1, hw, 1.5)))
    none = ctx.render_mesh_lookups(verts, tris[:0], views, 8, 8)               # nt == 0: empty buffers, no votes
    assert (none[1] == -1).all() and np.isinf(none[0]).all() and none[2][0] == 0
    assert _face_votes(ctx, verts, tris[:0], views, masks).shape == (0, 134)


@pytest.fixture(scope='module')
def many_views():
    hw, nt, V = (24, 40), 257, 65
    verts, tris = M.scene_mesh(nt, 321)
    q, t = synth.ring_views(V)
    K, masks = R.pinhole(*hw), synth.masks(V, hw[0], hw[1], 'iid')
    depth, uv2tri, straddling = M.lookups(verts, tris, K, q, t, hw, MAX_DEPTH)
    return hw, verts, tris, q, t, K, masks, depth, uv2tri


def test_pass_size_never_changes_a_vote(ctx, many_views):
    hw, verts, tris, q, t, K, masks, depth, uv2tri = many_views
    views = _views(K, hw, q, t)
    want = M.face_votes(uv2tri, masks, len(tris))
    pts = synth.cloud(500, seed=12)
    vis = M.visible_votes(pts, depth, K, q, t, masks, MAX_DEPTH, 0.05)
    assert want.sum() > 100 and 0 < vis.sum() < O.forward_votes(pts, K, q, t, masks, MAX_DEPTH).sum()
    for per in (0, 1, 2):
        assert _same(_face_votes(ctx, verts, tris, views, masks, MAX_DEPTH, per), want), per
        got = ctx.vote_visible_mesh(np.zeros((len(pts), 134)), pts, verts, tris, views, masks, MAX_DEPTH, 0.05, per)
        assert _same(got, vis), per


def test_two_walls_with_the_mesh_as_the_occluder():
    pts, far, K, q, t, masks, hw = R.two_walls()
    verts, tris = M.meshed_two_walls()
    cls, votes = fusion.project_vote_argmax_occluded(pts, verts, tris, K, q, t, masks, MAX_DEPTH, return_votes=True)
    assert cls.dtype == np.int64 and (cls[~far] == 86).all() and (cls[far] == 114).all()
    depth = M.lookups(verts, tris, K, q, t, hw, MAX_DEPTH)[0]
    assert _same(votes, M.visible_votes(pts, depth, K, q, t, masks, MAX_DEPTH, 0.05))


def test_watertight_where_the_splat_leaks():
    """512 x 384 at focal 240: the near wall's 2 cm grid projects to 2.4 px, so a splat of 0 leaves gaps in it (asserted), far-wall
    points show through and collect the near wall's label; the meshed walls leave no gap and mislabel nothing."""
    pts, far, _, q, t, _, _ = R.two_walls()
    hw = (384, 512)
    K = R.pinhole(*hw, 240.0)
    masks = np.empty((6, *hw), np.uint8)
    masks[:3], masks[3:] = 86, 114
    verts, tris = M.meshed_two_walls()
    splat_depth = fusion.render_lookups(pts, K, q, t, hw, MAX_DEPTH, 0)[0]
    mesh_depth = fusion.render_mesh_lookups(verts, tris, K, q, t, hw, MAX_DEPTH)[0]
    silhouette = np.isfinite(mesh_depth[0])
    assert silhouette.sum() > 10000 and np.isinf(splat_depth[0][silhouette]).mean() > 0.3          # the splat leaks
    leaky = fusion.project_vote_argmax_visible(pts, K, q, t, masks, MAX_DEPTH, splat=0, depth_tol=0.05)
    assert (leaky[far] != 114).sum() > 100
    cls = fusion.project_vote_argmax_occluded(pts, verts, tris, K, q, t, masks, MAX_DEPTH, depth_tol=0.05)
    assert (cls[~far] == 86).all() and (cls[far] == 114).all()


def test_empty_cells_hide_nothing(ctx):
    """A mesh that covers part of each image: points over uncovered pixels are visible; depth_tol = inf gives the votes of
    project_vote_argmax cell for cell; 0 and 0.05 equal the restatement."""
    hw, V = (24, 40), 4
    verts, tris = M.scene_mesh(257, 99)
    pts = synth.cloud(3000, seed=13)
    q, t = synth.ring_views(V)
    K, masks = R.pinhole(*hw), synth.masks(V, hw[0], hw[1], 'iid')
    views = _views(K, hw, q, t)
    depth = M.lookups(verts, tris, K, q, t, hw, MAX_DEPTH)[0]
    assert 0.05 < np.isinf(depth).mean() < 0.95
    full = O.forward_votes(pts, K, q, t, masks, MAX_DEPTH)
    for tol in (0.0, 0.05, np.inf):
        want = M.visible_votes(pts, depth, K, q, t, masks, MAX_DEPTH, tol)
        for cloud in (pts, pts.astype(np.float32)):
            got = ctx.vote_visible_mesh(np.zeros((len(pts), 134)), cloud, verts, tris, views, masks, MAX_DEPTH, tol)
            assert _same(got, want), tol
    assert _same(want, full) and np.array_equal(want, ctx.project_vote_argmax(pts, views, masks, 133, 0.5, None, return_votes=True)[1])
    strict = M.visible_votes(pts, depth, K, q, t, masks, MAX_DEPTH, 0.0)
    assert 0 < strict.sum() < full.sum()
    # with no triangle at all every cell is empty and every sample visible, at any tolerance
    got = ctx.vote_visible_mesh(np.zeros((len(pts), 134)), pts, verts, tris[:0], views, masks, MAX_DEPTH, 0.0)
    assert _same(got, full)
    cls, votes = fusion.project_vote_argmax_occluded(pts, verts, tris, K, q, t, masks, MAX_DEPTH, return_votes=True)
    assert _same(votes, M.visible_votes(pts, depth, K, q, t, masks, MAX_DEPTH, 0.05)) and _same(cls, O.segment(votes, 133, 0.5))


def test_label_faces(ctx):
    hw, V, nt = (24, 40), 3, 257
    verts, tris = M.scene_mesh(nt, 55)
    q, t = synth.ring_views(V)
    K = R.pinhole(*hw)
    masks = synth.masks(V, hw[0], hw[1], 'block64')
    masks[:, ::2] = 86                                                          # a triangle sees several labels, one often enough to win
    uv2tri = M.lookups(verts, tris, K, q, t, hw, MAX_DEPTH)[1]
    want = M.face_votes(uv2tri, masks, nt)
    cls, votes = meshUtils.label_faces(verts, tris, K, q, t, masks, MAX_DEPTH, return_votes=True)
    assert cls.dtype == np.int64 and _same(votes, want) and _same(cls, O.segment(want, 133, 0.5)) and (cls != 133).any()
    assert _same(meshUtils.label_faces((verts, tris), K, q, t, masks, MAX_DEPTH), cls)
    assert _same(meshUtils.label_faces(verts, tris, K, q, t, masks, MAX_DEPTH, filter_classes=[86, 5]), O.segment(want, 133, 0.5, [86, 5]))
    # composed by hand from the public pieces
    lut = fusion.render_mesh_lookups(verts, tris, K, q, t, hw, MAX_DEPTH)[1]
    by_hand = ctx.vote_uv2pt_batch(np.zeros((nt, 134)), lut, masks.reshape(V, -1), hw[0], hw[1])
    assert _same(lut, uv2tri) and _same(by_hand, votes) and _same(ctx.segment_votes(by_hand, 133, 0.5), cls)
    bad = masks.copy()
    seen = np.argwhere(uv2tri[1].reshape(hw) >= 0)[0]
    bad[1, seen[0], seen[1]] = 200                                             # on a covered pixel
    with pytest.raises(IndexError):
        M.face_votes(uv2tri, bad, nt)
    with pytest.raises(IndexError):
        meshUtils.label_faces(verts, tris, K, q, t, bad, MAX_DEPTH)
    empty = masks.copy()
    hole = np.argwhere(uv2tri[1].reshape(hw) < 0)[0]
    empty[1, hole[0], hole[1]] = 200                                           # on an empty one: never read as a label
    assert _same(meshUtils.label_faces(verts, tris, K, q, t, empty, MAX_DEPTH), cls)


def test_a_wall_of_two_triangles_fills_a_1024_view(ctx):
    """The realistic big path: both triangles go through the deferral list.  Every pixel is non-empty and within 2^-23 relative of
    the analytic ray-plane depth (a tolerance, because at this size the restatement is only evaluated per whole triangle -- it is
    compared too and may stay exact)."""
    hw = (1024, 1024)
    K = R.pinhole(*hw, 700.0)
    origin, eu, ev = [-3.0, -2.5, 2.0], [6.0, 0.0, 0.8], [0.0, 5.0, 0.5]
    verts, tris = M.grid_mesh(1, 1, origin, eu, ev)
    views = _views(K, hw, Q1, T1)
    gd, gl, counts = _dev_render(ctx, verts, tris, views, hw, np.inf, 0)
    assert counts['huge'] == 2 and counts['small'] == counts['medium'] == counts['overflow'] == 0
    z, inside = M.plane_depth(K, *hw, origin, eu, ev, 1, 1)
    assert inside.all() and (gl >= 0).all()
    rel = np.abs(gd[0].astype(np.float64) - z) / z
    assert rel.max() <= 2.0 ** -23, rel.max()
    want = M.lookups(verts, tris, K, Q1, T1, hw, np.inf)
    assert _same(gd, want[0]) and _same(gl, want[1])


def test_host_entries_equal_dev_and_repeat_bit_for_bit(ctx, many_views):
    import torch
    hw, verts, tris, q, t, K, masks, depth, uv2tri = many_views
    views = _views(K, hw, q, t)
    host = ctx.render_mesh_lookups(verts, tris, views, hw[0], hw[1], MAX_DEPTH)
    assert _same(host[0], depth) and _same(host[1], uv2tri)
    for _ in range(2):
        dev = _dev_render(ctx, verts, tris, views, hw, MAX_DEPTH)
        assert all(_same(a, b) for a, b in zip(dev, host))
    # device tensors in, device tensors out
    d = torch.device('cuda', 0)
    dv, dt, dm = torch.from_numpy(verts.astype(np.float32)).to(d), torch.from_numpy(tris.astype(np.int32)).to(d), torch.from_numpy(masks).to(d)
    out = fusion.render_mesh_lookups(dv, dt, K, q, t, hw, MAX_DEPTH)
    assert all(isinstance(x, torch.Tensor) and x.device == d for x in out) and all(_same(a.cpu().numpy(), b) for a, b in zip(out, host))
    cls, votes = meshUtils.label_faces(verts, tris, K, q, t, masks, MAX_DEPTH, return_votes=True)
    gc, gv = meshUtils.label_faces(dv, dt, K, q, t, dm, MAX_DEPTH, return_votes=True)
    assert all(isinstance(x, torch.Tensor) and x.device == d for x in (gc, gv)) and _same(gc.cpu().numpy(), cls) and _same(gv.cpu().numpy(), votes)
    pts = synth.cloud(500, seed=12)
    cls, votes = fusion.project_vote_argmax_occluded(pts, verts, tris, K, q, t, masks, MAX_DEPTH, return_votes=True)
    gc, gv = fusion.project_vote_argmax_occluded(torch.from_numpy(pts).to(d), dv, dt, K, q, t, dm, MAX_DEPTH, return_votes=True)
    assert all(isinstance(x, torch.Tensor) and x.device == d for x in (gc, gv)) and _same(gc.cpu().numpy(), cls) and _same(gv.cpu().numpy(), votes)
    assert votes.sum() > 0


def test_reserved_strict_context_allocates_nothing(many_views):
    import torch
    hw, verts, tris, q, t, K, masks, depth, uv2tri = many_views
    V, nt = len(q), len(tris)
    views = _views(K, hw, q, t)
    pts = synth.cloud(500, seed=12)
    dev = torch.device('cuda', 0)
    own = f3d.Context(0)
    s = torch.cuda.Stream(dev)
    dp, dv, dt = torch.from_numpy(pts).to(dev), torch.from_numpy(verts).to(dev), torch.from_numpy(tris).to(dev)
    dw, dm = torch.from_numpy(views).to(dev), torch.from_numpy(masks).to(dev)
    gd = torch.empty((V, *hw), dtype=torch.float32, device=dev)
    gl = torch.empty((V, hw[0] * hw[1]), dtype=torch.int32, device=dev)
    gs = torch.empty(V, dtype=torch.int64, device=dev)
    fv = torch.zeros((nt, 134), dtype=torch.float64, device=dev)
    pv = torch.zeros((len(pts), 134), dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    own.reserve_mesh_render(V, hw[0], hw[1])
    own.set_strict(True)
    before = own.alloc_count
    mesh = (dv.data_ptr(), f3d.F64, len(verts), dt.data_ptr(), f3d.I64, nt)
    own.render_mesh_lookups_dev(*mesh, dw.data_ptr(), V, hw[0], hw[1], MAX_DEPTH, gd.data_ptr(), gl.data_ptr(), gs.data_ptr(), s.cuda_stream)
    for per in (0, 2):
        own.vote_faces_dev(*mesh, dw.data_ptr(), V, dm.data_ptr(), hw[0], hw[1], MAX_DEPTH, fv.data_ptr(), 134, per, s.cuda_stream)
        own.vote_visible_mesh_dev(dp.data_ptr(), f3d.F64, len(pts), *mesh, dw.data_ptr(), V, dm.data_ptr(), hw[0], hw[1], MAX_DEPTH, 0.05,
                                  pv.data_ptr(), 134, per, s.cuda_stream)
    assert own.alloc_count == before
    own.take_device_error(s.cuda_stream)
    assert _same(gd.cpu().numpy(), depth) and _same(gl.cpu().numpy(), uv2tri)
    assert _same(fv.cpu().numpy(), 2 * M.face_votes(uv2tri, masks, nt))        # in place: two calls add up
    assert _same(pv.cpu().numpy(), 2 * M.visible_votes(pts, depth, K, q, t, masks, MAX_DEPTH, 0.05))
    with pytest.raises(MemoryError):                                             # a larger image than reserved: strict says so
        own.vote_faces_dev(*mesh, dw.data_ptr(), V, dm.data_ptr(), 4 * hw[0], 4 * hw[1], MAX_DEPTH, fv.data_ptr(), 134, 0, s.cuda_stream)
    own.close()


def test_an_index_out_of_range_writes_nothing(ctx):
    import torch
    verts, tris, K, good, _ = M.dropped_scene()
    hw = (8, 8)
    views, masks = _views(K, hw, Q1, T1), np.zeros((1, 8, 8), np.uint8)
    pts = np.array([[0.0, 0.0, 1.0]])
    for bad_index in (len(verts), -1):
        bad = tris.copy()
        bad[2, 1] = bad_index
        with pytest.raises(IndexError):
            ctx.render_mesh_lookups(verts, bad, views, 8, 8)
        votes = np.full((len(tris), 134), 7.0)
        with pytest.raises(IndexError):
            ctx.vote_faces(votes, verts, bad, views, masks)
        pvotes = np.full((1, 134), 7.0)
        with pytest.raises(IndexError):
            ctx.vote_visible_mesh(pvotes, pts, verts, bad, views, masks)
        assert (votes == 7.0).all() and (pvotes == 7.0).all()
        with pytest.raises(IndexError):
            meshUtils.label_faces(verts, bad, K, Q1, T1, masks)
        with pytest.raises(IndexError):
            fusion.project_vote_argmax_occluded(pts, verts, bad, K, Q1, T1, masks)
    # the _dev twins: a bit of their own, and the outputs keep what they held
    dev = torch.device('cuda', 0)
    own = f3d.Context(0)
    s = torch.cuda.Stream(dev)
    dv, dt, dw = torch.from_numpy(verts).to(dev), torch.from_numpy(bad).to(dev), torch.from_numpy(views).to(dev)
    dm, dp = torch.from_numpy(masks).to(dev), torch.from_numpy(pts).to(dev)
    gd = torch.full((1, 8, 8), -5.0, dtype=torch.float32, device=dev)
    gl = torch.full((1, 64), -5, dtype=torch.int32, device=dev)
    gs = torch.full((1,), -5, dtype=torch.int64, device=dev)
    fv = torch.full((len(tris), 134), 7.0, dtype=torch.float64, device=dev)
    pv = torch.full((1, 134), 7.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    mesh = (dv.data_ptr(), f3d.F64, len(verts), dt.data_ptr(), f3d.I64, len(bad))
    own.render_mesh_lookups_dev(*mesh, dw.data_ptr(), 1, 8, 8, np.inf, gd.data_ptr(), gl.data_ptr(), gs.data_ptr(), s.cuda_stream)
    own.vote_faces_dev(*mesh, dw.data_ptr(), 1, dm.data_ptr(), 8, 8, np.inf, fv.data_ptr(), 134, 0, s.cuda_stream)
    own.vote_visible_mesh_dev(dp.data_ptr(), f3d.F64, 1, *mesh, dw.data_ptr(), 1, dm.data_ptr(), 8, 8, np.inf, 0.05, pv.data_ptr(), 134, 0, s.cuda_stream)
    s.synchronize()
    assert (gd == -5.0).all() and (gl == -5).all() and (gs == -5).all() and (fv == 7.0).all() and (pv == 7.0).all()
    with pytest.raises(IndexError, match='mesh render'):
        own.take_device_error(s.cuda_stream)
    own.take_device_error(s.cuda_stream)
    good_votes = own.vote_faces(np.zeros((len(tris), 134)), verts, tris, views, masks)     # the context works on
    assert good_votes[good, 0] == 1 and good_votes.sum() == 1
    own.close()


def test_bad_arguments(ctx):
    verts, tris, K, _, _ = M.dropped_scene()
    views, masks = _views(K, (8, 8), Q1, T1), np.zeros((1, 8, 8), np.uint8)
    pts = np.array([[0.0, 0.0, 1.0]])
    with pytest.raises(ValueError):
        ctx.render_mesh_lookups(verts, tris, views, 8, 8, np.nan)
    with pytest.raises(ValueError):
        ctx.vote_faces(np.zeros((len(tris), 134)), verts, tris, views, masks, np.nan)
    with pytest.raises(ValueError):
        ctx.vote_faces(np.zeros((len(tris), 134)), verts, tris, views, masks, np.inf, -1)
    for tol, per, z_far in ((-1.0, 0, 10.0), (np.nan, 0, 10.0), (0.05, -1, 10.0), (0.05, 0, np.nan)):
        with pytest.raises(ValueError):
            ctx.vote_visible_mesh(np.zeros((1, 134)), pts, verts, tris, views, masks, z_far, tol, per)
    with pytest.raises(ValueError):
        fusion.project_vote_argmax_occluded(pts, verts, tris, K, Q1, T1, masks, depth_tol=-1)
    with pytest.raises(TypeError):
        ctx.render_mesh_lookups(verts, tris.astype(np.int16), views, 8, 8)
    with pytest.raises(ValueError):                                              # nt >= 2^31 is refused before anything is read
        ctx.render_mesh_lookups_dev(0, f3d.F64, 0, 1, f3d.I64, 1 << 31, 1, 1, 8, 8, np.inf, None, None, 1)
    assert ctx.vote_visible_mesh(np.zeros((1, 134)), pts, verts, tris, views, masks, np.inf, np.inf).sum() == 1    # the accepted ends
    assert ctx.vote_visible_mesh(np.zeros((1, 134)), pts, verts, tris, views, masks, np.inf, 0.0).sum() == 1       # in front of the mesh
