"""One case per kernel source, shared by the tests that run every family under some condition (tests/test_launch_shape_gpu.py: a capped
grid; tests/test_poison_gpu.py: poisoned scratch, staging and output memory).  The inputs are small (2500 points, 48 x 56 images): at three
blocks of 256 threads the per-point and per-pixel launches take four passes, the last one ragged, and wave-per-item kernels over a hundred.

A case is a function of a seed -> (run, want, check, rows): run(ctx) calls the public entries, want is what the reference says,
check(got, want) asserts that family's comparison, rows is the reference output whose rows must differ between two seeds (so that a
run on the other seed leaves stale values, not right ones, in every recycled buffer).  This is no test module: it holds no test."""
import functools
import math

import numpy as np

import f3d
import cvseg_ref
import door_window_ref
import face_graph_ref
import features_ref
import fused_families
import fusion_scenes
import icp_ref
import knn_ref
import lift_ref
import mesh_ref
import normals_ref
import planes_ref
import point_voting_ref
import quad_scenes
import raster_ref
import refinement_ref
import render_ref
import smooth_ref
import sort_ref
import tsdf_ref
from oracle import np_ref as O

N = 2500                                   # points: 10 blocks of 256, so 4 passes at cap 3 with 196 points in the last one
H, W = 48, 56                              # 2688 pixels: 10.5 blocks of 256
SEED, OTHER_SEED = 11, 12
Q0 = np.array([1.0, 0.0, 0.0, 0.0])


def same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    assert np.array_equal(got, want, equal_nan=got.dtype.kind == 'f'), int((got != want).sum())


def same_bits(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    assert got.tobytes() == want.tobytes()


def all_same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        same(g, w)


def csr_rows(offs, flat):
    return [tuple(flat[offs[i]:offs[i + 1]].tolist()) for i in range(len(offs) - 1)]


def cloud(rng, n=N):
    return rng.uniform(0.0, 1.0, (n, 3))


def cameras(rng, nviews):
    """nviews cameras on the plane z = -1.6 that look at the unit cube from a little off its axis -> (K, wxyz, translations)."""
    K = np.array([[0.9 * W, 0.0, W / 2.0 - 0.5], [0.0, 0.9 * W, H / 2.0 + 0.25], [0.0, 0.0, 1.0]])
    q = np.tile(Q0, (nviews, 1)) + rng.uniform(-0.03, 0.03, (nviews, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    t = np.array([0.5, 0.5, -1.6]) + rng.uniform(-0.15, 0.15, (nviews, 3))
    return K, q, t


# ---- radius searches ----------------------------------------------------------------------------------------------------------------
def radius_rows(data, queries, r):
    """KDTree(data).query_radius(queries, r) by brute force, ascending data index per query -> (offsets int64, neighbours int32)."""
    ok = knn_ref.dist2(queries, data) <= r * r
    offs = np.zeros(len(queries) + 1, np.int64)
    np.cumsum(ok.sum(axis=1), out=offs[1:])
    return offs, np.nonzero(ok)[1].astype(np.int32)


def case_graph(seed):
    """radius_graph and radius_query (bbox partials, cell sort of the grid, count and fill passes) against knn_ref's distances."""
    rng = np.random.default_rng(seed)
    pts, queries, r = cloud(rng), cloud(rng), 0.08
    want = radius_rows(pts, pts, r) + radius_rows(pts, queries, r)

    def run(ctx):
        return ctx.radius_graph(pts, r) + ctx.radius_query(pts, queries, r)

    def check(got, want):
        goffs, gnb = got[:2]
        same(goffs, want[0])
        same(np.concatenate([np.sort(gnb[goffs[i]:goffs[i + 1]]) for i in range(N)]), want[1])      # the graph's rows are in no stated order
        all_same(got[2:], want[2:])                                              # the query's rows ascend
    return run, want, check, csr_rows(want[0], want[1])


def case_knn(seed):
    """knn_query and transfer_labels against knn_ref.knn / plurality."""
    rng = np.random.default_rng(seed)
    data, queries, labels, k, r = cloud(rng), cloud(rng), rng.integers(-3, 9, N), 8, 0.12
    rows = knn_ref.knn(data, queries, k, r)[:3]
    want = rows + knn_ref.plurality(rows[0], labels, -5)

    def run(ctx):
        return ctx.knn_query(data, queries, k, r) + ctx.transfer_labels(data, labels, queries, k, r, fill=-5)
    return run, want, all_same, want[0]


def case_pointvote(seed):
    """point_vote_frames against point_voting_ref.vote: integer counts, exact."""
    rng = np.random.default_rng(seed)
    pts, ncols, r = cloud(rng), 9, 0.06
    frames = rng.uniform(0.0, 1.0, (2, H * W, 3))
    masks = rng.integers(0, ncols - 1, (2, H * W)).astype(np.uint8)
    want = point_voting_ref.vote(np.zeros((N, ncols)), pts, frames, masks, r)

    def run(ctx):
        return ctx.point_vote_frames(np.zeros((N, ncols)), pts, frames, masks, r)
    return run, want, same, want


def case_normals(seed):
    """estimate_normals: the neighbour selection exactly, the normals by normals_ref.check_against_oracle, the flip exactly."""
    rng = np.random.default_rng(seed)
    pts = cloud(rng)
    pts[:, 2] = 0.3 * pts[:, 0] + 0.05 * np.sin(7 * pts[:, 1]) + rng.normal(0, 0.002, N)        # a surface: normals are defined
    cam, r, max_nn = np.array([0.4, 0.6, 2.0]), 0.06, 16
    kept = normals_ref.neighbours(pts, r, max_nn)
    pad = np.full((N, max_nn), -1, np.int32)
    for i, k in enumerate(kept):
        pad[i, :len(k)] = k
    want = (np.array([len(k) for k in kept], np.int32), pad)

    def run(ctx):
        raw, counts, nb = ctx.estimate_normals(pts, cam, r, max_nn, orient=False, want_neighbours=True)
        return raw, counts, nb, ctx.estimate_normals(pts, cam, r, max_nn, orient=True)

    def check(got, want):
        raw, counts, nb, oriented = got
        same(counts, want[0]); same(nb, want[1])
        excluded, compared, _ = normals_ref.check_against_oracle(pts, r, max_nn, raw)
        assert compared >= N // 2, (excluded, compared)
        assert int((np.abs(normals_ref.orient_dots(pts, raw, cam)) < 1e-12).sum()) == 0
        same_bits(oriented, normals_ref.orient(pts, raw, cam))
    return run, want, check, pad


def case_smooth(seed):
    """smooth_votes (float64 and uint16, gated, two iterations) and smooth_segment against smooth_ref, exactly."""
    rng = np.random.default_rng(seed)
    pts = cloud(rng)
    offs, nbrs = smooth_ref.radius_csr(pts, 0.08)
    v = rng.integers(0, 9, (N, 70)).astype(np.float64)
    u = rng.integers(0, 65536, (N, 70)).astype(np.uint16)
    nrm = rng.standard_normal((N, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    kw = dict(normals=nrm, cos_angle=0.2, self_weight=2.0, iterations=2)
    want = (smooth_ref.smooth(v, offs, nbrs, **kw), smooth_ref.smooth(u, offs, nbrs), smooth_ref.smooth_segment(v, offs, nbrs, 69, 0.3, **kw))

    def run(ctx):
        return ctx.smooth_votes(v, offs, nbrs, **kw), ctx.smooth_votes(u, offs, nbrs), ctx.smooth_segment(v, offs, nbrs, 69, 0.3, **kw)
    return run, want, all_same, want[1]


def case_planes(seed):
    """extract_planes on the shuffled room corner (3600 points) against planes_ref.extract: labels and counts exactly."""
    pts, nrm, _ = planes_ref.room_corner(np.random.default_rng(seed))
    offs, nbrs = planes_ref.radius_csr(pts, 0.05)
    want = planes_ref.extract(pts, offs, nbrs, nrm)

    def run(ctx):
        return ctx.extract_planes(pts, offs, nbrs, nrm, math.cos(math.radians(10.0)), 0.01, 0.01, 0.01, 50, 64, len(pts) // 50)

    def check(got, want):
        labels, planes, corners, counts = got
        assert want.margin >= 1e-6, want.margin                                  # the scene is fit for an exact comparison
        same(counts, want.counts); same(labels, want.labels)
        assert planes.shape == (want.counts[0], 8) and corners.shape == (want.counts[0], 4, 3) and np.isfinite(planes).all()
    return run, want, check, want.labels


def case_mesh(seed):
    """meshUtils entries against mesh_ref (exact; cluster areas within mesh_ref.area_bound) and the face graph against face_graph_ref."""
    rng = np.random.default_rng(seed)
    verts, tris = mesh_ref.grid_mesh(40, 41, rng)
    tris = np.ascontiguousarray(tris[rng.permutation(len(tris))][:3001])
    mask = rng.random(len(verts)) < 0.1
    want = (mesh_ref.vertex_map(tris, len(verts)), mesh_ref.remove_faces(len(verts), tris, mask), mesh_ref.keep_faces(verts, tris, mask),
            mesh_ref.clusters(verts, tris), face_graph_ref.face_frames(verts, tris), face_graph_ref.graph_of(verts, tris, 30)[:2])

    def run(ctx):
        offs, nbrs, counts = ctx.mesh_face_graph(tris, len(verts), verts, math.cos(math.radians(30.0)))
        return (ctx.mesh_vertex_map(tris, len(verts)), ctx.mesh_remove_faces(tris, len(verts), mask), ctx.mesh_keep_faces(verts, tris, mask),
                ctx.mesh_triangle_clusters(verts, tris, want_tri_area=True), ctx.mesh_face_frames(verts, tris, True, True),
                (offs, nbrs[:counts[0]]))

    def check(got, want):
        for k in (0, 1, 2, 4, 5):
            all_same(got[k], want[k])
        (cl, n, ca, ta), (wcl, wn, wca, wta) = got[3], want[3]
        same(cl, wcl); same(n, wn); same(ta, wta)
        assert ca.dtype == np.float64 and ca.shape == wca.shape and np.all(np.abs(ca - wca) <= mesh_ref.area_bound(wn, wca))
    return run, want, check, want[4][0]


# ---- the entries of f3d_kernels.hip, f3d_geom.hip, f3d_groups.hip, f3d_obb.hip against the oracle -------------------------------------
def case_kernels(seed):
    """rotate, points2pixel, inside_polyhedra, segment_votes, vote_uv2pt (one frame and batched), sem_logits_to_mask, points_in_obb,
    relabel, unproject_depth (one frame, and three in one launch on sentinel-filled device memory) against oracle/np_ref.py, and
    segment_votes_lastcol against point_voting_ref.segment, exactly."""
    rng = np.random.default_rng(seed)
    pts = cloud(rng)
    K, q, t = cameras(rng, 1)
    q, t = q[0], t[0]
    pp = rng.uniform(0.3, 0.7, (3, 3))
    pn = np.array([0.5, 0.5, 0.5]) - pp + rng.normal(0, 0.3, (3, 3))                  # three planes that face the cube's centre, roughly
    votes = (rng.integers(1, 6, (N, 134)) * (rng.random((N, 134)) < 0.03)).astype(np.float64)
    luts = rng.integers(-1, N, (3, H * W)).astype(np.int32)
    masks = rng.integers(0, 133, (3, H * W)).astype(np.uint8)
    sem = rng.standard_normal((21, H, W)).astype(np.float32) * 3
    depth = rng.integers(0, 4000, (H, W)).astype(np.uint16)
    axes = np.linalg.qr(rng.standard_normal((12, 3, 3)))[0]
    centres, extents = rng.uniform(0, 1, (12, 3)), rng.uniform(0.2, 0.8, (12, 3))
    boxes = np.concatenate([centres, axes.reshape(12, 9), extents], axis=1)
    ids = rng.integers(0, 5, N).astype(np.int64)
    lastcol = votes.copy()
    lastcol[:, -1] = votes[:, :-1].sum(axis=1)                                       # the total that PointVotingSegmentation keeps there
    depths = rng.integers(0, 4000, (3, H, W)).astype(np.uint16)
    Kb, qb, tb = cameras(rng, 3)
    voted = np.zeros((N, 134))
    for f in range(3):
        O.vote_frame(voted, luts[f], masks[f])
    inside = np.stack([O.points_in_obb(pts, centres[b], axes[b], extents[b]) for b in range(12)], axis=1)
    want = (O.rotate(q, pts), O.points2pixel(pts, K, q, t), O.point_inside_polyhedra(pts, pp, pn), O.segment(votes, 133, 0.3), voted,
            O.sem_logits_to_mask(sem, 0.017, 133), inside, (inside[:, :, None] & inside[:, None, :]).any(axis=0), np.where(ids == 3, 7, ids),
            int((ids == 3).sum()), O.unproject_depth(depth, K, q, t), O.vote_frame(np.zeros((N, 134)), luts[0], masks[0]),
            point_voting_ref.segment(lastcol, 133, 0.3), np.stack([O.unproject_depth(depths[f], Kb, qb[f], tb[f]) for f in range(3)]))

    def run(ctx):
        relabelled = ids.copy()
        count = ctx.relabel(relabelled, 3, 7)
        return (ctx.rotate(pts, q), ctx.points2pixel(pts, K, q, t), ctx.inside_polyhedra(pts, pp, pn), ctx.segment_votes(votes, 133, 0.3),
                ctx.vote_uv2pt_batch(np.zeros((N, 134)), luts, masks, H, W), ctx.sem_logits_to_mask(sem, 0.017, 133),
                *ctx.points_in_obb(pts, boxes), relabelled, count, ctx.unproject_depth(depth, K, q, t),
                ctx.vote_uv2pt(np.zeros((N, 134)), luts[0], masks[0]), ctx.segment_votes_lastcol(lastcol, 133, 0.3), unproject_batch(ctx))

    def unproject_batch(ctx):
        import torch
        dd = torch.from_numpy(depths.view(np.int16)).cuda()
        out = torch.full((3, H * W, 3), float('nan'), dtype=torch.float64, device='cuda')
        torch.cuda.synchronize()
        ctx.unproject_depth_batch_dev(dd.data_ptr(), 2, 3, H, W, Kb, qb, tb, out.data_ptr(), 1000.0, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return out.cpu().numpy()

    def check(got, want):
        for k, (g, w) in enumerate(zip(got, want)):
            if k == 9:
                assert g == w
            else:
                assert np.array_equal(np.asarray(g), np.asarray(w)), k
    return run, want, check, want[0]


def unit_rows(v):
    return v / np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])[:, None]


def case_geom(seed):
    """The intersections.py primitives (lines_x_planes with as many planes as lines, 50 x 50) against their NumPy restatement below, to
    the 1e-11 of the golden comparison; flags exactly."""
    rng = np.random.default_rng(seed)
    o, d = rng.uniform(-1, 1, 3), rng.standard_normal(3)
    starts, ends = rng.uniform(-2, 2, (N, 3)), rng.uniform(-2, 2, (N, 3))
    on_ray, across = o + rng.uniform(-1, 3, (N // 2, 1)) * d, rng.standard_normal((N // 2, 3))       # every second line crosses the ray's line
    starts[::2], ends[::2] = on_ray + rng.uniform(0.1, 1, (N // 2, 1)) * across, on_ray - rng.uniform(0.1, 1, (N // 2, 1)) * across
    pp, pn = rng.uniform(-1, 1, 3), unit_rows(rng.standard_normal((1, 3)))[0]
    poly = np.array([[0.0, 0.0, 0.0], [1.0, 0.1, 0.0], [1.2, 1.0, 0.1], [0.1, 0.9, 0.0]]) + rng.uniform(-0.05, 0.05, (4, 3))
    dot = lambda a, b: (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]      # noqa: E731
    norm = lambda a: np.sqrt(dot(a, a))                                                               # noqa: E731
    # ray_x_lines
    perp, rlxl = np.cross(d, ends - starts), np.cross(starts - o, ends - starts)
    tt = dot(rlxl, perp) / dot(perp, perp)
    x = o + tt[:, None] * d
    rxl = (x, (norm(x - starts) + norm(x - ends) < norm(ends - starts) + 1e-6) & (tt > 0))
    # rays_x_plane (origins = starts, directions = ends)
    denom = dot(pn, ends)
    ok = denom < -1e-6
    tp = np.where(ok, dot(pp - starts, pn) / np.where(ok, denom, 1.0), 0.0)
    rxp = (starts + ends * tp[:, None], ok)
    # point_inside_polygon
    e, dv = np.roll(poly, -1, axis=0) - poly, starts[None, :, :] - poly[:, None, :]
    within = (dv[..., 0] * e[:, None, 0] + dv[..., 2] * e[:, None, 2]) + dv[..., 1] * e[:, None, 1] >= 0
    pip = ((within.sum(axis=0) == 0) | (within.sum(axis=0) == 4), within)
    # points_plane_projection and lines_plane_projection
    proj = lambda p: p + (dot(pp, pn) - dot(pn, p))[:, None] * pn                                     # noqa: E731
    sp, ep = proj(starts), proj(ends)
    # lines_x_planes, N == M: the segment test of pair (n, m) uses line m
    lo, le = starts[:50].copy(), ends[:50].copy()
    le[::2] = 2.0 * pp - lo[::2] + rng.uniform(-0.1, 0.1, (25, 3))                                    # every second line crosses the planes' region
    pps, pns = pp + rng.uniform(-0.2, 0.2, (50, 3)), unit_rows(rng.standard_normal((50, 3)))
    dn = norm(le - lo)
    dl = (le - lo) / dn[:, None]
    den = dot(dl[:, None, :], pns[None, :, :])
    okl = (den < -1e-6) | (den > 1e-6)
    tl = np.where(okl, dot(pps[None, :, :] - lo[:, None, :], pns[None, :, :]) / np.where(okl, den, 1.0), 0.0)
    xl = lo[:, None, :] + dl[:, None, :] * tl[..., None]
    lxp = (xl, (norm(xl - lo[None, :, :]) + norm(xl - le[None, :, :]) < dn[:, None] + 1e-6) & okl)
    want = rxl + rxp + pip + (sp, sp, ep, unit_rows(ep - sp)) + lxp

    def run(ctx):
        return (ctx.ray_x_lines(o, d, starts, ends) + ctx.rays_x_plane(pp, pn, starts, ends) + ctx.point_inside_polygon(starts, poly) +
                (ctx.points_plane_projection(starts, pp, pn),) + ctx.lines_plane_projection(starts, ends, pp, pn) +
                ctx.lines_x_planes(lo, le, pps, pns))

    def check(got, want):
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert g.shape == w.shape and g.dtype == w.dtype
            assert np.array_equal(g, w) if g.dtype == np.bool_ else np.allclose(g, w, rtol=1e-11, atol=1e-11)
    return run, want, check, sp


def grouping(ids, nids):
    """group_by_id restated: a stable argsort of the ids with everything outside [0, nids) last, and the first position of every key."""
    keys = np.where((ids >= 0) & (ids < nids), ids, nids)
    order = np.argsort(keys, kind='stable').astype(np.int32)
    return order, np.searchsorted(keys[order], np.arange(nids + 2), side='left').astype(np.int64)


def case_groups(seed):
    """group_by_id with 1000 ids (the key starts take four blocks) against the stable argsort."""
    rng = np.random.default_rng(seed)
    ids = rng.integers(-5, 1010, N).astype(np.int64)
    want = grouping(ids, 1000)

    def run(ctx):
        return ctx.group_by_id(ids, 1000)
    return run, want, all_same, want[0]


def check_extremes(ids, pts, ext, nids):
    """Every id's 26 extremes are members of it with the largest / smallest float32 dot along the 13 axes; an id without members has -1."""
    p32 = pts.astype(np.float32)
    x, y, z = p32[:, 0], p32[:, 1], p32[:, 2]
    dots = np.stack([x, y, z, x + y, x - y, x + z, x - z, y + z, y - z, (x + y) + z, (x + y) - z, (x - y) + z, (x - y) - z])
    assert ext.shape == (nids, 26) and ext.dtype == np.int32
    for k in range(nids):
        mem = np.flatnonzero(ids == k)
        if len(mem) == 0:
            assert (ext[k] == -1).all(), k
            continue
        assert (ids[ext[k]] == k).all(), k
        assert np.array_equal(dots[np.arange(13), ext[k, 0::2]], dots[:, mem].max(axis=1)), k
        assert np.array_equal(dots[np.arange(13), ext[k, 1::2]], dots[:, mem].min(axis=1)), k


def candidates_dev(ctx, pts, ids, nids, min_members):
    """group_by_id_dev -> obb_candidates_dev on sentinel-filled device outputs -> (order, starts, candidates, candidate starts)."""
    import torch
    st = torch.cuda.current_stream().cuda_stream
    x, di = torch.from_numpy(pts).cuda(), torch.from_numpy(ids).cuda()
    order, keys, cand = (torch.full((N,), -7, dtype=torch.int32, device='cuda') for _ in range(3))
    starts = torch.full((nids + 2,), -7, dtype=torch.int64, device='cuda')
    cs = torch.full((nids + 1,), -7, dtype=torch.int64, device='cuda')
    torch.cuda.synchronize()
    ctx.group_by_id_dev(di.data_ptr(), N, nids, order.data_ptr(), keys.data_ptr(), starts.data_ptr(), st)
    ctx.obb_candidates_dev(x.data_ptr(), f3d.F64, N, order.data_ptr(), keys.data_ptr(), starts.data_ptr(), nids, min_members, cand.data_ptr(),
                           cs.data_ptr(), st)
    torch.cuda.synchronize()
    return order.cpu().numpy(), starts.cpu().numpy(), cand.cpu().numpy(), cs.cpu().numpy()


MANY_IDS = 1000                            # 26 000 extremes (102 blocks) and 1001 candidate starts (4 blocks, 233 in the last)


def case_obb(seed):
    """group_by_id -> obb_extremes -> obb_hull_filter and the all-device candidate pipeline, by the properties tests/test_mirror_gpu.py
    asserts: the grouping exactly; extremes are members with the extreme float32 dot; the survivors are members, hold every hull vertex,
    and their oracle box is bit for bit the box of all members; candidates ascend inside an instance.  Twice: 6 ids of some 300 members
    (the hull filter drops points), and MANY_IDS ids of two or three members, so that the per-id kernels (the extremes' table read-out,
    the candidate starts) take several passes too; below min_members an instance keeps every member, so there the candidates are the
    grouping itself."""
    from scipy.spatial import ConvexHull
    rng = np.random.default_rng(seed)
    nids = 6
    ids = rng.integers(-1, nids + 1, N).astype(np.int64)
    ids[ids == 2] = 3                                                            # an id without members
    centres = rng.uniform(-4, 4, (nids + 1, 3))
    pts = centres[np.clip(ids, 0, nids)] + rng.normal(size=(N, 3)) * [0.4, 0.2, 0.1]
    many = rng.integers(-3, MANY_IDS + 3, N).astype(np.int64)                    # some outside [0, MANY_IDS), many ids without members
    want = grouping(ids, nids) + grouping(many, MANY_IDS)

    def run(ctx):
        order, starts = ctx.group_by_id(ids, nids)
        ext = ctx.obb_extremes(pts)
        fstart, eqs, margin = np.zeros(nids + 1, np.int32), [], np.zeros(nids)
        for k in range(nids):
            e = np.unique(ext[k][ext[k] >= 0])
            if len(e) >= 4 and k != 4:                                           # id 4 gets no facets: nothing may be dropped there
                eqs.append(ConvexHull(pts[e]).equations)
                fstart[k + 1] = len(eqs[-1])
                margin[k] = 1e-9 * (np.abs(pts[e]).max() + 1)
        np.cumsum(fstart, out=fstart)
        cand, cnt = ctx.obb_hull_filter(fstart, np.concatenate(eqs), margin)
        few = (order, starts, ext, fstart, cand, cnt) + candidates_dev(ctx, pts, ids, nids, 256)
        morder, mstarts = ctx.group_by_id(many, MANY_IDS)
        return few, (morder, mstarts, ctx.obb_extremes(pts)) + candidates_dev(ctx, pts, many, MANY_IDS, 256)

    def check(got, want):
        (order, starts, ext, fstart, cand, cnt, dorder, dstarts, dcand, dcs), (morder, mstarts, mext, mdorder, mdstarts, mdcand, mdcs) = got
        same(order, want[0]); same(starts, want[1]); same(dorder, want[0]); same(dstarts, want[1])
        same(morder, want[2]); same(mstarts, want[3]); same(mdorder, want[2]); same(mdstarts, want[3])
        check_extremes(ids, pts, ext, nids)
        check_extremes(many, pts, mext, MANY_IDS)
        assert (np.bincount(many[(many >= 0) & (many < MANY_IDS)], minlength=MANY_IDS) == 0).sum() > 10      # ids without members
        same(mdcs, want[3][:MANY_IDS + 1])                                       # every instance is below min_members: it keeps
        same(mdcand[:mdcs[-1]], want[2][:mdcs[-1]])                              #   every member, in ascending point index
        assert (ext[2] == -1).all() and dcs[0] == 0 and (np.diff(dcs) >= 0).all()
        dropped = 0
        for k in range(nids):
            mem = np.flatnonzero(ids == k)
            c = np.sort(cand[starts[k]:starts[k] + cnt[k]])
            dc = dcand[dcs[k]:dcs[k + 1]]
            assert set(c.tolist()) <= set(mem.tolist()) and np.array_equal(dc, np.sort(dc)) and set(dc.tolist()) <= set(mem.tolist()), k
            if len(mem) == 0:
                continue
            if fstart[k + 1] == fstart[k]:
                assert np.array_equal(c, mem), k
            hull = set(mem[ConvexHull(pts[mem]).vertices].tolist())
            assert hull <= set(c.tolist()) and hull <= set(dc.tolist()), k
            for some in (c, dc):
                for a, b in zip(O.obb_from_points(pts[some]), O.obb_from_points(pts[mem])):
                    assert np.array_equal(a, b), k                               # bit for bit the same box
            dropped += len(mem) - len(dc)
        assert dropped > 0                                                       # the filter removes members
    return run, want, check, np.stack([want[0], want[2]], axis=1)


# ---- z-buffers and what reads them -------------------------------------------------------------------------------------------------
def ring_scene(seed, nviews):
    from f3d import synth
    q, t = synth.ring_views(nviews, seed=5678 + seed)
    K, masks = render_ref.pinhole(H, W), synth.masks(nviews, H, W, 'iid', seed=seed)
    return K, q, t, masks, f3d.views_build(K, W, H, q, t, 10)


def case_render(seed):
    """render_lookups and vote_visible (splat 1) against render_ref, exactly."""
    from f3d import synth
    pts = synth.cloud(N, seed=seed)
    K, q, t, masks, views = ring_scene(seed, 3)
    want = render_ref.lookups(pts, K, q, t, (H, W), 10, 1) + (render_ref.visible_votes(pts, K, q, t, masks, 10, 1, 0.05),)

    def run(ctx):
        return ctx.render_lookups(pts, views, H, W, 1) + (ctx.vote_visible(np.zeros((N, 134)), pts, views, masks, 1, 0.05),)
    return run, want, all_same, want[0].reshape(3 * H, W)


def case_raster(seed):
    """render_mesh_lookups, vote_faces and vote_visible_mesh against raster_ref, exactly."""
    from f3d import synth
    verts, tris = raster_ref.scene_mesh(N, seed)
    pts = synth.cloud(N, seed=seed + 100)
    K, q, t, masks, views = ring_scene(seed, 2)
    depth, uv2tri, straddling = raster_ref.lookups(verts, tris, K, q, t, (H, W), 10)
    want = (depth, uv2tri, straddling, raster_ref.face_votes(uv2tri, masks, len(tris)),
            raster_ref.visible_votes(pts, depth, K, q, t, masks, 10, 0.05))

    def run(ctx):
        return ctx.render_mesh_lookups(verts, tris, views, H, W, 10) + (
            ctx.vote_faces(np.zeros((len(tris), 134)), verts, tris, views, masks, 10),
            ctx.vote_visible_mesh(np.zeros((N, 134)), pts, verts, tris, views, masks, 10, 0.05))
    return run, want, all_same, want[0].reshape(2 * H, W)


def case_features(seed):
    """fuse_features (a pass of 3 views: the few-views kernel; of 40: the general one) and features_finalize against features_ref,
    bit for bit."""
    from f3d import synth
    pts = synth.cloud(N, seed=seed)
    rng = np.random.default_rng(seed)
    scenes = []
    for nviews in (3, 40):
        K, q, t, _, views = ring_scene(seed, nviews)
        feats = rng.standard_normal((nviews, 12, 10, 20), dtype=np.float32)
        scenes.append((views, feats, features_ref.fuse(pts, K, q, t, feats, (H, W), 10, 1, 0.05)))
    want = tuple(x for _, _, sc in scenes for x in sc + (features_ref.finalize(*sc),))

    def run(ctx):
        out = ()
        for views, feats, _ in scenes:
            sums, counts = ctx.fuse_features(np.zeros((N, 20), np.float32), np.zeros(N, np.int32), pts, views, H, W, feats, 1, 0.05)
            out += (sums, counts, ctx.features_finalize(sums, counts))
        return out

    def check(got, want):
        assert len(got) == len(want)
        for g, w in zip(got, want):
            same_bits(g, w)
    return run, want, check, want[3]


def case_lift(seed):
    """segment_overlaps and lift_instances of segUtils.lifting against lift_ref, exactly (integer arithmetic)."""
    luts, inst = lift_ref.random_scene(seed, N, 6, H * W, 12, skew=1.0)
    want = (lift_ref.segment_overlaps(luts, inst, N, 12), lift_ref.lift_instances(luts, inst, N, 12))

    def run(ctx):
        from Fusion3DSeg.segUtils import lifting
        return lifting.segment_overlaps(luts, inst, N, 12), lifting.lift_instances(luts, inst, N, 12)

    def check(got, want):
        all_same(got[0], want[0])
        for name in ('ids', 'support', 'seen', 'seg2inst', 'inst_points'):
            same(getattr(got[1], name), getattr(want[1], name))
    return run, want, check, np.stack([want[1].ids, want[1].support, want[1].seen], axis=1)


# ---- floods ----------------------------------------------------------------------------------------------------------------------------
def blob_scene(seed):
    """A cloud with spatial class blobs over its radius graph (rows hold the point itself) and colours."""
    rng = np.random.default_rng(seed)
    pts = cloud(rng)
    offs, nbrs = smooth_ref.radius_csr(pts, 0.07)
    cell = np.floor(pts / 0.35).astype(np.int64)
    classes = ((cell[:, 0] + 2 * cell[:, 1] + 3 * cell[:, 2] + seed) % 4).astype(np.int64)
    colors = np.clip(0.5 + 0.4 * np.sin(3.0 * pts + seed) + rng.normal(0, 0.02, (N, 3)), 0.0, 1.0)      # smooth: floods grow
    return pts, colors, classes, (offs, nbrs)


def case_cc(seed):
    """CVSegmentation.instance_seperate (the ordered same-class flood) against cvseg_ref, by cvseg_ref.same_instances."""
    _, _, classes, adj = blob_scene(seed)
    want_classes = classes.copy()
    want = cvseg_ref.instance_seperate(want_classes, adj, [3, 1, 0], 5)

    def run(ctx):
        from Fusion3DSeg.segUtils.cv import CVSegmentation
        mine = classes.copy()
        return CVSegmentation(mine, adj).instance_seperate([3, 1, 0], 5), mine

    def check(got, want):
        same(got[1], want_classes)
        cvseg_ref.same_instances(got[0], (len(want[0]), want[1], want[2], want[3], list(want[4])))
        assert len(got[0][3]) > 10
    return run, want, check, want[1]


def case_color(seed):
    """CVSegmentation.color_segment (float64 and float32 colours) against cvseg_ref.color_segment, exactly."""
    _, colors, classes, adj = blob_scene(seed)
    offs, nbrs = adj
    _, ids, info, _, _ = cvseg_ref.instance_seperate(classes.copy(), adj, None, 1)
    ids = np.asarray(ids).copy()
    ids[np.isin(ids, [i for i, d in enumerate(info) if d['category_id'] == 1])] = 0           # a neutral region
    touch = np.add.reduceat((ids == 0)[nbrs].astype(np.int64), offs[:-1]) > 0
    seeds = np.random.default_rng(seed).choice(np.nonzero((ids != 0) & touch)[0], 40, replace=False)
    settings = ((np.float64, 0.3, 10), (np.float32, (0.35, 0.3, 0.4), 25))
    want = tuple(cvseg_ref.color_segment(None, adj, colors.astype(dt), ids.copy(), seeds, thr, (0,), ml) for dt, thr, ml in settings)

    def run(ctx):
        from Fusion3DSeg.segUtils.cv import CVSegmentation
        return tuple(CVSegmentation(classes.copy(), adj).color_segment(colors.astype(dt), ids.copy(), seeds, thr, (0,), ml)
                     for dt, thr, ml in settings)

    def check(got, want):
        all_same(got, want)
        assert (want[0] != ids).sum() > 50
    return run, want, check, want[0]


def case_refine(seed):
    """grow_depth, grow_color and plane_distance of segUtils.refinement against refinement_ref: the floods exactly, acceptance order
    included; the distances within refinement_ref.plane_distance_bound of the extended-precision value."""
    pts, colors, _, adj = blob_scene(seed)
    pp, nr = np.array([0.5, 0.5, 0.5]), np.array([0.3, -0.5, 0.81]) / np.linalg.norm([0.3, -0.5, 0.81])
    L = np.longdouble
    d = pts.astype(L) - pp.astype(L)
    exact = np.abs(d[:, 0] * L(nr[0]) + d[:, 1] * L(nr[1]) + d[:, 2] * L(nr[2]))
    dist = np.abs(((pts[:, 0] - pp[0]) * nr[0] + (pts[:, 1] - pp[1]) * nr[1]) + (pts[:, 2] - pp[2]) * nr[2])
    inst = np.nonzero(dist < 0.01)[0]
    want = (refinement_ref.depth_points(dist, adj, inst, 0.05, 50), refinement_ref.color_points(colors, adj, inst, 0.45, 50))

    def run(ctx):
        from Fusion3DSeg.segUtils import refinement
        return (refinement.grow_depth(dist, adj, inst, 0.05, 50, given=True), refinement.grow_color(colors, adj, inst, 0.45, 50, given=True),
                refinement.plane_distance(pts, pp, nr))

    def check(got, want):
        same(got[0], want[0]); same(got[1], want[1])
        assert len(want[0]) > 100 and len(want[1]) > 1000
        assert got[2].dtype == np.float64 and got[2].shape == (N,)
        assert (np.abs(got[2].astype(L) - exact).astype(np.float64) <= refinement_ref.plane_distance_bound(pts, pp, nr)).all()
    return run, want, check, exact.astype(np.float64)


def case_quads(seed):
    """door_window_quads for 800 instances (four blocks of them, 32 in the last) on 150 rectangles against door_window_ref.quads, exactly."""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(2, 4, 800).tolist()
    pts, ids, inst, verts, tris = quad_scenes.shuffled(quad_scenes.rect_scene(150, sizes, seed=seed, nother=N - sum(sizes)), seed)
    want = door_window_ref.quads(pts, ids, inst, verts, tris)

    def run(ctx):
        return ctx.door_window_quads(pts, ids, inst, verts, tris)

    def check(got, want):
        (q, st, tri, nrm), (wq, wst, wtri, wnrm) = got, want
        assert np.array_equal(nrm, wnrm) and np.array_equal(st, wst) and np.array_equal(tri, wtri)
        assert np.array_equal(q, wq, equal_nan=True)
        assert (st == door_window_ref.QUAD_OK).sum() >= 100
    return run, want, check, np.asarray(want[0]).reshape(800, 12)


# ---- frame fusion: the patch kernels and the per-frame steps --------------------------------------------------------------------------
def fusion_case(params):
    def case(seed):
        K, q, t, frames = fusion_scenes.curved_capture(H, W, 4, seed, quirks=False)
        want = fusion_scenes.run_fuse(K, W, H, q, t, fusion_scenes.copy_frames(frames), params, 5, 'oracle')

        def run(ctx):
            return fusion_scenes.run_fuse(K, W, H, q, t, fusion_scenes.copy_frames(frames), params, 5, 'host')
        return run, want, fusion_scenes.assert_same_fuse, want[0][0]
    return case


case_patch = fusion_case((0.05, 10, 6, 10, 1))
case_patch.__doc__ = """Fusion.fuse with a stride (patch matching and patch_downsample's seeds) against the oracle's fuse, bit for bit."""
case_fusion = fusion_case((0.03, 15, None, 10, 1))
case_fusion.__doc__ = """Fusion.fuse without a stride (the per-frame hit, update, lookup and new-seed steps) against the oracle, bit for bit."""


# ---- the cell sort and the fused vote -----------------------------------------------------------------------------------------------
def case_sort(seed):
    """cloud_sort_cells_dev (sentinel-filled outputs) against the stable argsort of sort_ref's keys; the sorted copy is x[perm]."""
    from f3d import synth
    x = synth.cloud(N, seed=seed)
    want = sort_ref.expected_perm(x)

    def run(ctx):
        import torch
        xd = torch.tensor(x).cuda()
        perm = torch.full((N,), -1, dtype=torch.int32, device='cuda')
        xs = torch.full_like(xd, float('nan'))
        torch.cuda.synchronize()
        ctx.cloud_sort_cells_dev(xd.data_ptr(), f3d.F64, N, xs.data_ptr(), perm.data_ptr())
        ctx.synchronize()
        return perm.cpu().numpy(), xs.cpu().numpy()

    def check(got, want):
        same(got[0], want)
        same_bits(got[1], x[want])
    return run, want, check, want


def case_fuse(seed):
    """project_vote_argmax (labels and the vote matrix, with and without a filter; the cell sort's riders code the masks) on the base
    cameras of fused_families against the oracle, bit for bit; the fast projection's audit finds no contradiction."""
    from f3d import synth
    _, K, q, t, max_depth, w, h, _ = fused_families.family('base')
    pts = synth.cloud(N, seed=seed)
    masks = synth.masks(len(t), h, w, 'iid', seed=seed)
    views = f3d.views_build(K, w, h, q, t, max_depth)
    with np.errstate(all='ignore'):
        votes = O.forward_votes(pts, K, q, t, masks, max_depth, ncols=134)
    settings = ((0.5, None), (0.0, [86, 114, 115]))
    want = (votes,) + tuple(O.segment(votes, 133, thr, flt) for thr, flt in settings)

    def run(ctx):
        out = [ctx.project_vote_argmax(pts, views, masks, 133, thr, flt, return_votes=True) for thr, flt in settings]
        plain = [ctx.project_vote_argmax(pts, views, masks, 133, thr, flt) for thr, flt in settings]
        return out, plain, ctx.fastpath_audit(pts, views, w, h)

    def check(got, want):
        out, plain, audit = got
        for (labels, votes), again, w_labels in zip(out, plain, want[1:]):
            assert votes.dtype == np.uint16 and np.array_equal(votes, want[0])
            assert np.array_equal(labels, w_labels) and np.array_equal(again, w_labels)
        audit = np.asarray(audit).reshape(-1)
        assert audit[0] > 0 and audit[2] == 0 and audit[3] == 0
    return run, want, check, want[0]


# ---- registration and reconstruction ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def icp_model():
    s = icp_ref.icp_scene()
    for a in s.values():
        a.setflags(write=False)
    return s


def case_icp(seed):
    """icp_sums and icp of a 64 x 72 frame (18 chunks of pixels) against the model maps of icp_ref.icp_scene, and tsdf_raycast of its
    volume, against icp_ref: every output bit for bit."""
    s = icp_model()
    rng = np.random.default_rng(seed)
    hm, wm = s['vertex'].shape[0] // icp_ref.W, icp_ref.W
    assert hm == icp_ref.H
    h, w, max_depth = 64, 72, 4.0
    K = tsdf_ref.intrinsics(h, w)
    depth = tsdf_ref.cast_depth(K, s['q'][1], s['t'][1], h, w)
    depth.reshape(-1)[3::41] = 0.0
    depth.reshape(-1)[11::67] = np.nan
    q, t = icp_ref.moved(s['q'][1], s['t'][1], (0.2, 0.9, -0.3), 0.7, rng.uniform(-0.01, 0.01, 3))
    model = (s['vertex'], s['normal'], hm, wm, s['K'], s['q'][0], s['t'][0], 0.1)
    qr, tr = icp_ref.moved(s['q'][0], s['t'][0], (0.5, -0.7, 0.4), 2.0, rng.uniform(-0.05, 0.05, 3))
    nsteps = int(np.floor(max_depth / icp_ref.VS)) + 1
    ray = (icp_ref.LO, icp_ref.VS, 1.0, s['K'], qr, tr, hm + 3, wm - 5, 0.0, icp_ref.VS, nsteps)
    want = (icp_ref.icp_sums(depth, K, q, t, 1.0, max_depth, *model), icp_ref.icp(depth, K, q, t, 1.0, max_depth, *model, 4, 100),
            icp_ref.raycast(s['tsdf'], s['weight'], *ray))

    def run(ctx):
        view = f3d.views_build(s['K'], wm, hm, s['q'][0][None], s['t'][0][None], max_depth)
        args = (depth, K, q, t, s['vertex'], s['normal'], hm, wm, view, 0.1, 1.0, max_depth)
        return ctx.icp_sums(*args), ctx.icp(*args, 4, 100), ctx.tsdf_raycast(np.array(s['tsdf']), np.array(s['weight']), *ray)

    def check(got, want):
        same_bits(got[0], want[0])
        assert got[1][2] == want[1][2] == icp_ref.OK
        same_bits(got[1][0], want[1][0]); same_bits(got[1][1], want[1][1])
        for g, x in zip(got[2], want[2]):
            same_bits(g, x)
        assert want[0][28] > 500 and (want[2][2] > 0).sum() > 100
    return run, want, check, want[2][0]


def case_tsdf(seed):
    """tsdf_integrate and tsdf_extract against tsdf_ref: tsdf, weight and vertices bit for bit, triangles exactly."""
    rng = np.random.default_rng(seed)
    dims, vs, lo, trunc, max_depth = (37, 29, 21), 0.05, np.array([-0.9, -0.7, 0.55]), 0.2, 4.0
    eyes = np.array([(0.0, 0.0, 0.0), (-0.5, 0.3, 0.8), (0.6, -0.4, 0.3)]) + rng.uniform(-0.05, 0.05, (3, 3))
    K, q, t, depths = tsdf_ref.scene([tuple(e) for e in eyes], [(0.0, 0.0, 1.0), (0.05, 0.0, 1.2), (0.0, 0.0, 1.1)], H, W)
    depths[0, 5:9, 7:12] = 0.0
    depths[1, 11:14, 20:26] = np.inf
    z = np.zeros(dims[::-1], np.float32)
    tsdf, weight = tsdf_ref.integrate(z, z, lo, vs, trunc, 64, depths, K, q, t, 1.0, max_depth)
    want = (tsdf, weight) + tuple(tsdf_ref.extract(tsdf, weight, lo, vs, 1.0))

    def run(ctx):
        got_t, got_w = np.zeros(dims[::-1], np.float32), np.zeros(dims[::-1], np.float32)
        ctx.tsdf_integrate(got_t, got_w, lo, vs, trunc, 64, depths, f3d.views_build(K, W, H, q, t, max_depth), 1.0, max_depth)
        return (got_t, got_w) + tuple(ctx.tsdf_extract(got_t.copy(), got_w.copy(), lo, vs, 1.0))

    def check(got, want):
        same_bits(got[0], want[0]); same_bits(got[1], want[1]); same_bits(got[2], want[2])
        assert got[3].dtype == np.int32 and np.array_equal(got[3], want[3]) and len(want[3]) > 100
    return run, want, check, want[0].reshape(-1, dims[0])


CASES = {
    'f3d_cc.hip': case_cc,
    'f3d_color.hip': case_color,
    'f3d_features.hip': case_features,
    'f3d_fuse.hip': case_fuse,
    'f3d_fusion.hip': case_fusion,
    'f3d_geom.hip': case_geom,
    'f3d_graph.hip': case_graph,
    'f3d_groups.hip': case_groups,
    'f3d_icp.hip': case_icp,
    'f3d_kernels.hip': case_kernels,
    'f3d_knn.hip': case_knn,
    'f3d_lift.hip': case_lift,
    'f3d_mesh.hip': case_mesh,
    'f3d_normals.hip': case_normals,
    'f3d_obb.hip': case_obb,
    'f3d_patch.hip': case_patch,
    'f3d_planes.hip': case_planes,
    'f3d_pointvote.hip': case_pointvote,
    'f3d_quads.hip': case_quads,
    'f3d_raster.hip': case_raster,
    'f3d_refine.hip': case_refine,
    'f3d_render.hip': case_render,
    'f3d_smooth.hip': case_smooth,
    'f3d_sort.hip': case_sort,
    'f3d_tsdf.hip': case_tsdf,
}


@functools.lru_cache(maxsize=None)
def prepared(name, seed):
    """(run, want, check, rows) of a case and seed: the input and its reference are built once and shared by both caps."""
    return CASES[name](seed)


def rows_that_differ(a, b):
    """How many rows of two reference outputs of the same kind differ (lists of tuples for CSR rows); rows beyond the shorter one count."""
    if isinstance(a, list):
        return sum(x != y for x, y in zip(a, b)) + abs(len(a) - len(b))
    a, b = np.asarray(a), np.asarray(b)
    a, b = a.reshape(len(a), -1), b.reshape(len(b), -1)
    m = min(len(a), len(b))
    return int((a[:m] != b[:m]).any(axis=1).sum()) + abs(len(a) - len(b)) if a.shape[1] == b.shape[1] else max(len(a), len(b))
