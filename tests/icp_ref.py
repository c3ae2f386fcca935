"""NumPy restatement of the registration contract of include/f3d.h (f3d_tsdf_raycast, f3d_icp_sums, f3d_icp) and of
segUtils/registration.py track_frames, operation for operation: float64 arithmetic, every product, sum, division and sqrt as the header
writes it.  No sample skipping, no launch shape: what the library returns must equal this bit for bit.
"""
import numpy as np

from oracle import np_ref as O
import tsdf_ref as T

CHUNK, NSUMS, PIVOT_EPS = 256, 29, 1e-10
OK, LOST = 0, 1


def normalise(q):
    q = np.asarray(q, np.float64)
    return q / np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


# ------------------------------------------------------------------------------------------------ raycast
def sample(tsdf, weight, lo, vs, min_weight, P):
    """F(P) of the header for the rows of P [n, 3] -> (valid bool [n], F float64 [n]; F is 0 where invalid)."""
    nz, ny, nx = tsdf.shape
    n = (nx, ny, nz)
    S, W = tsdf.reshape(-1), weight.reshape(-1)
    with np.errstate(all='ignore'):
        g = [(P[:, a] - lo[a]) / vs - 0.5 for a in range(3)]
        fl = [np.floor(x) for x in g]
        valid = np.ones(len(P), bool)
        for a in range(3):
            valid &= (fl[a] >= 0) & (fl[a] <= n[a] - 2)
        i = [np.where(valid, x, 0).astype(np.int64) for x in fl]
        f = [np.where(valid, g[a] - i[a].astype(np.float64), 0.0) for a in range(3)]
        at = (i[2] * ny + i[1]) * nx + i[0]
        at = np.where(valid, at, 0)
        if min(n) < 2:
            return np.zeros(len(P), bool), np.zeros(len(P))
        for c in range(8):
            o = (c & 1) + ((c >> 1) & 1) * nx + (c >> 2) * nx * ny
            valid &= W[at + o] >= np.float32(min_weight)
        c_jk = []
        for c in range(4):                                              # c = j + 2 k
            o = (c & 1) * nx + (c >> 1) * nx * ny
            t0, t1 = S[at + o].astype(np.float64), S[at + o + 1].astype(np.float64)
            c_jk.append(t0 + f[0] * (t1 - t0))
        c0 = c_jk[0] + f[1] * (c_jk[1] - c_jk[0])
        c1 = c_jk[2] + f[1] * (c_jk[3] - c_jk[2])
        F = c0 + f[2] * (c1 - c0)
    return valid, np.where(valid, F, 0.0)


def raycast(tsdf, weight, lo, vs, min_weight, K, q, t, h, w, near, step, nsteps):
    """-> (vertex float64 [h*w, 3], normal float64 [h*w, 3], depth float64 [h*w]) of the header's raycast."""
    K, lo, t = np.asarray(K, np.float64), np.asarray(lo, np.float64), np.asarray(t, np.float64)
    fx, cx, fy, cy = K[0, 0], K[0, 2], K[1, 1], K[1, 2]
    vv, uu = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing='ij')
    dc = np.stack([((uu.reshape(-1) + 0.5) - cx) / fx, ((vv.reshape(-1) + 0.5) - cy) / fy, np.ones(h * w)], axis=1)
    dw = O.rotate(normalise(q), dc)
    n = h * w
    point = lambda s: t[None, :] + s[:, None] * dw                      # noqa: E731
    done, hit = np.zeros(n, bool), np.zeros(n, bool)
    prev_ok, F_prev, s_star = np.zeros(n, bool), np.zeros(n), np.zeros(n)
    with np.errstate(all='ignore'):
        for k in range(nsteps):
            s = np.full(n, near + np.float64(k) * step)
            valid, F = sample(tsdf, weight, lo, vs, min_weight, point(s))
            ends = ~done & valid & (F < 0)
            hits = ends & prev_ok
            s_prev = near + np.float64(k - 1) * step
            s_star = np.where(hits, s_prev + step * (F_prev / (F_prev - F)), s_star)
            hit |= hits
            done |= ends
            prev_ok, F_prev = valid & (F >= 0), F
            if done.all():
                break
        V = point(s_star)
        G = []
        for a in range(3):
            e = np.zeros(3)
            e[a] = vs
            vp, Fp = sample(tsdf, weight, lo, vs, min_weight, np.where(e[None, :] != 0, V + e[None, :], V))
            vm, Fm = sample(tsdf, weight, lo, vs, min_weight, np.where(e[None, :] != 0, V - e[None, :], V))
            hit &= vp & vm
            G.append(Fp - Fm)
        G = np.stack(G, axis=1)
        length = np.sqrt((G[:, 0] * G[:, 0] + G[:, 1] * G[:, 1]) + G[:, 2] * G[:, 2])
        hit &= (length > 0) & np.isfinite(length)
        normal = np.where(hit[:, None], G / length[:, None], np.nan)
    return np.where(hit[:, None], V, np.nan), normal, np.where(hit, s_star, 0.0)


# ------------------------------------------------------------------------------------------------ ICP
def wave_sum(x):
    """planes_ref.wave_sum along axis 0 of x [n, ...]: lane l adds the items l, l + 64, .. left to right from 0.0, then the 64 lane
    sums meet in an xor butterfly 32, 16, .., 1."""
    x = np.asarray(x, np.float64)
    acc = np.zeros((64,) + x.shape[1:])
    for r in range(0, len(x), 64):
        part = x[r:r + 64]
        acc[:len(part)] = acc[:len(part)] + part
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[lane ^ off]
    return acc[0]


def shaped_sums(terms):
    """terms [npix, 29] -> the 29 totals: chunks of CHUNK pixels, each a wave_sum; the chunk sums summed the same way."""
    return wave_sum(np.stack([wave_sum(terms[k:k + CHUNK]) for k in range(0, len(terms), CHUNK)]))


def icp_terms(depth, K, q, t, depth_scale, max_depth, model_vertex, model_normal, hm, wm, model_K, model_q, model_t, max_dist):
    """The terms [h*w, 29] of every source pixel at the pose (q, t); zeros where a step of the header fails."""
    depth = np.asarray(depth)
    h, w = depth.shape
    K, mK, t, mt = np.asarray(K, np.float64), np.asarray(model_K, np.float64), np.asarray(t, np.float64), np.asarray(model_t, np.float64)
    fx, cx, fy, cy = K[0, 0], K[0, 2], K[1, 1], K[1, 2]
    MV, MN = np.asarray(model_vertex, np.float64).reshape(-1, 3), np.asarray(model_normal, np.float64).reshape(-1, 3)
    with np.errstate(all='ignore'):
        d = depth.reshape(-1).astype(np.float64) / np.float64(depth_scale)
        ok = (d > 0) & (d <= max_depth)
        d = np.where(ok, d, 1.0)
        vv, uu = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing='ij')
        c = np.stack([((uu.reshape(-1) + 0.5) - cx) * (d / fx), ((vv.reshape(-1) + 0.5) - cy) * (d / fy), d], axis=1)
        pr = O.rotate(normalise(q), c)
        p = pr + t[None, :]
        cam = O.rotate(O.quat_inverse(model_q), p - mt[None, :])
        h0 = (mK[0, 0] * cam[:, 0] + mK[0, 1] * cam[:, 1]) + mK[0, 2] * cam[:, 2]
        h1 = (mK[1, 0] * cam[:, 0] + mK[1, 1] * cam[:, 1]) + mK[1, 2] * cam[:, 2]
        h2 = (mK[2, 0] * cam[:, 0] + mK[2, 1] * cam[:, 1]) + mK[2, 2] * cam[:, 2]
        ok &= h2 > 0
        x, y = h0 / h2, h1 / h2
        ok &= (x >= 0) & (x < wm) & (y >= 0) & (y < hm)
        um, vm = np.where(ok, np.floor(x), 0).astype(np.int64), np.where(ok, np.floor(y), 0).astype(np.int64)
        V, N = MV[vm * wm + um], MN[vm * wm + um]
        ok &= np.isfinite(V).all(axis=1) & np.isfinite(N).all(axis=1)
        e = p - V
        ok &= (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2] <= max_dist * max_dist
        r = dot3(N, e)
        J = [pr[:, 1] * N[:, 2] - pr[:, 2] * N[:, 1], pr[:, 2] * N[:, 0] - pr[:, 0] * N[:, 2], pr[:, 0] * N[:, 1] - pr[:, 1] * N[:, 0],
             N[:, 0], N[:, 1], N[:, 2]]
        cols = [J[a] * J[b] for a in range(6) for b in range(a, 6)] + [J[a] * r for a in range(6)] + [r * r, np.ones(h * w)]
        return np.where(ok[:, None], np.stack(cols, axis=1), 0.0)


def icp_sums(depth, K, q, t, depth_scale, max_depth, model_vertex, model_normal, hm, wm, model_K, model_q, model_t, max_dist):
    return shaped_sums(icp_terms(depth, K, q, t, depth_scale, max_depth, model_vertex, model_normal, hm, wm, model_K, model_q, model_t, max_dist))


def solve(tot, min_pairs):
    """x = (omega, v) of the header's Cholesky solve, or None when the round is lost."""
    if tot[28] < min_pairs:
        return None
    A, j = np.zeros((6, 6)), 0
    for a in range(6):
        for c in range(a, 6):
            A[a, c] = A[c, a] = tot[j]
            j += 1
    b = -tot[21:27]
    maxd = A[0, 0]
    for a in range(1, 6):
        if A[a, a] > maxd:
            maxd = A[a, a]
    floor_ = PIVOT_EPS * maxd
    L = np.zeros((6, 6))
    with np.errstate(all='ignore'):
        for j in range(6):
            s = A[j, j]
            for k in range(j):
                s = s - L[j, k] * L[j, k]
            if not (np.isfinite(s) and s > floor_):
                return None
            L[j, j] = np.sqrt(s)
            for i in range(j + 1, 6):
                e = A[i, j]
                for k in range(j):
                    e = e - L[i, k] * L[j, k]
                L[i, j] = e / L[j, j]
        y, x = np.zeros(6), np.zeros(6)
        for i in range(6):
            s = b[i]
            for k in range(i):
                s = s - L[i, k] * y[k]
            y[i] = s / L[i, i]
        for i in range(5, -1, -1):
            s = y[i]
            for k in range(i + 1, 6):
                s = s - L[k, i] * x[k]
            x[i] = s / L[i, i]
    return x


def update(q, t, x):
    """(q', t') of the header's update."""
    b = normalise(q)
    a = np.array([1.0, x[0] / 2.0, x[1] / 2.0, x[2] / 2.0])
    qp = np.array([((a[0] * b[0] - a[1] * b[1]) - a[2] * b[2]) - a[3] * b[3],
                   ((a[0] * b[1] + a[1] * b[0]) + a[2] * b[3]) - a[3] * b[2],
                   ((a[0] * b[2] - a[1] * b[3]) + a[2] * b[0]) + a[3] * b[1],
                   ((a[0] * b[3] + a[1] * b[2]) - a[2] * b[1]) + a[3] * b[0]])
    return normalise(qp), np.asarray(t, np.float64) + x[3:6]


def icp(depth, K, q, t, depth_scale, max_depth, model_vertex, model_normal, hm, wm, model_K, model_q, model_t, max_dist, iterations, min_pairs):
    """-> (pose float64 [7], stats float64 [iterations, 3], status) of the header's f3d_icp."""
    q, t = np.asarray(q, np.float64).copy(), np.asarray(t, np.float64).copy()
    stats, lost = np.zeros((iterations, 3)), False
    for it in range(iterations):
        if lost:
            stats[it] = (0.0, 0.0, LOST)
            continue
        tot = icp_sums(depth, K, q, t, depth_scale, max_depth, model_vertex, model_normal, hm, wm, model_K, model_q, model_t, max_dist)
        x = solve(tot, min_pairs)
        stats[it] = (tot[28], tot[27], OK if x is not None else LOST)
        if x is None:
            lost = True
            continue
        q, t = update(q, t, x)
    return np.concatenate([q, t]), stats, LOST if lost else OK


# ------------------------------------------------------------------------------------------------ track_frames
def track_frames(tsdf, weight, lo, vs, trunc, max_weight, depths, K, wxyzs, translations, depth_scale=1.0, max_depth=10.0, max_dist=0.1,
                 iterations=10, min_pairs=100, min_weight=1.0, integrate=True):
    """-> (wxyzs [F, 4], translations [F, 3], status int32 [F], tsdf, weight) of registration.track_frames on a volume state."""
    depths = np.asarray(depths)
    F, h, w = depths.shape
    qs, ts = np.asarray(wxyzs, np.float64).copy(), np.asarray(translations, np.float64).copy()
    status = np.zeros(F, np.int32)
    nsteps = int(np.floor((max_depth - 0.0) / vs)) + 1
    for f in range(F):
        empty = not weight.any()
        if not empty:
            vertex, normal, _ = raycast(tsdf, weight, lo, vs, min_weight, K, qs[f], ts[f], h, w, 0.0, vs, nsteps)
            pose, _, status[f] = icp(depths[f], K, qs[f], ts[f], depth_scale, max_depth, vertex, normal, h, w, K, qs[f], ts[f], max_dist, iterations,
                                     min_pairs)
            if status[f] == OK:
                qs[f], ts[f] = pose[:4], pose[4:]
        if empty or integrate:
            tsdf, weight = T.integrate(tsdf, weight, lo, vs, trunc, max_weight, depths[f:f + 1], K, qs[f:f + 1], ts[f:f + 1], depth_scale, max_depth)
    return qs, ts, status, tsdf, weight


# ------------------------------------------------------------------------------------------------ scenes and pose errors of the tests
# The sphere-and-wall scene of tsdf_ref from the six poses of test_reconstructed_mesh_feeds_the_mesh_route, in a 37 x 29 x 21 volume
# placed so that the wall (z = 1.55) and a voxel on either side of it are valid sample positions: a raycast needs them for its normals.
H, W, MAX_DEPTH = 40, 48, 4.0
DIMS, VS, LO, TRUNC = (37, 29, 21), 0.05, np.array([-0.9, -0.7, 0.6]), 0.2
EYES = [(0.0, 0.0, 0.0), (-0.5, 0.1, 0.1), (0.5, -0.1, 0.1), (0.0, 0.45, 0.15), (0.0, -0.45, 0.15), (0.3, 0.3, 0.0)]
AXIS_N = np.array([0.0, 0.0, 1.0])                                      # the scene's symmetry axis: through the sphere's centre, along the wall's normal


def quat_mul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])


def moved(q, t, axis, degrees, shift):
    """The camera->world pose (q, t) rotated by `degrees` about `axis` (about the camera centre) and moved by `shift`; np trigonometry is
    fine here: only the contract avoids it."""
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    half = np.radians(degrees) / 2
    return quat_mul(np.concatenate([[np.cos(half)], np.sin(half) * axis]), np.asarray(q, np.float64)), np.asarray(t, np.float64) + shift


def rotation_matrix(q):
    return O.rotate(normalise(q), np.eye(3)).T


def rotation_angle(qa, qb):
    qa, qb = normalise(qa), normalise(qb)
    return 2 * np.arccos(min(1.0, abs(float(np.dot(qa, qb)))))


def scene_error(q, t, q_true, t_true, centre=T.SPHERE_C, axis=AXIS_N):
    """The pose error a depth camera can observe in this scene: (metres between the sphere's centre as the two cameras see it, radians
    between the wall's normal as they see it).  The scene maps onto itself under every rotation about the line through the sphere's
    centre along the wall's normal, so that angle is not observable from depth and is left out: the five numbers compared here are the
    other five degrees of freedom of the pose.  centre, axis: where the pose (q, t) believes the scene to be (the model's frame)."""
    Ra, Rb = rotation_matrix(q), rotation_matrix(q_true)
    seen, truth = Ra.T @ (np.asarray(centre) - t), Rb.T @ (T.SPHERE_C - t_true)
    return float(np.linalg.norm(seen - truth)), float(np.arccos(np.clip((Ra.T @ np.asarray(axis)) @ (Rb.T @ AXIS_N), -1.0, 1.0)))


def icp_scene():
    """K, the true poses and the depth frames of the scene; the state of the volume after integrating them at the true poses; the model
    maps ray-cast from the true pose of frame 0; the start pose of the ICP tests: frame 0's moved by 2 cm and rotated by 1 degree about
    an oblique axis."""
    K, q, t, depths = T.scene(EYES, [(0.05, -0.02, 1.0)] * 6, H, W)
    z = np.zeros(DIMS[::-1], np.float32)
    tsdf, weight = T.integrate(z, z, LO, VS, TRUNC, 64, depths, K, q, t, 1.0, MAX_DEPTH)
    vertex, normal, depth = raycast(tsdf, weight, LO, VS, 1.0, K, q[0], t[0], H, W, 0.0, VS, int(np.floor(MAX_DEPTH / VS)) + 1)
    shift = np.array([0.012, -0.011, 0.0115])
    q0, t0 = moved(q[0], t[0], (0.5, -0.7, 0.4), 1.0, shift * (0.02 / np.linalg.norm(shift)))
    return dict(K=K, q=q, t=t, depths=depths, tsdf=tsdf, weight=weight, vertex=vertex, normal=normal, depth=depth, q0=q0, t0=t0)


def tracking_priors(q, t, seed=5):
    """Every pose moved by 1 - 2 cm and rotated by 0.3 - 0.9 degrees, in directions drawn from `seed`."""
    rng = np.random.default_rng(seed)
    pq, pt = q.copy(), t.copy()
    for f in range(len(q)):
        axis, angle = rng.normal(size=3), rng.uniform(0.3, 0.9)
        shift = rng.normal(size=3)
        pq[f], pt[f] = moved(q[f], t[f], axis, angle, shift * (rng.uniform(0.01, 0.02) / np.linalg.norm(shift)))
    return pq, pt


def tracking_errors(pq, pt, q, t, q_true, t_true):
    """Mean scene_error of the poses (q, t) of frames 1.. against the true ones.  The model lives in the frame the first pose (pq[0],
    pt[0]: frame 0 is integrated where its prior puts it) gives it, so that is where the poses believe the scene to be."""
    E = rotation_matrix(pq[0]) @ rotation_matrix(q_true[0]).T
    centre, axis = E @ (T.SPHERE_C - t_true[0]) + pt[0], E @ AXIS_N
    errs = np.array([scene_error(q[f], t[f], q_true[f], t_true[f], centre, axis) for f in range(1, len(q))])
    return errs.mean(axis=0)


# ------------------------------------------------------------------------------------------------ scenes of the sample-range tests
# A sphere in a 23 x 19 x 17 volume, every weight 1, its radius (10.4 voxels) above the half extent on y (9.5) and z (8.5): the surface
# leaves through four faces, so rays meet it right behind the first valid sample.  The image is 15 x 17 with the principal point on a
# pixel centre: the centre column and the centre row have a camera-frame direction component of exactly 0.
RAY_DIMS, RAY_LO, RAY_H, RAY_W = (23, 19, 17), np.array([-0.6, -0.5, 0.5]), 15, 17
RAY_K = np.array([[16.0, 0.0, 8.5], [0.0, 16.0, 7.5], [0.0, 0.0, 1.0]])
RAY_SHIFT = np.array([1000.0, -2000.0, 500.0])
_R = np.sqrt(0.5)
AXIS_CAMERAS = {'+z': ([1.0, 0.0, 0.0, 0.0], 2), '-z': ([0.0, 1.0, 0.0, 0.0], 2), '+x': ([_R, 0.0, _R, 0.0], 0), '-x': ([_R, 0.0, -_R, 0.0], 0),
                '+y': ([_R, -_R, 0.0, 0.0], 1), '-y': ([_R, _R, 0.0, 0.0], 1)}      # looking along: (quaternion, axis)


def ray_volume(vs=0.05):
    """(tsdf, weight, lo, vs, centre): everything but lo scales with the voxel."""
    centre = RAY_LO + np.array(RAY_DIMS) * vs / 2 + np.array([0.013, -0.021, 0.007]) * (vs / 0.05)
    tsdf, weight = T.sphere_state(RAY_DIMS, RAY_LO, vs, centre, 10.4 * vs, 4 * vs)
    return tsdf, weight, RAY_LO, vs, centre


def ray_cases():
    """name -> dict(vs, lo, K, q, t, near, step, nsteps): the cameras and marches of the sample-range tests.  Lengths are in voxels of
    the case's volume: every camera but the distant ones stands 30 voxels from the sphere's centre and marches 80 voxels."""
    cases = {}

    def add(name, q, back, vs=0.05, K=RAY_K, near=0.0, step=1.0, nsteps=None, shift=None, sideways=(0.0, 0.0, 0.0)):
        centre = ray_volume(vs)[4]
        t = centre - np.asarray(back, np.float64) * vs + np.asarray(sideways, np.float64) * vs
        lo = RAY_LO
        if shift is not None:
            lo, t = lo + shift, t + shift
        nsteps = nsteps if nsteps is not None else int(np.floor(80.0 / step)) + 1
        cases[name] = dict(vs=vs, lo=lo, K=K, q=np.array(q, np.float64), t=t, near=near * vs, step=step * vs, nsteps=nsteps)

    def axis(name, distance=30.0):
        q, a = AXIS_CAMERAS[name]
        back = np.zeros(3)
        back[a] = distance if name[0] == '+' else -distance
        return q, back

    for name in AXIS_CAMERAS:
        add('axis' + name, *axis(name))
    add('fine-voxels', *axis('+x'), vs=1.0 / 64)
    # the centre column (dw_x == 0) runs beside the volume, three voxels outside it; the columns right of it still reach the sphere
    add('beside', *axis('+z'), sideways=(-(RAY_DIMS[0] / 2 + 0.26) - 3.0, 0.0, 0.0))
    # the centre row (dw_y == 0) runs inside the volume, a quarter voxel above the last valid sample position lo + (ny - 0.5) vs
    add('just-outside', *axis('+z'), sideways=(0.0, (RAY_DIMS[1] / 2 + 0.42) - 0.5 + 0.25, 0.0))
    # the same on the other side: three voxels beyond the +x face, and a quarter voxel below the first valid position lo + 0.5 vs
    add('beside-high', *axis('+z'), sideways=((RAY_DIMS[0] / 2 - 0.26) + 3.0, 0.0, 0.0))
    add('just-outside-low', *axis('+z'), sideways=(0.0, -(RAY_DIMS[1] / 2 - 0.42) + 0.5 - 0.25, 0.0))
    for c in range(8):                                                  # from beyond the eight corners, looking at the centre
        signs = np.array([1.0 if c >> a & 1 else -1.0 for a in range(3)])
        q, _ = T.look_at(signs * 17.5, np.zeros(3))
        add(f'corner{c}', q, -signs * 17.5)
    add('coarse-steps', *axis('-y'), step=2.7)
    add('fine-steps', cases['corner5']['q'], (-17.5, 17.5, -17.5), step=0.125)
    add('near-inside', *axis('-x'), near=19.5)
    add('near-beyond', *axis('+z'), near=45.0)
    add('ends-before', *axis('+x'), nsteps=18)
    add('ends-inside', *axis('+x'), nsteps=22)
    tele = np.array([[640.0, 0.0, 8.5], [0.0, 640.0, 7.5], [0.0, 0.0, 1.0]])
    add('distant', *axis('+z', 1200.0), K=tele, near=1160.0, nsteps=100)
    add('distant-shifted', *axis('+z', 1200.0), K=tele, near=1160.0, nsteps=100, shift=RAY_SHIFT)
    add('shifted', *axis('-x'), shift=RAY_SHIFT)
    return cases


def ray_rays(case, h=RAY_H, w=RAY_W):
    """dw float64 [h*w, 3] of the header's rays."""
    K = case['K']
    vv, uu = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing='ij')
    dc = np.stack([((uu.reshape(-1) + 0.5) - K[0, 2]) / K[0, 0], ((vv.reshape(-1) + 0.5) - K[1, 2]) / K[1, 1], np.ones(h * w)], axis=1)
    return O.rotate(normalise(case['q']), dc)


def first_valid(case, state, h=RAY_H, w=RAY_W):
    """int64 [h*w]: the first sample index of every ray that F(P) calls valid, -1 where none of the nsteps samples is; from `sample`
    alone."""
    tsdf, weight = state
    dw, fv = ray_rays(case, h, w), np.full(h * w, -1)
    for k in range(case['nsteps']):
        s = case['near'] + np.float64(k) * case['step']
        valid, _ = sample(tsdf, weight, case['lo'], case['vs'], 1.0, case['t'][None, :] + s * dw)
        fv = np.where((fv < 0) & valid, k, fv)
    return fv


def ray_case_maps(case, state, h=RAY_H, w=RAY_W, nsteps=None):
    return raycast(state[0], state[1], case['lo'], case['vs'], 1.0, case['K'], case['q'], case['t'], h, w, case['near'], case['step'],
                   case['nsteps'] if nsteps is None else nsteps)
