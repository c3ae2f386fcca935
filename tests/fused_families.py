"""Scene families for the fused path: the same room and rolled cameras, each family changing ONE thing -- where the scene sits, its
unit, the quaternion's norm, the intrinsic matrix -- plus, per family, an adversarial cloud whose points lie within a few ulp of the
frustum planes.  The error budgets of the fused tiers (float32 and float64 culls, centre + offset projection) have terms
proportional to |p|, |eye|, |K row| |q|^2: these families move those magnitudes away from the few metres around the origin where
every other fused test lives.  NumPy only, seeded, nothing here touches the GPU; arrays are cached and read-only."""
import functools

import numpy as np

from f3d import synth
from oracle import np_ref as O

W = H = 256
N_POINTS = 20_000
N_VIEWS = 8
K0 = np.array([[200., 0, 128], [0, 200., 128], [0, 0, 1]])
SHIFTS = {'shift1e3': (1e3, -2e3, 5e2), 'shift1e5': (1e5, 3e5, -2e5), 'shift4e6': (4e6, -7e6, 1e6)}
FAMILIES = ('base', 'shift1e3', 'shift1e5', 'shift4e6', 'mm', 'km', 'q_small', 'q_big', 'skew', 'pp_outside', 'wide', 'tele', 'many')
EXTRA_CAMERAS = ('tele_near',)                     # single-view kernels only: its views see < 0.3 % of the cloud
MASK_KIND = {name: ('iid', 'block64')[k % 2] for k, name in enumerate(FAMILIES + EXTRA_CAMERAS)}    # any-alphabet / packed instance
CAMERA_SEED = 17
PLANE_PER = {'many': 90}                           # on-plane points per (view, plane); 300 elsewhere: every cloud stays <= 32 000 points


def _quat_mul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
                     a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1],
                     a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])


def _rolled_cameras(V, radius, height, seed):
    """Eyes on a ring, targets in the room, every camera rolled about its optical axis: wxyz [V,4] (camera -> world), eyes [V,3].
    height: (lo, hi) of a uniform draw."""
    rng = np.random.default_rng(seed)
    th = 2 * np.pi * np.arange(V) / V + 0.1
    eyes = np.stack([radius * np.cos(th), radius * np.sin(th), rng.uniform(height[0], height[1], V)], axis=1)
    targets = rng.uniform([-2, -2, 0.5], [2, 2, 2.5], (V, 3))
    roll = rng.uniform(-np.pi, np.pi, V)
    q = np.stack([_quat_mul(synth._look_at_quat(e, g), np.array([np.cos(r / 2), 0, 0, np.sin(r / 2)]))
                  for e, g, r in zip(eyes, targets, roll)])
    return q, eyes


@functools.lru_cache(maxsize=None)
def family(name):
    """-> (points [n,3] float64, K [3,3], q_wxyz [V,4], t [V,3], max_depth, w, h, masks uint8 [V,h,w])."""
    V, n = (70, 5_000) if name == 'many' else (N_VIEWS, N_POINTS)
    pts = synth.cloud(n, seed=3)
    K, max_depth = K0.copy(), 10.0
    if name == 'tele':
        q, t = _rolled_cameras(V, 60.0, (20.0, 20.0), seed=CAMERA_SEED)
    else:
        q, t = _rolled_cameras(V, 4.0, (0.3, 2.7), seed=CAMERA_SEED)
    if name in SHIFTS or name == 'many':
        T = np.array(SHIFTS['shift1e5' if name == 'many' else name])
        pts, t = pts + T, t + T
    elif name == 'mm':
        pts, t, max_depth = pts * 1000.0, t * 1000.0, 1e4
    elif name == 'km':
        pts, t, max_depth = pts * 1e-3, t * 1e-3, 1e-2
    elif name == 'q_small':
        q = q * 1e-2
    elif name == 'q_big':
        q = q * 30.0
    elif name == 'skew':
        K[0, 1], K[1, 0], K[1, 1] = 60.0, -25.0, 520.0
    elif name == 'pp_outside':
        K[0, 2], K[1, 2] = -100.0, 420.0
    elif name == 'wide':
        K[0, 0] = K[1, 1] = 20.0
    elif name == 'tele':
        K[0, 0] = K[1, 1] = 5000.0
        max_depth = 100.0
    elif name == 'tele_near':
        K[0, 0] = K[1, 1] = 5000.0
    elif name != 'base':
        raise KeyError(name)
    masks = synth.masks(V, H, W, MASK_KIND[name])
    for a in (pts, K, q, t, masks):
        a.setflags(write=False)
    return pts, K, q, t, max_depth, W, H, masks


def _ulp_steps(x, steps):
    """x moved by `steps` (integers) units in the last place, element by element."""
    x = x.copy()
    for k in range(1, int(np.abs(steps).max()) + 1):
        up, down = steps >= k, steps <= -k
        x[up] = np.nextafter(x[up], np.inf)
        x[down] = np.nextafter(x[down], -np.inf)
    return x


def on_plane_points_of(K, q, t, max_depth, w, h, per, owners=None, seed=29):
    """The adversarial cloud of a scene, [len(owners) * 5 * per, 3] float64 in (owner, plane, draw) order (owners: view indices in
    the order given; None = every view in turn): per owner view, `per` points on each
    of the 4 side planes (eye + r (s a + (1 - s) b): a, b the unit rays through two adjacent image corners, built the way
    O.frustum_data builds them) and `per` on the far plane (eye + max_depth d / (d . lookat), d through pixels of the image
    grown by 20 % on every side).  The oracle's unit normal of a telephoto side plane -- the cross product of two nearly parallel
    rays -- is itself ~1e-15 rad off the plane those rays span: 30 ulp at the far end.  So every point takes one step onto the
    plane AS THE ORACLE EVALUATES IT (it ends within an ulp or two of n . (p - pp) = 0), and then every coordinate is moved by
    -3..3 ulp: each point straddles one plane of its own view."""
    rng = np.random.default_rng(seed)
    Kinv = O.inv3(K)
    eyes, lookats, _, _ = O.frustum_data(K, w, h, q, t)
    ppts, pnrm = O.frustum_planes(K, w, h, q, t, max_depth)
    out = []
    for j in (range(len(t)) if owners is None else owners):
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
    pts = _ulp_steps(pts, rng.integers(-3, 4, pts.shape))
    pts.setflags(write=False)
    return pts


@functools.lru_cache(maxsize=None)
def on_plane_points(name, per=300):
    """on_plane_points_of the family's scene, every view an owner: [V * 5 * per, 3] in (view, plane, draw) order."""
    _, K, q, t, max_depth, w, h, _ = family(name)
    return on_plane_points_of(K, q, t, max_depth, w, h, per)


def on_plane_owner(name, per=300):
    """The view every point of on_plane_points(name, per) was built for."""
    return np.repeat(np.arange(len(family(name)[3])), 5 * per)


def clouds(name):
    """{'random': ..., 'plane': ...} of a family, at the sizes the tests use."""
    return {'random': family(name)[0], 'plane': on_plane_points(name, PLANE_PER.get(name, 300))}
