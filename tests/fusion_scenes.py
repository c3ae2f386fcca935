"""Synthetic depth captures for the fusion tests (pure NumPy, deterministic from a seed).

``curved_capture`` ray-casts a sphere, a vertical cylinder and a tilted plane from a handful of rotated camera poses.  Only IEEE
operations that round the same on every host are used (+, -, *, /, sqrt, and the uniform draws of ``np.random.default_rng``), so
the frames regenerate bit for bit wherever the tests run: tests/golden/fuse_curved.npz stores a digest of them instead of the frames.
"""
import contextlib
import hashlib
import warnings

import numpy as np

S = 0.4                                      # scene scale: a pixel spans about 1.2 cm, a fraction of the test radii
SPHERE_C, SPHERE_R = S * np.array([0.05, 0.0, 2.6]), S * 0.55
CYL_XZ, CYL_R, CYL_Y = S * np.array([-0.75, 2.9]), S * 0.35, (S * -0.9, S * 0.5)
PLANE_P, PLANE_N = S * np.array([0.0, 0.0, 3.6]), np.array([0.15, -0.25, -1.0])
NOISE = {0: 0.07, 1: 0.45, 2: 0.03}          # normal noise per surface (sphere, cylinder, plane): angles spread around 5-30 degrees


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.sqrt((v[..., 0:1] * v[..., 0:1] + v[..., 1:2] * v[..., 1:2]) + v[..., 2:3] * v[..., 2:3])


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def _quat_from_axes(R):
    """Unit (w,x,y,z) quaternion of the rotation matrix R (columns = camera axes in the world)."""
    tr = (R[0, 0] + R[1, 1]) + R[2, 2]
    if tr > 0:
        s = np.sqrt(tr + 1.0) * 2
        q = np.array([0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s])
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = np.sqrt(((1.0 + R[i, i]) - R[j, j]) - R[k, k]) * 2
        q = np.zeros(4)
        q[0] = (R[k, j] - R[j, k]) / s
        q[1 + i] = 0.25 * s
        q[1 + j] = (R[j, i] + R[i, j]) / s
        q[1 + k] = (R[k, i] + R[i, k]) / s
    return q / np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])


def _pose(eye, target, down):
    """Camera -> world axes: z towards the target, y as close to `down` as possible, x = y cross z (x right, y down)."""
    z = _unit(target - eye)
    y = _unit(down - ((down[0] * z[0] + down[1] * z[1]) + down[2] * z[2]) * z)
    return np.stack([_cross(y, z), y, z], axis=1)


def _cast(eye, D):
    """First hit of the rays eye + t*D (t > 0): (t, surface id) with id 0 sphere, 1 cylinder, 2 plane, -1 none."""
    n = len(D)
    best, sid = np.full(n, np.inf), np.full(n, -1)
    dot = lambda a, b: (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]
    oc = eye - SPHERE_C
    a, b, c = dot(D, D), 2 * dot(D, oc[None, :]), dot(oc, oc) - SPHERE_R * SPHERE_R
    disc = b * b - 4 * a * c
    with np.errstate(invalid='ignore'):
        t = (-b - np.sqrt(disc)) / (2 * a)
    hit = (disc > 0) & (t > 0) & (t < best)
    best[hit], sid[hit] = t[hit], 0
    ox, oz = eye[0] - CYL_XZ[0], eye[2] - CYL_XZ[1]
    a = D[:, 0] * D[:, 0] + D[:, 2] * D[:, 2]
    b = 2 * (D[:, 0] * ox + D[:, 2] * oz)
    c = ox * ox + oz * oz - CYL_R * CYL_R
    disc = b * b - 4 * a * c
    with np.errstate(invalid='ignore'):
        t = (-b - np.sqrt(disc)) / (2 * a)
    y = eye[1] + t * D[:, 1]
    hit = (disc > 0) & (t > 0) & (t < best) & (y > CYL_Y[0]) & (y < CYL_Y[1])
    best[hit], sid[hit] = t[hit], 1
    pn = _unit(PLANE_N)
    with np.errstate(divide='ignore', invalid='ignore'):
        t = dot(PLANE_P - eye, pn) / dot(D, pn[None, :])
    hit = (t > 0) & (t < best)
    best[hit], sid[hit] = t[hit], 2
    return best, sid


def curved_capture(h, w, nframes, seed, quirks=None):
    """A capture of h x w depth frames -> (K, wxyz [F,4], translations [F,3], frames) with frames[j] = (name, points [h*w,3],
    normals, colours, valid [h*w]) in world coordinates, ready for ``Fusion.from_frames``.

    Rotated poses (frame 2's quaternion is scaled by 1.3: the reference never normalises it); analytic normals plus noise, so that
    many neighbouring normal pairs lie within a few degrees of the test thresholds (5, 10, 30 degrees); silhouette depth jumps
    between the three surfaces, random holes and a rectangular one.  With ``quirks`` (default: when nframes >= 6) frame 0 is all
    invalid (fusion starts at frame 1), frame 3 has one zero normal and one NaN point at valid pixels (the sequential order of
    events; both pixels stay free) and frame 4 is posed far away, seeing none of the cloud (the reference then down-samples it on
    frame 3's left-over mask)."""
    quirks = nframes >= 6 if quirks is None else quirks
    if quirks and nframes < 6:
        raise ValueError('the quirk frames need at least 6 frames')
    rng = np.random.default_rng(seed)
    f = 1.2 * w
    K = np.array([[f, 0.0, w / 2.0 - 0.5], [0.0, f, h / 2.0 + 0.25], [0.0, 0.0, 1.0]])
    uu, vv = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    d_cam = np.stack([((uu - K[0, 2]) / K[0, 0]).reshape(-1), ((vv - K[1, 2]) / K[1, 1]).reshape(-1), np.ones(h * w)], axis=1)
    qs, ts, frames = [], [], []
    for j in range(nframes):
        eye = S * (np.array([-0.2 + 0.07 * j, -0.06 + 0.025 * j, 0.03 * j]) + rng.uniform(-0.02, 0.02, 3))
        target = S * (np.array([-0.15, 0.0, 2.9]) + rng.uniform(-0.08, 0.08, 3))
        R = _pose(eye, target, np.array([rng.uniform(-0.25, 0.25), 1.0, rng.uniform(-0.1, 0.1)]))
        D = (R[None, :, 0] * d_cam[:, 0:1] + R[None, :, 1] * d_cam[:, 1:2]) + R[None, :, 2] * d_cam[:, 2:3]
        t, sid = _cast(eye, D)
        t = t * (1 + rng.uniform(-1e-3, 1e-3, h * w))
        pts = eye[None, :] + t[:, None] * D
        nrm = np.empty((h * w, 3))
        nrm[sid == 0] = (pts[sid == 0] - SPHERE_C) / SPHERE_R
        cyl = np.zeros((int((sid == 1).sum()), 3))
        cyl[:, 0], cyl[:, 2] = pts[sid == 1, 0] - CYL_XZ[0], pts[sid == 1, 2] - CYL_XZ[1]
        nrm[sid == 1] = cyl / CYL_R
        nrm[sid == 2] = _unit(PLANE_N)
        scale = np.zeros(h * w)
        for s, amp in NOISE.items():
            scale[sid == s] = amp
        nrm = _unit(nrm + scale[:, None] * rng.uniform(-1, 1, (h * w, 3)))
        clr = rng.integers(0, 256, (h * w, 3)) / 255.0                 # 8-bit colours, as a sensor gives them
        valid = (sid >= 0) & (rng.random(h * w) > 0.03)
        if j == 1:
            r0, c0 = h // 3, w // 5
            valid.reshape(h, w)[r0:r0 + max(1, h // 8), c0:c0 + max(1, w // 10)] = False
        q = _quat_from_axes(R)
        if j == 2:
            q = 1.3 * q
        if quirks:
            if j == 0:
                valid[:] = False
            elif j == 3:
                zp, nanp = (h // 2) * w + w // 2 + 3, (h // 4) * w + (3 * w) // 4
                valid[[zp, nanp]] = True
                nrm[zp] = 0.0
                pts[nanp, 1] = np.nan
            elif j == 4:
                eye = np.array([0.0, 0.0, 60.0])                         # the cloud lies behind this camera
        qs.append(q)
        ts.append(eye)
        frames.append((f'{200 + j}', pts, nrm, clr, valid))
    return K, np.array(qs), np.array(ts), frames


def capture_digest(K, wxyz, translations, frames):
    """SHA-256 over the bytes of everything curved_capture returns."""
    dg = hashlib.sha256()
    for a in (K, wxyz, translations):
        dg.update(np.ascontiguousarray(a, np.float64).tobytes())
    for name, pts, nrm, clr, valid in frames:
        dg.update(name.encode())
        for a in (pts, nrm, clr):
            dg.update(np.ascontiguousarray(a, np.float64).tobytes())
        dg.update(np.ascontiguousarray(valid, bool).tobytes())
    return dg.hexdigest()


def copy_frames(frames):
    return [(n, p.copy(), q.copy(), c.copy(), v.copy()) for n, p, q, c, v in frames]


# ---- one sequence through the oracle or the library, and the comparison of two such runs (tests/test_fusion_device_gpu.py and others)
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


@contextlib.contextmanager
def _quiet():
    with warnings.catch_warnings(), np.errstate(all='ignore'):
        warnings.simplefilter('ignore', RuntimeWarning)              # means of empty sets (zero normal / NaN point), as the reference
        yield


def run_fuse(K, w, h, q, t, frames, params, seed, how, lookup_dir=None):
    """`frames` through O.fuse ('oracle'), fuse ('host') or fuse_device ('device'), used as given (fuse and the oracle consume
    their masks) -> (five outputs as NumPy, [(name, lookup)] in the order they were handed out, the generator's next draw, the
    Fusion object)."""
    from oracle import np_ref as O
    lookups = []
    if how == 'oracle':
        np.random.seed(seed)
        with _quiet():
            *out, lookups = O.fuse(K, w, h, q, t, frames, *params)
        return out, lookups, np.random.random(), None

    def sink(name, lut):
        if how == 'device':
            assert lut.is_cuda and lut.dtype.is_signed and lut.element_size() == 4 and tuple(lut.shape) == (h * w,)
        else:
            assert isinstance(lut, np.ndarray) and lut.dtype == np.int32 and lut.shape == (h * w,)
        lookups.append((name, lut.clone() if how == 'device' else lut.copy()))
    from Fusion3DSeg.fusion import Fusion
    fu = Fusion.from_frames(K, w, h, q, t, frames, lookup_dir=lookup_dir, lookup_sink=sink)
    np.random.seed(seed)
    out = fu.fuse_device(*params) if how == 'device' else fu.fuse(*params)
    after = np.random.random()
    if how == 'device':
        out = [o.cpu().numpy() for o in out]
        lookups = [(n, lut.cpu().numpy()) for n, lut in lookups]
    return list(out), lookups, after, fu


def assert_same_fuse(got, want):
    (go, gl, ga, _), (wo, wl, wa, _) = got, want
    for k, (a, b) in enumerate(zip(go, wo)):
        assert same_bits(a, b), (k, a.dtype, b.dtype, a.shape, b.shape)
    assert [n for n, _ in gl] == [n for n, _ in wl]
    for (name, a), (_, b) in zip(gl, wl):
        assert same_bits(a, b), name
    assert ga == wa
