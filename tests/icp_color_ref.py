"""NumPy restatement of the colour part of the registration contract of include/f3d.h (f3d_tsdf_raycast_color, f3d_icp_color_sums,
f3d_icp_color) and of segUtils/registration.py track_frames(color_weight=...), operation for operation, on top of tests/icp_ref.py,
tests/tsdf_ref.py and tests/tsdf_color_ref.py: float64 arithmetic, every product, sum and division as the header writes it.  What the
library returns must equal this bit for bit.  Plus the textured version of the sphere-and-wall scene.
"""
import numpy as np

from oracle import np_ref as O
import icp_ref as I
import tsdf_color_ref as C
import tsdf_ref as T

NSUMS = 2 * I.NSUMS


def intensity(r, g, b):
    return ((0.299 * r + 0.587 * g) + 0.114 * b) / 255.0


# ------------------------------------------------------------------------------------------------ raycast
def sample_color(color, lo, vs, P):
    """The colour sample of the header at the rows of P [n, 3] -> (valid bool [n], rgb float64 [n, 3]; NaN where invalid)."""
    nz, ny, nx = color.shape[:3]
    n = (nx, ny, nz)
    Cs = np.ascontiguousarray(color, np.float32).reshape(-1, 4)
    if min(n) < 2:
        return np.zeros(len(P), bool), np.full((len(P), 3), np.nan)
    with np.errstate(all='ignore'):
        g = [(P[:, a] - lo[a]) / vs - 0.5 for a in range(3)]
        fl = [np.floor(x) for x in g]
        valid = np.ones(len(P), bool)
        for a in range(3):
            valid &= (fl[a] >= 0) & (fl[a] <= n[a] - 2)
        i = [np.where(valid, x, 0).astype(np.int64) for x in fl]
        f = [np.where(valid, g[a] - i[a].astype(np.float64), 0.0) for a in range(3)]
        at = (i[2] * ny + i[1]) * nx + i[0]
        for c in range(8):
            o = (c & 1) + ((c >> 1) & 1) * nx + (c >> 2) * nx * ny
            valid &= Cs[at + o, 3] > np.float32(0)
        out = []
        for ch in range(3):
            c_jk = []
            for c in range(4):                                          # c = j + 2 k
                o = (c & 1) * nx + (c >> 1) * nx * ny
                c0, c1 = Cs[at + o, ch].astype(np.float64), Cs[at + o + 1, ch].astype(np.float64)
                c_jk.append(c0 + f[0] * (c1 - c0))
            k0 = c_jk[0] + f[1] * (c_jk[1] - c_jk[0])
            k1 = c_jk[2] + f[1] * (c_jk[3] - c_jk[2])
            out.append(k0 + f[2] * (k1 - k0))
    return valid, np.where(valid[:, None], np.stack(out, axis=1), np.nan)


def raycast_color(tsdf, weight, color, lo, vs, min_weight, K, q, t, h, w, near, step, nsteps):
    """-> (vertex, normal, depth of icp_ref.raycast; rgb float64 [h*w, 3]; intensity float64 [h*w]) of the header's colour raycast."""
    vertex, normal, depth = I.raycast(tsdf, weight, lo, vs, min_weight, K, q, t, h, w, near, step, nsteps)
    hit = ~np.isnan(vertex[:, 0])
    valid, rgb = sample_color(color, np.asarray(lo, np.float64), vs, np.where(hit[:, None], vertex, 0.0))
    seen = hit & valid
    with np.errstate(invalid='ignore'):
        inten = np.where(seen, intensity(rgb[:, 0], rgb[:, 1], rgb[:, 2]), np.nan)
    return vertex, normal, depth, np.where(seen[:, None], rgb, np.nan), inten


# ------------------------------------------------------------------------------------------------ ICP
def source_intensity(rgb, h, w):
    """Is float64 [h*w]: the intensity of the colour pixel of every depth pixel (the pixel rule of integrate)."""
    rgb = np.asarray(rgb)
    assert rgb.dtype == np.uint8 and rgb.ndim == 3 and rgb.shape[2] == 3
    hc, wc = rgb.shape[:2]
    vv, uu = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    pix = rgb[C.color_pixel(vv.reshape(-1), h, hc), C.color_pixel(uu.reshape(-1), w, wc)].astype(np.float64)
    return intensity(pix[:, 0], pix[:, 1], pix[:, 2])


def pair_parts(depth, rgb, K, q, t, depth_scale, max_depth, model_vertex, model_normal, model_intensity, hm, wm, model_K, model_q, model_t, max_dist):
    """Everything the header names on the way to a photometric pair, per source pixel -> dict(geo = icp_ref.icp_terms [h*w, 29],
    ok = the pixel has a pair, rc, Jc [h*w, 6], x, y, fa, fb, i0, j0); values of pixels without a pair are arbitrary."""
    depth = np.asarray(depth)
    h, w = depth.shape
    geo = I.icp_terms(depth, K, q, t, depth_scale, max_depth, model_vertex, model_normal, hm, wm, model_K, model_q, model_t, max_dist)
    K, mK, t, mt = np.asarray(K, np.float64), np.asarray(model_K, np.float64), np.asarray(t, np.float64), np.asarray(model_t, np.float64)
    fx, cx, fy, cy = K[0, 0], K[0, 2], K[1, 1], K[1, 2]
    MI = np.asarray(model_intensity, np.float64).reshape(-1)
    assert MI.size == hm * wm
    with np.errstate(all='ignore'):
        ok = geo[:, 28] == 1.0                                          # passed step 5
        d = np.where(ok, depth.reshape(-1).astype(np.float64) / np.float64(depth_scale), 1.0)
        vv, uu = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing='ij')
        c = np.stack([((uu.reshape(-1) + 0.5) - cx) * (d / fx), ((vv.reshape(-1) + 0.5) - cy) * (d / fy), d], axis=1)
        pr = O.rotate(I.normalise(q), c)
        p = pr + t[None, :]
        qinv = O.quat_inverse(model_q)
        cam = O.rotate(qinv, p - mt[None, :])
        h0 = (mK[0, 0] * cam[:, 0] + mK[0, 1] * cam[:, 1]) + mK[0, 2] * cam[:, 2]
        h1 = (mK[1, 0] * cam[:, 0] + mK[1, 1] * cam[:, 1]) + mK[1, 2] * cam[:, 2]
        h2 = (mK[2, 0] * cam[:, 0] + mK[2, 1] * cam[:, 1]) + mK[2, 2] * cam[:, 2]
        x, y = h0 / h2, h1 / h2
        Is = source_intensity(rgb, h, w)
        a, b = x - 0.5, y - 0.5
        i0, j0 = np.floor(a), np.floor(b)
        ok &= (i0 >= 0) & (i0 <= wm - 2) & (j0 >= 0) & (j0 <= hm - 2)
        fa, fb = a - i0, b - j0
        at = np.where(ok, j0 * wm + i0, 0).astype(np.int64)
        if hm < 2 or wm < 2:
            ok &= False
            I00 = I10 = I01 = I11 = np.zeros(h * w)
        else:
            I00, I10, I01, I11 = MI[at], MI[at + 1], MI[at + wm], MI[at + wm + 1]
        ok &= np.isfinite(I00) & np.isfinite(I10) & np.isfinite(I01) & np.isfinite(I11)
        top = I00 + fa * (I10 - I00)
        bot = I01 + fa * (I11 - I01)
        Im = top + fb * (bot - top)
        dx0, dx1 = I10 - I00, I11 - I01
        gx = dx0 + fb * (dx1 - dx0)
        gy = bot - top
        rc = Im - Is
        gc = np.stack([(gx * (mK[0, k] - x * mK[2, k]) + gy * (mK[1, k] - y * mK[2, k])) / h2 for k in range(3)], axis=1)
        gw = O.rotate(qinv * np.array([1.0, -1.0, -1.0, -1.0]), np.where(ok[:, None], gc, 0.0))
        Jc = np.stack([pr[:, 1] * gw[:, 2] - pr[:, 2] * gw[:, 1], pr[:, 2] * gw[:, 0] - pr[:, 0] * gw[:, 2], pr[:, 0] * gw[:, 1] - pr[:, 1] * gw[:, 0],
                       gw[:, 0], gw[:, 1], gw[:, 2]], axis=1)
    return dict(geo=geo, ok=ok, rc=rc, Jc=Jc, x=x, y=y, fa=fa, fb=fb, i0=i0, j0=j0)


def color_terms(depth, rgb, K, q, t, depth_scale, max_depth, model_vertex, model_normal, model_intensity, hm, wm, model_K, model_q, model_t, max_dist):
    """The terms [h*w, 58] of every source pixel at the pose (q, t): icp_ref.icp_terms, then the 29 of the photometric pair; zeros where
    the pixel has none."""
    P = pair_parts(depth, rgb, K, q, t, depth_scale, max_depth, model_vertex, model_normal, model_intensity, hm, wm, model_K, model_q, model_t, max_dist)
    J, r = P['Jc'], P['rc']
    with np.errstate(all='ignore'):
        cols = [J[:, a] * J[:, b] for a in range(6) for b in range(a, 6)] + [J[:, a] * r for a in range(6)] + [r * r, np.ones(len(r))]
        return np.concatenate([P['geo'], np.where(P['ok'][:, None], np.stack(cols, axis=1), 0.0)], axis=1)


def icp_color_sums(depth, rgb, K, q, t, depth_scale, max_depth, model_vertex, model_normal, model_intensity, hm, wm, model_K, model_q, model_t, max_dist):
    return I.shaped_sums(color_terms(depth, rgb, K, q, t, depth_scale, max_depth, model_vertex, model_normal, model_intensity, hm, wm, model_K, model_q,
                                     model_t, max_dist))


def weighted(tot, color_weight):
    """The 29 numbers the header's solve reads: A = A_g + color_weight * A_c, the sums b of which is the negative likewise, and the
    geometric r r and count."""
    mixed = tot[:I.NSUMS].copy()
    mixed[:27] = tot[:27] + np.float64(color_weight) * tot[I.NSUMS:I.NSUMS + 27]
    return mixed


def icp_color(depth, rgb, K, q, t, depth_scale, max_depth, model_vertex, model_normal, model_intensity, hm, wm, model_K, model_q, model_t, max_dist,
              color_weight, iterations, min_pairs):
    """-> (pose float64 [7], stats float64 [iterations, 5], status) of the header's f3d_icp_color."""
    q, t = np.asarray(q, np.float64).copy(), np.asarray(t, np.float64).copy()
    stats, lost = np.zeros((iterations, 5)), False
    for it in range(iterations):
        if lost:
            stats[it] = (0.0, 0.0, I.LOST, 0.0, 0.0)
            continue
        tot = icp_color_sums(depth, rgb, K, q, t, depth_scale, max_depth, model_vertex, model_normal, model_intensity, hm, wm, model_K, model_q, model_t,
                             max_dist)
        x = I.solve(weighted(tot, color_weight), min_pairs)
        stats[it] = (tot[28], tot[27], I.OK if x is not None else I.LOST, tot[29 + 28], tot[29 + 27])
        if x is None:
            lost = True
            continue
        q, t = I.update(q, t, x)
    return np.concatenate([q, t]), stats, I.LOST if lost else I.OK


# ------------------------------------------------------------------------------------------------ track_frames
def track_frames_color(tsdf, weight, color, lo, vs, trunc, max_weight, depths, rgbs, K, wxyzs, translations, color_weight, depth_scale=1.0,
                       max_depth=10.0, max_dist=0.1, iterations=10, min_pairs=100, min_weight=1.0, integrate=True):
    """-> (wxyzs [F, 4], translations [F, 3], status int32 [F], tsdf, weight, color) of registration.track_frames(colors=rgbs,
    color_weight=color_weight) on a volume state."""
    depths = np.asarray(depths)
    F, h, w = depths.shape
    qs, ts = np.asarray(wxyzs, np.float64).copy(), np.asarray(translations, np.float64).copy()
    status = np.zeros(F, np.int32)
    nsteps = int(np.floor((max_depth - 0.0) / vs)) + 1
    for f in range(F):
        empty = not weight.any()
        if not empty:
            vertex, normal, _, _, inten = raycast_color(tsdf, weight, color, lo, vs, min_weight, K, qs[f], ts[f], h, w, 0.0, vs, nsteps)
            pose, _, status[f] = icp_color(depths[f], rgbs[f], K, qs[f], ts[f], depth_scale, max_depth, vertex, normal, inten, h, w, K, qs[f], ts[f],
                                           max_dist, color_weight, iterations, min_pairs)
            if status[f] == I.OK:
                qs[f], ts[f] = pose[:4], pose[4:]
        if empty or integrate:
            tsdf, weight, color = C.integrate_color(tsdf, weight, color, lo, vs, trunc, max_weight, depths[f:f + 1], rgbs[f:f + 1], K, qs[f:f + 1],
                                                    ts[f:f + 1], depth_scale, max_depth)
    return qs, ts, status, tsdf, weight, color


# ------------------------------------------------------------------------------------------------ the textured scene
# Each channel is a sinusoid of the world point a pixel sees: byte = round(128 + AMPLITUDE sin(2 pi k . p / WAVELENGTH)).  None of
# the unit wave vectors is parallel to icp_ref.AXIS_N (each has a large component across it), so no rotation about the scene's
# symmetry axis leaves a channel as it is.
WAVELENGTH, AMPLITUDE = 0.5, 100.0
WAVE_VECTORS = np.array([[1.0, 0.3, 0.2], [-0.4, 1.0, 0.3], [0.7, -0.7, 0.5]])
WAVE_VECTORS /= np.linalg.norm(WAVE_VECTORS, axis=1)[:, None]


def texture(p):
    """uint8 [n, 3] of the world points p [n, 3]."""
    phase = 2.0 * np.pi * (p @ WAVE_VECTORS.T) / WAVELENGTH
    return np.clip(np.round(128.0 + AMPLITUDE * np.sin(phase)), 0, 255).astype(np.uint8)


def textured_images(K, wxyzs, translations, depths):
    """uint8 [F, h, w, 3]: the texture at the world point each pixel sees through its centre (u + 0.5, v + 0.5); black without a depth."""
    F, h, w = depths.shape
    uu, vv = np.meshgrid(np.arange(w) + 0.5, np.arange(h) + 0.5)
    dc = np.stack([((uu - K[0, 2]) / K[0, 0]).reshape(-1), ((vv - K[1, 2]) / K[1, 1]).reshape(-1), np.ones(h * w)], axis=1)
    out = np.zeros((F, h, w, 3), np.uint8)
    for f in range(F):
        d = depths[f].reshape(-1)
        p = np.asarray(translations[f], np.float64)[None, :] + O.rotate(np.asarray(wxyzs[f], np.float64), dc) * d[:, None]
        out[f] = np.where((d > 0)[:, None], texture(p), 0).reshape(h, w, 3)
    return out


def color_scene():
    """icp_ref.icp_scene() with colour: rgbs uint8 [6, H, W, 3] of the textured scene, the colour state after integrating the frames
    with them at the true poses (tsdf and weight are icp_scene's), and the five maps ray-cast from the true pose of frame 0."""
    s = I.icp_scene()
    s['rgbs'] = textured_images(s['K'], s['q'], s['t'], s['depths'])
    z = np.zeros(I.DIMS[::-1], np.float32)
    tsdf, weight, color = C.integrate_color(z, z, np.zeros(I.DIMS[::-1] + (4,), np.float32), I.LO, I.VS, I.TRUNC, 64, s['depths'], s['rgbs'], s['K'],
                                            s['q'], s['t'], 1.0, I.MAX_DEPTH)
    assert np.array_equal(tsdf, s['tsdf']) and np.array_equal(weight, s['weight'])
    s['color'] = color
    maps = raycast_color(tsdf, weight, color, I.LO, I.VS, 1.0, s['K'], s['q'][0], s['t'][0], I.H, I.W, 0.0, I.VS, int(np.floor(I.MAX_DEPTH / I.VS)) + 1)
    assert np.array_equal(maps[0], s['vertex'], equal_nan=True) and np.array_equal(maps[2], s['depth'])
    s['rgb'], s['intensity'] = maps[3], maps[4]
    return s
