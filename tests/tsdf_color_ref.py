"""NumPy restatement of the colour part of the TSDF contract of include/f3d.h (f3d_tsdf_integrate_color's step 7 and
f3d_tsdf_extract_colors), operation for operation, on top of tests/tsdf_ref.py: float64 arithmetic, every product, sum and division as
the header writes it, float32 storage.  No culling, no lazy reads, no launch shape: what the library returns must equal this bit for
bit.  Plus the two-colour version of the sphere-and-wall scene and the frames the tests integrate.
"""
import numpy as np

import tsdf_ref as R

# the base scene of tests/test_tsdf_gpu.py: its volume, its image and its five poses (tests/test_tsdf_color_cpu.py compares them)
DIMS, VS, LO, TRUNC = (37, 29, 21), 0.05, np.array([-0.9, -0.7, 0.55]), 0.2
H, W, MAX_DEPTH = 40, 48, 4.0
EYES = [(0.0, 0.0, 0.0), (-0.5, 0.3, 0.8), (1.5, 1.2, 0.9), (0.0, 0.0, -1.0), (0.6, -0.4, 0.3)]
TARGETS = [(0.0, 0.0, 1.0), (0.05, 0.0, 1.2), (1.0, 0.8, 1.7), (0.0, 0.0, -3.0), (0.0, 0.0, 1.1)]
# the two-colour scene: the same but for lo_z, so that the volume's first layer is not cut by the sphere's near pole
TWO_LO = np.array([-0.9, -0.7, 0.6])
SPHERE_RGB, WALL_RGB = np.array([200, 30, 90], np.uint8), np.array([20, 160, 250], np.uint8)


# ------------------------------------------------------------------------------------------------ the pixel rule
def color_pixel(u, n_depth, n_color):
    """The colour pixel of depth pixel u along one axis: (int64)u * n_color / n_depth (non-negative operands: // is C's division)."""
    return np.asarray(u, np.int64) * np.int64(n_color) // np.int64(n_depth)


# ------------------------------------------------------------------------------------------------ integrate (step 7)
def integrate_color(tsdf, weight, color, lo, vs, trunc, max_weight, depths, rgb, K, wxyzs, translations, depth_scale=1.0, max_depth=10.0,
                    every_update=False):
    """Returns the new (tsdf, weight, color); the inputs are left as they are.  tsdf and weight are tsdf_ref.integrate's.  With
    every_update the colour follows every TSDF update instead of the in-band ones only: NOT the contract, but the rule the contract
    rejects, which the tests show to bleed the background's colour over a silhouette."""
    nz, ny, nx = tsdf.shape
    T, Wt = R.integrate(tsdf, weight, lo, vs, trunc, max_weight, depths, K, wxyzs, translations, depth_scale, max_depth)
    Cs = np.ascontiguousarray(color, np.float32).reshape(-1, 4).copy()
    wmax = np.float64(np.float32(max_weight))
    depths, rgb = np.asarray(depths), np.asarray(rgb)
    F, h, w = depths.shape
    assert rgb.dtype == np.uint8 and rgb.shape[0] == F and rgb.shape[3] == 3
    hc, wc = rgb.shape[1:3]
    with np.errstate(all='ignore'):
        for f in range(F):
            terms = R.frame_terms(K, wxyzs[f], translations[f], lo, (nx, ny, nz), vs, depths[f], depth_scale)
            ok = R.applied(terms, max_depth, trunc).reshape(-1)            # steps 1 - 4 have passed
            val = terms['sdf'].reshape(-1) / np.float64(trunc)             # as step 4 computes it, before the clamp
            band = ok if every_update else ok & ~(val > 1.0)
            u = np.where(band, np.floor(terms['px'].reshape(-1)), 0).astype(np.int64)
            v = np.where(band, np.floor(terms['py'].reshape(-1)), 0).astype(np.int64)
            pix = rgb[f][color_pixel(v, h, hc), color_pixel(u, w, wc)].astype(np.float64)
            wo = Cs[:, 3].astype(np.float64)
            Cn = ((Cs[:, :3].astype(np.float64) * wo[:, None] + pix) / (wo[:, None] + 1.0)).astype(np.float32)
            Wn = np.minimum(wo + 1.0, wmax).astype(np.float32)
            Cs = np.where(band[:, None], np.concatenate([Cn, Wn[:, None]], axis=1), Cs)
    return T, Wt, Cs.reshape(nz, ny, nx, 4)


# ------------------------------------------------------------------------------------------------ vertex colours
def vertex_colors(tsdf, weight, color, min_weight=1.0):
    """-> (rgb uint8 [nv, 3], colored uint8 [nv]) of the header's vertex-colour rule; vertex ids as in tsdf_ref.extract."""
    nz, ny, nx = tsdf.shape
    N = nx * ny * nz
    st = (1, nx, nx * ny)
    S = tsdf.reshape(-1)
    Cs = np.ascontiguousarray(color, np.float32).reshape(-1, 4)
    obs = weight.reshape(-1) >= np.float32(min_weight)
    with np.errstate(invalid='ignore'):
        inside = obs & (S < 0)
    lin = np.arange(N, dtype=np.int64)
    P = (lin % nx, (lin // nx) % ny, lin // (nx * ny))
    cl = lin[(P[0] <= nx - 2) & (P[1] <= ny - 2) & (P[2] <= nz - 2)]
    all_obs, nin = np.ones(len(cl), bool), np.zeros(len(cl), np.int64)
    for c in range(8):
        at = cl + (c & 1) * st[0] + ((c >> 1) & 1) * st[1] + (c >> 2) * st[2]
        all_obs &= obs[at]
        nin += inside[at]
    al = cl[all_obs & (nin > 0) & (nin < 8)]                              # the active cells, ascending: their ranks are the vertex ids
    sums, count = np.zeros((len(al), 3)), np.zeros(len(al), np.int64)
    with np.errstate(all='ignore'):
        for a in range(3):
            b, c = (a + 1) % 3, (a + 2) % 3
            for oc in (0, 1):
                for ob in (0, 1):                                       # e = 4 a + 2 oc + ob ascending
                    at0 = al + ob * st[b] + oc * st[c]
                    at1 = at0 + st[a]
                    cross = inside[at0] != inside[at1]
                    s0, s1 = S[at0].astype(np.float64), S[at1].astype(np.float64)
                    L = s0 / (s0 - s1)
                    c0, c1 = Cs[at0, :3].astype(np.float64), Cs[at1, :3].astype(np.float64)
                    has0, has1 = Cs[at0, 3] > np.float32(0), Cs[at1, 3] > np.float32(0)
                    both = c0 + L[:, None] * (c1 - c0)
                    col = np.where((has0 & has1)[:, None], both, np.where(has0[:, None], c0, c1))
                    use = cross & (has0 | has1)
                    sums = np.where(use[:, None], sums + col, sums)
                    count += use
        m = np.where(count[:, None] > 0, sums / count[:, None].astype(np.float64), 0.0)
        m = np.where(m > 0.0, m, 0.0)                                   # max(m, 0); NaN -> 0
        m = np.where(m < 255.0, m, 255.0)
        rgb = np.floor(m + 0.5).astype(np.uint8)
    return rgb, (count > 0).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ scenes
def base_frames():
    """K, wxyzs, translations, depths float64 [5, 40, 48] of test_tsdf_gpu.py's frames fixture: the sphere-and-wall scene from the
    five poses with its holes (0, NaN, +inf, beyond max_depth, negative) and the unnormalised quaternion of pose 4."""
    K, q, t, depths = R.scene(EYES, TARGETS, H, W)
    q[4] = 1.3 * q[4]
    depths[0, 5:9, 7:12] = 0.0
    depths[0, 20, 3:30] = np.nan
    depths[1, 11:14, 20:26] = np.inf
    depths[4, 30:34, 10:20] = 50.0
    depths[1, 0, 0] = -1.0
    return K, q, t, depths


def two_colour_images(K, wxyzs, translations, depths, hc, wc):
    """uint8 [F, hc, wc, 3]: SPHERE_RGB where the ray through the centre of the depth pixel that a colour pixel belongs to ends on
    the sphere, WALL_RGB elsewhere.  A colour pixel (vc, uc) belongs to the depth pixel whose colour pixel it is, so the images are
    constant over the colour pixels of one depth pixel: exact at any resolution that is a multiple of the depth frames'."""
    F, h, w = depths.shape
    assert hc % h == 0 and wc % w == 0
    out = np.empty((F, hc, wc, 3), np.uint8)
    uu, vv = np.meshgrid(np.arange(w) + 0.5, np.arange(h) + 0.5)
    dc = np.stack([((uu - K[0, 2]) / K[0, 0]).reshape(-1), ((vv - K[1, 2]) / K[1, 1]).reshape(-1), np.ones(h * w)], axis=1)
    for f in range(F):
        p = np.asarray(translations[f], np.float64)[None, :] + R.O.rotate(np.asarray(wxyzs[f], np.float64), dc) * depths[f].reshape(-1, 1)
        on_sphere = np.abs(np.linalg.norm(p - R.SPHERE_C[None, :], axis=1) - R.SPHERE_R) < 1e-6
        img = np.where(on_sphere[:, None], SPHERE_RGB[None, :], WALL_RGB[None, :]).reshape(h, w, 3)
        out[f] = np.repeat(np.repeat(img, hc // h, axis=0), wc // w, axis=1)
    return out


def two_colour_scene(sel=(0, 1, 2, 3, 4), hc=H, wc=W):
    """K, wxyzs, translations, depths, rgb of the two-colour scene from the poses `sel` of the five (no holes)."""
    sel = list(sel)
    K, q, t, depths = R.scene([EYES[i] for i in sel], [TARGETS[i] for i in sel], H, W)
    return K, q, t, depths, two_colour_images(K, q, t, depths, hc, wc)


def random_color_state(rng, shape, max_weight):
    """A prior colour state float32 [nz, ny, nx, 4]: finite colours (fractions included), weights 0, max_weight and values between."""
    color = rng.uniform(0, 255, tuple(shape) + (4,)).astype(np.float32)
    wc = rng.integers(0, int(max_weight) + 1, shape).astype(np.float32)
    pick = rng.random(shape)
    wc[pick < 0.25] = 0
    wc[pick > 0.8] = max_weight
    color[..., 3] = wc
    return color
