"""NumPy restatement of the coarse-to-fine part of the registration contract of include/f3d.h (f3d_depth_half, f3d_maps_half,
f3d_icp_levels) and of the pyramids segUtils/registration.py builds from them, operation for operation on top of tests/icp_ref.py and
tests/icp_color_ref.py: float64 arithmetic, every sum and division in the order the header writes it.  What the library returns must
equal this bit for bit.  Plus the corrugated scene on which a single level fails.
"""
import numpy as np

from oracle import np_ref as O
import icp_color_ref as CR
import icp_ref as I

MAX_LEVELS = 6


def four(a, h2, w2):
    """The four input pixels of every output pixel, in the header's order: (2v, 2u), (2v, 2u+1), (2v+1, 2u), (2v+1, 2u+1)."""
    return [a[0:2 * h2:2, 0:2 * w2:2], a[0:2 * h2:2, 1:2 * w2:2], a[1:2 * h2:2, 0:2 * w2:2], a[1:2 * h2:2, 1:2 * w2:2]]


def half_K(K):
    K = np.array(K, np.float64)
    K[:2] /= 2.0
    return K


def depth_half(depth, depth_scale, max_depth, gate):
    """-> float64 [h // 2, w // 2] of the header's f3d_depth_half."""
    depth = np.asarray(depth)
    h2, w2 = depth.shape[0] // 2, depth.shape[1] // 2
    with np.errstate(all='ignore'):
        d = [x.astype(np.float64) / np.float64(depth_scale) for x in four(depth, h2, w2)]
        ok = [(x > 0) & (x <= max_depth) for x in d]
        dmin = np.full((h2, w2), np.inf)
        for k in range(4):
            dmin = np.where(ok[k] & (d[k] < dmin), d[k], dmin)
        total, count = np.zeros((h2, w2)), np.zeros((h2, w2))
        for k in range(4):
            used = ok[k] & (d[k] - dmin <= gate)
            total = np.where(used, total + d[k], total)
            count = count + used
        return np.where(count > 0, total / np.where(count > 0, count, 1.0), 0.0)


def maps_half(vertex, normal, intensity, hm, wm, model_K, model_q, model_t, gate):
    """-> (vertex [hm2*wm2, 3], normal [hm2*wm2, 3], intensity [hm2*wm2] or None) of the header's f3d_maps_half."""
    hm2, wm2 = hm // 2, wm // 2
    mK, mt = np.asarray(model_K, np.float64), np.asarray(model_t, np.float64)
    V = four(np.asarray(vertex, np.float64).reshape(hm, wm, 3), hm2, wm2)
    N = four(np.asarray(normal, np.float64).reshape(hm, wm, 3), hm2, wm2)
    inten = None if intensity is None else four(np.asarray(intensity, np.float64).reshape(hm, wm), hm2, wm2)
    qinv = O.quat_inverse(np.asarray(model_q, np.float64))
    with np.errstate(all='ignore'):
        z, ok = [], []
        for k in range(4):
            cam = O.rotate(qinv, (V[k] - mt[None, None, :]).reshape(-1, 3)).reshape(hm2, wm2, 3)
            z.append((mK[2, 0] * cam[..., 0] + mK[2, 1] * cam[..., 1]) + mK[2, 2] * cam[..., 2])
            ok.append(np.isfinite(V[k]).all(axis=2) & np.isfinite(N[k]).all(axis=2) & (z[k] > 0))
        zmin = np.full((hm2, wm2), np.inf)
        for k in range(4):
            zmin = np.where(ok[k] & (z[k] < zmin), z[k], zmin)
        S, G, count = np.zeros((hm2, wm2, 3)), np.zeros((hm2, wm2, 3)), np.zeros((hm2, wm2))
        si, ci = np.zeros((hm2, wm2)), np.zeros((hm2, wm2))
        for k in range(4):
            used = ok[k] & (z[k] - zmin <= gate)
            S = np.where(used[..., None], S + V[k], S)
            G = np.where(used[..., None], G + N[k], G)
            count = count + used
            if inten is not None:
                seen = used & np.isfinite(inten[k])
                si = np.where(seen, si + inten[k], si)
                ci = ci + seen
        length = np.sqrt((G[..., 0] * G[..., 0] + G[..., 1] * G[..., 1]) + G[..., 2] * G[..., 2])
        good = (count > 0) & (length > 0) & np.isfinite(length)
        safe = np.where(count > 0, count, 1.0)
        vertex2 = np.where(good[..., None], S / safe[..., None], np.nan).reshape(-1, 3)
        normal2 = np.where(good[..., None], G / length[..., None], np.nan).reshape(-1, 3)
        inten2 = None if inten is None else np.where(ci > 0, si / np.where(ci > 0, ci, 1.0), np.nan).reshape(-1)
    return vertex2, normal2, inten2


def level_min_pairs(min_pairs, level):
    return max(6, min_pairs >> (2 * level))


def pyramid(depth, K, depth_scale, max_depth, vertex, normal, intensity, hm, wm, model_K, model_q, model_t, max_dist, gate, rounds, min_pairs):
    """The levels registration.icp builds, coarsest first: `rounds` holds the rounds per level, finest first.  Each level is a dict with
    the keys icp_levels reads."""
    levels, K, mK = [], np.asarray(K, np.float64), np.asarray(model_K, np.float64)
    for l, iterations in enumerate(rounds):
        if l:
            depth, depth_scale = depth_half(depth, depth_scale, max_depth, gate), 1.0
            vertex, normal, intensity = maps_half(vertex, normal, intensity, hm, wm, mK, model_q, model_t, gate)
            K, mK, hm, wm = half_K(K), half_K(mK), hm // 2, wm // 2
        levels.append(dict(depth=depth, K=K, depth_scale=depth_scale, model_vertex=vertex, model_normal=normal, model_intensity=intensity, hm=hm, wm=wm,
                           model_K=mK, model_q=model_q, model_t=model_t, max_dist=max_dist, iterations=iterations,
                           min_pairs=level_min_pairs(min_pairs, l)))
    return levels[::-1]


def icp_levels(levels, q, t, max_depth, rgb=None, color_weight=None):
    """-> (pose float64 [7], stats float64 [sum of iterations, 3 or 5], status) of the header's f3d_icp_levels: one icp_ref.icp (or
    icp_color_ref.icp_color) call per level from the pose the call before returned, the stats rows concatenated; once a call is lost
    the pose stays and every later row is {0, 0, 1} (with colour {0, 0, 1, 0, 0})."""
    assert 1 <= len(levels) <= MAX_LEVELS
    pose, rows, lost = np.concatenate([np.asarray(q, np.float64), np.asarray(t, np.float64)]), [], False
    width = 3 if rgb is None else 5
    for lv in levels:
        if lost:
            block = np.zeros((lv['iterations'], width))
            block[:, 2] = I.LOST
            rows.append(block)
            continue
        model = (lv['hm'], lv['wm'], lv['model_K'], lv['model_q'], lv['model_t'], lv['max_dist'])
        if rgb is None:
            pose, stats, status = I.icp(lv['depth'], lv['K'], pose[:4], pose[4:], lv['depth_scale'], max_depth, lv['model_vertex'], lv['model_normal'],
                                        *model, lv['iterations'], lv['min_pairs'])
        else:
            pose, stats, status = CR.icp_color(lv['depth'], rgb, lv['K'], pose[:4], pose[4:], lv['depth_scale'], max_depth, lv['model_vertex'],
                                               lv['model_normal'], lv['model_intensity'], *model, color_weight, lv['iterations'], lv['min_pairs'])
        rows.append(stats)
        lost = status == I.LOST
    return pose, np.concatenate(rows), I.LOST if lost else I.OK


# ------------------------------------------------------------------------------------------------ the corrugated scene
# A bump on a wall that carries a corrugation of period 0.08 m and amplitude 0.015 m: 5.9 pixels per period at 1.5 m, which projective
# ICP at full resolution locks onto one period off.  The model camera sits at the origin with the identity rotation.
CH, CW, CMAX_DEPTH = 96, 128, 4.0
CK = np.array([[110.0, 0.0, 64.0], [0.0, 110.0, 48.0], [0.0, 0.0, 1.0]])
PERIOD, AMPLITUDE = 0.08, 0.015
START_AXIS, START_SHIFT = (0.3, 0.8, 0.5), np.array([1.0, 0.3, 0.2])
IDENT = np.array([1.0, 0.0, 0.0, 0.0])


def surface(x, y):
    """z(x, y) of the scene and its two partial derivatives."""
    k = 2.0 * np.pi / PERIOD
    bump = 0.3 * np.exp(-((x - 0.1) ** 2 + (y + 0.05) ** 2) / (2.0 * 0.25 ** 2))
    z = 1.5 - bump + AMPLITUDE * np.sin(k * x) * np.cos(k * y)
    zx = bump * (x - 0.1) / 0.25 ** 2 + AMPLITUDE * k * np.cos(k * x) * np.cos(k * y)
    zy = bump * (y + 0.05) / 0.25 ** 2 - AMPLITUDE * k * np.sin(k * x) * np.sin(k * y)
    return z, zx, zy


def corrugated_scene():
    """depth float64 [CH, CW] rendered per pixel centre by the fixed point d <- z(rx d, ry d), 200 times from 1.5; the analytic vertex
    and normal maps [CH*CW, 3] (normals towards the camera); K; the model pose (identity)."""
    vv, uu = np.meshgrid(np.arange(CH, dtype=np.float64), np.arange(CW, dtype=np.float64), indexing='ij')
    rx, ry = ((uu + 0.5) - CK[0, 2]) / CK[0, 0], ((vv + 0.5) - CK[1, 2]) / CK[1, 1]
    d = np.full((CH, CW), 1.5)
    for _ in range(200):
        d = surface(rx * d, ry * d)[0]
    _, zx, zy = surface(rx * d, ry * d)
    normal = np.stack([zx, zy, -np.ones_like(zx)], axis=-1)
    normal /= np.linalg.norm(normal, axis=-1, keepdims=True)
    vertex = np.stack([rx * d, ry * d, d], axis=-1)
    return dict(K=CK.copy(), depth=d, vertex=vertex.reshape(-1, 3), normal=normal.reshape(-1, 3), q=IDENT.copy(), t=np.zeros(3))


def corrugated_start(shift, degrees):
    """The start pose: the true one (identity) rotated by `degrees` about START_AXIS and moved by `shift` metres along START_SHIFT."""
    return I.moved(IDENT, np.zeros(3), START_AXIS, degrees, START_SHIFT * (shift / np.linalg.norm(START_SHIFT)))


def corrugated_run(scene, start, rounds, max_dist=0.1, min_pairs=50, gate=None):
    """icp_levels on the scene from `start` with `rounds` per level, finest first -> (pose, stats, status)."""
    s = scene
    levels = pyramid(s['depth'], s['K'], 1.0, CMAX_DEPTH, s['vertex'], s['normal'], None, CH, CW, s['K'], s['q'], s['t'], max_dist,
                     max_dist if gate is None else gate, rounds, min_pairs)
    return icp_levels(levels, start[0], start[1], CMAX_DEPTH)


def pose_error(pose):
    """(metres, radians) between a pose and the scene's true one."""
    return float(np.linalg.norm(pose[4:])), I.rotation_angle(pose[:4], IDENT)
