"""Test-only NumPy restatement of the feature fusion contract of include/f3d.h (f3d_fuse_features, f3d_features_finalize), on top of
tests/render_ref.py: the samples, the depth keys and the visibility rule are those of render_ref.visible_votes, the payload is a
feature row instead of a label."""
import numpy as np

from render_ref import _views, unpack


def feature_pixel(u, v, hw, fhw):
    """(uf, vf) of the samples at (u, v): uf = u * wf // w, vf = v * hf // h in int64."""
    (h, w), (hf, wf) = hw, fhw
    return np.asarray(u, np.int64) * wf // w, np.asarray(v, np.int64) * hf // h


def visible_samples(points, K, wxyzs, translations, hw, max_depth=10, splat=1, depth_tol=0.05):
    """Per view in ascending order, (j, idx, u, v) of the samples within depth_tol of the front surface of their pixel, exactly as
    render_ref.visible_votes takes them.  It does not depend on the features: tests compute it once per scene."""
    H, W = hw
    out = []
    if not len(translations):
        return out
    for j, (idx, u, v, z32), zkey in _views(points, K, wxyzs, translations, H, W, max_depth, splat):
        zmin32 = unpack(zkey)[0][v * W + u]
        with np.errstate(invalid='ignore'):
            vis = z32.astype(np.float64) <= zmin32.astype(np.float64) + np.float64(depth_tol)
        out.append((j, idx[vis], u[vis], v[vis]))
    return out


def fuse(points, K, wxyzs, translations, feats, hw, max_depth=10, splat=1, depth_tol=0.05, sums=None, counts=None, visible=None):
    """(sums float32 [N, d], counts int32 [N]): per view in ascending order, sums[i] = float32(sums[i] + float32(feats[j, vf, uf])) and
    counts[i] += 1 for every visible sample.  sums / counts continue an accumulation (copies); visible = visible_samples(...) of the
    same scene, when the caller already has it."""
    feats = np.asarray(feats)
    V, hf, wf, d = feats.shape
    sums = np.zeros((len(points), d), np.float32) if sums is None else np.array(sums, np.float32)
    counts = np.zeros(len(points), np.int32) if counts is None else np.array(counts, np.int32)
    if visible is None:
        visible = visible_samples(points, K, wxyzs, translations, hw, max_depth, splat, depth_tol)
    for j, idx, u, v in visible:
        uf, vf = feature_pixel(u, v, hw, (hf, wf))
        with np.errstate(over='ignore', invalid='ignore'):
            sums[idx] = sums[idx] + feats[j, vf, uf].astype(np.float32)              # the indices are unique per view; float32 add
        counts[idx] += 1
    return sums, counts


def finalize(sums, counts, normalize=True):
    """float32 [N, d]: m = sums / float32(count) (zeros for count 0); with normalize, m / sqrt(sum of the float64 squares) rounded to
    float32 (zeros when the sum is 0)."""
    sums, counts = np.asarray(sums, np.float32), np.asarray(counts)
    seen = counts > 0
    m = np.zeros_like(sums)
    with np.errstate(over='ignore', invalid='ignore'):
        m[seen] = sums[seen] / counts[seen].astype(np.float32)[:, None]                # float32 / float32: correctly rounded
    if not normalize:
        return m
    m64 = m.astype(np.float64)
    with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
        s = np.sum(m64 * m64, axis=1)
        out = (m64 / np.sqrt(s)[:, None]).astype(np.float32)
    out[s == 0] = 0
    return out


def one_hot(masks, ncols, dtype=np.float32):
    """[V, H, W, ncols] maps with a 1 in channel masks[j, v, u]."""
    masks = np.asarray(masks)
    out = np.zeros(masks.shape + (ncols,), dtype)
    np.put_along_axis(out, masks[..., None].astype(np.int64), 1, axis=-1)
    return out
