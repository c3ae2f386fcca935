"""Feature fusion: per-point pooling of per-pixel feature maps over the views that see the point (no reference counterpart).

The reference, and every other 2D -> 3D path here, moves one byte per pixel: the argmax of the 2D network.  The network produces
more: ``[C, H, W]`` logits or probabilities, and open-vocabulary models produce a per-pixel embedding that is compared with text
embeddings afterwards.  ``fuse_features`` pools such maps onto the cloud: every sample of a point that a view really sees (the
occlusion test of ``project_vote_argmax_visible``) adds the feature row of its pixel to the point's row of sums
(f3d_fuse_features, include/f3d.h states the contract; tests/features_ref.py restates it in NumPy).  The means are soft votes
(``soft_votes`` -> ``segment_votes`` / ``VotingSegmentation.segment(votes=...)``) or pooled embeddings (``classify_features``).

The maps are channel-last, ``[V, hf, wf, d]``, float16 or float32, at any resolution: a sample taken at ``hw`` reads the nearest
feature pixel.  The feature maps of a real capture do not fit in memory at once: ``FeatureFusion.add`` takes them in chunks, and
the result does not depend on how they were cut.

NumPy arrays in, NumPy arrays back; device tensors for ``points`` or ``features`` in, device tensors back, with no host round trip.
"""
import numpy as np

import f3d
from f3d.tensors import device_points, dtype_code, on_device, torch_device, upload, work_stream

__all__ = ['fuse_features', 'FeatureFusion', 'soft_votes', 'classify_features']


def _is_tensor(a):
    return hasattr(a, 'is_cuda')


def _image_size(features, hw):
    if not hasattr(features, 'shape') or len(features.shape) != 4:
        raise ValueError('features must be [V, hf, wf, d] (channel-last)')
    H, W = (int(x) for x in (features.shape[1:3] if hw is None else hw))
    if H < 1 or W < 1:
        raise ValueError(f'hw must be positive, got {(H, W)}')
    return H, W


def _fuse(points, K, wxyzs, translations, features, H, W, max_depth, splat, depth_tol, sums, counts):
    """One call of f3d_fuse_features on the host or the device route; `sums` / `counts` None = start from zeros."""
    if not hasattr(features, 'dtype'):
        features = np.asarray(features)
    V, d = int(features.shape[0]), int(features.shape[3])
    npts = int(points.shape[0]) if hasattr(points, 'shape') else len(points)
    device = on_device(points) or on_device(features) or on_device(sums)
    if (sums is None) != (counts is None):
        raise ValueError('sums and counts come together')
    if sums is None and not 1 <= d <= f3d.FEAT_MAX_D:
        raise ValueError(f'd must be in [1, {f3d.FEAT_MAX_D}], got {d}')
    if not device:
        features = np.asarray(features)
        if sums is None:
            sums, counts = np.zeros((npts, d), np.float32), np.zeros(npts, np.int32)
        f3d.features_check(sums, counts, features if features.flags.c_contiguous else np.ascontiguousarray(features), len(translations), npts)
        views = f3d.views_build(K, W, H, wxyzs, translations, max_depth)
        return f3d.default_context().fuse_features(sums, counts, points, views, H, W, np.ascontiguousarray(features), splat, depth_tol)
    if sums is not None:
        if not (on_device(sums) and on_device(counts)):
            raise TypeError('sums and counts must be device tensors when points or features are')
        f3d.features_check(sums, counts, None, None, npts)
    if str(features.dtype).replace('torch.', '') not in ('float16', 'float32'):
        raise TypeError(f'features must be float16 or float32, got {features.dtype}')
    if V != len(translations):
        raise ValueError(f'{len(translations)} views for {V} feature maps')
    ctx = f3d.default_context()
    torch, dev = torch_device(ctx, 'fuse_features')
    views = f3d.views_build(K, W, H, wxyzs, translations, max_depth)
    pts = device_points(points, dev, 'points')
    feats = (features if _is_tensor(features) else torch.from_numpy(np.ascontiguousarray(features))).to(dev).contiguous()
    with torch.cuda.device(dev), work_stream(dev) as work:
        fresh = sums is None
        if fresh:
            sums = torch.zeros((npts, d), dtype=torch.float32, device=dev)
            counts = torch.zeros(npts, dtype=torch.int32, device=dev)
        ft = f3d.features_check(sums, counts, feats, len(views), len(pts))
        dviews = upload(views, dev)
        ctx.fuse_features_dev(pts.data_ptr(), dtype_code(pts), len(pts), dviews.data_ptr(), V, H, W, feats.data_ptr(), ft,
                              int(feats.shape[1]), int(feats.shape[2]), d, splat, depth_tol, sums.data_ptr(), counts.data_ptr(), 0,
                              work.cuda_stream)
    if fresh:
        for t in (sums, counts):                                             # allocated on the work stream, handed to the caller's
            t.record_stream(torch.cuda.current_stream(dev))
    return sums, counts


def fuse_features(points, K, wxyzs, translations, features, hw=None, max_depth=10, splat=1, depth_tol=0.05, sums=None, counts=None):
    """Pools per-pixel feature maps onto the cloud -> (sums float32 [N, d], counts int32 [N]).

    points [N, 3] (float64 or float32), K [3, 3], wxyzs [V, 4] camera->world (w, x, y, z), translations [V, 3], features float16 /
    float32 [V, hf, wf, d], one channel-last map per view.  ``hw`` = (H, W), the image size the frustum, the samples and the
    z-buffer are taken at (the size K belongs to); it defaults to the feature maps' own size.  Per view the samples are those of
    ``project_vote_argmax_visible``; a sample counts iff its depth is within ``depth_tol`` of the nearest depth the cloud renders
    into its pixel (``splat``), ``depth_tol=inf`` takes every sample.  Its feature pixel is (v * hf // H, u * wf // W).

    ``sums`` / ``counts`` continue an earlier accumulation, in place; the float32 adds happen in ascending view order, so cutting
    the views into calls changes nothing, bit for bit (f3d.h, f3d_fuse_features).  ``sums / counts`` is the mean: ``FeatureFusion``
    does the bookkeeping.  NumPy in, NumPy out; a torch device tensor for ``points`` or ``features`` gives device tensors, ordered
    with torch's current stream."""
    H, W = _image_size(features, hw)
    return _fuse(points, K, wxyzs, translations, features, H, W, max_depth, splat, depth_tol, sums, counts)


class FeatureFusion:
    """Running feature pooling of one cloud: ``add`` a chunk of views and their feature maps as often as needed, then read
    ``features()`` (mean rows, unit length by default) or ``counts``.  ``hw`` = (H, W) as in ``fuse_features``; the channel count is
    fixed by the first ``add``.  The state lives where the cloud lives: NumPy arrays for a NumPy cloud, device tensors for a device
    tensor."""

    def __init__(self, points, hw, max_depth=10, splat=1, depth_tol=0.05):
        if not hasattr(points, 'shape') or len(points.shape) != 2 or points.shape[1] != 3:
            raise ValueError('points must be [N, 3]')
        self.points = points
        self.hw = tuple(int(x) for x in hw)
        if len(self.hw) != 2 or min(self.hw) < 1:
            raise ValueError(f'hw must be (H, W), got {hw}')
        self.max_depth, self.splat, self.depth_tol = max_depth, splat, depth_tol
        self.sums = self.counts = None

    def add(self, K, wxyzs, translations, features):
        """The views of one chunk: K [3, 3], wxyzs [C, 4], translations [C, 3], features [C, hf, wf, d].  -> self"""
        _image_size(features, self.hw)
        if self.sums is not None and int(features.shape[3]) != int(self.sums.shape[1]):
            raise ValueError(f'features has {int(features.shape[3])} channels, the earlier chunks {int(self.sums.shape[1])}')
        if self.sums is None and on_device(features) and not on_device(self.points):     # the state follows the first chunk
            self.points = device_points(self.points, features.device, 'points')
        self.sums, self.counts = _fuse(self.points, K, wxyzs, translations, features, *self.hw, self.max_depth, self.splat, self.depth_tol,
                                       self.sums, self.counts)
        return self

    def features(self, normalize=True):
        """float32 [N, d]: the mean feature row of every point, scaled to unit length with ``normalize``; zeros where no view saw
        the point (f3d.h, f3d_features_finalize)."""
        if self.sums is None:
            raise ValueError('no features were added')
        ctx = f3d.default_context()
        if not on_device(self.sums):
            return ctx.features_finalize(self.sums, self.counts, normalize)
        torch, dev = torch_device(ctx, 'FeatureFusion.features')
        with torch.cuda.device(dev), work_stream(dev) as work:
            out = torch.empty_like(self.sums)
            ctx.features_finalize_dev(self.sums.data_ptr(), self.counts.data_ptr(), self.sums.shape[0], self.sums.shape[1], normalize,
                                      out.data_ptr(), work.cuda_stream)
        out.record_stream(torch.cuda.current_stream(dev))
        return out


def soft_votes(sums):
    """Sums of per-class probabilities (or logits) as float64 [N, d] votes, the layout of ``VotingSegmentation``: ready for
    ``f3d.Context.segment_votes`` or ``VotingSegmentation.segment(votes=...)``.  With one-hot maps they are the hard votes."""
    if _is_tensor(sums):
        import torch
        return sums.to(torch.float64)
    return np.asarray(sums).astype(np.float64)


def classify_features(features, text_embeddings, chunk=1 << 18, counts=None):
    """Open-vocabulary labels of pooled embeddings -> (labels int64 [N], best score float32 [N]).

    features float32 [N, d] (``FeatureFusion.features()``), text_embeddings [T, d]: the score of (point, text) is their dot
    product, a cosine when both are unit length.  A point no view saw -- count 0 when ``counts`` is given, otherwise an all-zero
    row -- gets label -1 and score 0.  The products are one ``torch.matmul`` per ``chunk`` points on the context's device (the
    GEMM library's work, not a kernel of this project).  NumPy in, NumPy out; device tensors in, device tensors out."""
    if len(features.shape) != 2 or len(text_embeddings.shape) != 2 or features.shape[1] != text_embeddings.shape[1]:
        raise ValueError(f'features must be [N, d] and text_embeddings [T, d], got {tuple(features.shape)} and {tuple(text_embeddings.shape)}')
    if int(text_embeddings.shape[0]) < 1:
        raise ValueError('text_embeddings must hold at least one row')
    if counts is not None and tuple(counts.shape) != (int(features.shape[0]),):
        raise ValueError(f'counts must be [{int(features.shape[0])}], got {tuple(counts.shape)}')
    if int(chunk) < 1:
        raise ValueError('chunk must be positive')
    device = on_device(features)
    torch, dev = torch_device(f3d.default_context(), 'classify_features')
    to_t = lambda a: a if _is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))   # noqa: E731
    with torch.cuda.device(dev):
        f = to_t(features).to(dev, torch.float32)
        t = to_t(text_embeddings).to(dev, torch.float32).t().contiguous()
        seen = to_t(counts).to(dev) > 0 if counts is not None else None
        labels = torch.empty(len(f), dtype=torch.int64, device=dev)
        best = torch.empty(len(f), dtype=torch.float32, device=dev)
        for a in range(0, len(f), int(chunk)):
            rows = f[a:a + int(chunk)]
            score, arg = torch.matmul(rows, t).max(dim=1)
            ok = seen[a:a + int(chunk)] if seen is not None else (rows != 0).any(dim=1)
            labels[a:a + int(chunk)] = torch.where(ok, arg, torch.full_like(arg, -1))
            best[a:a + int(chunk)] = torch.where(ok, score, torch.zeros_like(score))
    return (labels, best) if device else (labels.cpu().numpy(), best.cpu().numpy())
