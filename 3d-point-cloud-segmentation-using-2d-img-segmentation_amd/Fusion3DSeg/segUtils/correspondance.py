"""Drop-in surface of the reference's Fusion3DSeg/segUtils/correspondance.py: pixel <-> fused point lookups.

``PointCorrespondance`` (reference :162-283) maps every pixel of every frame to the fused points within ``radius`` of it.  Its
``merge_maps`` -- ``KDTree(dense, leaf_size=2).query_radius(sparse, r)`` inverted by a Python double loop in the reference -- is
built on the GPU by the radius query of libf3d_hip (f3d.h ``f3d_radius_query_*``) and held as CSR (``offsets`` int64 [N+1],
``indices`` int32); rows list sparse indices in ascending order, the order the reference's loop appends them in.  The reference's
object array is made on first access of ``merge_maps`` only (``save`` needs it), by the same ``np.array(..., dtype=object)`` call,
so a map whose rows all have the same length is a 2-D object array there as well.  ``get_point`` works on the CSR.

Given torch device tensors (say the frames of ``frames_world_dev`` and the cloud of ``Fusion.fuse_device``), the lookup tables and
the CSR stay on the device and ``get_point`` takes and returns device tensors.  There is no CPU fallback.

``Correspondance`` (reference :18-160) is the host NumPy class; its scatter of the merge maps into the pixel images is vectorised.

Not ported: the ``viz_proj`` / ``viz_reproj`` helpers (they need cv2 / open3d).

The lookup tables are the reference's, quirks included: ``pcd2xy`` is the per-frame (x, y) table stacked side by side, int64
[h*w, 2*nframes] (``np.hstack`` of 2-D arrays), ``imgids`` int64 [nframes*h*w], ``pcdimgs`` int32 [nframes, h, w].
"""
import pickle
from typing import NamedTuple

import numpy as np

import f3d
from f3d.tensors import dtype_code, on_device, torch_device, work_stream


class CSR(NamedTuple):
    """Rows of a merge map: row p = ``indices[offsets[p]:offsets[p + 1]]`` (NumPy arrays or torch tensors)."""
    offsets: object
    indices: object


def _csr_of(merge_maps):
    """The reference's merge maps (object array, 1-D of lists or 2-D, or a list of lists) -> CSR on the host."""
    if isinstance(merge_maps, CSR):
        return merge_maps
    m = np.asarray(merge_maps, dtype=object) if not isinstance(merge_maps, np.ndarray) else merge_maps
    if m.ndim == 2:                                      # every row has m.shape[1] entries
        n, k = m.shape
        return CSR(np.arange(n + 1, dtype=np.int64) * k, m.astype(np.int64).reshape(-1).astype(np.int32))
    rows = [np.asarray(r, dtype=np.int64).reshape(-1) for r in m]
    offs = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=offs[1:])
    idx = np.concatenate(rows).astype(np.int32) if rows else np.zeros(0, np.int32)
    return CSR(offs, idx)


def _objects(csr):
    """CSR -> the reference's ``np.array(merge_maps, dtype=object)`` (lists of Python ints)."""
    offs, idx = csr
    if on_device(offs):
        offs, idx = offs.cpu().numpy(), idx.cpu().numpy()
    flat = idx.tolist()
    o = offs.tolist()
    return np.array([flat[o[p]:o[p + 1]] for p in range(len(o) - 1)], dtype=object)


def _rows(idx, n):
    """NumPy indexing of n rows by idx: negative indices wrap, out-of-range ones raise IndexError."""
    idx = np.asarray(idx)
    if idx.dtype == object or not np.issubdtype(idx.dtype, np.integer):
        raise IndexError('only integers are valid row indices')
    idx = idx.astype(np.int64).reshape(-1)
    bad = (idx < -n) | (idx >= n)
    if bad.any():
        raise IndexError(f'index {int(idx[bad][0])} is out of bounds for axis 0 with size {n}')
    return np.where(idx < 0, idx + n, idx)


def _gather(csr, idx):
    """(concatenated rows idx of csr as int32, row lengths int64) on the host."""
    offs, nb = csr
    if idx.size == 0:
        raise ValueError('need at least one array to concatenate')     # np.hstack of no rows (reference :269)
    start = offs[idx]
    lens = offs[idx + 1] - start
    total = int(lens.sum())
    pos = np.repeat(start - (np.cumsum(lens) - lens), lens) + np.arange(total, dtype=np.int64)
    return nb[pos].astype(np.int32), lens.astype(np.int64)


def _points(a, name):
    p = np.asarray(a)
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError(f'{name} must be [N,3], got {p.shape}')
    if len(p) == 0:
        raise ValueError(f'{name}: found an array with 0 sample(s) (sklearn raises ValueError)')
    if p.dtype != np.float32:
        p = p.astype(np.float64)
    if not np.isfinite(p).all():
        raise ValueError(f'{name} contains NaN or infinity (sklearn raises ValueError)')
    return p


def _radius(radius):
    r = float(radius)
    if r == float('inf'):
        raise ValueError('radius = +inf is not supported (sklearn would return every pair)')
    return r


class PointCorrespondance:
    def __init__(self, sparse_points, dense_points, radius, nframes, depth_hw, load=None):
        """sparse_points [M,3] (the fused cloud), dense_points [N,3] (every pixel of every frame, N = nframes*h*w), radius,
        nframes, depth_hw = (h, w); or load = a .pkl file written by ``save`` (or by the reference).  NumPy inputs -> NumPy
        tables and CSR; torch device tensors -> everything stays on the device."""
        self._maps = None
        self._csr = None
        if load is not None:
            with open(load, 'rb') as fp:
                args = pickle.load(fp)
            self.pcdimgs, self.pcd2xy, self.imgids, self.merge_maps, self.nframes = args
            return
        if hasattr(sparse_points, 'is_cuda') or hasattr(dense_points, 'is_cuda'):        # torch tensors; CPU ones are uploaded
            self._init_device(sparse_points, dense_points, radius, nframes, depth_hw)
            return
        pcd2xy, imgids, pcdimgs = self.get_lookups(nframes, depth_hw)
        self.pcdimgs = pcdimgs
        self.pcd2xy = pcd2xy
        self.imgids = imgids
        self._csr = self.get_merge_csr(sparse_points, dense_points, radius)
        self.nframes = nframes

    def _init_device(self, sparse_points, dense_points, radius, nframes, depth_hw):
        ctx = f3d.default_context()
        torch, dev = torch_device(ctx, 'PointCorrespondance on tensors')
        h, w = (int(x) for x in depth_hw)
        hw, F = h * w, int(nframes)
        i64 = dict(dtype=torch.int64, device=dev)
        xy = torch.stack([torch.arange(w, **i64).repeat(h), torch.arange(h, **i64).repeat_interleave(w)], 1)
        self.pcd2xy = xy.repeat(1, F)                                       # [h*w, 2*nframes], as np.hstack makes it
        self.imgids = torch.arange(F, **i64).repeat_interleave(hw)
        self.pcdimgs = torch.arange(F * hw, dtype=torch.int32, device=dev).reshape(F, h, w)
        self._csr = self._merge_csr_device(ctx, torch, dev, sparse_points, dense_points, radius)
        self.nframes = nframes

    @staticmethod
    def _merge_csr_device(ctx, torch, dev, sparse_points, dense_points, radius):
        r = _radius(radius)

        def prep(a, name):
            t = torch.as_tensor(a).to(dev)
            if t.dim() != 2 or t.shape[1] != 3:
                raise ValueError(f'{name} must be [N,3], got {tuple(t.shape)}')
            if t.shape[0] == 0:
                raise ValueError(f'{name}: found an array with 0 sample(s) (sklearn raises ValueError)')
            if t.dtype != torch.float32:
                t = t.to(torch.float64)
            return t.contiguous()
        s = prep(sparse_points, 'sparse_points')
        d = prep(dense_points, 'dense_points')
        offs = torch.empty(len(d) + 1, dtype=torch.int64, device=dev)
        with work_stream(dev) as work:                                      # the count is read back: complete when this returns
            nnz = ctx.radius_query_dev(s.data_ptr(), dtype_code(s), len(s), d.data_ptr(), dtype_code(d), len(d), r, offs.data_ptr(),
                                       work.cuda_stream)
        nb = torch.empty(nnz, dtype=torch.int32, device=dev)                # between the blocks: memory of the caller's stream
        if nnz:
            with work_stream(dev) as work:
                ctx.radius_query_fill_dev(d.data_ptr(), dtype_code(d), len(d), offs.data_ptr(), nb.data_ptr(), work.cuda_stream)
        return CSR(offs, nb)

    @classmethod
    def get_xys(cls, h, w):
        """int64 [h*w, 2]: (x, y) of every pixel in row-major order (reference :188-202)."""
        xs = np.tile(np.arange(w), h)
        ys = np.repeat(np.arange(h), w)
        return np.vstack((xs, ys)).T.copy()

    @classmethod
    def get_lookups(cls, nframes, depth_hw):
        """(pcd2xy int64 [h*w, 2*nframes], imgids int64 [nframes*h*w], pcdimgs int32 [nframes, h, w]) (reference :204-232)."""
        h, w = depth_hw
        hw = h * w
        pcd2xy = cls.get_xys(h, w)
        pcdimg = np.arange(hw, dtype=np.int32).reshape(h, w)
        pcdimgs = np.stack([pcdimg + i * hw for i in range(nframes)])
        pcd2xys = np.hstack([pcd2xy for _ in range(nframes)])
        imgids = np.hstack([np.full(hw, i, dtype=int) for i in range(nframes)])
        return pcd2xys, imgids, pcdimgs

    @classmethod
    def get_merge_csr(cls, sparse_points, dense_points, radius=0.1):
        """The merge maps as CSR on the GPU: row p lists, ascending, every sparse index within radius of dense point p."""
        r = _radius(radius)
        d = _points(dense_points, 'dense_points')                           # the tree's data is checked first
        s = _points(sparse_points, 'sparse_points')
        offs, nb = f3d.default_context().radius_query(s, d, r)
        return CSR(offs, nb)

    @classmethod
    def get_merge_maps(cls, sparse_points, dense_points, radius=0.1):
        """The reference's object array (reference :234-242)."""
        return _objects(cls.get_merge_csr(sparse_points, dense_points, radius))

    @property
    def csr(self):
        """The merge maps as CSR (offsets int64 [N+1], indices int32), NumPy or device tensors."""
        return self._csr

    @property
    def merge_maps(self):
        if self._maps is None:
            self._maps = _objects(self._csr)
        return self._maps

    @merge_maps.setter
    def merge_maps(self, value):
        self._maps = None if isinstance(value, CSR) else value
        self._csr = _csr_of(value)

    def save(self, filename):
        """Pickle (pcdimgs, pcd2xy, imgids, merge_maps, nframes) as the reference does (device tables are saved as NumPy)."""
        host = [t.cpu().numpy() if on_device(t) else t for t in (self.pcdimgs, self.pcd2xy, self.imgids)]
        with open(filename, 'wb') as fp:
            pickle.dump((host[0], host[1], host[2], self.merge_maps, self.nframes), fp)

    def get_point(self, images, coords):
        """images [k] frame ids, coords [k, 2] (x, y) -> (indices int32 [p], frequency int64 [k]): the cloud points of every
        queried pixel, concatenated, and how many each pixel has (reference :253-271; NumPy indexing: negative coordinates
        wrap, out-of-range ones raise IndexError)."""
        if on_device(self._csr.offsets):
            return self._get_point_device(images, coords)
        x, y = np.asarray(coords).T
        indices = self.pcdimgs[images, y, x]
        return _gather(self._csr, _rows(indices, len(self._csr.offsets) - 1))

    def _get_point_device(self, images, coords):
        import torch
        offs, nb = self._csr
        dev = offs.device
        c = torch.as_tensor(coords).to(dev).to(torch.int64)
        img = torch.as_tensor(images).to(dev).to(torch.int64)
        img, x, y = torch.broadcast_tensors(img, c[..., 0], c[..., 1])
        dims = self.pcdimgs.shape
        parts = []
        for v, n in zip((img, y, x), dims):                                 # NumPy's rules, checked before any device gather
            bad = (v < -n) | (v >= n)
            if bool(bad.any()):
                raise IndexError(f'index {int(v[bad][0])} is out of bounds for an axis with size {n}')
            parts.append(torch.where(v < 0, v + n, v))
        rows = self.pcdimgs[parts[0], parts[1], parts[2]].reshape(-1).to(torch.int64)
        if rows.numel() == 0:
            raise ValueError('need at least one array to concatenate')
        start = offs[rows]
        lens = offs[rows + 1] - start
        total = int(lens.sum())
        base = torch.repeat_interleave(start - (torch.cumsum(lens, 0) - lens), lens, output_size=total)
        return nb[base + torch.arange(total, dtype=torch.int64, device=dev)], lens


class Correspondance:
    def __init__(self, pcdimgs, invalids, imgids, pcd2xy, merge_maps, depth_hw, load=None):
        """pcdimgs [M, H, W] (written in place, as in the reference), invalids bool [N], imgids [N], pcd2xy [N, 2],
        merge_maps: one list of dense indices per sparse point (the reference's form) or a ``CSR`` pair, depth_hw; or load =
        a .pkl file.  Pixel values: the largest sparse index whose list covers the pixel, -1 where that list covers it with
        an invalid point (reference :44-49)."""
        if load is not None:
            with open(load, 'rb') as fp:
                args = pickle.load(fp)
            self.pcdimgs, self.pcd2xy, self.imgids, self.merge_maps, self.nframes = args
            return
        nframes = len(pcdimgs)
        offs, nb = _csr_of(merge_maps)
        dense = nb.astype(np.int64)
        sparse = np.repeat(np.arange(len(offs) - 1, dtype=np.int64), np.diff(offs))
        if len(dense):
            xs, ys = pcd2xy[dense].T
            ids = imgids[dense]
            invs = np.asarray(invalids[dense], dtype=bool)
            F, H, W = pcdimgs.shape
            pix = (_rows(ids, F) * H + _rows(ys, H)) * W + _rows(xs, W)
            # the last write of the reference's loop: largest sparse index, and -1 if that list holds an invalid point there
            order = np.lexsort((invs, sparse, pix))
            p, s, v = pix[order], sparse[order], invs[order]
            last = np.ones(len(p), bool)
            last[:-1] = p[1:] != p[:-1]
            pcdimgs.reshape(-1)[p[last]] = np.where(v[last], -1, s[last])
        self.pcdimgs = pcdimgs
        self.pcd2xy = pcd2xy
        self.imgids = imgids
        self.merge_maps = merge_maps
        self.nframes = nframes

    def save(self, filename):
        with open(filename, 'wb') as fp:
            pickle.dump((self.pcdimgs, self.pcd2xy, self.imgids, self.merge_maps, self.nframes), fp)

    def get_point(self, images, coords):
        """images [k], coords [k, 2] (x, y) -> the sparse index of every queried pixel (reference :68-82)."""
        x, y = np.asarray(coords).T
        return self.pcdimgs[images, y, x]

    def _row(self, i):
        if isinstance(self.merge_maps, CSR):
            offs, nb = self.merge_maps
            i = int(_rows([i], len(offs) - 1)[0])
            return nb[offs[i]:offs[i + 1]].astype(np.int64)
        return self.merge_maps[i]

    def get_pixel(self, idx):
        """Sparse point index (int or list) -> (image ids, (x, y) coordinates) of the dense points merged into it (reference :84-104)."""
        if isinstance(idx, int):
            indices = self._row(idx)
        else:
            indices = np.hstack([self._row(i) for i in idx])
        return self.imgids[indices], self.pcd2xy[indices]
