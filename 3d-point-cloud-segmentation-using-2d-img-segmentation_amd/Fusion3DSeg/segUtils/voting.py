"""Drop-in for the reference's Fusion3DSeg/segUtils/voting.py (classes VotingSegmentation and PointVotingSegmentation).

Same constructor, attributes, methods, return types and quirks (reference file:line in each
method); the scatter vote and the segmentation run as HIP kernels (f3d_vote_uv2pt*, f3d_segment_votes*), and so does
the radius search fused with the frame vote of PointVotingSegmentation (f3d_point_vote_frames*).
``smooth_votes`` / ``smooth_segment`` (no reference counterpart) put a spatial prior between a vote and the instance split: every
row becomes the sum of itself and its neighbours' rows over an adjacency (f3d_smooth_votes / f3d_smooth_segment, include/f3d.h).
The vote matrix stays on the GPU for the whole ``vote()`` loop and is downloaded once.
OpenCV is optional: masks are read with cv2 when it is importable, else with Pillow, and the
nearest-neighbour resize is done here (same index rule as cv2.INTER_NEAREST).
"""
import math
import os
from pathlib import Path

import numpy as np

import f3d
from f3d.tensors import CSR_ADJACENCY, device_csr, dtype_code, host_csr, on_device, torch_device, work_stream
from Fusion3DSeg.segUtils.cv import adjacency_to_csr


def _imread_gray(path):
    """cv2.imread(path, 0) equivalent for 8-bit label PNGs (reference voting.py:66)."""
    try:
        import cv2
        return cv2.imread(str(path), 0)
    except ImportError:
        from PIL import Image
        with Image.open(path) as im:
            return np.asarray(im.convert('L'), dtype=np.uint8)


def resize_nearest(mask, w, h):
    """cv2.resize(mask, (w, h), interpolation=INTER_NEAREST): src index = min(floor(dst * src/dst), src-1)."""
    sh, sw = mask.shape[:2]
    if (sh, sw) == (h, w):
        return mask
    xs = np.minimum(np.floor(np.arange(w) * (1.0 / (w / sw))).astype(np.int64), sw - 1)
    ys = np.minimum(np.floor(np.arange(h) * (1.0 / (h / sh))).astype(np.int64), sh - 1)
    return mask[ys[:, None], xs[None, :]]


class VotingSegmentation:
    """Voting based 3D point-cloud segmentation from 2D masks and uv2pt lookups (reference voting.py:11-137)."""

    def __init__(self, npts, depth_hw, maskdir, uv2ptdir, nclasses, votes_file=None):
        if votes_file is None:
            self.npts = npts
            self.depth_hw = depth_hw
            self.nclasses = nclasses
            self.votes = np.zeros((npts, nclasses + 1))
            self.mask_files, self.uv2pt_files = self._get_filenames(maskdir, uv2ptdir)
            self.nframes = len(self.mask_files)
        else:                                            # quirk Q2: nclasses becomes the column count (reference :39-40)
            self.votes = np.load(votes_file)
            self.nclasses = self.votes.shape[1]

    def _get_filenames(self, maskdir, uv2ptdir):
        """Frames present in both directories, paired by stem (reference :42-54)."""
        maskdir, uv2ptdir = Path(maskdir), Path(uv2ptdir)
        masks = {p.stem: p for p in maskdir.iterdir() if p.is_file()}
        luts = {p.stem: p for p in uv2ptdir.iterdir() if p.is_file()}
        mask_ext = next(iter(masks.values())).suffix
        lut_ext = next(iter(luts.values())).suffix
        common = set(masks) & set(luts)
        return ([(maskdir / s).with_suffix(mask_ext) for s in common],
                [(uv2ptdir / s).with_suffix(lut_ext) for s in common])

    def _read_data(self, idx):
        return _imread_gray(self.mask_files[idx]), np.load(self.uv2pt_files[idx])

    def zero(self):
        self.votes = np.zeros_like(self.votes)

    def vote(self, resize=True, verbose=False, filename=None):
        """Accumulate the votes of every frame (reference :75-104); returns float64 [npts, nclasses+1].

        Per frame ``votes[uv2pt[valid], mask[valid]] += 1`` with NumPy's buffered semantics: a (point, label)
        pair adds 1 per frame however many pixels map to it (quirk Q1); an out-of-range label or point raises
        IndexError before the frame changes anything.
        """
        h, w = self.depth_hw
        ctx = f3d.default_context()
        session = _DeviceVotes(ctx, self.votes)
        if verbose:
            print('voting ... ')
        # frames are read on the host and handed to the GPU a batch at a time: one upload of all lookups and masks, one
        # kernel pair for the batch (f3d_vote_uv2pt_batch*) instead of two copies and three launches per frame
        batch_l, batch_m, pending_error = [], [], None
        for i in range(self.nframes):
            if verbose:
                print(f'frame/total = {i + 1}/{self.nframes}, progress = {((i + 1) * 100 / self.nframes):.3}%')
            mask, uv2pt = self._read_data(i)
            mask = resize_nearest(mask, w, h) if resize else mask
            mask = np.ascontiguousarray(mask, dtype=np.uint8).reshape(-1)
            lut = np.asarray(uv2pt, dtype=np.int32).reshape(-1)
            if len(lut) != len(mask):                       # NumPy raises at this frame; the earlier ones stay applied
                pending_error = IndexError(f'boolean index did not match: uv2pt has {len(lut)} entries, the mask {len(mask)}')
                break
            if len(lut) != h * w:                           # a lookup of another size than depth_hw: its own single-frame call
                session.add_frames(batch_l, batch_m, h, w); batch_l, batch_m = [], []
                session.add_frame(lut, mask)
                continue
            batch_l.append(lut); batch_m.append(mask)
            if len(batch_l) * h * w >= 1 << 26:             # ~64 frames of 1024^2: bound the host staging memory
                session.add_frames(batch_l, batch_m, h, w); batch_l, batch_m = [], []
        session.add_frames(batch_l, batch_m, h, w)
        try:
            self.votes = session.download()
            if pending_error is not None:
                raise pending_error
        except IndexError:
            self.votes = session.download(check=False)      # frames before the offending one stay applied, as in the reference
            raise
        if filename is not None:
            Path(filename).parent.mkdir(exist_ok=True, parents=True)
            np.save(filename, self.votes)
        return self.votes

    def segment(self, threshold=0.5, filter_classes=None, votes=None):
        """Per-point class from the votes (reference :106-137) -> int64 [npts].

        argmax over all columns or over ``votes[:, filter_classes]`` (first maximum wins), ``nclasses`` for points
        with no votes, with max/total < threshold or with a zero maximum; then the reference's sequential
        index->class remap (which aliases when a class id is smaller than the list length, quirk Q3).
        """
        votes = self.votes if votes is None else votes
        votes = self.vote() if votes is None else votes
        return f3d.default_context().segment_votes(votes, self.nclasses, threshold, filter_classes)


class _DeviceVotes:
    """Keeps the vote matrix resident on the GPU across frames when torch is available (device memory plumbing);
    otherwise every frame goes through the host-pointer entry point (still the HIP kernels)."""

    def __init__(self, ctx, votes):
        self.ctx, self.host = ctx, np.ascontiguousarray(votes, dtype=np.float64)
        self.torch, self.error = None, None
        try:
            import torch
            if torch.cuda.is_available():
                self.torch = torch
                self.dev = torch.device('cuda', ctx.device)
                self.t = torch.from_numpy(self.host).to(self.dev)
                self.stream = torch.cuda.Stream(self.dev)
        except ImportError:
            pass

    def add_frames(self, luts, masks, h, w):
        """Frames of h*w lookups each, in order, as ONE batched call.  The lookups may be device tensors (the int32 [h*w] ones
        Fusion.fuse_device hands its lookup_sink): they are stacked on the caller's current stream, so the caller may free or rewrite
        them as soon as this returns; the vote of the stacked copies follows on the session's stream."""
        if not luts:
            return
        if self.torch is not None and isinstance(luts[0], self.torch.Tensor):
            torch = self.torch
            caller = torch.cuda.current_stream(self.dev)
            dl = torch.stack([t.reshape(-1).to(self.dev, torch.int32) for t in luts])
            dm = torch.stack([torch.as_tensor(mk).reshape(-1).to(self.dev, torch.uint8) for mk in masks])
            self.stream.wait_stream(caller)
            with torch.cuda.stream(self.stream):
                self.ctx.vote_uv2pt_batch_dev(dl.data_ptr(), dm.data_ptr(), len(luts), h, w, self.t.data_ptr(), self.t.shape[0], self.t.shape[1],
                                              self.stream.cuda_stream)
            for t in (dl, dm):                                          # memory of the caller's stream, read on the session's
                t.record_stream(self.stream)
            return
        lut = np.ascontiguousarray(np.stack(luts), dtype=np.int32)
        m = np.ascontiguousarray(np.stack(masks), dtype=np.uint8)
        if self.torch is None:
            if self.error is not None:                                  # the reference stopped at the offending frame
                return
            try:
                self.ctx.vote_uv2pt_batch(self.host, lut, m, h, w)
            except IndexError as exc:                                   # frames before the offending one are applied, like NumPy
                self.error = self.error or exc
            return
        torch = self.torch
        with torch.cuda.stream(self.stream):
            dl = torch.from_numpy(lut).to(self.dev)
            dm = torch.from_numpy(m).to(self.dev)
            self.ctx.vote_uv2pt_batch_dev(dl.data_ptr(), dm.data_ptr(), len(lut), h, w, self.t.data_ptr(), self.t.shape[0], self.t.shape[1],
                                          self.stream.cuda_stream)

    def add_frame(self, uv2pt, mask_flat):
        lut = np.array(uv2pt, dtype=np.int32).reshape(-1)               # private, writable copies
        m = np.array(mask_flat, dtype=np.uint8).reshape(-1)
        if len(lut) != len(m):
            raise IndexError(f'boolean index did not match: uv2pt has {len(lut)} entries, the mask {len(m)}')
        if self.torch is None:
            if self.error is None:
                try:
                    self.ctx.vote_uv2pt(self.host, lut, m)
                except IndexError as exc:
                    self.error = exc
            return
        torch = self.torch
        with torch.cuda.stream(self.stream):
            dl = torch.from_numpy(lut).to(self.dev)
            dm = torch.from_numpy(m).to(self.dev)
            self.ctx.vote_uv2pt_dev(dl.data_ptr(), dm.data_ptr(), len(lut), self.t.data_ptr(), self.t.shape[0], self.t.shape[1],
                                    self.stream.cuda_stream)
            # no per-frame synchronisation: an out-of-range index sets a sticky device flag, the offending frame and every
            # later one write nothing, and download() raises the IndexError -- the same votes state as the reference's
            # exception at that frame (voting.py:98)

    def download(self, check=True):
        if self.torch is None:
            if check and self.error is not None:
                raise self.error
            return self.host
        self.stream.synchronize()
        if check:
            self.ctx.take_device_error(self.stream.cuda_stream)     # IndexError for the first bad frame, if any
        return self.t.cpu().numpy()


class PointVotingSegmentation:
    """Framewise voting of ANY [M, 3] cloud from the frames' world-space depth points and masks (reference voting.py:140-299,
    marked deprecated there for the host cost of one KDTree.query_radius of h*w points per frame).

    Per frame every pixel pairs with every cloud point within ``radius`` of its depth point (float64 squared distance
    ``(dx*dx + dy*dy) + dz*dz <= radius*radius``, inclusive), then ``votes[i, mask[q]] += 1`` and ``votes[i, -1] += 1`` over
    all pairs with NumPy's buffered rule: each distinct cell gets +1 per frame however many pairs hit it.  So a point can
    receive several labels from one frame, and the last column counts the frames that saw the point.

    Column collision: ``votes`` has ``nclasses + 1`` columns and the last one is that total, so a mask label equal to
    ``nclasses`` (the 2-D stage's "low confidence" label 133 when nclasses = 133) is a legal index that lands on the total
    column: a point a frame sees with that label gets +2 there from that frame.  A label > nclasses raises IndexError, but
    only when its pixel has at least one neighbour; non-finite depth points raise ValueError (sklearn's); both leave the
    earlier frames applied.  No pixel is skipped: a dropout pixel sits at its camera centre and votes like any other.
    """

    def __init__(self, tofcameradata, sparse_points, depth_hw, maskdir, nclasses, prefix='', extension='png', zfill=2,
                 votes_file=None):
        self._dev_votes = None
        self._cloud_dev = None
        if votes_file is None:
            self.nclasses = nclasses
            self.depth_hw = depth_hw
            self.tofcameradata = tofcameradata
            cloud = np.asarray(sparse_points)
            if cloud.ndim != 2 or cloud.shape[0] == 0:
                raise ValueError(f'sparse_points must be a non-empty [M, 3] array, got {cloud.shape}')    # sklearn's KDTree raises too
            self._cloud = np.ascontiguousarray(cloud if cloud.dtype == np.float32 else cloud.astype(np.float64))
            if not np.isfinite(self._cloud).all():
                raise ValueError('sparse_points contains NaN or infinity')                               # (reference :173, sklearn)
            if len(self._cloud) >= 1 << 31:
                raise ValueError('sparse_points must hold fewer than 2^31 points')
            self._ctx = f3d.default_context()                   # F3DUnavailable without a library or a device: no CPU fallback
            self.votes = np.zeros((len(self._cloud), nclasses + 1))
            self.maskdir = maskdir
            self.prefix = prefix
            self.ext = extension
            self.zfill = zfill
        else:                                                   # (reference :181-182; the column count minus the total)
            self.votes = np.load(votes_file)
            self.nclasses = self.votes.shape[1] - 1

    # the vote matrix lives where it was last written: vote_frames leaves it on the device, reading ``votes`` brings it back
    @property
    def votes(self):
        if self._dev_votes is not None:
            self._host_votes = self._dev_votes.cpu().numpy()    # (synchronises with the stream the votes were enqueued on)
            self._dev_votes = None
        return self._host_votes

    @votes.setter
    def votes(self, value):
        self._host_votes, self._dev_votes = value, None

    def zero(self):
        self.votes = np.zeros_like(self.votes)

    @classmethod
    def read_mask(cls, name, dirname='./', prefix='', extension='png', zfill=0):
        """dirname/prefix + name.zfill(zfill) + '.' + extension as a grey image, None when the file is absent (reference :190-206)."""
        filename = os.path.join(dirname, prefix + str(name).zfill(zfill) + '.' + extension)
        return _imread_gray(filename) if os.path.isfile(filename) else None

    def get_nns(self, query_points, radius=0.01):
        """(int32 cloud indices of all queries, flattened; per-query counts) (reference :208-222).  A query's indices ascend
        (sklearn's order inside a row is its tree traversal's, which it does not specify)."""
        offs, nbrs = self._ctx.radius_query(self._cloud, query_points, radius)
        return nbrs, np.diff(offs)

    def _device_state(self):
        """torch, the device, and the cloud and the vote matrix as device tensors (uploaded when the host copy is the current one)."""
        torch, dev = torch_device(self._ctx, 'vote_frames')
        if self._cloud_dev is None:
            self._cloud_dev = torch.from_numpy(self._cloud).to(dev)
        if self._dev_votes is None:
            self._dev_votes = torch.from_numpy(np.ascontiguousarray(self._host_votes, dtype=np.float64)).to(dev)
        return torch, dev, self._cloud_dev, self._dev_votes

    def vote_frames(self, points, masks, radius=0.01, check=True):
        """The vote of F frames that are already on the device: ``points`` [F, hw, 3] float64 / float32 (what
        RTAB_utils.ios_rtab.frames_world_dev returns), ``masks`` uint8 [F, hw] or [F, h, w] at the depth resolution (what
        get2DSeg.masks_to_device returns).  No host copy, no file; the vote matrix stays on the device (returned as a float64
        tensor [M, nclasses + 1]; ``self.votes`` downloads it).  Ordered with torch's current stream
        (``f3d.tensors.work_stream``).  ``check`` (synchronises): raise the IndexError of a label > nclasses now instead of
        leaving it to ``f3d.Context.take_device_error``; the ValueError of non-finite points is always raised here."""
        torch, dev, cloud, votes = self._device_state()
        if not (isinstance(points, torch.Tensor) and isinstance(masks, torch.Tensor) and points.is_cuda and masks.is_cuda):
            raise ValueError('vote_frames takes device tensors (vote() reads frames from the host)')
        if points.dim() != 3 or points.shape[2] != 3 or points.dtype not in (torch.float64, torch.float32):
            raise ValueError(f'points must be float64 / float32 [F, hw, 3], got {points.dtype} {tuple(points.shape)}')
        F, hw = int(points.shape[0]), int(points.shape[1])
        if masks.dtype != torch.uint8 or masks.shape[0] != F or masks.numel() != F * hw:
            raise ValueError(f'masks must be uint8 [F, hw], got {masks.dtype} {tuple(masks.shape)} for {F} frames of {hw} pixels')
        points, masks = points.to(dev).contiguous(), masks.to(dev).contiguous()
        with work_stream(dev) as work:
            self._ctx.point_vote_frames_dev(cloud.data_ptr(), dtype_code(cloud), cloud.shape[0], points.data_ptr(), dtype_code(points),
                                            masks.data_ptr(), F, hw, radius, votes.data_ptr(), votes.shape[1], work.cuda_stream)
            if check:
                self._ctx.take_device_error(work.cuda_stream)
        return votes

    def vote(self, frame_numbers=None, skip=1, radius=0.01, resize=True, filename=None, verbose=False):
        """Accumulate the votes of ``frame_numbers[::skip]`` (reference :224-265); returns float64 [M, nclasses + 1].

        A frame whose mask file is absent is skipped silently.  Frames are read on the host and handed to the GPU in bounded
        batches (one upload and one fused search + vote per batch); the vote matrix stays on the device across the loop.
        """
        h, w = self.depth_hw
        frame_numbers = np.arange(len(self.tofcameradata)) if frame_numbers is None else frame_numbers
        total = len(frame_numbers) // skip
        try:
            torch, dev = torch_device(self._ctx, 'vote')
        except f3d.F3DUnavailable:                                # no torch: the frames go through the host-pointer entry
            torch = None
        if verbose:
            print('Framewise voting ... ')
        batch_q, batch_m, error = [], [], None

        def flush():
            nonlocal batch_q, batch_m
            if not batch_q:
                return
            q, m = np.stack(batch_q), np.stack(batch_m)
            batch_q, batch_m = [], []
            if torch is None:
                host = np.ascontiguousarray(self._host_votes, dtype=np.float64)
                self._host_votes = host
                self._ctx.point_vote_frames(host, self._cloud, q, m, radius)     # (the votes are copied back on an error as well)
                return
            self.vote_frames(torch.from_numpy(q).to(dev), torch.from_numpy(m).to(dev), radius, check=False)

        for i, idx in enumerate(frame_numbers[::skip]):
            data = self.tofcameradata[idx]
            if verbose:
                print(f'frame/total = {i + 1}/{total}, progress = {((i + 1) * 100 / total):.3}%')
            query = np.asarray(data['modPoints'])
            fnum = int(data['frameNumber'])
            mask = self.read_mask(fnum, self.maskdir, self.prefix, self.ext, self.zfill)
            if mask is None:
                continue
            mask = resize_nearest(mask, w, h) if resize else mask
            mask = np.ascontiguousarray(mask, dtype=np.uint8).reshape(-1)
            query = np.ascontiguousarray(query if query.dtype == np.float32 else query.astype(np.float64)).reshape(-1, 3)
            try:
                if len(query) != len(mask):                       # np.repeat(mask, frequency) raises at this frame (reference :257)
                    flush()
                    raise ValueError(f'operands could not be broadcast together: {len(mask)} mask pixels, {len(query)} query points')
                if batch_q and (batch_q[0].shape != query.shape or batch_q[0].dtype != query.dtype):
                    flush()                                       # a frame of another size or type starts a batch of its own
                batch_q.append(query); batch_m.append(mask)
                if len(batch_q) * len(query) >= 1 << 22:          # ~100 MB of float64 points: bound the host staging memory
                    flush()
            except (ValueError, IndexError) as exc:               # earlier frames stay applied, later ones never run
                error = exc
                break
        try:
            if error is None:
                flush()
        except (ValueError, IndexError) as exc:
            error = exc
        votes = self.votes                                        # (the download waits for every batch)
        if torch is not None:
            try:                                                  # an IndexError recorded on the device precedes a later ValueError
                self._ctx.take_device_error(None)
            except IndexError as exc:
                error = exc
        if error is not None:
            raise error
        if filename is not None:
            if verbose:
                print('writing file ... ')
            os.makedirs(os.path.dirname(filename), exist_ok=True)
            np.save(filename, votes)
        return votes

    def segment(self, threshold, filter_classes=None, votes=None):
        """Per-point class from the votes (reference :267-299) -> int64 [M].

        As VotingSegmentation.segment (first-maximum argmax, ``nclasses`` for no votes, for max/total < threshold and for a
        zero maximum, the sequential index->class remap with its aliasing, quirk Q3), except that the total is the LAST
        COLUMN, not the row sum, and the unfiltered candidates are ``votes[:, :-1]``.
        """
        votes = self.votes if votes is None else votes
        return f3d.default_context().segment_votes_lastcol(votes, self.nclasses, threshold, filter_classes)


# ------------------------------------------------------------------------------------------------ neighbour-summed votes
def _shape(a):
    return tuple(a.shape) if hasattr(a, 'shape') else np.shape(a)


def _smooth_scalars(what, votes, normals, angle, colors, max_color_dist, self_weight, iterations):
    """The shapes and scalars of smooth_votes / smooth_segment, checked -> (n, ncols, cos_angle, max_color_dist, self_weight, iterations)."""
    shape = _shape(votes)
    if len(shape) != 2:
        raise ValueError(f'{what}: votes must be [N, ncols], got {shape}')
    n, ncols = shape
    if not 1 <= ncols <= f3d.SMOOTH_MAX_COLS:
        raise ValueError(f'{what}: votes must have 1 to {f3d.SMOOTH_MAX_COLS} columns, got {ncols}')
    iterations = int(iterations)
    if iterations < 1:
        raise ValueError(f'{what}: iterations must be at least 1, got {iterations}')
    self_weight = float(self_weight)
    if not math.isfinite(self_weight) or self_weight < 0:
        raise ValueError(f'{what}: self_weight must be finite and not negative, got {self_weight}')
    if (normals is None) != (angle is None):
        raise ValueError(f'{what}: normals and angle go together (the gate needs both)')
    if (colors is None) != (max_color_dist is None):
        raise ValueError(f'{what}: colors and max_color_dist go together (the gate needs both)')
    cos_angle = 0.0
    if normals is not None:
        cos_angle = math.cos(math.radians(float(angle)))
        if math.isnan(cos_angle):
            raise ValueError(f'{what}: angle must be a number of degrees, got {angle}')
        if _shape(normals) != (n, 3):
            raise ValueError(f'{what}: normals must be [{n}, 3], got {_shape(normals)}')
    limit = 0.0
    if colors is not None:
        limit = float(max_color_dist)
        if not limit >= 0:
            raise ValueError(f'{what}: max_color_dist must not be negative, got {max_color_dist}')
        if _shape(colors) != (n, 3):
            raise ValueError(f'{what}: colors must be [{n}, 3], got {_shape(colors)}')
    return n, ncols, cos_angle, limit, self_weight, iterations


def _smooth_device_inputs(what, votes, adj, n, normals, colors):
    import torch
    dev = votes.device
    u16 = (torch.int16,) + ((torch.uint16,) if hasattr(torch, 'uint16') else ())           # uint16 counts may travel as int16 bits
    if votes.dtype != torch.float64 and votes.dtype not in u16:
        raise TypeError(f'{what}: votes must be float64 or uint16 (int16 bits as a tensor), got {votes.dtype}')
    if normals is not None and (not on_device(normals) or normals.dtype != torch.float64):
        raise TypeError(f'{what}: normals must be a float64 device tensor for device votes')
    if colors is not None and (not on_device(colors) or colors.dtype not in (torch.float64, torch.float32)):
        raise TypeError(f'{what}: colors must be a float64 or float32 device tensor for device votes')
    offs, nbrs = device_csr(adj, n, dev, 'device votes')
    return (dev, votes.contiguous(), offs, nbrs, None if normals is None else normals.to(dev).contiguous(),
            None if colors is None else colors.to(dev).contiguous())


def _smooth_host_inputs(what, votes, adj, n, normals, colors):
    v = np.asarray(votes)
    if v.dtype not in (np.float64, np.uint16):
        raise TypeError(f'{what}: votes must be float64 or uint16, got {v.dtype}')
    if normals is not None:
        if on_device(normals) or np.asarray(normals).dtype != np.float64:
            raise TypeError(f'{what}: normals must be a float64 array for host votes')
        normals = np.ascontiguousarray(normals)
    if colors is not None:
        if on_device(colors) or np.asarray(colors).dtype not in (np.float64, np.float32):
            raise TypeError(f'{what}: colors must be a float64 or float32 array for host votes')
        colors = np.ascontiguousarray(colors)
    if isinstance(adj, tuple) and any(on_device(a) for a in adj):
        raise TypeError(f'{what}: host votes need a host adjacency (a device CSR pair goes with device tensors)')
    offs, nbrs = host_csr(*adjacency_to_csr(adj, n), n, CSR_ADJACENCY)
    return np.ascontiguousarray(v), offs, nbrs, normals, colors


def _dptr(t):
    return None if t is None else t.data_ptr()


def _overlaps(a, b):
    """Two device tensors share memory."""
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a0 < b0 + b.numel() * b.element_size() and b0 < a0 + a.numel() * a.element_size()


def smooth_votes(votes, adj, normals=None, angle=None, colors=None, max_color_dist=None, self_weight=1.0, iterations=1, out=None):
    """Every vote row becomes ``self_weight`` times itself plus the rows of its neighbours, `iterations` times (include/f3d.h
    f3d_smooth_votes).  votes float64 or uint16 [N, ncols] (a uint16 tensor may come as int16 bits), ncols <= 256; adj a list of rows or a CSR pair, any CSR: rows need not be
    symmetric, the point itself is skipped, a duplicate entry counts twice.  With normals (float64 [N, 3]) and `angle` in degrees only
    neighbours whose normal lies within `angle` of the point's (either sign) contribute; with colors (float64 / float32 [N, 3]) and
    max_color_dist only neighbours within that colour distance.  Neighbour weights are 1.  The sums have one fixed order, so equal input
    gives equal bits.  -> float64 [N, ncols] (`out` when given: C-contiguous float64, not sharing memory with votes).  Device tensors
    with a device CSR pair stay on the device.  Every argument is checked before anything is launched."""
    what = 'smooth_votes'
    n, ncols, cos_angle, limit, self_weight, iterations = _smooth_scalars(what, votes, normals, angle, colors, max_color_dist, self_weight,
                                                                          iterations)
    if out is not None and _shape(out) != (n, ncols):
        raise ValueError(f'{what}: out must be [{n}, {ncols}], got {_shape(out)}')
    if on_device(votes):
        import torch
        dev, v, offs, nbrs, nrm, col = _smooth_device_inputs(what, votes, adj, n, normals, colors)
        if out is None:
            out = torch.empty((n, ncols), dtype=torch.float64, device=dev)
        elif not on_device(out) or out.dtype != torch.float64 or out.device != dev or not out.is_contiguous():
            raise TypeError(f'{what}: out must be a contiguous float64 tensor on {dev}')
        elif _overlaps(out, v):
            raise ValueError(f'{what}: out must not share memory with votes')
        ctx = f3d.default_context(dev.index)
        with work_stream(dev) as work:
            ctx.smooth_votes_dev(v.data_ptr(), f3d._vtype(v), n, ncols, offs.data_ptr(), nbrs.data_ptr(), _dptr(nrm), cos_angle, _dptr(col),
                                 f3d.F64 if col is None else dtype_code(col), limit, self_weight, iterations, out.data_ptr(), work.cuda_stream)
            ctx.take_device_error(work.cuda_stream)                       # synchronises the stream: the result is complete
        return out
    v, offs, nbrs, nrm, col = _smooth_host_inputs(what, votes, adj, n, normals, colors)
    if out is not None:
        if not isinstance(out, np.ndarray) or out.dtype != np.float64 or not out.flags.c_contiguous:
            raise TypeError(f'{what}: out must be a C-contiguous float64 array')
        if np.shares_memory(out, v):
            raise ValueError(f'{what}: out must not share memory with votes')
    return f3d.default_context().smooth_votes(v, offs, nbrs, nrm, cos_angle, col, limit, self_weight, iterations, out=out)


def smooth_segment(votes, adj, nclasses, threshold=0.5, filter_classes=None, lastcol=False, normals=None, angle=None, colors=None,
                   max_color_dist=None, self_weight=1.0, iterations=1):
    """``segment`` of the matrix ``smooth_votes`` would return, without writing its last iteration: VotingSegmentation.segment's rules
    (lastcol: PointVotingSegmentation.segment's, the last column being the total) on the smoothed rows.  For integer votes and an
    integer self_weight (every voter here) the classes equal segmenting ``smooth_votes``' result bit for bit.  Arguments as for
    smooth_votes.  -> classes int64 [N] (a device tensor for device votes)."""
    what = 'smooth_segment'
    n, ncols, cos_angle, limit, self_weight, iterations = _smooth_scalars(what, votes, normals, angle, colors, max_color_dist, self_weight,
                                                                          iterations)
    nclasses, threshold = int(nclasses), float(threshold)
    flt = None if filter_classes is None else [int(c) for c in filter_classes]
    if flt is not None and any(c >= ncols or c < -ncols for c in flt):
        raise IndexError(f'{what}: a filter class is out of bounds for {ncols} vote columns')
    if lastcol and ncols < 2 and not flt:
        raise ValueError(f'{what}: attempt to get argmax of an empty sequence')
    if on_device(votes):
        import torch
        dev, v, offs, nbrs, nrm, col = _smooth_device_inputs(what, votes, adj, n, normals, colors)
        cls = torch.empty(n, dtype=torch.int64, device=dev)
        ctx = f3d.default_context(dev.index)
        with work_stream(dev) as work:
            ctx.smooth_segment_dev(v.data_ptr(), f3d._vtype(v), n, ncols, offs.data_ptr(), nbrs.data_ptr(), _dptr(nrm), cos_angle, _dptr(col),
                                   f3d.F64 if col is None else dtype_code(col), limit, self_weight, iterations, nclasses, threshold, flt,
                                   lastcol, cls.data_ptr(), work.cuda_stream)
            ctx.take_device_error(work.cuda_stream)
        return cls
    v, offs, nbrs, nrm, col = _smooth_host_inputs(what, votes, adj, n, normals, colors)
    return f3d.default_context().smooth_segment(v, offs, nbrs, nclasses, threshold, flt, lastcol, nrm, cos_angle, col, limit, self_weight,
                                                iterations)
