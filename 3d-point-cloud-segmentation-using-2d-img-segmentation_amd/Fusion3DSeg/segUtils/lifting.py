"""Mask lifting: 3D instances from the per-frame instance ids of the 2D network (no reference counterpart).

The reference votes the semantic map of every frame and throws the network's instance map away; its only way to 3D instances is
``split_into_instances``, a flood of the radius graph within a class, which fuses two chairs that touch.  The 2D network does
separate them, in every frame, but its ids are local to a frame.  ``lift_instances`` makes them consistent over the cloud: the
segments (frame, id) that share enough points are merged, every point then takes the instance most of its segments belong to
(f3d_lift_instances, include/f3d.h states the contract; tests/lift_ref.py restates it in NumPy).  Work grows with the sum over
the points of seen^2, seen = the segments a point lies in.

NumPy arrays in, NumPy arrays back; device tensors in, device tensors back, with no host round trip besides the one readback of
the counts.
"""
from pathlib import Path
from types import SimpleNamespace

import numpy as np

import f3d
from f3d.tensors import on_device, torch_device, work_stream
from Fusion3DSeg.segUtils.voting import resize_nearest

__all__ = ['segment_overlaps', 'lift_instances', 'split_by_lift', 'lift_from_dirs', 'read_instance_map']


def _host_inputs(what, luts, inst):
    luts = np.asarray(luts)
    inst = np.asarray(inst)
    if luts.ndim != 2 or inst.shape != luts.shape:
        raise ValueError(f'{what}: luts and inst must both be [F, HW], got {luts.shape} and {inst.shape}')
    if luts.dtype.kind not in 'iu' or inst.dtype.kind not in 'iu':
        raise TypeError(f'{what}: luts and inst must be integer arrays')
    if inst.size and (int(inst.min()) < 0 or int(inst.max()) > 65535):
        raise ValueError(f'{what}: instance ids must lie in [0, 65535]')
    if luts.size and (int(luts.max()) > 0x7fffffff or int(luts.min()) < -0x80000000):
        raise IndexError(f'{what}: a lookup does not fit int32')
    return np.ascontiguousarray(luts, dtype=np.int32), np.ascontiguousarray(inst, dtype=np.uint16)


def _device_inputs(what, luts, inst):
    import torch
    if not on_device(inst) or not on_device(luts) or inst.device != luts.device:
        raise TypeError(f'{what}: luts and inst must be tensors on one device')
    if luts.dim() != 2 or inst.shape != luts.shape:
        raise ValueError(f'{what}: luts and inst must both be [F, HW], got {tuple(luts.shape)} and {tuple(inst.shape)}')
    if luts.dtype != torch.int32:
        raise TypeError(f'{what}: luts must be an int32 tensor')
    if inst.dtype == torch.uint8:
        inst = inst.to(torch.int16)
    if inst.dtype not in (torch.uint16, torch.int16):                  # (int16: the bits of a uint16 map)
        raise TypeError(f'{what}: inst must be a uint16 tensor (or its bits as int16), or uint8')
    return luts.device, luts.contiguous(), inst.contiguous()


def _shape_checks(what, nframes, hw, npoints, max_ids):
    if npoints < 0:
        raise ValueError(f'{what}: npoints must not be negative')
    if not 1 <= max_ids <= 65535:
        raise ValueError(f'{what}: max_ids must be in [1, 65535], got {max_ids}')
    if nframes * max_ids >= 1 << 31 or nframes * hw >= 1 << 31 or npoints >= 1 << 31:
        raise ValueError(f'{what}: frames * max_ids, frames * pixels and npoints must stay below 2^31')


def _wide(inst):
    """The ids of a device map as int32 (an int16 tensor holds the bits of a uint16 map)."""
    import torch
    return inst.to(torch.int32) & 0xffff


def _max_id(inst):
    """max(inst), at least 1 (one scalar readback for a tensor)."""
    if on_device(inst):
        return max(1, int(_wide(inst).max())) if inst.numel() else 1
    return max(1, int(np.max(inst))) if np.size(inst) else 1


def _first_cap(nframes, hw, max_ids):
    nseg = nframes * max_ids
    return int(min(nseg * (nseg - 1) // 2, max(1 << 16, nframes * hw // 8)))


def _check_without_points(luts, inst, max_ids):
    """npoints == 0: the library wants a point, so the contract's errors are judged here (a readback for tensors)."""
    ids = _wide(inst) if on_device(inst) else inst
    if bool((luts >= 0).any()) or bool((ids > max_ids).any()):
        raise IndexError('lift: an instance id exceeds max_ids, or a lookup is not below npoints')


def segment_overlaps(luts, inst, npoints, max_ids):
    """Sizes and pairwise overlaps of the segments.  luts int32 [F, HW] (pixel -> point, negative = none), inst uint16 [F, HW] (the
    pixel's instance id within its frame, 0 = none); the segment of (frame f, id k) has index f * max_ids + k - 1.
    -> (sizes int32 [F * max_ids] distinct points per segment, pairs int32 [P, 2] the pairs a < b that share a point, ascending,
    counts int32 [P] the points they share).  An id > max_ids or a lookup >= npoints raises IndexError."""
    what = 'segment_overlaps'
    npoints, max_ids = int(npoints), int(max_ids)
    if on_device(luts) or on_device(inst):
        import torch
        dev, l, i = _device_inputs(what, luts, inst)
        nf, hw = l.shape
        _shape_checks(what, nf, hw, npoints, max_ids)
        if nf == 0 or hw == 0 or npoints == 0:
            if npoints == 0:
                _check_without_points(l, i, max_ids)
            return (torch.zeros(nf * max_ids, dtype=torch.int32, device=dev), torch.zeros((0, 2), dtype=torch.int32, device=dev),
                    torch.zeros(0, dtype=torch.int32, device=dev))
        ctx = f3d.default_context(dev.index)
        sizes = torch.zeros(nf * max_ids, dtype=torch.int32, device=dev)
        cap = _first_cap(nf, hw, max_ids)
        with work_stream(dev) as work:
            while True:
                pairs = torch.empty((cap, 2), dtype=torch.int32, device=dev)
                counts = torch.empty(cap, dtype=torch.int32, device=dev)
                stats = ctx.lift_overlaps_dev(l.data_ptr(), i.data_ptr(), nf, hw, npoints, max_ids, sizes.data_ptr(),
                                              pairs.data_ptr() if cap else None, counts.data_ptr() if cap else None, cap, work.cuda_stream)
                if stats[0] <= cap:
                    break
                cap = int(stats[0])                                        # rare: more pairs than the first guess had room for
        p = int(stats[0])
        return sizes, pairs[:p], counts[:p]
    l, i = _host_inputs(what, luts, inst)
    nf, hw = l.shape
    _shape_checks(what, nf, hw, npoints, max_ids)
    if nf == 0 or hw == 0 or npoints == 0:
        if npoints == 0:
            _check_without_points(l, i, max_ids)
        return np.zeros(nf * max_ids, np.int32), np.zeros((0, 2), np.int32), np.zeros(0, np.int32)
    ctx = f3d.default_context()
    cap = _first_cap(nf, hw, max_ids)
    while True:
        sizes, pairs, counts, stats = ctx.lift_overlaps(l, i, npoints, max_ids, cap)
        if stats[0] <= cap:
            break
        cap = int(stats[0])
    p = int(stats[0])
    return sizes, pairs[:p], counts[:p]


def lift_instances(luts, inst, npoints, max_ids=None, ratio=0.5, min_overlap=10, seg_classes=None, min_points=1):
    """Consistent 3D instance ids from per-frame 2D instance ids.

    luts int32 [F, HW]: pixel -> cloud point, negative = none (uv2pt of Fusion.fuse, render_lookups, render_mesh_lookups).
    inst uint16 [F, HW]: the pixel's instance id within its frame, 0 = none.  max_ids: the largest id a frame may use (None:
    max(inst), at least 1).  Two segments are merged when they share at least min_overlap points and at least ratio * the points
    of the smaller one and, with seg_classes (int32 [F * max_ids], the class of every segment), carry the same class; merging is
    transitive.  Every point takes the instance most of its segments belong to (a tie: the smaller id); instances that win fewer
    than min_points points are dropped, their points become 0, and the rest is renumbered.

    -> an object with ids int32 [N] (0 = none), support uint16 [N] (the winning count), seen uint16 [N] (segments the point lies
    in), seg2inst int32 [F * max_ids] (0 = empty or dropped) and inst_points int64 [I + 1] (points per instance, entry 0 the
    unlabelled ones).  An id > max_ids or a lookup >= npoints raises IndexError."""
    what = 'lift_instances'
    npoints, ratio, min_overlap, min_points = int(npoints), float(ratio), int(min_overlap), int(min_points)
    device = on_device(luts) or on_device(inst)
    if device:
        import torch
        dev, l, i = _device_inputs(what, luts, inst)
    else:
        l, i = _host_inputs(what, luts, inst)
    max_ids = _max_id(i) if max_ids is None else int(max_ids)
    nf, hw = l.shape
    _shape_checks(what, nf, hw, npoints, max_ids)
    nseg = nf * max_ids
    if seg_classes is not None:
        if device:
            if not on_device(seg_classes) or seg_classes.device != dev or seg_classes.numel() != nseg:
                raise ValueError(f'{what}: seg_classes must be a tensor of {nseg} entries on {dev}')
            seg_classes = seg_classes.reshape(-1).to(torch.int32).contiguous()
        else:
            seg_classes = np.ascontiguousarray(np.asarray(seg_classes).reshape(-1), dtype=np.int32)
            if len(seg_classes) != nseg:
                raise ValueError(f'{what}: seg_classes must have {nseg} entries, got {len(seg_classes)}')
    if nf == 0 or hw == 0 or npoints == 0:
        if npoints == 0:
            _check_without_points(l, i, max_ids)
        if device:
            z = lambda n, dt: torch.zeros(n, dtype=dt, device=dev)            # noqa: E731
            ip = torch.full((1,), npoints, dtype=torch.int64, device=dev)
            return SimpleNamespace(ids=z(npoints, torch.int32), support=z(npoints, torch.uint16), seen=z(npoints, torch.uint16),
                                   seg2inst=z(nseg, torch.int32), inst_points=ip)
        return SimpleNamespace(ids=np.zeros(npoints, np.int32), support=np.zeros(npoints, np.uint16), seen=np.zeros(npoints, np.uint16),
                               seg2inst=np.zeros(nseg, np.int32), inst_points=np.array([npoints], np.int64))
    if device:
        ctx = f3d.default_context(dev.index)
        ids = torch.zeros(npoints, dtype=torch.int32, device=dev)
        support = torch.zeros(npoints, dtype=torch.uint16, device=dev)
        seen = torch.zeros(npoints, dtype=torch.uint16, device=dev)
        seg2inst = torch.zeros(nseg, dtype=torch.int32, device=dev)
        inst_points = torch.zeros(nseg + 1, dtype=torch.int64, device=dev)
        with work_stream(dev) as work:
            stats = ctx.lift_instances_dev(l.data_ptr(), i.data_ptr(), nf, hw, npoints, max_ids, ratio, min_overlap,
                                           None if seg_classes is None else seg_classes.data_ptr(), min_points, ids.data_ptr(),
                                           support.data_ptr(), seen.data_ptr(), seg2inst.data_ptr(), inst_points.data_ptr(), work.cuda_stream)
    else:
        ids, support, seen, seg2inst, inst_points, stats = f3d.default_context().lift_instances(l, i, npoints, max_ids, ratio, min_overlap,
                                                                                                  seg_classes, min_points)
    return SimpleNamespace(ids=ids, support=support, seen=seen, seg2inst=seg2inst, inst_points=inst_points[:int(stats[1]) + 1])


def split_by_lift(ids, lifted, return_parent=False):
    """Subdivides the instances `ids` (e.g. of split_into_instances) by the lifted ids: the new id of a point is the dense rank,
    from 0, of its (ids, lifted) pair in ascending order, so points with lifted == 0 stay together with the other such points of
    their instance, and the instances keep their order.  -> new ids (int64, as `ids`); with return_parent also the old id of every
    new id."""
    if on_device(ids) or on_device(lifted):
        import torch
        if not (on_device(ids) and on_device(lifted)) or ids.shape != lifted.shape or ids.dim() != 1:
            raise ValueError('split_by_lift: ids and lifted must be tensors of one length on one device')
        key = ids.to(torch.int64) * (1 << 32) + lifted.to(torch.int64)
        uniq, inv = torch.unique(key, sorted=True, return_inverse=True)
        return (inv, uniq >> 32) if return_parent else inv
    a, b = np.asarray(ids), np.asarray(lifted)
    if a.shape != b.shape or a.ndim != 1:
        raise ValueError('split_by_lift: ids and lifted must be arrays of one length')
    if len(b) and (int(b.min()) < 0 or int(b.max()) >= 1 << 32):
        raise ValueError('split_by_lift: lifted ids must lie in [0, 2^32)')
    key = a.astype(np.int64) * (1 << 32) + b.astype(np.int64)
    uniq, inv = np.unique(key, return_inverse=True)
    inv = inv.reshape(-1).astype(np.int64)
    return (inv, uniq >> 32) if return_parent else inv


def read_instance_map(path):
    """An 8-bit or 16-bit single-channel PNG of per-pixel instance ids -> uint16 [H, W]."""
    try:
        import cv2
        im = cv2.imread(str(path), cv2.IMREAD_UNCHANGED)
    except ImportError:
        from PIL import Image
        with Image.open(path) as pil:
            im = np.asarray(pil)
    if im is None or im.ndim != 2 or im.dtype not in (np.uint8, np.uint16, np.int32):
        raise ValueError(f'{path}: expected a single-channel 8-bit or 16-bit id image')
    if im.dtype == np.int32 and im.size and (im.min() < 0 or im.max() > 65535):
        raise ValueError(f'{path}: ids outside [0, 65535]')
    return im.astype(np.uint16)


def _paired_files(instance_dir, uv2pt_dir):
    """Frames present in both directories, paired by stem as VotingSegmentation pairs masks with lookups, in stem order."""
    maps = {p.stem: p for p in Path(instance_dir).iterdir() if p.is_file()}
    luts = {p.stem: p for p in Path(uv2pt_dir).iterdir() if p.is_file()}
    common = sorted(set(maps) & set(luts))
    return [maps[s] for s in common], [luts[s] for s in common]


def lift_from_dirs(instance_dir, uv2pt_dir, npoints, depth_hw, max_ids=None, batch_pixels=1 << 26, **kw):
    """lift_instances over the frames of two directories: per-frame id PNGs (8 or 16 bit; resized to depth_hw with the nearest-
    neighbour rule of voting.resize_nearest) and the uv2pt lookups (.npy), paired by stem.  The frames are read and uploaded
    batch_pixels pixels at a time, so the host holds one batch; the lift itself needs all frames on the device.  Remaining
    keywords go to lift_instances.  -> its result, NumPy arrays, plus `frames` (the stems in segment order)."""
    h, w = depth_hw
    map_files, lut_files = _paired_files(instance_dir, uv2pt_dir)
    nf, hw = len(map_files), h * w
    torch, dev = torch_device(f3d.default_context(), 'lift_from_dirs')
    luts = torch.empty((nf, hw), dtype=torch.int32, device=dev)
    inst = torch.empty((nf, hw), dtype=torch.int16, device=dev)
    per = max(1, int(batch_pixels) // max(hw, 1))
    for f0 in range(0, nf, per):
        bl, bi = [], []
        for mp, lp in zip(map_files[f0:f0 + per], lut_files[f0:f0 + per]):
            lut = np.asarray(np.load(lp), dtype=np.int32).reshape(-1)
            ids = np.ascontiguousarray(resize_nearest(read_instance_map(mp), w, h)).reshape(-1)
            if len(lut) != hw or len(ids) != hw:
                raise IndexError(f'{lp.name}: the lookup has {len(lut)} entries, depth_hw {hw} pixels')
            bl.append(lut); bi.append(ids.view(np.int16))
        luts[f0:f0 + len(bl)] = torch.from_numpy(np.stack(bl)).to(dev)
        inst[f0:f0 + len(bi)] = torch.from_numpy(np.stack(bi)).to(dev)
    seg_classes = kw.pop('seg_classes', None)
    if seg_classes is not None:
        seg_classes = torch.as_tensor(np.asarray(seg_classes, dtype=np.int32)).to(dev)
    r = lift_instances(luts, inst, npoints, max_ids=max_ids, seg_classes=seg_classes, **kw)
    return SimpleNamespace(ids=r.ids.cpu().numpy(), support=r.support.cpu().numpy(), seen=r.seen.cpu().numpy(),
                           seg2inst=r.seg2inst.cpu().numpy(), inst_points=r.inst_points.cpu().numpy(), frames=[p.stem for p in map_files])
