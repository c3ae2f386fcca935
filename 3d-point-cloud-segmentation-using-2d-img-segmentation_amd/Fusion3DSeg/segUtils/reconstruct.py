"""TSDF reconstruction: a triangle mesh from posed depth frames (no reference counterpart).

The reference takes its mesh from an external exporter.  A capture of posed depth frames -- the main route here, through
``Fusion.fuse`` -- has none, which leaves the mesh route (``render_mesh_lookups``, ``project_vote_argmax_occluded``,
``meshUtils.label_faces``, ``face_adjacency``, ``segment_faces``) out of reach.  ``TSDFVolume`` integrates the depth frames into a
truncated signed distance volume and extracts a triangle mesh from it by surface nets, on the GPU (f3d_tsdf_integrate,
f3d_tsdf_extract_count -> _fill: include/f3d.h states the contract, tests/tsdf_ref.py restates it in NumPy).

``TSDFVolume(..., color=True)`` also keeps a colour per voxel, a running average with a weight of its own that only the samples
within the truncation band of the surface update (f3d_tsdf_integrate_color), from uint8 colour images of any size, one per depth
frame; ``extract_mesh(colors=True)`` then returns a colour per vertex (f3d_tsdf_extract_colors; tests/tsdf_color_ref.py).

NumPy arrays in, NumPy arrays back; ``device=True`` or device tensors in keep the state and the mesh on the GPU, ordered with
torch's current stream.  There is no CPU fallback.  Out of scope: voxel hashing, label or feature channels (labels reach the mesh
through ``label_faces``), depth interpolation, bilinear colour sampling, float or RGBA colour images, mesh simplification.
"""
import math

import numpy as np

import f3d
from f3d.tensors import depth_code, on_device, torch_device, upload, work_stream

__all__ = ['TSDFVolume', 'reconstruct_mesh', 'depth_images']

MAX_WEIGHT = float(1 << 24)


def _positive(name, x):
    x = float(x)
    if not (x > 0.0 and math.isfinite(x)):
        raise ValueError(f'{name} must be finite and positive, got {x}')
    return x


class TSDFVolume:
    """A dense volume of ``dims = (nx, ny, nz)`` voxels of edge ``voxel`` with its corner at ``lo``; voxel (i, j, k) has its centre
    at ``lo + (idx + 0.5) * voxel``.  It owns the two state arrays ``tsdf`` and ``weight``, float32 [nz, ny, nx]: NumPy arrays, or
    torch tensors on the context's device with ``device=True`` (and from the first ``integrate`` that is fed device tensors).  With
    ``color=True`` it owns ``color`` as well, float32 [nz, ny, nx, 4]: (r, g, b) on a 0..255 scale and the colour's weight."""

    def __init__(self, lo, dims, voxel, trunc=None, max_weight=64, device=False, color=False):
        lo = np.asarray(lo, dtype=np.float64).reshape(-1)
        if lo.shape != (3,) or not np.isfinite(lo).all():
            raise ValueError('lo must be 3 finite coordinates')
        dims = tuple(int(d) for d in np.asarray(dims).reshape(-1))
        if len(dims) != 3 or min(dims) < 1 or dims[0] * dims[1] * dims[2] >= 1 << 31:
            raise ValueError(f'dims must be three sizes >= 1 with a product below 2^31, got {dims}')
        self.lo, self.dims = np.ascontiguousarray(lo), dims
        self.voxel = _positive('voxel', voxel)
        self.trunc = _positive('trunc', 4.0 * self.voxel if trunc is None else trunc)
        self.max_weight = float(max_weight)
        if not 1.0 <= self.max_weight <= MAX_WEIGHT:
            raise ValueError(f'max_weight must be in [1, 2^24], got {max_weight}')
        shape = dims[::-1]
        self.tsdf, self.weight = np.zeros(shape, np.float32), np.zeros(shape, np.float32)
        self.color = np.zeros(shape + (4,), np.float32) if color else None
        if device:
            self._to_device()

    @property
    def on_device(self):
        return on_device(self.tsdf)

    def _to_device(self):
        if not self.on_device:
            ctx = f3d.default_context()
            torch, dev = torch_device(ctx, 'TSDFVolume(device=True)')
            self.tsdf, self.weight = upload(self.tsdf, dev), upload(self.weight, dev)
            if self.color is not None:
                self.color = upload(self.color, dev)

    def integrate(self, depths, K, wxyzs, translations, depth_scale=1.0, max_depth=10, colors=None):
        """Integrates the depth frames ``depths`` [F, h, w] (uint16, float32 or float64; raw / depth_scale = metres along the camera
        z axis) taken at the camera->world poses ``wxyzs`` [F, 4], ``translations`` [F, 3] with the intrinsics ``K`` of the depth
        images, in frame order.  Depths that are 0, not finite or beyond ``max_depth`` contribute nothing.  ``colors``: the frames'
        colour images, uint8 [F, hc, wc, 3] of any size (a depth pixel takes the colour pixel of the nearest rule,
        ``uc = u * wc // w``), for a volume built with ``color=True``; without them the frames leave ``color`` untouched."""
        if not on_device(depths):
            depths = np.asarray(depths)
        if len(depths.shape) != 3:
            raise ValueError(f'depths must be [F, h, w], got {tuple(depths.shape)}')
        code = depth_code(depths)
        F, h, w = (int(x) for x in depths.shape)
        depth_scale, max_depth = _positive('depth_scale', depth_scale), _positive('max_depth', max_depth)
        if h < 1 or w < 1:
            raise ValueError('depth frames must have pixels')
        if colors is not None:
            colors = self._color_images(colors, F)
        if F == 0:
            return self
        views = f3d.views_build(K, w, h, wxyzs, translations, max_depth)
        if len(views) != F:
            raise ValueError(f'{len(views)} poses for {F} depth frames')
        ctx = f3d.default_context()
        if not (on_device(depths) or self.on_device or (colors is not None and on_device(colors))):
            if colors is None:
                ctx.tsdf_integrate(self.tsdf, self.weight, self.lo, self.voxel, self.trunc, self.max_weight, depths, views, depth_scale, max_depth)
            else:
                ctx.tsdf_integrate_color(self.tsdf, self.weight, self.color, self.lo, self.voxel, self.trunc, self.max_weight, depths, colors, views,
                                         depth_scale, max_depth)
            return self
        torch, dev = torch_device(ctx, 'TSDFVolume.integrate')
        self._to_device()
        d = (depths if on_device(depths) else torch.from_numpy(np.ascontiguousarray(depths))).to(dev).contiguous()
        used = [d]
        if colors is not None:
            rgb = (colors if on_device(colors) else torch.from_numpy(np.ascontiguousarray(colors))).to(dev).contiguous()
            used.append(rgb)
        with torch.cuda.device(dev), work_stream(dev) as work:
            dviews = upload(views, dev)
            if colors is None:
                ctx.tsdf_integrate_dev(self.tsdf.data_ptr(), self.weight.data_ptr(), self.dims, self.lo, self.voxel, self.trunc, self.max_weight,
                                       d.data_ptr(), code, F, h, w, depth_scale, max_depth, dviews.data_ptr(), work.cuda_stream)
            else:
                ctx.tsdf_integrate_color_dev(self.tsdf.data_ptr(), self.weight.data_ptr(), self.color.data_ptr(), self.dims, self.lo, self.voxel,
                                             self.trunc, self.max_weight, d.data_ptr(), code, rgb.data_ptr(), F, h, w, int(rgb.shape[1]),
                                             int(rgb.shape[2]), depth_scale, max_depth, dviews.data_ptr(), work.cuda_stream)
        for t in used + [dviews]:
            t.record_stream(torch.cuda.current_stream(dev))
        return self

    def _color_images(self, colors, nframes):
        """The checks of ``integrate``'s colour images, before any device call: uint8 [F, hc, wc, 3], F = the depth frames."""
        if self.color is None:
            raise ValueError('colors need a volume built with color=True')
        if on_device(colors):
            import torch
            if colors.dtype != torch.uint8:
                raise TypeError(f'colour images must be uint8, got {colors.dtype}')
        else:
            colors = np.asarray(colors)
            if colors.dtype != np.uint8:
                raise TypeError(f'colour images must be uint8, got {colors.dtype}')
        shape = tuple(int(x) for x in colors.shape)
        if len(shape) != 4 or shape[3] != 3 or shape[1] < 1 or shape[2] < 1:
            raise ValueError(f'colour images must be [F, hc, wc, 3] with pixels, got {shape}')
        if shape[0] != nframes:
            raise ValueError(f'{shape[0]} colour images for {nframes} depth frames')
        return colors

    def extract_mesh(self, min_weight=1, colors=False):
        """The surface-nets mesh of the voxels seen at least ``min_weight`` times -> (vertices float64 [V, 3], triangles int32
        [M, 3]), consistently wound with the normals pointing from inside (behind the surface) to outside (towards the cameras).
        With ``colors`` (a volume built with ``color=True``) -> (vertices, triangles, rgb uint8 [V, 3], colored uint8 [V]): the
        vertex colours, and 0 in ``colored`` (with a black ``rgb``) for a vertex none of whose cell's crossing edges has a coloured end."""
        min_weight = float(min_weight)
        if not min_weight >= 1.0:
            raise ValueError(f'min_weight must be at least 1, got {min_weight}')
        if colors and self.color is None:
            raise ValueError('vertex colours need a volume built with color=True')
        ctx = f3d.default_context()
        if not self.on_device:
            if colors:
                return ctx.tsdf_extract_colors(self.tsdf, self.weight, self.color, self.lo, self.voxel, min_weight)
            return ctx.tsdf_extract(self.tsdf, self.weight, self.lo, self.voxel, min_weight)
        torch, dev = torch_device(ctx, 'TSDFVolume.extract_mesh')
        with torch.cuda.device(dev), work_stream(dev) as work:
            nv, nt = ctx.tsdf_extract_count_dev(self.tsdf.data_ptr(), self.weight.data_ptr(), self.dims, min_weight, work.cuda_stream)
            verts = torch.empty((nv, 3), dtype=torch.float64, device=dev)
            tris = torch.empty((nt, 3), dtype=torch.int32, device=dev)
            out = [verts, tris]
            ctx.tsdf_extract_fill_dev(self.tsdf.data_ptr(), self.dims, self.lo, self.voxel, verts.data_ptr() if nv else None,
                                      tris.data_ptr() if nt else None, work.cuda_stream)
            if colors:
                out += [torch.empty((nv, 3), dtype=torch.uint8, device=dev), torch.empty((nv,), dtype=torch.uint8, device=dev)]
                if nv:
                    ctx.tsdf_extract_colors_dev(self.tsdf.data_ptr(), self.color.data_ptr(), self.dims, out[2].data_ptr(), out[3].data_ptr(),
                                                work.cuda_stream)
        for t in out:
            t.record_stream(torch.cuda.current_stream(dev))
        return tuple(out)


def reconstruct_mesh(depths, K, wxyzs, translations, lo, dims, voxel, trunc=None, max_weight=64, depth_scale=1.0, max_depth=10, min_weight=1,
                     device=False, colors=None):
    """``TSDFVolume(lo, dims, voxel, trunc, max_weight).integrate(...).extract_mesh(min_weight)`` in one call ->
    (vertices float64 [V, 3], triangles int32 [M, 3]); device tensors for ``depths`` (or ``device=True``) give device tensors.  With
    ``colors`` (uint8 [F, hc, wc, 3]) the volume keeps colour -> (vertices, triangles, rgb uint8 [V, 3], colored uint8 [V])."""
    vol = TSDFVolume(lo, dims, voxel, trunc, max_weight, device=device, color=colors is not None)
    vol.integrate(depths, K, wxyzs, translations, depth_scale, max_depth, colors=colors)
    return vol.extract_mesh(min_weight, colors=colors is not None)


def depth_images(frame_points, wxyzs, translations, valid=None):
    """Camera-z images of organised world-point frames: ``frame_points`` [F, h, w, 3] (what ``FrameData`` and ``Fusion``'s frames
    hold, unprojected with the camera->world poses ``wxyzs`` / ``translations``) -> float64 [F, h, w], the z of
    ``rotate(p - t, inverse(q))``; 0 where a point is not finite or not ``valid`` ([F, h, w], optional).  NumPy in, NumPy out; device
    tensors in, a device tensor out."""
    q = np.asarray(wxyzs, dtype=np.float64).reshape(-1, 4)
    t = np.asarray(translations, dtype=np.float64).reshape(-1, 3)
    shape = tuple(frame_points.shape)
    if len(shape) != 4 or shape[3] != 3 or len(q) != shape[0] or len(t) != shape[0]:
        raise ValueError(f'frame_points must be [F, h, w, 3] with F poses, got {shape} and {len(q)} poses')
    F, h, w = shape[:3]
    qinv = [f3d.quat_inverse(q[f]) for f in range(F)]
    ctx = f3d.default_context()
    if not on_device(frame_points):
        pts = np.asarray(frame_points, dtype=np.float64)
        out = np.zeros((F, h, w))
        for f in range(F):
            cam = ctx.rotate((pts[f] - t[f]).reshape(-1, 3), qinv[f])
            ok = np.isfinite(pts[f]).all(axis=-1)
            if valid is not None:
                ok &= np.asarray(valid[f], dtype=bool).reshape(h, w)
            out[f][ok] = cam[:, 2].reshape(h, w)[ok]
        return out
    torch, dev = torch_device(ctx, 'depth_images')
    pts = frame_points.to(dev, torch.float64)
    out = torch.zeros((F, h, w), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev), work_stream(dev) as work:
        for f in range(F):
            rel = (pts[f] - upload(t[f], dev)).reshape(-1, 3).contiguous()
            cam = torch.empty_like(rel)
            ctx.rotate_dev(rel.data_ptr(), len(rel), qinv[f], cam.data_ptr(), work.cuda_stream)
            ok = torch.isfinite(pts[f]).all(dim=-1)
            if valid is not None:
                ok &= torch.as_tensor(valid[f], device=dev).to(torch.bool).reshape(h, w)
            out[f] = torch.where(ok, cam[:, 2].reshape(h, w), out[f])
    out.record_stream(torch.cuda.current_stream(dev))
    return out
