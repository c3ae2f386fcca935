"""``generate_mesh`` of the reference's Fusion3DSeg/segUtils/door_window_bbox.py (:65-150) on the GPU.

Every door / window instance of the panoptic result (category 86, 115 or 116, in ``info`` order) is snapped to the triangle of the
PolyFit mesh its points lie on, and replaced by a quad in that triangle's plane spanned by the extents of its projected points.
The quads go to ``panoptic_segmentation/door_window_mesh.ply``, the instance id of every quad triangle to ``triangle_ids.npy``.

The whole per-instance computation (triangle normals, distance sums over points x triangles, the candidate band, the inside
counts, the basis and the extents) is one f3d_door_window_quads call (csrc/f3d_quads.hip); this module reads and writes files
and assembles the mesh.  There is no CPU fallback.  Open3D is not needed: the OFF reader and the PLY writer are restated here and
in get3DSeg (``TriangleMesh``, ``write_triangle_mesh``); their rules (fan triangulation of polygon faces, the triangle normal,
the PLY layout) are listed in DESIGN §7.

Like the reference, a door / window instance without a candidate triangle (no points, a distance sum of 0 or not finite), a
mesh without triangles, or no quad kept at all raise ValueError.
"""
import json
import pickle
from pathlib import Path

import numpy as np

import f3d
from f3d.tensors import on_device, work_stream

DOOR_WINDOW = (86, 115, 116)                   # :72


def _hex_to_rgb(hex_color):
    hex_color = hex_color.lstrip('#')
    return tuple(int(hex_color[i:i + 2], 16) for i in (0, 2, 4))


def read_off(path):
    """Vertices float64 [V, 3] and triangles int64 [T, 3] of an OFF file (``OFF`` or ``COFF`` header, ``#`` comments); a face of
    n > 3 vertices becomes the fan (f0, fj, fj+1), j = 1 .. n - 2; per-face colours are ignored."""
    toks = []
    for line in Path(path).read_text().splitlines():
        line = line.split('#', 1)[0].strip()
        if line:
            toks += line.split()
    if not toks or toks[0] not in ('OFF', 'COFF'):
        raise ValueError(f'{path}: not an OFF file')
    stride = 3 if toks[0] == 'OFF' else 7
    try:
        nv, nf = int(toks[1]), int(toks[2])
        at = 4
        verts = np.array(toks[at:at + stride * nv], dtype=np.float64).reshape(nv, stride)[:, :3]
        at += stride * nv
        tris = []
        for _ in range(nf):
            m = int(toks[at])
            f = [int(x) for x in toks[at + 1:at + 1 + m]]
            if len(f) != m or m < 3:
                raise ValueError
            at += 1 + m
            while at < len(toks) and '.' in toks[at]:         # optional face colour
                at += 1
            tris += [[f[0], f[j], f[j + 1]] for j in range(1, m - 1)]
    except (ValueError, IndexError) as exc:
        raise ValueError(f'{path}: truncated or malformed OFF file') from exc
    return np.ascontiguousarray(verts), np.array(tris, dtype=np.int64).reshape(-1, 3)


def _door_window_entries(info):
    return [d for d in info if d['category_id'] in set(DOOR_WINDOW)]


def _run(ctx, points, ids, uniq, vertices, triangles):
    """(quads [k, 4, 3], status [k], chosen triangle [k]) as NumPy arrays, for the distinct instance ids `uniq`."""
    if on_device(points):
        import torch
        dev = points.device
        pts = points.to(torch.float64).contiguous()
        if pts.ndim != 2 or pts.shape[1] != 3:
            raise ValueError(f'points must be [N, 3], got {tuple(pts.shape)}')
        ids_d = torch.as_tensor(ids, device=dev).to(torch.int64).reshape(-1).contiguous()
        if len(ids_d) != len(pts):
            raise ValueError(f'{len(ids_d)} ids for {len(pts)} points')
        verts = torch.as_tensor(vertices, device=dev).to(torch.float64).reshape(-1, 3).contiguous()
        tris = torch.as_tensor(triangles, device=dev).to(torch.int64).reshape(-1, 3).contiguous()
        inst = torch.as_tensor(np.asarray(uniq, np.int64), device=dev)
        k = len(uniq)
        quads = torch.empty((k, 4, 3), dtype=torch.float64, device=dev)
        status = torch.empty(k, dtype=torch.int32, device=dev)
        tri = torch.empty(k, dtype=torch.int32, device=dev)
        with work_stream(dev) as work:
            ctx.door_window_quads_dev(pts.data_ptr(), len(pts), ids_d.data_ptr(), inst.data_ptr(), k, verts.data_ptr(), len(verts),
                                      tris.data_ptr(), len(tris), quads.data_ptr(), status.data_ptr(), tri.data_ptr(), None,
                                      work.cuda_stream)
            ctx.take_device_error(work.cuda_stream)          # synchronises the stream: the results are complete
        return quads.cpu().numpy(), status.cpu().numpy(), tri.cpu().numpy()
    quads, status, tri, _ = ctx.door_window_quads(points, ids, uniq, vertices, triangles)
    return quads, status, tri


def door_window_quads(points, ids, info, vertices, triangles, ctx=None):
    """The array-level generate_mesh: -> (triangle_ids int32 [2k], quad vertices float64 [4k, 3], quad triangles int64 [2k, 3],
    vertex colours float64 [4k, 3]) for the door / window entries of `info` (in order) that are not skipped as horizontal.
    points [N, 3] / ids [N] / vertices [V, 3] / triangles [T, 3] are NumPy arrays or device tensors (then the call runs on the
    tensors' device, ordered after the current stream)."""
    shape = tuple(points.shape) if hasattr(points, 'shape') else np.shape(points)
    nids = int(np.prod(tuple(ids.shape))) if hasattr(ids, 'shape') else len(ids)
    vshape = tuple(vertices.shape) if hasattr(vertices, 'shape') else np.shape(vertices)
    tshape = tuple(triangles.shape) if hasattr(triangles, 'shape') else np.shape(triangles)
    if len(shape) != 2 or shape[1] != 3:
        raise ValueError(f'points must be [N, 3], got {shape}')
    if nids != shape[0]:
        raise ValueError(f'{nids} ids for {shape[0]} points')              # the boolean mask ids == id must match the points
    if (len(vshape) != 2 or vshape[1] != 3) and vshape != (0,):
        raise ValueError(f'vertices must be [V, 3], got {vshape}')
    if (len(tshape) != 2 or tshape[1] != 3) and tshape != (0,):
        raise ValueError(f'triangles must be [T, 3], got {tshape}')
    entries = _door_window_entries(info)
    ntri = tshape[0] if len(tshape) == 2 else 0
    if entries and ntri == 0:
        raise ValueError('attempt to get argmin of an empty sequence')          # tri_dist.argmin() on an empty mesh (:96)
    if not entries:
        raise ValueError('need at least one array to concatenate')               # np.vstack([]) (:140)
    wanted = np.array([int(d['id']) for d in entries], np.int64)
    ctx = ctx or f3d.default_context(points.device.index if on_device(points) else None)
    uniq, slot = np.unique(wanted, return_inverse=True)
    quads, status, _ = _run(ctx, points, ids, uniq, vertices, triangles)
    status, quads = status[slot], quads[slot]
    if (status == f3d.QUAD_NO_CANDIDATE).any():
        raise ValueError('attempt to get argmax of an empty sequence')           # np.argmax of no candidate (:111)
    keep = np.nonzero(status == f3d.QUAD_OK)[0]
    if not len(keep):
        raise ValueError('need at least one array to concatenate')
    abc = np.array([[0, 1, 2], [2, 3, 0]])
    verts = quads[keep].reshape(-1, 3)
    faces = np.vstack([abc + 4 * b for b in range(len(keep))])
    colors = np.vstack([[_hex_to_rgb(entries[e]['hexcolor'])] * 4 for e in keep]) / 255
    tids = np.repeat(wanted[keep], 2).astype(np.int32)
    return tids, verts, faces, colors


def door_window_mesh(points, ids, info, vertices, triangles, filename=None, ctx=None):
    """-> (triangle_ids, TriangleMesh) of door_window_quads; the mesh is written to `filename` as PLY when given."""
    from get3DSeg import TriangleMesh, write_triangle_mesh
    tids, verts, faces, colors = door_window_quads(points, ids, info, vertices, triangles, ctx)
    mesh = TriangleMesh(verts, faces, colors)
    if filename is not None:
        Path(filename).parent.mkdir(exist_ok=True, parents=True)
        write_triangle_mesh(filename, mesh)
    return tids, mesh


def generate_mesh(input_dir, *args, **kwargs):
    """fusion/fusion_data.pkl + panoptic_segmentation/{ids.npy, info.json} + the first polyfit/*.off -> door_window_mesh.ply and
    triangle_ids.npy under panoptic_segmentation/; returns (triangle_ids, mesh) (:65-150)."""
    dirname = Path(input_dir)
    with (dirname / 'fusion/fusion_data.pkl').open('rb') as fp:
        data = pickle.load(fp)
    pts = np.asarray(data['points'])
    ids = np.load(dirname / 'panoptic_segmentation/ids.npy')
    with open(dirname / 'panoptic_segmentation/info.json') as fp:
        info = json.load(fp)
    vertices, triangles = read_off(str(list((dirname / 'polyfit').glob('*.off'))[0]))
    triangle_ids, mesh = door_window_mesh(pts, ids, info, vertices, triangles,
                                          filename=str(dirname / 'panoptic_segmentation/door_window_mesh.ply'))
    np.save(dirname / 'panoptic_segmentation/triangle_ids.npy', triangle_ids)
    return triangle_ids, mesh
