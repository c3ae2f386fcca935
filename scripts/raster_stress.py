#!/usr/bin/env python3
"""The triangle z-buffer at size, beside the point splat on the same inputs in the same process.  HIP events around every call after a
warm-up; a figure is the median of `--calls` calls, reported as [min, max] of that median over `--repeats` repetitions.

  huge   a wall of two triangles that fills one 1024 x 1024 view, against render_lookups_dev(splat=0) of one point per pixel of the
         same view (the same 2^20 winning cells, the same key buffer): both whole calls (fill + raster / splat + unpack), and the
         fill + raster / fill + splat parts from the device events inside the two diagnostics.  The condition fixed in advance
         (DESIGN section 7): the wall takes at most 4x the splat.
  fine   a box room (the synth box) as a grid mesh of about --triangles triangles, --views ring views at 1024 x 1024, float64 device
         tensors: fill + raster with the tier split (f3d_debug_raster_counts), meshUtils.label_faces, and
         fusion.project_vote_argmax_occluded on the mesh's vertices; for orientation fusion.render_lookups(splat=1) and
         fusion.project_vote_argmax_visible(splat=1) on the same vertices.
One JSON line per part.  python scripts/raster_stress.py [--part huge,fine] [--triangles 2000000] [--views 64]"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / '3d-point-cloud-segmentation-using-2d-img-segmentation_amd'))
import f3d                                        # noqa: E402
from f3d import synth                             # noqa: E402
from Fusion3DSeg import fusion                    # noqa: E402
from Fusion3DSeg.segUtils import meshUtils        # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--part', default='huge,fine')
ap.add_argument('--triangles', type=int, default=2_000_000)
ap.add_argument('--views', type=int, default=64)
ap.add_argument('--calls', type=int, default=10)
ap.add_argument('--repeats', type=int, default=3)
args = ap.parse_args()

import torch                                      # noqa: E402

ctx = f3d.default_context()
dev = torch.device('cuda', ctx.device)
H = W = 1024
MAX_DEPTH = 10.0


def timed(fn):
    s = torch.cuda.current_stream(dev)
    torch.cuda.synchronize(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    fn()
    e1.record(s)
    e1.synchronize()
    return e0.elapsed_time(e1)


def measure(fns):
    """{name: [min, max] over the repetitions of the median of args.calls calls}, the calls of the different names alternated"""
    for fn in fns.values():
        fn()                                      # warm-up: code load, scratch, the allocator's pools
    meds = {k: [] for k in fns}
    for _ in range(args.repeats):
        ts = {k: [] for k in fns}
        for _ in range(args.calls):
            for k, fn in fns.items():
                ts[k].append(fn() if getattr(fn, 'returns_ms', False) else timed(fn))
        for k in fns:
            meds[k].append(float(np.median(ts[k])))
    return {k: [round(min(v), 3), round(max(v), 3)] for k, v in meds.items()}


def grid(origin, eu, ev, nx, ny):
    i, j = np.meshgrid(np.arange(nx + 1.0), np.arange(ny + 1.0), indexing='ij')
    verts = np.asarray(origin, np.float64) + i.reshape(-1, 1) * np.asarray(eu, np.float64) + j.reshape(-1, 1) * np.asarray(ev, np.float64)
    vid = np.arange((nx + 1) * (ny + 1)).reshape(nx + 1, ny + 1)
    a, b, c, d = vid[:-1, :-1], vid[1:, :-1], vid[1:, 1:], vid[:-1, 1:]
    return verts, np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)]).astype(np.int64)


def part_huge():
    K = np.array([[700.0, 0.0, 512.0], [0.0, 700.0, 512.0], [0.0, 0.0, 1.0]])
    q, t = np.array([[1.0, 0.0, 0.0, 0.0]]), np.zeros((1, 3))
    origin, eu, ev = np.array([-3.0, -2.5, 2.0]), np.array([6.0, 0.0, 0.8]), np.array([0.0, 5.0, 0.5])
    verts, tris = grid(origin, eu, ev, 1, 1)
    n = np.cross(eu, ev)
    sx, sy = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    d = np.stack([(sx - 512.0) / 700.0, (sy - 512.0) / 700.0, np.ones_like(sx)], -1).reshape(-1, 3)
    pts = d * ((n @ origin) / (d @ n))[:, None]                                # one point per pixel, on the wall
    views = f3d.views_build(K, W, H, q, t, MAX_DEPTH)
    dv, dt, dp, dw = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (verts, tris, pts, views))
    depth = torch.empty((1, H, W), dtype=torch.float32, device=dev)
    lut = torch.empty((1, H * W), dtype=torch.int32, device=dev)
    strad = torch.empty(1, dtype=torch.int64, device=dev)
    sh = lambda: torch.cuda.current_stream(dev).cuda_stream                      # noqa: E731
    mesh = (dv.data_ptr(), f3d.F64, len(verts), dt.data_ptr(), f3d.I64, len(tris))

    def diag_mesh():
        c = ctx.raster_counts_dev(*mesh, dw.data_ptr(), 1, H, W, MAX_DEPTH, 0, None, None, sh())
        return c['fill_ms'] + c['raster_ms']

    def diag_splat():
        c = ctx.render_counts_dev(dp.data_ptr(), f3d.F64, len(pts), dw.data_ptr(), 1, H, W, 0, sh())
        return c['fill_ms'] + c['splat_ms']

    diag_mesh.returns_ms = diag_splat.returns_ms = True
    with torch.cuda.stream(torch.cuda.Stream(dev)):
        out = measure({
            'wall_call_ms': lambda: ctx.render_mesh_lookups_dev(*mesh, dw.data_ptr(), 1, H, W, MAX_DEPTH, depth.data_ptr(), lut.data_ptr(),
                                                                strad.data_ptr(), sh()),
            'splat_call_ms': lambda: ctx.render_lookups_dev(dp.data_ptr(), f3d.F64, len(pts), dw.data_ptr(), 1, H, W, 0, depth.data_ptr(),
                                                            lut.data_ptr(), sh()),
            'wall_fill_raster_ms': diag_mesh,
            'splat_fill_splat_ms': diag_splat})
        ctx.render_mesh_lookups_dev(*mesh, dw.data_ptr(), 1, H, W, MAX_DEPTH, depth.data_ptr(), lut.data_ptr(), strad.data_ptr(), sh())
        filled_mesh = float((lut >= 0).float().mean())
        ctx.render_lookups_dev(dp.data_ptr(), f3d.F64, len(pts), dw.data_ptr(), 1, H, W, 0, depth.data_ptr(), lut.data_ptr(), sh())
        filled_splat = float((lut >= 0).float().mean())
        tiers = ctx.raster_counts_dev(*mesh, dw.data_ptr(), 1, H, W, MAX_DEPTH, 0, None, None, sh())
    out.update(part='huge', hw=[H, W], filled_mesh=filled_mesh, filled_splat=filled_splat, tiers={k: tiers[k] for k in ('small', 'medium', 'huge', 'overflow')},
               ratio_calls=round(out['wall_call_ms'][1] / out['splat_call_ms'][0], 3),
               ratio_fill_raster=round(out['wall_fill_raster_ms'][1] / out['splat_fill_splat_ms'][0], 3))
    out['within_4x'] = bool(out['ratio_calls'] <= 4.0 and out['ratio_fill_raster'] <= 4.0)      # worst wall over best splat
    print(json.dumps(out), flush=True)


def part_fine():
    V = args.views
    cell = np.sqrt(320.0 / (args.triangles / 2.0))                              # the box has 320 m^2 of surface
    n10, n3 = max(int(round(10.0 / cell)), 1), max(int(round(3.0 / cell)), 1)
    faces = [([-5, -5, 0], [10.0 / n10, 0, 0], [0, 10.0 / n10, 0], n10, n10), ([-5, -5, 3], [10.0 / n10, 0, 0], [0, 10.0 / n10, 0], n10, n10),
             ([-5, -5, 0], [10.0 / n10, 0, 0], [0, 0, 3.0 / n3], n10, n3), ([-5, 5, 0], [10.0 / n10, 0, 0], [0, 0, 3.0 / n3], n10, n3),
             ([-5, -5, 0], [0, 10.0 / n10, 0], [0, 0, 3.0 / n3], n10, n3), ([5, -5, 0], [0, 10.0 / n10, 0], [0, 0, 3.0 / n3], n10, n3)]
    vs, ts, off = [], [], 0
    for f in faces:
        v, t = grid(*f)
        vs.append(v); ts.append(t + off); off += len(v)
    verts, tris = np.concatenate(vs), np.concatenate(ts)
    K = np.array([[0.8 * W, 0.0, W / 2.0], [0.0, 0.8 * W, H / 2.0], [0.0, 0.0, 1.0]])
    q, t = synth.ring_views(V)
    masks = synth.masks(V, H, W, 'block64')
    views = f3d.views_build(K, W, H, q, t, MAX_DEPTH)
    dv, dt, dm, dw = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (verts, tris, masks, views))
    mesh = (dv.data_ptr(), f3d.F64, len(verts), dt.data_ptr(), f3d.I64, len(tris))
    keep = {}

    def diag():
        c = ctx.raster_counts_dev(*mesh, dw.data_ptr(), V, H, W, MAX_DEPTH, 0, None, None, torch.cuda.current_stream(dev).cuda_stream)
        keep.update(c)
        return c['fill_ms'] + c['raster_ms']

    diag.returns_ms = True
    out = measure({
        'fill_raster_ms': diag,
        'label_faces_ms': lambda: meshUtils.label_faces(dv, dt, K, q, t, dm, MAX_DEPTH),
        'occluded_ms': lambda: fusion.project_vote_argmax_occluded(dv, dv, dt, K, q, t, dm, MAX_DEPTH),
        'splat1_render_lookups_ms': lambda: fusion.render_lookups(dv, K, q, t, (H, W), MAX_DEPTH, 1),
        'splat1_visible_ms': lambda: fusion.project_vote_argmax_visible(dv, K, q, t, dm, MAX_DEPTH, splat=1)})
    pairs = len(tris) * V
    faces_cls = meshUtils.label_faces(dv, dt, K, q, t, dm, MAX_DEPTH)
    lut = fusion.render_mesh_lookups(dv, dt, K, q, t, (H, W), MAX_DEPTH)
    out.update(part='fine', triangles=len(tris), vertices=len(verts), views=V, hw=[H, W], pairs=pairs,
               tiers={k: keep[k] for k in ('small', 'medium', 'huge', 'overflow')},
               filled_pixels=float((lut[1] >= 0).float().mean()), straddling=int(lut[2].sum()), labelled_faces=int((faces_cls != 133).sum()))
    print(json.dumps(out), flush=True)


for part in args.part.split(','):
    {'huge': part_huge, 'fine': part_fine}[part]()
