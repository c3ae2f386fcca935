#!/usr/bin/env python3
"""PointVotingSegmentation at capture size: the fused radius search + frame vote (f3d_point_vote_frames_dev) against the composition
that exists without it -- PointCorrespondance's radius query on the device (every (pixel, point) pair materialised as CSR), a torch
``unique`` over (frame, point, label) and an ``index_add_`` -- alternated in one process, HIP-event times after a warm-up; pairs,
torch's peak allocation and the context's scratch for each; the two vote matrices compared bit for bit; sklearn on the host on a
slice of frames for context (scaled to the capture and flagged "extrapolated").  Run the script in several processes to see the
process-to-process noise.  One JSON line per radius, then one with all of them.

Scene of scripts/corr_stress.py (seeded): 256 frames of 192 x 256 pixels of a camera walking down a corridor, 5 % dropouts at the
camera centres, a cloud of 1M points drawn from the capture with 5 mm noise; masks in 32 x 32 blocks of labels 0 .. 133.
python scripts/point_vote_stress.py --radii 0.01,0.05"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / '3d-point-cloud-segmentation-using-2d-img-segmentation_amd'))
import f3d                     # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--frames', type=int, default=256)
ap.add_argument('--cloud', type=int, default=1_000_000)
ap.add_argument('--nclasses', type=int, default=133)
ap.add_argument('--radii', default='0.01,0.05')
ap.add_argument('--repeats', type=int, default=3, help='alternations of (fused, composition) after the warm-up')
ap.add_argument('--host-frames', type=int, default=1, help='frames of the sklearn slice')
ap.add_argument('--no-host', action='store_true')
ap.add_argument('--no-composition', action='store_true')
args = ap.parse_args()

import torch                   # noqa: E402

ctx = f3d.default_context()
dev = torch.device('cuda', ctx.device)
F, H, W, M, NCOLS = args.frames, 192, 256, args.cloud, args.nclasses + 1
HW = H * W


def capture(seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    f = 210.0 * W / 256
    v, u = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float64), torch.arange(W, device=dev, dtype=torch.float64), indexing='ij')
    dx, dy = (u - W / 2) / f, (v - H / 2) / f
    z = torch.minimum(torch.full_like(dx, 2.5), torch.where(dy > 1e-9, 1.2 / dy.clamp_min(1e-9), torch.full_like(dy, float('inf'))))
    out = torch.empty((F, HW, 3), dtype=torch.float64, device=dev)
    for j in range(F):
        zz = z + torch.randn(z.shape, generator=g, device=dev, dtype=torch.float64) * 0.001
        p = torch.stack([dx * zz + 0.5 * j, dy * zz, zz], -1).reshape(-1, 3)
        drop = torch.rand(HW, generator=g, device=dev) < 0.05
        p[drop] = torch.tensor([0.5 * j, 0.0, 0.0], dtype=torch.float64, device=dev)
        out[j] = p
    masks = ((u // 32 + (v // 32) * 8)[None] + torch.arange(F, device=dev, dtype=torch.float64)[:, None, None] * 5) % NCOLS
    return out, masks.to(torch.uint8).reshape(F, HW).contiguous()


points, masks = capture()
g1 = torch.Generator(device=dev).manual_seed(1)
flat = points.reshape(-1, 3)
cloud = (flat[torch.randint(0, len(flat), (M,), generator=g1, device=dev)] +
         torch.randn((M, 3), generator=g1, device=dev, dtype=torch.float64) * 0.005).contiguous()
stream = torch.cuda.Stream(dev)                  # (a null-stream handle would select the context's own stream)
votes = torch.zeros((M, NCOLS), dtype=torch.float64, device=dev)


def device_used():
    free, total = torch.cuda.mem_get_info(dev)
    return total - free


def fused(r):
    votes.zero_()
    ctx.point_vote_frames_dev(cloud.data_ptr(), f3d.F64, M, points.data_ptr(), f3d.F64, masks.data_ptr(), F, HW, r, votes.data_ptr(), NCOLS,
                              stream.cuda_stream)
    return votes


def composition(r):
    """Every pair in memory: the CSR of the radius query, one key per pair, a sort-based unique, two scatters."""
    offs = torch.empty(F * HW + 1, dtype=torch.int64, device=dev)
    nnz = ctx.radius_query_dev(cloud.data_ptr(), f3d.F64, M, flat.data_ptr(), f3d.F64, F * HW, r, offs.data_ptr(), stream.cuda_stream)
    nb = torch.empty(nnz, dtype=torch.int32, device=dev)
    ctx.radius_query_fill_dev(flat.data_ptr(), f3d.F64, F * HW, offs.data_ptr(), nb.data_ptr(), stream.cuda_stream)
    out = torch.zeros((M, NCOLS), dtype=torch.float64, device=dev)
    q = torch.repeat_interleave(torch.arange(F * HW, device=dev), offs[1:] - offs[:-1], output_size=nnz)
    key = ((q // HW) * M + nb.to(torch.int64)) * NCOLS + masks.reshape(-1)[q].to(torch.int64)
    del q
    ukey = torch.unique(key)                                        # sorted: (frame, point, label)
    del key
    one = torch.ones(1, dtype=torch.float64, device=dev)
    out.view(-1).index_add_(0, ukey % (M * NCOLS), one.expand(len(ukey)))
    seen = torch.unique_consecutive(ukey // NCOLS)                  # (frame, point)
    out.view(-1).index_add_(0, (seen % M) * NCOLS + (NCOLS - 1), one.expand(len(seen)))
    return out, nnz


def timed(fn, r):
    torch.cuda.synchronize(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        e0.record(stream)
        res = fn(r)
        e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1), torch.cuda.max_memory_allocated(dev) - base, res


def host_slice(r, nf):
    from sklearn.neighbors import KDTree
    c, p, m = cloud.cpu().numpy(), points[:nf].cpu().numpy(), masks[:nf].cpu().numpy()
    t0 = time.perf_counter()
    tree = KDTree(c, leaf_size=2)
    t_tree = time.perf_counter() - t0
    v = np.zeros((M, NCOLS))
    t0 = time.perf_counter()
    for j in range(nf):
        nns = tree.query_radius(p[j], r=r)
        freq = np.array([len(x) for x in nns])
        idx = np.hstack(nns).astype(np.int32)
        if idx.shape[0]:
            v[idx, np.repeat(m[j], freq)] += 1
            v[idx, -1] += 1
    return t_tree, time.perf_counter() - t0


results = []
for r in (float(x) for x in args.radii.split(',')):
    used0, reserved0 = device_used(), torch.cuda.memory_reserved(dev)
    timed(fused, r)                                                 # warm-up: scratch growth, code load
    torch.cuda.synchronize(dev)
    scratch = (device_used() - used0) - (torch.cuda.memory_reserved(dev) - reserved0)
    row = {'frames': F, 'hw': [H, W], 'cloud': M, 'ncols': NCOLS, 'radius': r, 'ctx_scratch_bytes_grown': int(scratch),
           'votes_bytes': votes.numel() * 8, 'fused_ms': [], 'fused_torch_peak_bytes': 0}
    if not args.no_composition:
        timed(composition, r)
        row.update(composition_ms=[], composition_torch_peak_bytes=0)
    for _ in range(args.repeats):
        ms, peak, got = timed(fused, r)
        row['fused_ms'].append(round(ms, 2)); row['fused_torch_peak_bytes'] = max(row['fused_torch_peak_bytes'], int(peak))
        if not args.no_composition:
            ms, peak, (want, nnz) = timed(composition, r)
            row['composition_ms'].append(round(ms, 2)); row['composition_torch_peak_bytes'] = max(row['composition_torch_peak_bytes'], int(peak))
            row['pairs'] = int(nnz)
            row['equal'] = bool(torch.equal(got, want))
            del want
    ctx.take_device_error(stream.cuda_stream)
    row['votes_cast'] = float(votes[:, :-1].sum()); row['points_seen'] = int((votes[:, -1] > 0).sum())
    row['fused_ms_median'] = float(np.median(row['fused_ms']))
    if not args.no_composition:
        row['composition_ms_median'] = float(np.median(row['composition_ms']))
    if not args.no_host:
        t_tree, secs = host_slice(r, args.host_frames)
        row['host'] = {'frames': args.host_frames, 'tree_s': round(t_tree, 2), 'vote_s': round(secs, 2),
                       's_extrapolated': round(t_tree + secs * F / args.host_frames, 1), 'extrapolated': True}
    print(json.dumps(row), flush=True)
    results.append(row)
    torch.cuda.empty_cache()
print(json.dumps({'point_vote_stress': results}))
