#!/usr/bin/env python3
"""The point-splat z-buffer and the visibility-tested forward vote at the C3 size of f3d/synth.py (10M points x 64 views x 1024 x 1024),
splat 0 and 1, beside the fused forward path (Context.project_vote_argmax_dev) on the same inputs in the same process.  HIP-event
times after a warm-up of every shape, the calls alternated `--repeats` times:
  fill_ms, splat_ms   the key fill and the splat kernel, device events inside f3d_debug_render_counts (the counting build of the
                      splat kernel: three more register adds per sample), with the samples, the cells they cover and the atomics
                      that were issued (the rest found a smaller key in the cell and skipped theirs);
  render_ms           render_lookups_dev: fill + splat + unpack of every pass, uv2pt and depth written;
  visible_vote_ms     vote_visible_dev: fill + splat + vote of every pass;  vote_ms = visible_vote_ms - fill_ms - splat_ms (derived);
  segment_ms          segment_votes_dev over the float64 votes;
  forward_ms          project_vote_argmax_dev (cell sort inside the call), classes only.
One JSON line per splat.  Kernel-by-kernel times: run it under `rocprofv3 --kernel-trace --stats -- python scripts/render_stress.py`.
python scripts/render_stress.py [--config C3] [--n N]"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / '3d-point-cloud-segmentation-using-2d-img-segmentation_amd'))
import f3d                     # noqa: E402
from f3d import synth          # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--config', default='C3')
ap.add_argument('--n', type=int, default=None)
ap.add_argument('--repeats', type=int, default=3)
ap.add_argument('--depth-tol', type=float, default=0.05)
ap.add_argument('--splats', default='0,1')
args = ap.parse_args()

import torch                   # noqa: E402

ctx = f3d.default_context()
dev = torch.device('cuda', ctx.device)
sc = synth.scene(args.config, n=args.n)
N, V, H, W, NCLS = len(sc['points']), len(sc['masks']), sc['h'], sc['w'], sc['nclasses']
views = f3d.views_build(sc['K'], W, H, sc['wxyzs'], sc['translations'], sc['max_depth'])
xyz, dviews, masks = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (sc['points'], views, sc['masks']))
votes = torch.zeros((N, NCLS + 1), dtype=torch.float64, device=dev)
classes = torch.empty(N, dtype=torch.int64, device=dev)
forward = torch.empty(N, dtype=torch.int64, device=dev)
depth = torch.empty((V, H, W), dtype=torch.float32, device=dev)
uv2pt = torch.empty((V, H * W), dtype=torch.int32, device=dev)
stream = torch.cuda.Stream(dev)                  # (a null-stream handle would select the context's own stream)
ctx.reserve(N, V, H, W)
ctx.reserve_render(N, V, H, W)
X, D, M, sh = xyz.data_ptr(), dviews.data_ptr(), masks.data_ptr(), stream.cuda_stream


def timed(fn):
    torch.cuda.synchronize(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


def calls(splat):
    return {
        'render_ms': lambda: ctx.render_lookups_dev(X, f3d.F64, N, D, V, H, W, splat, depth.data_ptr(), uv2pt.data_ptr(), sh),
        'visible_vote_ms': lambda: ctx.vote_visible_dev(X, f3d.F64, N, D, V, M, H, W, splat, args.depth_tol, votes.data_ptr(), NCLS + 1, 0, sh),
        'segment_ms': lambda: ctx.segment_votes_dev(votes.data_ptr(), N, NCLS + 1, NCLS, 0.5, None, classes.data_ptr(), sh),
        'forward_ms': lambda: ctx.project_vote_argmax_dev(X, f3d.F64, N, D, V, M, H, W, NCLS, 0.5, None, forward.data_ptr(), None, sh, f3d.FUSE_SORT),
    }


for splat in (int(x) for x in args.splats.split(',')):
    fns = calls(splat)
    for fn in fns.values():                      # warm-up: code load, scratch
        fn()
    ctx.render_counts_dev(X, f3d.F64, N, D, V, H, W, splat, sh)
    row = {'config': args.config, 'n': N, 'views': V, 'hw': [H, W], 'splat': splat, 'depth_tol': args.depth_tol, 'fill_ms': [], 'splat_ms': []}
    row.update({k: [] for k in fns})
    for _ in range(args.repeats):
        votes.zero_()
        for k, fn in fns.items():
            row[k].append(round(timed(fn), 3))
        c = ctx.render_counts_dev(X, f3d.F64, N, D, V, H, W, splat, sh)
        row['fill_ms'].append(round(c['fill_ms'], 3)); row['splat_ms'].append(round(c['splat_ms'], 3))
    ctx.take_device_error(sh)
    row.update(samples=c['samples'], cells=c['cells'], atomics=c['atomics'], atomic_fraction=round(c['atomics'] / max(c['cells'], 1), 4))
    med = {k: float(np.median(row[k])) for k in list(fns) + ['fill_ms', 'splat_ms']}
    med['vote_ms_derived'] = round(med['visible_vote_ms'] - med['fill_ms'] - med['splat_ms'], 3)
    row['median'] = med
    row['filled_pixels'] = float((uv2pt >= 0).float().mean())
    row['labelled_visible'], row['labelled_forward'] = int((classes != NCLS).sum()), int((forward != NCLS).sum())
    row['labels_changed_by_the_test'] = int((classes != forward).sum())
    print(json.dumps(row), flush=True)
