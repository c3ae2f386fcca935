#!/usr/bin/env python3
"""Fusion.fuse on a synthetic capture (f3d.synth.depth_sequence): wall-clock per frame of the drop-in (NumPy frames in, NumPy cloud
out; the frame loop runs on the GPU with the cloud resident).  With --device, Fusion.fuse and Fusion.fuse_device (the same loop, the
cloud and lookups left on the device) run alternately on the same frames and seed: ms per frame of each and the host shuffle's share
are printed."""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / '3d-point-cloud-segmentation-using-2d-img-segmentation_amd'))
from f3d import synth                      # noqa: E402
from Fusion3DSeg.fusion import Fusion      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--frames', type=int, default=12)
ap.add_argument('--height', type=int, default=192)
ap.add_argument('--width', type=int, default=256)
ap.add_argument('--step', type=float, default=0.03, help='camera translation per frame in metres (small = high overlap, as in a real capture)')
ap.add_argument('--device', action='store_true', help='also run Fusion.fuse_device on the same frames, alternating with fuse')
ap.add_argument('--repeats', type=int, default=2, help='with --device: runs of each path (the first of each is a warm-up)')
args = ap.parse_args()
K, q, t, frames = synth.depth_sequence(args.height, args.width, args.frames, step=args.step)


def run(device):
    """One fuse / fuse_device call on fresh copies of the frames (fuse consumes the masks) -> seconds, fused points, the object."""
    import torch
    luts = {}
    copies = [(n, p, nn, c, v.copy()) for n, p, nn, c, v in frames]
    fu = Fusion.from_frames(K, args.width, args.height, q, t, copies,
                            lookup_sink=lambda name, lut: luts.__setitem__(name, lut if device else np.array(lut, copy=True)))
    np.random.seed(1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fu.fuse_device(0.05, 10, None, 10, 1) if device else fu.fuse(0.05, 10, None, 10, 1)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, len(out[0]), fu


if args.device:
    times = {False: [], True: []}
    for r in range(args.repeats):
        (ht, _, _), (dtime, npts, dfu) = run(False), run(True)
        times[False].append(ht)
        times[True].append(dtime)
        st = dfu.fuse_device_stats
        print(f'run {r}: fuse {1e3 * ht / args.frames:.2f} ms/frame, fuse_device {1e3 * dtime / args.frames:.2f} ms/frame '
              f'(host shuffle {1e3 * st["shuffle_s"] / args.frames:.2f} ms/frame, {st["rounds"]} seed rounds, '
              f'{st["sequential_frames"]} sequential frames, {st["draws_undone"]} draws undone, {st["capacity_growths"]} growths); '
              f'{npts} fused points')
    best = {k: min(v[1:] or v) for k, v in times.items()}
    print(f'fuse_stress --device: {args.frames} frames of {args.height}x{args.width}: fuse {1e3 * best[False] / args.frames:.2f} ms/frame, '
          f'fuse_device {1e3 * best[True] / args.frames:.2f} ms/frame (best of the runs after the first)')
    sys.exit(0)
fu = Fusion.from_frames(K, args.width, args.height, q, t, frames)
np.random.seed(1)
t0 = time.perf_counter()
pts, nrm, clr, nmerges, occ = fu.fuse(0.05, 10, None, 10, 1)
dt = time.perf_counter() - t0
print(f'fuse: {args.frames} frames of {args.height}x{args.width}: {dt:.2f} s = {1e3 * dt / args.frames:.0f} ms per frame; '
      f'{len(pts)} fused points from {args.frames * args.height * args.width} pixels, occurrences up to {int(occ.max())}')
