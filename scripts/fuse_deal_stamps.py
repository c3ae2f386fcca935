#!/usr/bin/env python
"""Reads the block stamps of a libf3d_hip.so built with -DF3D_EXP_STAMP (scripts/build_variant.sh stamp -DF3D_EXP_STAMP; the loader is
pointed at it through F3D_LIBRARY): one headline-shaped fused call (F3D_FUSE_SORT, 64 views, 1024^2 masks), then the head of the label
vector, where every block of the selected k_fuse instance left (index, clock at entry, at its first tile's turn, at its last wave's exit).

Per XCD (blockIdx.x & 7) the blocks are laid onto resident slots the way the dispatcher must have done it (a block that enters takes the
slot whose previous block ended last before that entry), and the script prints
  (a) tail idle: the mean over slots of (end of the kernel - end of the slot's last block),
  (b) the finish time of each XCD relative to the first one to finish,
  (c) the mean entry-to-first-tile time (a block's start-up),
and how many blocks, slots and start-ups there were.  Labels of a stamped build are wrong by construction."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / '3d-point-cloud-segmentation-using-2d-img-segmentation_amd'))
sys.path.insert(0, str(ROOT))

TICK_US = 0.01                                            # wall_clock64: 100 MHz
WORDS = 4 * 8192


def slots_of(entry, exit_):
    """Greedy reconstruction of resident slots from entry/exit times of one XCD's blocks -> last exit per slot."""
    order = np.argsort(entry, kind='stable')
    ends = []                                             # last exit of every slot opened so far
    for b in order:
        free = [k for k, e in enumerate(ends) if e <= entry[b]]
        if free:
            k = max(free, key=lambda k: ends[k])
            ends[k] = exit_[b]
        else:
            ends.append(exit_[b])
    return np.array(ends)


def analyse(st):
    st = st.reshape(-1, 4)
    ok = (st[:, 0] == np.arange(len(st))) & (st[:, 1] > 1000) & (st[:, 3] >= st[:, 2]) & (st[:, 2] >= st[:, 1])
    idx = np.flatnonzero(ok)
    if idx.size == 0:
        raise SystemExit('no stamps: is F3D_LIBRARY a -DF3D_EXP_STAMP build?')
    t0 = st[idx, 1].min()
    entry, first, exit_ = ((st[idx, c] - t0) * TICK_US for c in (1, 2, 3))
    end = exit_.max()
    xcd = idx & 7
    rows, idle_sum, nslots = [], 0.0, 0
    for x in range(8):
        m = xcd == x
        if not m.any():
            continue
        ends = slots_of(entry[m], exit_[m])
        idle_sum += float((end - ends).sum())
        nslots += len(ends)
        rows.append(dict(xcd=x, blocks=int(m.sum()), slots=len(ends), finish_us=round(float(exit_[m].max()), 2),
                         tail_idle_own_us=round(float((exit_[m].max() - ends).mean()), 2),
                         tail_idle_us=round(float((end - ends).mean()), 2)))
    fin = np.array([r['finish_us'] for r in rows])
    return dict(blocks=int(idx.size), slots=nslots, kernel_us=round(float(end), 2),
                tail_idle_us=round(idle_sum / nslots, 2),
                xcd_finish_spread_us=round(float(fin.max() - fin.min()), 2),
                startup_us=round(float((first - entry).mean()), 2), startup_p90_us=round(float(np.percentile(first - entry, 90)), 2),
                block_us_mean=round(float((exit_ - entry).mean()), 2),
                last_entry_us=round(float(entry.max()), 2), per_xcd=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--points', type=int, default=10_000_000)
    ap.add_argument('--views', type=int, default=64)
    ap.add_argument('--size', type=int, default=1024)
    ap.add_argument('--masks', default='block64')
    ap.add_argument('--calls', type=int, default=3, help='stamped calls analysed (after two warm-up calls)')
    ap.add_argument('--raw', metavar='NPY', default=None, help='also save the stamp words of the last call ([blocks, 4] int64)')
    args = ap.parse_args()
    import torch
    import f3d
    from f3d import synth
    if args.points < WORDS:
        raise SystemExit(f'a stamped build needs at least {WORDS} points')
    dev = torch.device('cuda', 0)
    ctx = f3d.Context(0)
    V, S, n = args.views, args.size, args.points
    K = np.array([[800., 0, S / 2], [0, 800., S / 2], [0, 0, 1]])
    q, t = synth.ring_views(V)
    views = torch.from_numpy(f3d.views_build(K, S, S, q, t, 10.0)).to(dev)
    xyz = torch.from_numpy(synth.cloud(n)).to(dev)
    masks = torch.from_numpy(synth.masks(V, S, S, args.masks)).to(dev)
    classes = torch.empty(n, dtype=torch.int64, device=dev)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    for call in range(2 + args.calls):
        ctx.project_vote_argmax_dev(xyz.data_ptr(), f3d.F64, n, views.data_ptr(), V, masks.data_ptr(), S, S, 133, 0.5, None,
                                    classes.data_ptr(), None, stream.cuda_stream, flags=f3d.FUSE_SORT, perm_ptr=None)
        stream.synchronize()
        if call >= 2:
            words = classes[:WORDS].cpu().numpy()
            if args.raw:
                np.save(args.raw, words.reshape(-1, 4))
            r = analyse(words)
            r.update(points=n, masks=args.masks, call=call - 2)
            print(json.dumps(r))


if __name__ == '__main__':
    main()
