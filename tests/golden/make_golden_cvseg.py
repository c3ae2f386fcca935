#!/usr/bin/env python3
"""Generate tests/golden/cvseg.npz by RUNNING the reference's CVSegmentation (Fusion3DSeg/segUtils/cv.py, NumPy only) here.

Run in the build container only (needs the reference checkout):   python tests/golden/make_golden_cvseg.py [REFERENCE_ROOT]

Small radius graphs with shuffled row order; instance_seperate with instance_classes None, a list with 0 last (the class-0
re-flood), a duplicate class, a repeated 0 with relabelling in between, minimum_points 1 and > 1; color_segment with a scalar and a
3-tuple threshold, neutral ids (0,) and (0, k), seeds whose id an earlier seed overwrote, a seed inside a neutral region,
max_level 0 (no limit), 1, 2, 3, 4 and 10, float64 and float32 colours.  The independent restatement (tests/cvseg_ref.py) is checked against the
reference before anything is written.
"""
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
REF = Path(sys.argv[1] if len(sys.argv) > 1 else '/root/reference')
sys.dont_write_bytecode = True
sys.path.insert(0, str(REF))
sys.path.insert(0, str(HERE.parent))

import cvseg_ref as R  # noqa: E402


def graph(rng, n, r):
    xy = rng.uniform(0, 10, (n, 2))
    d2 = ((xy[:, None, :] - xy[None, :, :]) ** 2).sum(-1)
    rows = [rng.permutation(np.nonzero(d2[i] < r * r)[0]).astype(np.int64) for i in range(n)]   # shuffled row order
    return xy, rows


def csr(rows):
    offs = np.cumsum([0] + [len(a) for a in rows]).astype(np.int64)
    return offs, np.concatenate(rows).astype(np.int64)


def main():
    from Fusion3DSeg.segUtils.cv import CVSegmentation
    rng = np.random.default_rng(20261016)
    g = {}
    graphs = []
    for gi, (n, r, labels, p) in enumerate([(140, 1.3, [0, 5, 7, 9], [0.2, 0.35, 0.3, 0.15]),
                                            (120, 1.0, [0, 3, 5, 7], [0.15, 0.3, 0.3, 0.25]),
                                            (90, 1.6, [2, 5, 7], [0.4, 0.3, 0.3])]):
        xy, rows = graph(rng, n, r)
        cls = rng.choice(labels, n, p=p).astype(np.int64)
        offs, nb = csr(rows)
        g[f'g{gi}_classes'], g[f'g{gi}_offsets'], g[f'g{gi}_neighbours'], g[f'g{gi}_xy'] = cls, offs, nb, xy
        graphs.append((cls, rows))
    g['ngraphs'] = np.array(len(graphs))

    icases = [(0, None, 1), (0, None, 4), (0, [5, 7, 0], 3), (0, [5, 5, 7], 3), (0, [7, 0, 5, 0], 4), (0, [9], 1),
              (1, None, 3), (1, [3, 5, 0], 5), (1, [7], 2), (2, None, 1), (2, [5, 2], 6)]
    for k, (gi, ic, mp) in enumerate(icases):
        cls, rows = graphs[gi]
        c_ref, c_mine = cls.copy(), cls.copy()
        want = CVSegmentation(c_ref, rows).instance_seperate(ic, mp)
        mine = R.instance_seperate(c_mine, rows, ic, mp)
        a, b = {}, {}
        R.encode_instances(want, 'x', a)
        R.encode_instances(mine, 'x', b)
        assert all(np.array_equal(a[key], b[key]) for key in a), f'restatement differs from the reference in instance case {k}'
        assert np.array_equal(c_ref, c_mine)
        p = f'i{k}_'
        g[p + 'graph'] = np.array(gi)
        g[p + 'has_instance_classes'] = np.array(ic is not None)
        g[p + 'instance_classes'] = np.array([] if ic is None else ic, np.int64)
        g[p + 'minimum_points'] = np.array(mp)
        g[p + 'classes_after'] = c_ref
        R.encode_instances(want, p, g)
    g['nicases'] = np.array(len(icases))

    # colour cases: ids of an instance case with a neutral (0) region, smooth colours with a few outliers
    ccases = [(0, 1, 0.3, (0,), 10, np.float64, 'first'), (0, 1, (0.2, 0.4, 0.3), (0, 3), 2, np.float64, 'overwrite'), (0, 1, (0.3, 0.4, 0.3), (0, 3), 4, np.float64, 'overwrite'),
              (0, 4, 0.25, (0,), 1, np.float64, 'first'), (1, 7, 0.35, (0, 2), 10, np.float32, 'neutral'),
              (1, 6, (0.5, 0.3, 0.4), (0,), 3, np.float32, 'overwrite'), (2, 9, 0.4, (0, 1), 10, np.float64, 'neutral'),
              (2, 10, 0.15, (0,), 10, np.float32, 'first'), (0, 4, 1, (0, 2), 0, np.float64, 'neutral')]
    for k, (gi, ik, thr, neutral, ml, dt, how) in enumerate(ccases):
        cls, rows = graphs[gi]
        xy = g[f'g{gi}_xy']
        ids0 = g[f'i{ik}_ids'].copy()
        ids0[(xy[:, 0] > 3 + k % 3) & (xy[:, 1] < 7)] = 0                  # a neutral region around the seeds' instances
        colors = np.stack([np.sin(xy[:, 0]), np.cos(xy[:, 1]), np.sin(0.5 * (xy[:, 0] + xy[:, 1]))], 1) * 0.5 + 0.5
        colors[rng.choice(len(xy), 6, replace=False)] = rng.uniform(0, 1, (6, 3))
        colors = colors.astype(dt)
        neutral_pts = np.nonzero(np.isin(ids0, neutral))[0]
        other = np.nonzero(~np.isin(ids0, neutral))[0]
        seeds = list(rng.choice(other, 4, replace=False))
        if how == 'neutral' and len(neutral_pts):
            seeds.insert(1, rng.choice(neutral_pts))
        if how == 'overwrite':
            # a seed that an earlier seed's flood takes: run the first seed alone and pick a point it relabelled
            probe = CVSegmentation(cls.copy(), rows).color_segment(colors, ids0.copy(), seeds[:1], thr, neutral, ml)
            taken = np.nonzero((probe != ids0))[0]
            if len(taken):
                seeds.append(taken[-1])
        seeds = np.array(seeds, np.int64)
        want = CVSegmentation(cls.copy(), rows).color_segment(colors, ids0.copy(), seeds, thr, neutral, ml)
        mine = R.color_segment(None, rows, colors, ids0.copy(), seeds, thr, neutral, ml)
        assert np.array_equal(want, mine), f'restatement differs from the reference in colour case {k}'
        p = f'c{k}_'
        g[p + 'graph'], g[p + 'ids_in'], g[p + 'colors'], g[p + 'seeds'] = np.array(gi), ids0, colors, seeds
        g[p + 'threshold'] = np.array(thr, np.float64)
        g[p + 'threshold_is_scalar'] = np.array(np.ndim(thr) == 0)
        g[p + 'neutral_ids'] = np.array(neutral, np.int64)
        g[p + 'max_level'] = np.array(ml)
        g[p + 'ids_out'] = want
        g[p + 'changed'] = np.array(int((want != ids0).sum()))
    g['nccases'] = np.array(len(ccases))
    np.savez_compressed(HERE / 'cvseg.npz', **g)
    print(f'wrote {HERE / "cvseg.npz"}: {(HERE / "cvseg.npz").stat().st_size} bytes, {len(icases)} instance / {len(ccases)} colour cases',
          [int(g[f'c{k}_changed']) for k in range(len(ccases))])


if __name__ == '__main__':
    main()
