#!/usr/bin/env python3
"""Golden vectors of the reference's PointVotingSegmentation (Fusion3DSeg/segUtils/voting.py), run from the reference.

Run in the build container (the reference is mounted at /root/reference): ``python tests/golden/make_golden_point_voting.py``.
Like make_golden_correspondance.py, the class is compiled from the reference's file by ``ast``; nothing of it is copied.  The
namespace holds NumPy, os, sklearn's KDTree and a stand-in ``cv2`` whose ``imread`` reads 8-bit PNGs through Pillow (``resize=False``
everywhere, so ``cv2.resize`` is never reached).

Coordinates sit on a 1/64 m lattice and r = 5/64, so many pairs lie exactly on r*r and all arithmetic is exact.  Contents:
* ``sig_*``: ``str(inspect.signature(...))`` of the constructor and the methods;
* ``cloud``, ``frames`` [4, 192, 3], ``frame_numbers`` (the frames' ``frameNumber``), ``radius``, ``hw``, ``nclasses``; 10 % dropout
  pixels sit at their camera centre (a clump of cloud points waits at camera 1), a few pixels are far from every cloud point;
* ``a_masks`` [4, 192] with labels 0 .. nclasses, ``a_present`` (frame 1 has no mask file): ``a_votes_all`` = vote(),
  ``a_votes_skip2`` = vote(skip=2), ``a_votes_subset`` = vote(frame_numbers=a_subset), ``a_votes_twice`` = two vote() calls;
* ``b_masks``: label 200 on pixels without a neighbour: no error, ``b_votes``;
* ``c_masks``: label 200 on a pixel with neighbours in frame 2 of 4: ``c_error`` names the exception, ``c_votes`` what the object
  holds after it;
* ``d_votes`` (a_votes_all plus hand-made rows), ``d_thresholds``, ``d_filter_<k>`` / ``d_classes_<k>_<t>`` (k = 0: no filter),
  ``d_file_nclasses`` / ``d_file_classes``: a votes_file round trip;
* ``e_nns`` / ``e_frequency``: get_nns(frames[0], radius).
"""
import inspect
import os
import sys
import tempfile
import types
from pathlib import Path

import numpy as np
from PIL import Image
from sklearn.neighbors import KDTree

OUT = Path(__file__).resolve().parent
sys.path.insert(0, str(OUT))
from make_golden import _defs_from  # noqa: E402
from make_golden_correspondance import frames as lattice_frames  # noqa: E402

PREFIX, EXT, ZFILL = 'm_', 'png', 3


def _imread(path, flag):
    assert flag == 0
    with Image.open(path) as im:
        return np.asarray(im.convert('L'), dtype=np.uint8)


def write_masks(dirname, masks, present, numbers, hw):
    for m, p, n in zip(masks, present, numbers):
        if p:
            Image.fromarray(m.reshape(hw)).save(os.path.join(dirname, PREFIX + str(n).zfill(ZFILL) + '.' + EXT))


def main():
    rng = np.random.default_rng(20261017)
    ns = {'np': np, 'os': os, 'KDTree': KDTree, 'cv2': types.SimpleNamespace(imread=_imread), 'Path': Path}
    _defs_from('Fusion3DSeg/segUtils/voting.py', ['PointVotingSegmentation'], ns)
    PV = ns['PointVotingSegmentation']
    g = {'sig_init': str(inspect.signature(PV.__init__)), 'sig_zero': str(inspect.signature(PV.zero)),
         'sig_read_mask': str(inspect.signature(PV.read_mask)), 'sig_get_nns': str(inspect.signature(PV.get_nns)),
         'sig_vote': str(inspect.signature(PV.vote)), 'sig_segment': str(inspect.signature(PV.segment))}

    F, h, w, nclasses, r = 4, 12, 16, 5, 5 / 64
    dense = lattice_frames(rng, F, h, w)
    cloud = dense[rng.choice(len(dense), 300, replace=False)] + rng.integers(-3, 4, (300, 3)) / 64
    cloud = np.concatenate([cloud, np.array([0.125, 0.0, 0.0]) + rng.integers(-1, 2, (40, 3)) / 64])     # a clump at camera 1
    fr = dense.reshape(F, h * w, 3).copy()
    far = np.stack([rng.choice(h * w, 6, replace=False) for _ in range(F)])                              # pixels that see nothing
    for j in range(F):
        fr[j, far[j]] += [0.0, 0.0, 8.0]
    numbers = np.array([7, 12, 3, 104])
    tof = [{'modPoints': fr[j], 'frameNumber': str(numbers[j])} for j in range(F)]
    tree = KDTree(cloud)
    counts = np.stack([tree.query_radius(fr[j], r=r, count_only=True) for j in range(F)])
    assert (counts[np.arange(F)[:, None], far] == 0).all() and (counts > 0).mean() > 0.5
    g.update(cloud=cloud, frames=fr, frame_numbers=numbers, radius=np.float64(r), hw=np.array([h, w]), nclasses=np.int64(nclasses),
             far_pixels=far)

    def run(masks, present, calls):
        with tempfile.TemporaryDirectory() as d:
            write_masks(d, masks, present, numbers, (h, w))
            pv = PV(tof, cloud, (h, w), d, nclasses, prefix=PREFIX, extension=EXT, zfill=ZFILL)
            out = []
            for kw in calls:
                if kw == 'zero':
                    pv.zero()
                    continue
                try:
                    pv.vote(radius=r, resize=False, **kw)
                    out.append((pv.votes.copy(), ''))
                except Exception as exc:                                # noqa: BLE001
                    out.append((pv.votes.copy(), type(exc).__name__))
            return out, pv

    a_masks = rng.integers(0, nclasses + 1, (F, h * w)).astype(np.uint8)
    a_masks[:, : 3 * w] = nclasses                                       # a band of the low-confidence label: the column collision
    a_present = np.array([True, False, True, True])
    subset = np.array([3, 0, 1])
    res, _ = run(a_masks, a_present, [{}, 'zero', {'skip': 2}, 'zero', {'frame_numbers': subset}, 'zero', {}, {}])
    assert all(e == '' for _, e in res)
    g.update(a_masks=a_masks, a_present=a_present, a_subset=subset, a_votes_all=res[0][0], a_votes_skip2=res[1][0],
             a_votes_subset=res[2][0], a_votes_twice=res[4][0])
    assert (res[0][0][:, -1] > res[0][0][:, :-1].max(1)).any()           # the collision shows

    b_masks = a_masks.copy()
    for j in range(F):
        b_masks[j, far[j]] = 200
    res, _ = run(b_masks, np.ones(F, bool), [{}])
    assert res[0][1] == ''
    g.update(b_masks=b_masks, b_votes=res[0][0])

    c_masks = b_masks.copy()
    hit = int(np.argmax(counts[2]))
    c_masks[2, hit] = 200
    res, _ = run(c_masks, np.ones(F, bool), [{}])
    assert res[0][1] == 'IndexError'
    g.update(c_masks=c_masks, c_error=res[0][1], c_votes=res[0][0], c_pixel=np.int64(hit))

    extra = np.array([[2, 2, 0, 0, 0, 4], [0, 1, 1, 0, 0, 2], [3, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 2], [0, 0, 0, 0, 0, 0],
                      [1, 0, 0, 2, 0, 8], [0, 0, 0, 0, 3, 3], [0, 3, 0, 0, 0, 12]], np.float64)
    d_votes = np.concatenate([g['a_votes_all'], extra])
    thresholds = np.array([0.0, 0.5, 0.25])                              # 0.5 and 0.25 are exact ratios of the rows above
    filters = [None, (1, 3), (2, 0, 1), (4, -1), (0, 1, 2, 3, 4, 5)]     # (2, 0, 1): the remap aliases; -1 / 5: the total column
    with tempfile.TemporaryDirectory() as d:
        np.save(os.path.join(d, 'v.npy'), d_votes)
        pf = PV(None, None, None, None, None, votes_file=os.path.join(d, 'v.npy'))
        g.update(d_file_nclasses=np.int64(pf.nclasses), d_file_classes=pf.segment(0.5))
    pv = PV(tof, cloud, (h, w), '.', nclasses)
    g.update(d_votes=d_votes, d_thresholds=thresholds)
    for k, flt in enumerate(filters):
        g[f'd_filter_{k}'] = np.array([] if flt is None else flt, np.int64)
        for t, thr in enumerate(thresholds):
            g[f'd_classes_{k}_{t}'] = pv.segment(float(thr), filter_classes=flt, votes=d_votes)

    g['e_nns'], g['e_frequency'] = pv.get_nns(fr[0], r)
    np.savez_compressed(OUT / 'point_voting.npz', **g)
    print('point_voting.npz', (OUT / 'point_voting.npz').stat().st_size, 'bytes; pairs per frame', counts.sum(1).tolist(),
          'votes', g['a_votes_all'].sum(), 'c pixel', hit)


if __name__ == '__main__':
    main()
