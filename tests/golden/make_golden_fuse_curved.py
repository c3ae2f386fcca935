#!/usr/bin/env python3
"""Golden vectors for Fusion.fuse on a harder capture (tests/fusion_scenes.curved_capture), run from the reference.

Run in the build container: ``python tests/golden/make_golden_fuse_curved.py``.  As in make_golden_fuse.py the reference's
``Fusion`` class is compiled from its file by ``ast`` (make_golden.load_reference; nothing of it is copied), an instance is made
without the file readers and ``_save_uv2pt`` collects the per-frame lookups.  The capture itself is NOT stored: it regenerates bit
for bit from its seed, and the file keeps a SHA-256 of it so that a test knows it is fusing the same frames.  Stored per case: the
parameters, the five outputs, the lookups and the next draw of the global NumPy generator after the run.
"""
import sys
import warnings
from pathlib import Path

import numpy as np

OUT = Path(__file__).resolve().parent
sys.path.insert(0, str(OUT.parent.parent))
sys.path.insert(0, str(OUT.parent))
sys.path.insert(0, str(OUT))
from make_golden import load_reference  # noqa: E402
from fusion_scenes import capture_digest, copy_frames, curved_capture  # noqa: E402

H, W, F, SEED = 48, 64, 6, 5
CASES = [dict(radius=0.05, angle=10, stride=None, max_depth=10, skip=1, seed=21),
         dict(radius=0.03, angle=5, stride=4, max_depth=10, skip=1, seed=22),
         dict(radius=0.05, angle=30, stride=16, max_depth=10, skip=2, seed=23)]


def main():
    _, _, _, _, Fusion, _ = load_reference()
    K, q, t, frames = curved_capture(H, W, F, SEED)
    out = {'hw': np.array([H, W]), 'nframes': np.array(F), 'capture_seed': np.array(SEED),
           'capture_sha256': np.array(capture_digest(K, q, t, frames))}
    for ci, c in enumerate(CASES):
        fu = object.__new__(Fusion)
        fu.K, fu.w, fu.h, fu.xyzws, fu.translations = K, W, H, q, t
        fu.frames = copy_frames(frames)
        fu.nframes, fu.npts = F, H * W
        fu.ds_radius, fu.ds_angle = None, None
        fu.eyes, fu.lookats, fu.frustum_spoke_origins, fu.frutsum_face_normals = Fusion._get_frustum_data(K, W, H, q, t, np.arange(F))
        fu.pcdimg = np.arange(H * W).reshape(H, W)
        fu.pt2u, fu.pt2v = (np.arange(H * W) % W).astype(np.int32), (np.arange(H * W) // W).astype(np.int32)
        fu.save_lookups = True
        store = {}
        fu._save_uv2pt = lambda uv2pt, name, store=store: store.__setitem__(name, np.array(uv2pt, copy=True))
        np.random.seed(c['seed'])
        with warnings.catch_warnings(), np.errstate(all='ignore'):     # the zero normal / NaN point: means of empty sets
            warnings.simplefilter('ignore', RuntimeWarning)
            ds_pts, ds_norms, ds_clrs, nmerges, occ = fu.fuse(c['radius'], c['angle'], c['stride'], c['max_depth'], c['skip'])
        out[f'c{ci}_next_draw'] = np.array(np.random.random())
        out[f'c{ci}_params'] = np.array([c['radius'], c['angle'], -1 if c['stride'] is None else c['stride'], c['max_depth'], c['skip'],
                                         c['seed']], np.float64)
        out[f'c{ci}_ds_pts'], out[f'c{ci}_ds_norms'], out[f'c{ci}_ds_clrs'] = ds_pts, ds_norms, ds_clrs
        out[f'c{ci}_nmerges'], out[f'c{ci}_occurences'] = np.asarray(nmerges), np.asarray(occ)
        names = list(store)                                              # in the order the reference saved them
        out[f'c{ci}_uv2pt_names'] = np.array(names)
        out[f'c{ci}_uv2pt'] = np.stack([store[nm] for nm in names])
        print(f'case {ci}: {len(ds_pts)} fused points, lookups for frames {names}, nmerges sum {int(np.sum(nmerges))}, '
              f'occurences max {int(np.max(occ))}, NaN rows {int(np.isnan(ds_pts).any(axis=1).sum())}')
    out['ncases'] = np.array(len(CASES))
    np.savez_compressed(OUT / 'fuse_curved.npz', **out)
    print('fuse_curved.npz', (OUT / 'fuse_curved.npz').stat().st_size, 'bytes')


if __name__ == '__main__':
    main()
