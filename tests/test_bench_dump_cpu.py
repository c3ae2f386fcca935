"""bench.py --dump-outputs: what it writes (no GPU; the timed step itself is exercised by running bench.py on the GPU box)."""
import importlib.util

import numpy as np

from conftest import ROOT


def _bench():
    spec = importlib.util.spec_from_file_location('f3d_bench', ROOT / 'bench.py')
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_writes_every_label_as_float32(tmp_path):
    b = _bench()
    labels = np.random.default_rng(1).integers(0, 134, 100_003)
    info = b.dump_outputs(tmp_path, labels, 0, 1, 0)
    assert info['files'] == ['labels.npy'] and not info['sampled']
    got = np.load(tmp_path / 'labels.npy')
    assert got.dtype == np.float32 and np.array_equal(got, labels)


def test_dump_of_a_large_output_is_a_fixed_sample_within_the_limit(tmp_path, monkeypatch):
    b = _bench()
    monkeypatch.setattr(b, 'DUMP_LIMIT_BYTES', 120_000)
    labels = np.random.default_rng(2).integers(0, 134, 1_000_000)
    for world, rank, lo in ((1, 0, 0), (2, 1, 1_000_000)):
        dirs = [tmp_path / f'w{world}a', tmp_path / f'w{world}b']
        for d in dirs:
            b.dump_outputs(d, labels, rank, world, lo)
        sfx = '' if world == 1 else f'_rank{rank}'
        lab, idx = np.load(dirs[0] / f'labels{sfx}.npy'), np.load(dirs[0] / f'labels_index{sfx}.npy')
        assert lab.dtype == np.float32 and idx.dtype == np.float64
        assert lab.nbytes + idx.nbytes <= 120_000 // world and len(lab) > 0
        assert np.all(np.diff(idx) > 0) and np.array_equal(lab, labels[idx.astype(np.int64) - lo])
        for name in (f'labels{sfx}.npy', f'labels_index{sfx}.npy'):         # the same sample every run
            assert np.array_equal(np.load(dirs[0] / name), np.load(dirs[1] / name))
