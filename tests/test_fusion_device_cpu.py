"""CPU-side checks of Fusion.fuse / fuse_device: the probe of the host's dot order, and no CPU fallback without a device."""
import numpy as np
import pytest

import f3d
from Fusion3DSeg import fusion


def _fma_dot(v):
    x, y, z = (float(c) for c in v)
    return fusion._fma(z, z, fusion._fma(y, y, x * x))


def _plain_dot(v):
    x, y, z = (float(c) for c in v)
    return (x * x + y * y) + z * z


def test_norm_probe_vectors_separate_the_two_orders():
    vectors = fusion._norm_probe_vectors()
    assert len(vectors) == 64
    assert all(_fma_dot(v) != _plain_dot(v) for v in vectors)


def test_norm_probe_classifies_fma_and_plain_dots():
    assert fusion._probe_norm_mode(_fma_dot) == f3d.NORM_FMA
    assert fusion._probe_norm_mode(_plain_dot) == f3d.NORM_PLAIN
    assert fusion._probe_norm_mode(lambda v: float(v[0] * v[0] + (v[1] * v[1] + v[2] * v[2]))) == f3d.NORM_HOST
    # whatever this host's BLAS does, the probe's verdict reproduces its v.dot(v) (or hands normalisation to the host)
    mode = fusion._probe_norm_mode()
    vectors = fusion._norm_probe_vectors()
    dots = np.array([v.dot(v) for v in vectors])
    if mode == f3d.NORM_FMA:
        assert np.array_equal(dots, [_fma_dot(v) for v in vectors])
    elif mode == f3d.NORM_PLAIN:
        assert np.array_equal(dots, [_plain_dot(v) for v in vectors])
    else:
        assert mode == f3d.NORM_HOST


def test_fuse_device_has_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip('a HIP device is present')
    from f3d import synth
    K, q, t, frames = synth.depth_sequence(8, 8, 2)
    fu = fusion.Fusion.from_frames(K, 8, 8, q, t, frames)
    with pytest.raises(f3d.F3DUnavailable):
        fu.fuse_device()


def test_fuse_has_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip('a HIP device is present')
    from f3d import synth
    K, q, t, frames = synth.depth_sequence(8, 8, 2)
    fu = fusion.Fusion.from_frames(K, 8, 8, q, t, frames)
    with pytest.raises(f3d.F3DUnavailable):
        fu.fuse()
