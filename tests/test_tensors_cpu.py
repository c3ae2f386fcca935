"""f3d.tensors on the host (no GPU): the host CSR check, the dtype codes, the device-tensor test, and torch stays optional."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import f3d
from f3d import tensors as T

ROOT = Path(__file__).resolve().parent.parent
PKG = ROOT / '3d-point-cloud-segmentation-using-2d-img-segmentation_amd'


def test_host_csr_casts_a_valid_pair():
    offs, nbrs = T.host_csr([0, 2, 2, 3], np.array([1, 2, 0], np.int64), 3)
    assert offs.dtype == np.int64 and nbrs.dtype == np.int32 and offs.flags.c_contiguous and nbrs.flags.c_contiguous
    assert offs.tolist() == [0, 2, 2, 3] and nbrs.tolist() == [1, 2, 0]
    strided = np.arange(8, dtype=np.int32)[::2]                          # [0, 2, 4, 6]: made contiguous
    offs, nbrs = T.host_csr(strided, np.zeros(6, np.int8), 3)
    assert offs.dtype == np.int64 and offs.flags.c_contiguous and offs.tolist() == [0, 2, 4, 6] and nbrs.dtype == np.int32
    same = np.array([0, 1], np.int64), np.array([0], np.int32)           # already right: passed through, not copied
    assert all(a is b for a, b in zip(T.host_csr(*same, 1), same))


def test_host_csr_rejects_what_the_kernels_would_read_past():
    with pytest.raises(ValueError, match='n\\+1 entries ending at len\\(neighbours\\)'):
        T.host_csr([0, 1, 2], [0, 1], 3)                                 # n + 1 violated
    with pytest.raises(ValueError):
        T.host_csr([0, 1, 2, 3, 3], [0, 1, 2], 3)
    with pytest.raises(ValueError):
        T.host_csr([0, 1, 2, 4], [0, 1, 2], 3)                           # the last offset is not len(neighbours)
    with pytest.raises(ValueError):
        T.host_csr([0, 1, 2, 2], [0, 1, 2], 3)
    with pytest.raises(ValueError, match='^CSR adjacency: offsets must have n \\+ 1 entries'):
        T.host_csr([0, 1], [0, 1], 1, T.CSR_ADJACENCY)                   # the drop-in modules' wording
    # n == 0: one offset is required, and no row is read, so the last offset is not compared
    with pytest.raises(ValueError):
        T.host_csr([], [], 0)
    offs, nbrs = T.host_csr([0], [], 0)
    assert offs.tolist() == [0] and len(nbrs) == 0 and nbrs.dtype == np.int32
    assert T.host_csr([0], [5], 0)[1].tolist() == [5]


def test_dtype_and_index_codes_on_arrays_and_cpu_tensors():
    import torch
    assert (f3d.F64, f3d.F32) == (0, 1) and (f3d.I64, f3d.I32) == (0, 1)
    for mk in (lambda t: np.zeros((2, 3), getattr(np, t)), lambda t: torch.zeros((2, 3), dtype=getattr(torch, t))):
        assert T.dtype_code(mk('float32')) == f3d.F32 and T.dtype_code(mk('float64')) == f3d.F64
        assert T.index_code(mk('int32')) == f3d.I32 and T.index_code(mk('int64')) == f3d.I64


def test_on_device_is_false_on_the_host():
    import torch
    assert T.on_device(np.zeros(3)) is False and T.on_device(torch.zeros(3)) is False
    assert T.on_device([1, 2]) is False and T.on_device(None) is False


def test_importing_the_module_does_not_import_torch():
    code = 'import sys, f3d.tensors\nassert "torch" not in sys.modules, "torch was imported"\nprint("ok")\n'
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([str(ROOT), str(PKG)]))
    r = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == 'ok', r.stdout + r.stderr
