"""f3d_bits_for (csrc/f3d_kernels.h) without a GPU: a stand-alone host program prints its values, which must equal what the four loops
it replaced computed.  A changed count changes the number of radix passes of a sort, so the old loops are kept here, restated."""
import os
import subprocess

import pytest

from conftest import ROOT, PKG

VALUES = sorted({0, 1, 2, 3} | {(1 << k) + d for k in range(2, 40) for d in (-1, 0, 1)})

PROGRAM = r'''
#include <stdio.h>
#include <stdlib.h>
#include "f3d_kernels.h"
int main(int argc, char** argv) {
    for (int i = 1; i < argc; ++i) {
        const long long v = atoll(argv[i]);
        printf("%lld %d %d %d %d\n", v, f3d_bits_for(v, 0), f3d_bits_for(v, 1), f3d_bits_for(v + 1, 1), f3d_bits_for(v + 1, 0));
    }
    return 0;
}
'''


def _at_least(v, b):
    """The loop of the mesh and plane sorts (b = 1) and of the normals' cell keys (b = 0): smallest b' >= b with 2^b' >= v."""
    while (1 << b) < v:
        b += 1
    return b


def _id_key_bits(nids):
    """The loop of group_by_id: keys 0 .. nids."""
    b = 1
    while (1 << b) <= nids:
        b += 1
    return b


def _flood_key_bits(k):
    """The loop of flood_order: 32 root bits and the ranks 0 .. k above them."""
    bits = 32
    while bits < 64 and (1 << (bits - 32)) < k + 1:
        bits += 1
    return bits


def test_the_old_loops_are_what_the_table_says():
    assert [_at_least(v, 1) for v in (0, 1, 2, 3, 4, 5, 8, 9)] == [1, 1, 1, 2, 2, 3, 3, 4]
    assert [_at_least(v, 0) for v in (0, 1, 2, 3, 4, 5, 8, 9)] == [0, 0, 1, 2, 2, 3, 3, 4]
    assert [_id_key_bits(v) for v in (0, 1, 2, 3, 4, 7, 8)] == [1, 1, 2, 2, 3, 3, 4]
    assert [_flood_key_bits(v) for v in (0, 1, 2, 3, 4)] == [32, 33, 34, 34, 35]


@pytest.fixture(scope='module')
def printed(tmp_path_factory):
    work = tmp_path_factory.mktemp('bits_for')
    (work / 'bits_for.cpp').write_text(PROGRAM)
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    subprocess.run([hipcc, '-x', 'hip', '--cuda-host-only', '-O1', '-std=c++17', f'-I{ROOT / "include"}', f'-I{PKG / "csrc"}',
                    str(work / 'bits_for.cpp'), '-o', str(work / 'bits_for')], check=True, capture_output=True)
    out = subprocess.run([str(work / 'bits_for')] + [str(v) for v in VALUES], check=True, capture_output=True, text=True).stdout
    rows = [tuple(int(x) for x in line.split()) for line in out.splitlines()]
    assert [r[0] for r in rows] == VALUES
    return rows


def test_bits_for_equals_the_loops_it_replaced(printed):
    for v, min0, min1, plus1, plus1_min0 in printed:
        assert min0 == _at_least(v, 0), v                  # f3d_capi.cpp: cell and frame bits of the normals' keys
        assert min1 == _at_least(v, 1), v                  # f3d_mesh.hip, f3d_planes.hip: bits_for
        assert plus1 == _id_key_bits(v), v                 # f3d_obb.hip: key_bits(nids) is now f3d_bits_for(nids + 1, 1)
        if v < (1 << 31):
            assert 32 + plus1_min0 == _flood_key_bits(v), v                   # f3d_cc.hip: 32 + f3d_bits_for(k + 1, 0)
