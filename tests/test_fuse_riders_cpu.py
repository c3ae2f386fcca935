"""f3d_rider_role (csrc/f3d_kernels.h): the block-uniform map from a block index of a sort launch with rider blocks to (rider?, number).
Compiled for the host and run: every sort tile and every rider block is hit exactly once, and the riders are spread through the grid."""
import os
import subprocess

import pytest

from conftest import ROOT, PKG

PROGRAM = r'''
#include <cstdio>
#include <cstdlib>
#include "f3d_kernels.h"
int main(int argc, char** argv) {       // tiles extra -> one line per block: "rider index"
    const unsigned tiles = (unsigned)atoll(argv[1]), extra = (unsigned)atoll(argv[2]), grid = tiles + extra;
    for (unsigned b = 0; b < grid; ++b) { const f3d_block_role r = f3d_rider_role(b, grid, extra); printf("%d %d\n", r.rider ? 1 : 0, r.index); }
    return 0;
}
'''
TILES = [1, 2, 1221, 2049, 262144]       # 262144 tiles: 2^31 points
EXTRA = [0, 1, 9, 256, 2048]


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    work = tmp_path_factory.mktemp('rider_role')
    (work / 'rider_role.cpp').write_text(PROGRAM)
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    subprocess.run([hipcc, '-x', 'hip', '--cuda-host-only', '-O1', '-std=c++17', f'-I{ROOT / "include"}', f'-I{PKG / "csrc"}',
                    str(work / 'rider_role.cpp'), '-o', str(work / 'rider_role')], check=True, capture_output=True)
    return work / 'rider_role'


@pytest.mark.parametrize('extra', EXTRA)
@pytest.mark.parametrize('tiles', TILES)
def test_every_tile_and_every_rider_exactly_once(program, tiles, extra):
    out = subprocess.run([str(program), str(tiles), str(extra)], check=True, capture_output=True, text=True).stdout
    rows = [tuple(int(x) for x in line.split()) for line in out.splitlines()]
    assert len(rows) == tiles + extra
    riders = [i for r, i in rows if r]
    own = [i for r, i in rows if not r]
    assert riders == list(range(extra))                    # each once, ascending with the block index
    assert own == list(range(tiles))
    if extra > 1:                                          # spread evenly: no gap between two riders beyond the mean spacing, rounded up
        at = [b for b, (r, _) in enumerate(rows) if r]
        step = -(-(tiles + extra) // extra)
        assert max(b - a for a, b in zip(at[:-1], at[1:])) <= step and at[0] < step
