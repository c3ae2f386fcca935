"""f3d_deal (csrc/f3d_fuse_deal.h): how k_fuse's tile positions of one XCD are dealt to its blocks in layers of shrinking width.
Compiled for the host and run: the program prints the deal and the walk of every block; every position is walked exactly once, the
blocks dispatched first walk the most tiles and the last ones a single tile.

CAP: the most blocks per XCD.  A block walks one position per layer and there are F3D_DEAL_LAYERS = 16 layers, so a one-tile tail for
32768 positions needs more than 32768 / 16 = 2048 blocks: the properties are checked with 4096, and with the launcher's own 1024
(F3D_FUSE_GRID / 8), where the largest list falls back to the stride walk, everything but the one-tile tail."""
import os
import subprocess

import pytest

from conftest import ROOT, PKG

PROGRAM = r'''
#include <cstdio>
#include <cstdlib>
#include "f3d_fuse_deal.h"
int main(int argc, char** argv) {       // positions slots cap -> "nlayers", then "width start" per layer, then one line per block: its positions
    const int positions = atoi(argv[1]), slots = atoi(argv[2]), cap = atoi(argv[3]);
    const f3d_deal d = f3d_deal_make(positions, slots, cap);
    printf("%d\n", d.nlayers);
    for (int k = 0; k < d.nlayers; ++k) printf("%d %d\n", d.width[k], d.start[k]);
    for (int bx = 0; bx < d.width[0]; ++bx) {
        for (f3d_deal_pos p = f3d_deal_next(d, positions, bx, -1); p.k >= 0; p = f3d_deal_next(d, positions, bx, p.k)) printf("%d ", p.pos);
        printf("\n");
    }
    return 0;
}
'''
POSITIONS = [1, 2, 127, 128, 129, 305, 1027, 2496, 32768]
SLOTS = [32, 64, 96, 128]
LAYERS = 16
CAP, CAP_LAUNCHER = 4096, 1024


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    work = tmp_path_factory.mktemp('fuse_deal')
    (work / 'fuse_deal.cpp').write_text(PROGRAM)
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    subprocess.run([hipcc, '-x', 'hip', '--cuda-host-only', '-O1', '-std=c++17', f'-I{ROOT / "include"}', f'-I{PKG / "csrc"}',
                    str(work / 'fuse_deal.cpp'), '-o', str(work / 'fuse_deal')], check=True, capture_output=True)
    return work / 'fuse_deal'


def _deal(program, positions, slots, cap):
    lines = subprocess.run([str(program), str(positions), str(slots), str(cap)], check=True, capture_output=True, text=True).stdout.split('\n')
    nlayers = int(lines[0])
    layers = [tuple(int(x) for x in line.split()) for line in lines[1:1 + nlayers]]
    walks = [[int(x) for x in line.split()] for line in lines[1 + nlayers:1 + nlayers + layers[0][0]]]
    return layers, walks


def _check_common(layers, walks, positions, slots, cap):
    width, start = [w for w, _ in layers], [s for _, s in layers]
    assert 1 <= len(layers) <= LAYERS
    assert 1 <= width[0] <= cap
    assert all(a >= b for a, b in zip(width[:-1], width[1:]))                       # layers shrink
    assert start == [sum(width[:k]) for k in range(len(width))]
    assert sorted(p for w in walks for p in w) == list(range(positions))            # every position exactly once
    assert all(w == sorted(w) for w in walks)                                       # a block walks upwards
    sizes = [len(w) for w in walks]
    assert all(a >= b for a, b in zip(sizes[:-1], sizes[1:]))                       # tiles per block do not increase with bx
    if positions <= slots:
        assert sizes == [1] * positions                                             # the deal of a small cloud: one tile per block
    return sizes


@pytest.mark.parametrize('slots', SLOTS)
@pytest.mark.parametrize('positions', POSITIONS)
def test_deal_covers_every_position_and_ends_on_one_tile_blocks(program, positions, slots):
    layers, walks = _deal(program, positions, slots, CAP)
    sizes = _check_common(layers, walks, positions, slots, CAP)
    if positions > 2 * slots:
        assert all(s <= 1 for s in sizes[-slots:])                                  # the blocks dispatched last
    if positions >= 16 * slots:
        assert sizes[0] >= 3 and len(walks) < positions // 2                        # ... and the first ones save start-ups


@pytest.mark.parametrize('slots', SLOTS)
@pytest.mark.parametrize('positions', POSITIONS)
def test_deal_within_the_launchers_cap(program, positions, slots):
    layers, walks = _deal(program, positions, slots, CAP_LAUNCHER)
    sizes = _check_common(layers, walks, positions, slots, CAP_LAUNCHER)
    if 2 * slots < positions <= 2496:
        assert all(s <= 1 for s in sizes[-slots:])
    if positions == 32768:                                                          # more than 16 layers of 1024 blocks: the stride walk
        assert layers == [(CAP_LAUNCHER, 0)] and sizes == [32] * CAP_LAUNCHER
