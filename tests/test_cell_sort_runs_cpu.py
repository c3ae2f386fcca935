"""f3d_run_span_of / f3d_run_at (csrc/f3d_kernels.h): how pass 1 of the cell sort finds the run of a tile position -- a bitmap of run
starts, per 64-bit word the number of runs that start in front of it, and a table compacted by the rank of the non-empty run.  Compiled
for the host and run: the tables are built from a vector of 256 digit counts exactly as the kernel's 256 owner threads build them, and
every position of the tile is held to a plain loop over the counts."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, PKG

PROGRAM = r'''
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "f3d_kernels.h"
int main(int argc, char** argv) {       // 256 counts -> one line per position: "rank of its run among the non-empty, digit value of that rank"
    const unsigned nwords = 128;        // RS_TILE / 64
    std::vector<unsigned long long> starts(nwords, 0ull);
    std::vector<unsigned> before(nwords, 0xDEADu), value_of(256, 0xDEADu);     // only before[0] is initialised by the kernel
    before[0] = 0;
    unsigned start = 0, rank = 0;
    for (int d = 0; d < 256; ++d) {
        const unsigned c = (unsigned)atoll(argv[1 + d]);
        if (c) {
            const f3d_run_span sp = f3d_run_span_of(start, c, nwords);
            starts[sp.word] |= 1ull << sp.bit;
            value_of[rank] = (unsigned)d;
            for (unsigned w = sp.first; w <= sp.last; ++w) before[w] = rank + 1;
            ++rank;
        }
        start += c;
    }
    for (unsigned j = 0; j < start; ++j) { const unsigned r = f3d_run_at(starts[j >> 6], before[j >> 6], j & 63u); printf("%u %u\n", r, r < 256 ? value_of[r] : 0xDEADu); }
    return 0;
}
'''
TILE = 8192


def _counts():
    """name -> 256 counts (sum <= 8192): the count vectors of the tiles of tests/test_cell_sort_runs_gpu.py."""
    rng = np.random.default_rng(51)
    out = {}

    def one(value, total):
        c = np.zeros(256, np.int64)
        c[value] = total
        return c
    for total in (1, 63, 64, 65, 509, 8187, 8192):
        out[f'one_value_0x5A_{total}'] = one(0x5A, total)
    out['one_value_0_full'] = one(0, TILE)
    out['one_value_255_full'] = one(255, TILE)
    c = one(0x5A, 8188); c[255] = 4
    out['one_value_and_anchors'] = c
    c = one(0xFF, 1)
    out['an_anchor_alone'] = c
    for a, b in ((0x12, 0x92), (0x34, 0xB4), (0x40, 0x41)):
        for total in (509, 8192):
            c = np.zeros(256, np.int64); c[a] = total // 2; c[b] = total - total // 2
            out[f'two_values_{a:#x}_{b:#x}_{total}'] = c
    out['every_value_32'] = np.full(256, 32)
    c = np.bincount(np.repeat(np.arange(256), 32)[rng.permutation(TILE)][:8187], minlength=256)
    out['every_value_32_cut'] = c
    c = np.bincount(np.repeat(np.arange(256), 32)[rng.permutation(TILE)][:509], minlength=256)
    out['every_value_32_cut_509'] = c
    for total in (509, 8187, 8189, 8192):
        c = np.ones(256, np.int64); c[0] = total - 255
        out[f'singles_big_lowest_{total}'] = c
        c = np.ones(256, np.int64); c[255] = total - 255
        out[f'singles_big_highest_{total}'] = c
    c = np.ones(256, np.int64); c[0] = 0
    out['singles_only_255'] = c
    out['random_multinomial'] = rng.multinomial(TILE, rng.dirichlet(np.ones(256)))
    out['random_sparse'] = rng.multinomial(8191, rng.dirichlet(np.ones(256))) * (rng.random(256) < 0.3)
    c = np.zeros(256, np.int64); c[[3, 4, 200]] = [63, 1, 64]                # runs that end on, start on and fill a word boundary
    out['word_boundaries'] = c
    c = np.zeros(256, np.int64); c[[0, 7, 9, 255]] = [64, 64, 128, 7936]
    out['runs_of_whole_words'] = c
    return out


COUNTS = _counts()


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    work = tmp_path_factory.mktemp('run_lookup')
    (work / 'run_lookup.cpp').write_text(PROGRAM)
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    subprocess.run([hipcc, '-x', 'hip', '--cuda-host-only', '-O1', '-std=c++17', f'-I{ROOT / "include"}', f'-I{PKG / "csrc"}',
                    str(work / 'run_lookup.cpp'), '-o', str(work / 'run_lookup')], check=True, capture_output=True)
    return work / 'run_lookup'


@pytest.mark.parametrize('name', sorted(COUNTS))
def test_every_position_finds_its_run(program, name):
    c = np.asarray(COUNTS[name], np.int64)
    assert len(c) == 256 and 0 < c.sum() <= TILE
    out = subprocess.run([str(program)] + [str(int(v)) for v in c], check=True, capture_output=True, text=True).stdout
    rows = np.array([[int(v) for v in line.split()] for line in out.splitlines()], np.int64).reshape(-1, 2)
    want_rank, want_value = [], []                                     # the plain loop: position by position through the runs
    rank = 0
    for d in range(256):
        if c[d]:
            want_rank += [rank] * int(c[d])
            want_value += [d] * int(c[d])
            rank += 1
    assert len(rows) == c.sum()
    assert np.array_equal(rows[:, 0], want_rank)
    assert np.array_equal(rows[:, 1], want_value)
