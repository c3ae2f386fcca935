"""f3d_decided_unlabelled (csrc/f3d_fuse_decide.h): "every completion of this point's vote ends unlabelled".
Compiled for the host and run against brute force: for a threshold, the table cmin is built with the reference's own float64
division (voting.py:128), and for every state (b = the leader's count, s = the counted votes, R = the views still out) every
completion -- r' <= R further counted votes, a <= r' of them to the winner, any final winner count up to b + a -- is passed through
the rules of segment_point (voting.py:120-135).  The function must say "decided" exactly when all of them end unlabelled: that is
soundness (no label is lost) and tightness (no decision is missed)."""
import math
import os
import subprocess

import pytest

from conftest import ROOT, PKG

PROGRAM = r'''
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cstdint>
#include "f3d_fuse_decide.h"
// segment_point's rules for one finished point: true = unlabelled
static bool unlabelled(int win, int total, double threshold) {
    if (total == 0) return true;                                   // voting.py:126
    if ((double)win / (double)total < threshold) return true;      // :128-130
    return win == 0;                                               // :131
}
int main(int argc, char** argv) {       // threshold (as the 16 hex digits of its bits), tmax of the full sweep; the strip: totals lo .. hi with at most rmax views out
    unsigned long long bits = strtoull(argv[1], nullptr, 16);
    double threshold; memcpy(&threshold, &bits, 8);
    const int tmax = atoi(argv[2]), lo = atoi(argv[3]), hi = atoi(argv[4]), rmax = atoi(argv[5]);
    uint16_t cmin[256];
    for (int t = 0; t < 256; ++t) { int c = 0; for (int k = 0; k <= t; ++k) c += ((double)k / (double)t < threshold) ? 1 : 0; cmin[t] = (uint16_t)c; }
    long long states = 0, decided = 0, unsound = 0, loose = 0;
    for (int total = 0; total <= hi; ++total) {
        if (total > tmax && total < lo) continue;
        for (int R = 0; R <= (total > tmax ? (rmax < total ? rmax : total) : total); ++R) {
            const int s = total - R;
            for (int b = 0; b <= s; ++b) {
                bool all = true;
                for (int r = 0; r <= R && all; ++r)
                    for (int a = 0; a <= r && all; ++a)
                        for (int w = 0; w <= b + a && all; ++w) all = unlabelled(w, s + r, threshold);
                const bool got = f3d_decided_unlabelled((unsigned)b, (unsigned)s, (unsigned)R, cmin);
                ++states; decided += got ? 1 : 0;
                if (got && !all) { if (!unsound) printf("unsound b=%d s=%d R=%d\n", b, s, R); ++unsound; }
                if (!got && all) { if (!loose) printf("loose b=%d s=%d R=%d\n", b, s, R); ++loose; }
            }
        }
    }
    printf("states %lld decided %lld unsound %lld loose %lld\n", states, decided, unsound, loose);
    return 0;
}
'''
THRESHOLDS = [0.0, 1e-300, 0.3, 1.0 / 3.0, 0.5, 0.7, 1.0, 1.5, math.nan]
FULL_TO, STRIP = 64, (248, 255, 12)      # every total up to 64, and a strip of totals up to the table's end with up to 12 views out


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    work = tmp_path_factory.mktemp('fuse_decide')
    (work / 'fuse_decide.cpp').write_text(PROGRAM)
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    subprocess.run([hipcc, '-x', 'hip', '--cuda-host-only', '-O2', '-std=c++17', '-ffp-contract=off', f'-I{ROOT / "include"}',
                    f'-I{PKG / "csrc"}', str(work / 'fuse_decide.cpp'), '-o', str(work / 'fuse_decide')], check=True, capture_output=True)
    return work / 'fuse_decide'


def _run(program, threshold):
    import struct
    bits = struct.unpack('<Q', struct.pack('<d', threshold))[0]
    out = subprocess.run([str(program), f'{bits:016x}', str(FULL_TO), str(STRIP[0]), str(STRIP[1]), str(STRIP[2])], check=True, capture_output=True,
                         text=True).stdout.strip().split('\n')
    last = out[-1].split()
    return dict(zip(last[0::2], map(int, last[1::2]))), out[:-1]


@pytest.mark.parametrize('threshold', THRESHOLDS, ids=lambda t: repr(t))
def test_decided_exactly_when_every_completion_is_unlabelled(program, threshold):
    r, complaints = _run(program, threshold)
    assert r['states'] > 50000
    assert r['unsound'] == 0 and r['loose'] == 0, complaints


def test_what_the_thresholds_allow(program):
    # threshold 0 and NaN: nothing is below the threshold, only a point that can get no winner at all is decided (b = R = 0);
    # threshold 1.5: every share is below it, every state is decided; 0.5: some are, some are not
    for t in (0.0, math.nan):
        r, _ = _run(program, t)
        assert 0 < r['decided'] < r['states'] // 50
    r, _ = _run(program, 1.5)
    assert r['decided'] == r['states']
    r, _ = _run(program, 0.5)
    assert r['states'] // 10 < r['decided'] < r['states']
