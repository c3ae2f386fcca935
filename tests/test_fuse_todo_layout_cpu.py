"""f3d_fuse_todo_layout (csrc/f3d_fuse_todo.h) without a GPU: the layout of the fused call's todo block -- counters, the two deferred
lists, the open-view masks umask[slot][group] and the parked bins park[slot][word] -- printed by a stand-alone host program for the
sizes where an index could leave the block, and compared with DESIGN.md section 3 restated here in Python integers.  k_fuse and
k_fuse_mid index umask with `slot * ngroups + g` and park with `slot * park_stride + word` for slot < park_slots: the last element
of each region must lie inside the block, whatever F3D_DEBUG_PARK_SLOTS says."""
import os
import subprocess

import pytest

from conftest import ROOT, PKG

NS = [0, 1, 15, 16, 127, 128, 129, 4095, 4096, 65_535, 65_536, 10_000_000, 0x7ffff000]
VIEWS = [0, 1, 63, 64, 65, 128, 129, 255, 256, 1024, 1025, 4096]
NCLASSES = [0, 1, 9, 10, 133, 253]
MAX_NCLASSES, MAX_GROUPS = 253, 16                     # F3D_CODE_MAX_NCLASSES, F3D_PART_MAX_GROUPS


def env_values(n):
    """F3D_DEBUG_PARK_SLOTS: unset (None), and -1, 0, 1, n - 1, n, n + 1."""
    return [None, -1, 0, 1, n - 1, n, n + 1]


ROWS = [(n, v, c, e) for n in NS for v in VIEWS for c in NCLASSES for e in env_values(n)]

PROGRAM = r'''
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "f3d_fuse_todo.h"
int main(int argc, char** argv) {       // rows of "n views nclasses env" from the file argv[1]; env "-" = the variable is not set
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    long long n; int views, nclasses; char env[64];
    while (fscanf(f, "%lld %d %d %63s", &n, &views, &nclasses, env) == 4) {
        if (!strcmp(env, "-")) unsetenv("F3D_DEBUG_PARK_SLOTS"); else setenv("F3D_DEBUG_PARK_SLOTS", env, 1);
        const f3d_fuse_todo t = f3d_fuse_todo_layout((int64_t)n, views, nclasses);
        char* const base = (char*)(uintptr_t)4096;     // the accessors are pointer arithmetic on the base: print what they add
        printf("%zu %zu %zu %zu %d %d %d %td %td %td %td %td\n", t.bytes, t.list2_off, t.umask_off, t.park_off, t.park_slots, t.park_stride, t.ngroups,
               (char*)f3d_fuse_todo::counters(base) - base, (char*)f3d_fuse_todo::list(base) - base, (char*)t.list2(base) - base,
               (char*)t.umask(base) - base, (char*)t.park(base) - base);
    }
    fclose(f);
    printf("%d %d %zu\n", F3D_PART_MAX_GROUPS, F3D_CODE_MAX_NCLASSES, sizeof(size_t));
    return 0;
}
'''
FIELDS = ('bytes', 'list2_off', 'umask_off', 'park_off', 'park_slots', 'park_stride', 'ngroups', 'p_counters', 'p_list', 'p_list2', 'p_umask', 'p_park')


def contract(n, views, nclasses, env):
    """DESIGN.md section 3, "deferred lists": 4 counters, 2 x int32[n], then for the park_slots parked slots of the first list one 64-bit
    mask per 64-view group, and behind all the masks the parked bins, `words` dwords of four 8-bit counts per slot -- one count per
    label 0..nclasses and per code "no sample" and "rejected".  park_slots = n / 16 + 4096 (F3D_DEBUG_PARK_SLOTS overrides), never more
    than n, never negative; none without views or beyond MAX_GROUPS groups of views."""
    ngroups = (views + 63) // 64
    slots = 0
    if 0 < views <= 64 * MAX_GROUPS:
        slots = min(max(n // 16 + 4096 if env is None else env, 0), n)
    words = (nclasses + 1 + 2 + 3) // 4
    list_off = 4 * 4
    list2_off = list_off + 4 * n
    umask_off = list2_off + 4 * n
    park_off = umask_off + 8 * slots * ngroups
    return dict(bytes=park_off + 4 * slots * words, list2_off=list2_off, umask_off=umask_off, park_off=park_off, park_slots=slots,
                park_stride=words, ngroups=ngroups, p_counters=0, p_list=list_off, p_list2=list2_off, p_umask=umask_off, p_park=park_off)


@pytest.fixture(scope='module')
def printed(tmp_path_factory):
    work = tmp_path_factory.mktemp('fuse_todo')
    (work / 'fuse_todo.cpp').write_text(PROGRAM)
    (work / 'rows.txt').write_text(''.join(f'{n} {v} {c} {"-" if e is None else e}\n' for n, v, c, e in ROWS))
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    subprocess.run([hipcc, '-x', 'hip', '--cuda-host-only', '-O1', '-std=c++17', f'-I{ROOT / "include"}', f'-I{PKG / "csrc"}',
                    str(work / 'fuse_todo.cpp'), '-o', str(work / 'fuse_todo')], check=True, capture_output=True)
    env = {k: v for k, v in os.environ.items() if k != 'F3D_DEBUG_PARK_SLOTS'}
    lines = subprocess.run([str(work / 'fuse_todo'), str(work / 'rows.txt')], check=True, capture_output=True, text=True, env=env).stdout.splitlines()
    assert len(lines) == len(ROWS) + 1
    return [dict(zip(FIELDS, map(int, ln.split()))) for ln in lines[:-1]], tuple(int(x) for x in lines[-1].split())


def test_the_constants_restated_here_are_the_headers(printed):
    assert printed[1] == (MAX_GROUPS, MAX_NCLASSES, 8)                     # (size_t of 8 bytes: the sums below are compared unwrapped)
    assert len(ROWS) == len(NS) * len(VIEWS) * len(NCLASSES) * 7


def test_every_field_is_the_contract(printed):
    for row, got in zip(ROWS, printed[0]):
        assert got == contract(*row), row


def test_regions_are_ordered_disjoint_aligned_and_end_at_bytes(printed):
    for (n, views, nclasses, env), t in zip(ROWS, printed[0]):
        row = (n, views, nclasses, env)
        regions = [(t['p_counters'], 16), (t['p_list'], 4 * n), (t['p_list2'], 4 * n), (t['p_umask'], 8 * t['park_slots'] * t['ngroups']),
                   (t['p_park'], 4 * t['park_slots'] * t['park_stride'])]     # counters, list, list2, umask, park: (offset, size)
        end = 0
        for off, size in regions:
            assert off == end, row                                             # in that order, back to back: disjoint, no gap
            end = off + size
        assert end == t['bytes'], row
        assert t['umask_off'] % 8 == 0 and t['park_off'] % 4 == 0 and t['list2_off'] % 4 == 0, row


def test_the_last_element_a_kernel_may_index_lies_inside_the_block(printed):
    for (n, views, nclasses, env), t in zip(ROWS, printed[0]):
        row = (n, views, nclasses, env)
        k, g, w = t['park_slots'], t['ngroups'], t['park_stride']
        if k > 0:
            last_mask = t['umask_off'] + 8 * ((k - 1) * g + g - 1)             # umask[(park_slots - 1) * ngroups + ngroups - 1]
            assert t['umask_off'] <= last_mask and last_mask + 8 <= t['park_off'], row
            last_bin = t['park_off'] + 4 * ((k - 1) * w + w - 1)               # park[(park_slots - 1) * park_stride + park_stride - 1]
            assert t['park_off'] <= last_bin and last_bin + 4 <= t['bytes'], row
        if n > 0:
            assert 16 + 4 * (n - 1) + 4 <= t['list2_off'], row                  # list[n - 1]
            assert t['list2_off'] + 4 * (n - 1) + 4 <= t['umask_off'], row      # list2[n - 1]
        assert 4 * w >= nclasses + 3, row                                       # a byte per label 0..nclasses, "no sample" and "rejected"


def test_parked_slots_exist_exactly_up_to_sixteen_groups(printed):
    seen = set()
    for (n, views, nclasses, env), t in zip(ROWS, printed[0]):
        row = (n, views, nclasses, env)
        if views == 0 or views > 1024:
            assert t['park_slots'] == 0, row
        else:
            want = min(max(n // 16 + 4096 if env is None else env, 0), n)
            assert t['park_slots'] == want and t['ngroups'] <= MAX_GROUPS, row
            seen.add((want == 0, want == n))
        assert 0 <= t['park_slots'] <= n, row
    assert seen == {(True, True), (True, False), (False, True), (False, False)}   # no slots of no points, none forced, every point, some


def test_the_reserved_size_covers_every_number_of_classes(printed):
    """f3d_ctx_reserve sizes the block with F3D_CODE_MAX_NCLASSES: no call with fewer classes may need more."""
    by = {row: t['bytes'] for row, t in zip(ROWS, printed[0])}
    for (n, views, nclasses, env), b in by.items():
        assert by[(n, views, MAX_NCLASSES, env)] >= b, (n, views, nclasses, env)


def test_nothing_overflows_at_the_largest_cloud(printed):
    """n = 0x7ffff000 (the launcher's limit) with 1024 views and every number of parked slots: the sums in Python integers beside
    the program's size_t, the slot count inside an int, the largest element index inside 63 bits."""
    n = 0x7ffff000
    rows = [(row, t) for row, t in zip(ROWS, printed[0]) if row[0] == n and row[1] == 1024]
    assert len(rows) == len(NCLASSES) * 7
    for (_, views, nclasses, env), t in rows:
        slots = min(max(n // 16 + 4096 if env is None else env, 0), n)
        assert t['park_slots'] == slots < 2 ** 31
        words = (nclasses + 6) // 4
        total = 16 + 8 * n + 8 * slots * 16 + 4 * slots * words
        assert t['bytes'] == total < 2 ** 63
        assert (slots * 16 + 15) < 2 ** 63 and slots * words + words - 1 < 2 ** 63
    assert max(t['bytes'] for _, t in rows) == 16 + 8 * n + n * (8 * 16 + 4 * 64)      # every point parked, 253 classes: 0.8 TB, no wrap
