"""f3d_grid_for (csrc/f3d_kernels.h) without a GPU: its clamp and the process-wide debug cap, printed by a stand-alone host program
and compared with the clamp restated here; and two readings of the kernel sources -- every file that sizes a grid with it has a case in
tests/family_cases.py (which tests/test_launch_shape_gpu.py runs under the cap), and every kernel launched with such a grid walks its items with a gridDim.x stride."""
import ast
import os
import re
import subprocess

import pytest

from conftest import ROOT, PKG

CSRC = PKG / 'csrc'
PER_BLOCK_AND_CAP = [(256, 8192), (128, 2048), (4, 65536), (1, 8192), (256, 64), (16, 1 << 20)]
DEBUG_CAPS = [0, 1, 3, (1 << 20) + 5]                      # off, one block, three blocks, above every cap


def items_for(per_block, cap):
    return [0, 1, per_block - 1, per_block, per_block + 1, cap * per_block - 1, cap * per_block, cap * per_block + 1, 1 << 40]


ROWS = [(n, pb, cap, dbg) for dbg in DEBUG_CAPS for pb, cap in PER_BLOCK_AND_CAP for n in items_for(pb, cap)]

PROGRAM = r'''
#include <stdio.h>
#include <stdlib.h>
#include "f3d_kernels.h"
int main(int argc, char** argv) {
    for (int i = 1; i + 3 < argc; i += 4) {
        const long long n = atoll(argv[i]);
        const int per_block = atoi(argv[i + 1]), cap = atoi(argv[i + 2]), dbg = atoi(argv[i + 3]);
        f3d_grid_debug_state.blocks.store(dbg);
        printf("%d\n", f3d_grid_for(n, per_block, cap));
    }
    printf("%lld %lld\n", f3d_grid_debug_state.calls.load(), f3d_grid_debug_state.lowered.load());
    return 0;
}
'''


def clamp(n, per_block, cap):
    """ceil(n / per_block) clamped to [1, cap]: what f3d_grid_for returned before it knew of a debug cap."""
    return min(max(-(-n // per_block), 1), cap)


def capped(n, per_block, cap, dbg):
    """The debug cap is one more upper bound when it is on (dbg > 0): it never raises a grid and never goes below one block."""
    g = clamp(n, per_block, cap)
    return min(g, dbg) if dbg > 0 else g


@pytest.fixture(scope='module')
def printed(tmp_path_factory):
    work = tmp_path_factory.mktemp('grid_for')
    (work / 'grid_for.cpp').write_text(PROGRAM)
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    subprocess.run([hipcc, '-x', 'hip', '--cuda-host-only', '-O1', '-std=c++17', f'-I{ROOT / "include"}', f'-I{CSRC}',
                    str(work / 'grid_for.cpp'), '-o', str(work / 'grid_for')], check=True, capture_output=True)
    args = [str(x) for row in ROWS for x in row]
    lines = subprocess.run([str(work / 'grid_for')] + args, check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(lines) == len(ROWS) + 1
    return [int(x) for x in lines[:-1]], tuple(int(x) for x in lines[-1].split())


def test_the_restated_clamp_is_what_its_comment_says():
    assert [clamp(n, 256, 8192) for n in (0, 1, 255, 256, 257, 8192 * 256, 8192 * 256 + 1, 1 << 40)] == [1, 1, 1, 1, 2, 8192, 8192, 8192]
    assert [capped(2500, 256, 8192, d) for d in (0, 1, 3, 9, 10, 11)] == [10, 1, 3, 9, 10, 10]
    assert capped(0, 256, 8192, 3) == 1 and capped(70, 256, 64, 1 << 20) == 1 and capped(1 << 40, 4, 64, 1 << 20) == 64


def test_grid_for_is_the_clamp_under_every_debug_cap(printed):
    grids, _ = printed
    for row, g in zip(ROWS, grids):
        assert g == capped(*row), row
        assert 1 <= g <= clamp(*row[:3]), row                              # never below one block, never above the uncapped grid


def test_the_counters_count_the_capped_and_the_lowered_calls(printed):
    _, (calls, lowered) = printed
    assert calls == sum(1 for row in ROWS if row[3] > 0)
    assert lowered == sum(1 for row in ROWS if row[3] > 0 and capped(*row) < clamp(*row[:3]))
    assert 0 < lowered < calls                                             # the rows hold both kinds


# ---- the sources ------------------------------------------------------------------------------------------------------------------

def sources_with_grid_for():
    return sorted(p.name for p in CSRC.glob('*.hip') if 'f3d_grid_for(' in p.read_text())


def cases_keys():
    """The keys of the CASES table of tests/family_cases.py as its source lists them: a key written twice shows here, in the dict it would not."""
    tree = ast.parse((ROOT / 'tests' / 'family_cases.py').read_text())
    for node in tree.body:
        if isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id == 'CASES' for t in node.targets):
            assert isinstance(node.value, ast.Dict)
            return [ast.literal_eval(k) for k in node.value.keys]
    raise AssertionError('family_cases.py has no CASES table')


def test_every_source_that_sizes_a_grid_has_a_launch_shape_case():
    import family_cases
    keys = cases_keys()
    assert len(keys) == len(set(keys)) and sorted(keys) == sorted(family_cases.CASES)     # the table the GPU tests import is the one read here
    assert sorted(keys) == sources_with_grid_for()                         # none uncovered, none stale


def _block(text, at):
    """The {...} that opens at or after text[at]."""
    i = text.index('{', at)
    depth = 0
    for j in range(i, len(text)):
        depth += text[j] == '{'
        depth -= text[j] == '}'
        if depth == 0:
            return text[i:j + 1]
    raise AssertionError('unbalanced braces')


def _call_args(text, at):
    """The top-level arguments of the call whose '(' is text[at]."""
    depth, args, start = 0, [], at + 1
    for j in range(at, len(text)):
        c = text[j]
        if c in '(<[' and not (c == '<' and text[j + 1] in ' =<'):
            depth += 1
        elif c in ')>]' and not (c == '>' and text[j - 1] in ' -'):
            depth -= 1
            if depth == 0:
                args.append(text[start:j])
                return args
        elif c == ',' and depth == 1:
            args.append(text[start:j])
            start = j + 1
    raise AssertionError('unbalanced call')


def striders(text):
    """Names of the function-like macros and __device__ functions of `text` whose own text holds a gridDim.x stride."""
    names = set()
    for m in re.finditer(r'#define\s+(\w+)\([^)]*\)((?:.*\\\n)*.*)', text):
        if 'gridDim.x' in m.group(2):
            names.add(m.group(1))
    for m in re.finditer(r'__device__[^;{}()]*?\b(\w+)\s*\(', text):
        if 'gridDim.x' in _block(text, m.end()):
            names.add(m.group(1))
    return names


def kernels_of(text):
    out = {}
    for m in re.finditer(r'__global__(?:\s+void|\s+__launch_bounds__\([^)]*\)|\s+static)*\s+(\w+)\s*\(', text):
        out[m.group(1)] = _block(text, m.end())
    return out


def grid_makers(text):
    """f3d_grid_for and the file's functions that return it (grid_of, lift_grid, knn_grid, capped)."""
    return {'f3d_grid_for'} | {m.group(1) for m in re.finditer(r'\b(\w+)\s*\([^()]*\)\s*\{[^{}]*?return\s+[^;]*f3d_grid_for\(', text)}


def grid_variables(body, makers):
    """The dim3 / int variables of a function body that are initialised from one of the makers: `g(f3d_grid_for(..`, `gp = lift_grid(..`."""
    pattern = r'\b(\w+)\s*(?:=|\()\s*(?:dim3\()?\s*(?:\(unsigned\))?\s*(?:' + '|'.join(sorted(makers)) + r')\('
    return {m.group(1) for m in re.finditer(pattern, body)} - {'dim3', 'return'}


def launches_without_stride():
    shared = set()
    for h in CSRC.glob('*.h'):
        shared |= striders(h.read_text())
    found, missing = 0, []
    for name in sources_with_grid_for():
        text = (CSRC / name).read_text()
        walk = shared | striders(text)
        kernels = kernels_of(text)
        makers = grid_makers(text)
        # a function's variables are its own: the launches are read function by function
        seen = set()
        for fm in re.finditer(r'^(?:hipError_t|void|static|template|int|dim3)\b[^;{}]*\{', text, re.M):
            if fm.end() in seen:                                               # (a template's function matches at both of its lines)
                continue
            seen.add(fm.end())
            body = _block(text, fm.start())
            grids = makers | grid_variables(body, makers)
            for lm in re.finditer(r'hipLaunchKernelGGL\(', body):
                args = _call_args(body, lm.end() - 1)
                if not any(re.search(r'\b' + g + r'\b', args[1]) for g in grids):
                    continue
                kernel = re.match(r'[\s(]*(\w+)', args[0]).group(1)
                found += 1
                kbody = kernels[kernel]
                if 'gridDim.x' not in kbody and not any(re.search(r'\b' + w + r'\b', kbody) for w in walk):
                    missing.append(f'{name}: {kernel}')
    return found, sorted(set(missing))


def test_every_kernel_behind_f3d_grid_for_has_a_grid_stride():
    """A kernel that computes `k = blockIdx.x * B + threadIdx.x; if (k >= count) return;` is right only while its grid covers every
    item, which f3d_grid_for does not promise: above its cap, or under the debug cap, the rest would stay unwritten.

    What this reads: every hipLaunchKernelGGL of the files that call f3d_grid_for whose grid argument holds f3d_grid_for(...), one of
    the file's functions that return it (grid_of, lift_grid, knn_grid, capped) or a variable of the same function initialised from either.
    The launched kernel's text must hold `gridDim.x`, or use a macro or __device__ function (of the file or of a csrc header) whose
    text does: MESH_LOOP, PL_LOOP, f3d_chunk_heads, f3d_group_waves, lift_rows, the rider blocks of f3d_fuse_blocks.h.

    What it does not catch: a kernel that names gridDim.x without striding by it (or strides over the wrong count); a grid that reaches
    the launch through a struct member or a function argument (the riders of the cell sort, which take their block count as an
    argument); launches hidden in a macro's text.  tests/test_launch_shape_gpu.py covers those by running them under the cap."""
    found, missing = launches_without_stride()
    assert found >= 100, found                                             # the reading still finds the launches (92 call sites, several used twice)
    assert missing == []
