"""tests/route_cases.py is complete and well-formed, without a GPU: every public device route of the packages and every ``*_dev`` method of
f3d.Context is in its tables or in NOT_COVERED (so a new route or entry without a case fails here), nothing is named twice, nothing
unknown is named, the caps on what may be left out hold, and the two seeds of every case agree in shape and dtype and differ in rows."""
import ast
import inspect
import sys
from pathlib import Path

import numpy as np
import pytest

import f3d
import family_cases as F
import route_cases as R

PKG = Path(f3d.__file__).resolve().parent.parent
MARKS = ('on_device', 'torch_device', 'work_stream')


def _sources():
    return sorted(list((PKG / 'Fusion3DSeg').rglob('*.py')) + list((PKG / 'RTAB_utils').rglob('*.py')) + [PKG / 'get2DSeg.py'])


def _hands_off(node):
    """The definition calls on_device / torch_device / work_stream or reads a .cuda_stream."""
    for n in ast.walk(node):
        if isinstance(n, ast.Call):
            f = n.func
            if (f.id if isinstance(f, ast.Name) else f.attr if isinstance(f, ast.Attribute) else None) in MARKS:
                return True
        if isinstance(n, ast.Attribute) and n.attr == 'cuda_stream':
            return True
    return False


def routes_of(source):
    """The public top-level functions and classes of a module that hand tensors to the library: themselves, or through a private
    top-level helper of the module that they name (transitively)."""
    tops = {n.name: n for n in ast.parse(source).body if isinstance(n, (ast.FunctionDef, ast.ClassDef))}
    hit = {k for k, n in tops.items() if _hands_off(n)}
    grown = True
    while grown:
        grown = False
        for k, n in tops.items():
            if k not in hit:
                named = {x.id for x in ast.walk(n) if isinstance(x, ast.Name)} | {x.attr for x in ast.walk(n) if isinstance(x, ast.Attribute)}
                if any(r in hit and r.startswith('_') for r in named):
                    hit.add(k)
                    grown = True
    return [k for k in tops if k in hit and not k.startswith('_')]


def all_routes():
    return [f'{p.relative_to(PKG).as_posix()}::{name}' for p in _sources() for name in routes_of(p.read_text())]


def dev_entries():
    return [name for name, fn in inspect.getmembers(f3d.Context, inspect.isfunction) if name.endswith('_dev')]


def test_the_walk_finds_routes_through_private_helpers():
    src = ('from f3d.tensors import work_stream\n'
           'def _inner(x):\n    with work_stream(x.device) as w:\n        return w\n'
           'def _middle(x):\n    return _inner(x)\n'
           'def outer(x):\n    return _middle(x)\n'
           'def plain(x):\n    return x + 1\n'
           'class Keeps:\n    def go(self, s):\n        return s.cuda_stream\n')
    assert routes_of(src) == ['outer', 'Keeps']


def test_every_public_route_has_a_case_or_a_reason():
    routes = all_routes()
    assert len(routes) == len(set(routes)) and len(routes) >= 45
    left_out = [k for k in R.NOT_COVERED if '::' in k]
    assert not set(R.ROUTES) & set(left_out), 'a route is both covered and left out'
    missing = sorted(set(routes) - set(R.ROUTES) - set(left_out))
    assert not missing, f'device routes without a case in tests/route_cases.py: {missing}'
    unknown = sorted((set(R.ROUTES) | set(left_out)) - set(routes))
    assert not unknown, f'tests/route_cases.py names routes the packages do not have: {unknown}'
    assert all(isinstance(reason, str) and len(reason) > 20 for reason in R.NOT_COVERED.values())


def test_every_dev_entry_has_a_case_or_a_reason():
    entries = dev_entries()
    assert len(entries) >= 75
    left_out = [k for k in R.NOT_COVERED if '::' not in k]
    assert not set(R.DEV_ENTRIES) & set(left_out), 'an entry is both covered and left out'
    missing = sorted(set(entries) - set(R.DEV_ENTRIES) - set(left_out))
    assert not missing, f'*_dev entries of f3d.Context without a case in tests/route_cases.py: {missing}'
    unknown = sorted((set(R.DEV_ENTRIES) | set(left_out)) - set(entries))
    assert not unknown, f'tests/route_cases.py names entries f3d.Context does not have: {unknown}'
    assert len(left_out) <= R.MAX_ENTRIES_LEFT_OUT == 8
    assert R.NEVER_LEFT_OUT == ('project_vote_argmax_dev', 'fuse_chunk', 'radius_query', 'estimate_normals_batch_dev', 'tsdf_', 'icp')
    protected = [e for e in entries if e == 'project_vote_argmax_dev' or e == 'estimate_normals_batch_dev' or e.startswith(('fuse_chunk', 'radius_query',
                                                                                                                             'tsdf_', 'icp'))]
    assert len(protected) >= 17 and not set(protected) & set(left_out)
    for name in ('project_vote_argmax_dev', 'cloud_sort_cells_dev', 'render_counts_dev', 'raster_counts_dev', 'segment_votes_lastcol_dev',
                 'sem_logits_to_mask_dev'):
        assert R.DEV_ENTRIES.get(name), name                                     # no package route reaches these: cases drive them directly


def test_a_new_route_or_entry_without_a_case_is_noticed(monkeypatch):
    monkeypatch.setattr(f3d.Context, 'brand_new_dev', lambda self: None, raising=False)
    with pytest.raises(AssertionError, match='brand_new_dev'):
        test_every_dev_entry_has_a_case_or_a_reason()
    found = all_routes()
    dummy = 'from f3d.tensors import work_stream\ndef _go(x):\n    with work_stream(x.device) as w:\n        return w\ndef brand_new_route(x):\n    return _go(x)\n'
    monkeypatch.setattr(sys.modules[__name__], 'all_routes', lambda: found + [f'Fusion3DSeg/fusion.py::{n}' for n in routes_of(dummy)])
    with pytest.raises(AssertionError, match='without a case.*brand_new_route'):
        test_every_public_route_has_a_case_or_a_reason()
    monkeypatch.setattr(sys.modules[__name__], 'all_routes', lambda: found)
    monkeypatch.setitem(R.ROUTES, 'Fusion3DSeg/fusion.py::no_such_route', ['plane_distance'])
    with pytest.raises(AssertionError, match='do not have.*no_such_route'):
        test_every_public_route_has_a_case_or_a_reason()


def test_the_table_is_consistent():
    for name, r in R.TABLE.items():
        assert r.routes or r.entries, name
        assert r.case.__doc__, name
        if not r.routes:                                                         # a directly driven entry: none of the packages' routes reaches it
            assert all(R.DEV_ENTRIES[e] for e in r.entries)
    stateful = {n for n, r in R.TABLE.items() if r.stateful}
    assert {'fuse_device_votes', 'FeatureFusion', 'TSDFVolume', 'track_frames'} <= stateful


@pytest.mark.parametrize('name', sorted(R.TABLE))
def test_both_seeds_of_a_case(name):
    """Seed A and seed B give inputs of the same names, shapes and dtypes that differ, and reference rows that differ: a route that read
    the decoy cannot pass the scene's check by accident."""
    r = R.TABLE[name]
    a, b = R.prepared(name, R.SEED), R.prepared(name, R.OTHER_SEED)
    assert list(a[0]) == list(b[0]) and a[0]
    differing = 0
    for key in a[0]:
        x, y = a[0][key], b[0][key]
        assert isinstance(x, np.ndarray) and x.flags.c_contiguous and x.dtype == y.dtype and x.shape == y.shape, key
        differing += not np.array_equal(x, y, equal_nan=x.dtype.kind == 'f')
    assert differing >= 1
    assert set(r.inplace) <= set(a[0]) and set(r.alt) <= set(a[0]) and set(r.names) <= set(a[0]), name
    for key, dtypes in r.alt.items():                                            # the other dtypes hold the same values
        for dt in dtypes:
            back = a[0][key].astype(dt).astype(a[0][key].dtype)
            assert np.array_equal(back, a[0][key], equal_nan=True) if back.dtype.kind == 'f' else (back == a[0][key]).all(), (key, dt)
    rows_a, rows_b = a[4], b[4]
    assert len(rows_a) > 0 and 2 * F.rows_that_differ(rows_a, rows_b) >= min(len(rows_a), len(rows_b)), F.rows_that_differ(rows_a, rows_b)
    assert callable(a[1]) and callable(a[3])
