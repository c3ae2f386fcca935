"""smooth_votes / smooth_segment on the GPU (f3d_smooth_*, csrc/f3d_smooth.hip) against the restatement tests/smooth_ref.py.  The
contract fixes every rounding, so every comparison is array_equal: shapes around the 64-column chunks, row lengths around the
64-entry rounds, the gates with their ties and NaNs, self weights, iterations, both input types, the segment epilogue against
segment_votes of the written matrix, the call paths, a strict context, index errors, and the chain into split_into_instances."""
import functools
import math

import numpy as np
import pytest

import f3d
import smooth_ref as R
from oracle import np_ref as O

pytestmark = pytest.mark.gpu

COS30 = math.cos(math.radians(30.0))


def V():
    from Fusion3DSeg.segUtils import voting
    return voting


def _np(x):
    return x.cpu().numpy() if hasattr(x, 'cpu') else np.asarray(x)


def _dev(*arrays):
    import torch
    out = []
    for a in arrays:
        if a is None:
            out.append(None)
        elif np.asarray(a).dtype == np.uint16:                                  # uint16 travels as int16 bits
            out.append(torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda())
        else:
            out.append(torch.as_tensor(np.array(a), device='cuda'))
    return tuple(out)


def _graph(n, rng, max_len=12):
    """A random CSR: asymmetric, rows of 0 .. max_len entries drawn with replacement (duplicates, the point itself now and then)."""
    lens = rng.integers(0, max_len + 1, n)
    offs = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=offs[1:])
    return offs, rng.integers(0, n, offs[-1]).astype(np.int32)


def _csr(rows):
    offs = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=offs[1:])
    return offs, (np.concatenate([np.asarray(r, np.int64) for r in rows]) if offs[-1] else np.zeros(0)).astype(np.int32)


def _votes(n, ncols, rng, kind):
    if kind == 'u16':
        return rng.integers(0, 65536, (n, ncols)).astype(np.uint16)
    if kind == 'int':                                                           # vote counts as the voters write them, with empty rows
        v = rng.integers(0, 9, (n, ncols)).astype(np.float64)
        v[rng.random(n) < 0.2] = 0
        return v
    return rng.standard_normal((n, ncols)) * 10.0 ** rng.integers(-3, 4, (n, ncols))


def _normals(n, rng):
    v = rng.standard_normal((n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _ctx():
    return f3d.default_context()


# ------------------------------------------------------------------------------------------------ shapes
SHAPES = [(n, c) for n in (1, 2, 63, 64, 65, 257) for c in (1, 2, 63, 64, 65, 134, 256)] + [(5000, 134), (5000, 256)]


@pytest.mark.parametrize('n,ncols', SHAPES, ids=[f'{n}x{c}' for n, c in SHAPES])
def test_shapes(n, ncols):
    rng = np.random.default_rng(n * 1000 + ncols)
    offs, nbrs = _graph(n, rng)
    v = _votes(n, ncols, rng, 'f64')
    assert np.array_equal(_ctx().smooth_votes(v, offs, nbrs), R.smooth(v, offs, nbrs))
    u = _votes(n, ncols, rng, 'u16')
    want = R.smooth(u, offs, nbrs, self_weight=2.0)
    assert np.array_equal(_ctx().smooth_votes(u, offs, nbrs, self_weight=2.0), want)
    assert np.array_equal(_ctx().smooth_segment(u, offs, nbrs, ncols - 1, 0.0, self_weight=2.0), O.segment(want, ncols - 1, 0.0))


# ------------------------------------------------------------------------------------------------ rows
@functools.lru_cache(maxsize=None)
def _row_scene():
    """400 points, 134 columns.  Rows 0 .. 11: empty; the point alone; another point alone; 63, 64, 65 and 300 entries; the point
    listed first, last and not at all; an entry listed twice; a row that is the point three times.  The rest: a random asymmetric graph."""
    rng = np.random.default_rng(7)
    n = 400
    offs, nbrs = _graph(n, rng)
    rows = [nbrs[offs[i]:offs[i + 1]].tolist() for i in range(n)]
    rows[0] = []
    rows[1] = [1]
    rows[2] = [7]
    for i, m in ((3, 63), (4, 64), (5, 65), (6, 300)):
        rows[i] = rng.integers(0, n, m).tolist()
    rows[7] = [7, 20, 21, 22]
    rows[8] = [20, 21, 22, 8]
    rows[9] = [20, 21, 22]
    rows[10] = [30, 31, 30, 32]
    rows[11] = [11, 11, 11]
    assert any(a not in rows[b] for a in range(12, 40) for b in rows[a] if b >= 12)          # asymmetric
    return n, _csr(rows), _votes(n, 134, rng, 'f64'), _votes(n, 134, rng, 'int'), _normals(n, rng), rng.random((n, 3))


@pytest.mark.parametrize('gate', ['none', 'normals', 'both'])
def test_rows(gate):
    n, (offs, nbrs), v, vi, nrm, col = _row_scene()
    kw = {}
    if gate != 'none':
        kw.update(normals=nrm, cos_angle=0.4)
    if gate == 'both':
        kw.update(colors=col, max_color_dist=0.7)
    want = R.smooth(v, offs, nbrs, **kw)
    got = _ctx().smooth_votes(v, offs, nbrs, **kw)
    assert np.array_equal(got, want)
    if gate == 'none':                                                         # the named rows, spelt out
        assert np.array_equal(got[0], v[0]) and np.array_equal(got[1], v[1]) and np.array_equal(got[2], v[2] + v[7])
        assert np.array_equal(got[7], ((v[7] + v[20]) + v[21]) + v[22])
        assert np.array_equal(got[8], ((v[8] + v[20]) + v[21]) + v[22]) and np.array_equal(got[9], ((v[9] + v[20]) + v[21]) + v[22])
        assert np.array_equal(got[10], (((v[10] + v[30]) + v[31]) + v[30]) + v[32]) and np.array_equal(got[11], v[11])
    else:                                                                      # the gate closes some entries of the long rows and not all
        a, b = nrm[6], nrm[nbrs[offs[6]:offs[7]]]
        passed = np.abs((a[0] * b[:, 0] + a[1] * b[:, 1]) + a[2] * b[:, 2]) >= 0.4
        assert 30 < passed.sum() < 270
    assert np.array_equal(_ctx().smooth_segment(vi, offs, nbrs, 133, 0.5, **kw), R.smooth_segment(vi, offs, nbrs, 133, 0.5, **kw))


# ------------------------------------------------------------------------------------------------ gates
@functools.lru_cache(maxsize=None)
def _gate_scene():
    rng = np.random.default_rng(11)
    n = 300
    offs, nbrs = _graph(n, rng, 90)
    nrm = _normals(n, rng)
    nrm[rng.random(n) < 0.05] = np.nan                                         # NaN normals: their comparisons are false
    nrm[5, 1] = np.nan
    col = rng.random((n, 3))
    col[17] = np.nan
    return n, offs, nbrs, _votes(n, 70, rng, 'f64'), nrm, col


@pytest.mark.parametrize('gate', ['none', 'normals', 'colors32', 'colors64', 'both32', 'both64'])
def test_gates(gate):
    n, offs, nbrs, v, nrm, col = _gate_scene()
    kw = {}
    if gate in ('normals', 'both32', 'both64'):
        kw.update(normals=nrm, cos_angle=0.5)
    if gate.endswith('32'):
        kw.update(colors=col.astype(np.float32), max_color_dist=0.6)
    if gate.endswith('64'):
        kw.update(colors=col, max_color_dist=0.6)
    want = R.smooth(v, offs, nbrs, **kw)
    assert np.array_equal(_ctx().smooth_votes(v, offs, nbrs, **kw), want)
    if 'normals' in kw:                                                        # a NaN normal: the point keeps its own row, and gives to nobody
        bad = np.flatnonzero(np.isnan(nrm).any(1))
        assert len(bad) > 5 and np.array_equal(want[bad], v[bad])
    plain = R.smooth(v, offs, nbrs)
    assert (gate == 'none') == np.array_equal(want, plain)


def test_gate_ties_are_inside():
    """|dot| == cos_angle with axis-aligned normals and cos_angle = 1.0; a colour distance equal to the limit (3-4-5)."""
    v = np.array([[1.0, 0.5], [10.0, 0.25], [100.0, 0.125], [1000.0, 0.0625], [1e4, 0.03125]])
    offs, nbrs = _csr([[1, 2, 3, 4], [], [], [], []])
    nrm = np.array([[1.0, 0, 0], [1.0, 0, 0], [-1.0, 0, 0], [0, 1.0, 0], [0, 0, -1.0]])
    got = _ctx().smooth_votes(v, offs, nbrs, normals=nrm, cos_angle=1.0)
    assert np.array_equal(got, R.smooth(v, offs, nbrs, normals=nrm, cos_angle=1.0))
    assert np.array_equal(got[0], (v[0] + v[1]) + v[2])                        # +x and -x pass at equality, y and z do not
    col = np.array([[0.0, 0, 0], [3.0, 4.0, 0], [3.0, 4.0, 0.001], [0, 5.0, 0], [0, 0, 5.5]])
    for c in (col, col.astype(np.float32)):
        got = _ctx().smooth_votes(v, offs, nbrs, colors=c, max_color_dist=5.0)
        assert np.array_equal(got, R.smooth(v, offs, nbrs, colors=c, max_color_dist=5.0))
        assert np.array_equal(got[0], (v[0] + v[1]) + v[3])                    # 9 + 16 == 25 passes, a hair more does not


# ------------------------------------------------------------------------------------------------ self weight, iterations, inputs
@pytest.mark.parametrize('iterations', [1, 2, 3])
@pytest.mark.parametrize('self_weight', [0.0, 1.0, 3.0, 0.5])
def test_self_weight_and_iterations(self_weight, iterations):
    rng = np.random.default_rng(23)
    n, ncols = 257, 65
    offs, nbrs = _graph(n, rng)
    nrm = _normals(n, rng)
    for kind in ('f64', 'u16'):                                                # non-integer float64 too: the order is fixed
        v = _votes(n, ncols, rng, kind)
        kw = dict(self_weight=self_weight, iterations=iterations)
        assert np.array_equal(_ctx().smooth_votes(v, offs, nbrs, **kw), R.smooth(v, offs, nbrs, **kw))
        kw.update(normals=nrm, cos_angle=0.3)
        assert np.array_equal(_ctx().smooth_votes(v, offs, nbrs, **kw), R.smooth(v, offs, nbrs, **kw))
    if self_weight == int(self_weight):
        vi = _votes(n, ncols, rng, 'int')
        kw = dict(self_weight=self_weight, iterations=iterations)
        assert np.array_equal(_ctx().smooth_segment(vi, offs, nbrs, 64, 0.5, **kw), R.smooth_segment(vi, offs, nbrs, 64, 0.5, **kw))


# ------------------------------------------------------------------------------------------------ smooth_segment
@functools.lru_cache(maxsize=None)
def _segment_scene():
    """Integer votes over 134 columns; the points 0 .. 39 vote nothing and see only each other, so their rows end with total 0."""
    rng = np.random.default_rng(31)
    n = 500
    offs, nbrs = _graph(n, rng, 20)
    rows = [nbrs[offs[i]:offs[i + 1]].tolist() for i in range(n)]
    for i in range(40):
        rows[i] = rng.integers(0, 40, 5).tolist()
    v = np.zeros((n, 134))
    hot = rng.integers(0, 134, (n, 3))                                         # a few classes per row, as a real vote has them
    for k in range(3):
        v[np.arange(n), hot[:, k]] += rng.integers(1, 9, n)
    v[:40] = 0
    v[rng.random(n) < 0.1] = 0
    v[:, 133] = np.maximum(v[:, 133], v[:, :133].sum(1))                       # a plausible last column for the lastcol rules
    return n, _csr(rows), v


FILTERS = {'none': None, 'three': [86, 114, 115], 'aliasing': [2, 0, 1, 86], 'long': list(range(133, 60, -1))}


@pytest.mark.parametrize('lastcol', [False, True], ids=['rowsum', 'lastcol'])
@pytest.mark.parametrize('flt', list(FILTERS))
@pytest.mark.parametrize('threshold', [0.0, 0.5])
def test_smooth_segment(threshold, flt, lastcol):
    n, (offs, nbrs), v = _segment_scene()
    flt = FILTERS[flt]
    ctx = _ctx()
    for kw in (dict(), dict(iterations=2, self_weight=2.0)):
        got = ctx.smooth_segment(v, offs, nbrs, 133, threshold, flt, lastcol, **kw)
        matrix = ctx.smooth_votes(v, offs, nbrs, **kw)
        two_step = (ctx.segment_votes_lastcol if lastcol else ctx.segment_votes)(matrix, 133, threshold, flt)
        assert np.array_equal(got, two_step)
        assert np.array_equal(got, R.smooth_segment(v, offs, nbrs, 133, threshold, flt, lastcol, **kw))
        assert (matrix[:40] == 0).all() and (got[:40] == 133).all()                # rows that end with total 0
    u = v.astype(np.uint16)
    assert np.array_equal(ctx.smooth_segment(u, offs, nbrs, 133, threshold, flt, lastcol), R.smooth_segment(v, offs, nbrs, 133, threshold, flt, lastcol))


# ------------------------------------------------------------------------------------------------ call paths
@pytest.mark.parametrize('kind', ['f64', 'u16'])
def test_host_dev_and_tensor_paths_agree_and_repeat(kind):
    import torch
    n, (offs, nbrs), _, _, nrm, col = _row_scene()
    rng = np.random.default_rng(41)
    v = _votes(n, 134, rng, kind if kind == 'u16' else 'int')
    col32 = col.astype(np.float32)
    kw = dict(normals=nrm, cos_angle=COS30, colors=col32, max_color_dist=0.8, self_weight=2.0, iterations=3)
    want = R.smooth(v, offs, nbrs, **kw)
    want_cls = O.segment(want, 133, 0.5, [86, 114, 115])
    ctx = _ctx()
    host = ctx.smooth_votes(v, offs, nbrs, **kw)
    assert np.array_equal(host, want) and np.array_equal(ctx.smooth_votes(v, offs, nbrs, **kw), host)
    assert np.array_equal(ctx.smooth_segment(v, offs, nbrs, 133, 0.5, [86, 114, 115], **kw), want_cls)
    dv, do, db, dn, dc = _dev(v, offs, nbrs, nrm, col32)
    st = torch.cuda.current_stream().cuda_stream
    for _ in range(2):                                                         # the _dev entries, twice: identical bits
        out = torch.full((n, 134), -7.0, dtype=torch.float64, device='cuda')
        cls = torch.full((n,), -7, dtype=torch.int64, device='cuda')
        torch.cuda.synchronize()
        ctx.smooth_votes_dev(dv.data_ptr(), f3d._vtype(dv), n, 134, do.data_ptr(), db.data_ptr(), dn.data_ptr(), COS30, dc.data_ptr(), f3d.F32,
                             0.8, 2.0, 3, out.data_ptr(), st)
        ctx.smooth_segment_dev(dv.data_ptr(), f3d._vtype(dv), n, 134, do.data_ptr(), db.data_ptr(), dn.data_ptr(), COS30, dc.data_ptr(), f3d.F32,
                               0.8, 2.0, 3, 133, 0.5, [86, 114, 115], False, cls.data_ptr(), st)
        ctx.take_device_error(st)
        assert np.array_equal(_np(out), want) and np.array_equal(_np(cls), want_cls)
    gates = dict(normals=dn, angle=30.0, colors=dc, max_color_dist=0.8, self_weight=2.0, iterations=3)
    got = V().smooth_votes(dv, (do, db), **gates)                              # device tensors through the module
    assert got.is_cuda and np.array_equal(_np(got), want)
    mine = torch.empty((n, 134), dtype=torch.float64, device='cuda')
    assert V().smooth_votes(dv, (do, db), out=mine, **gates) is mine and np.array_equal(_np(mine), want)
    got = V().smooth_segment(dv, (do, db), 133, 0.5, [86, 114, 115], **gates)
    assert got.is_cuda and np.array_equal(_np(got), want_cls)
    hgates = dict(gates, normals=nrm, colors=col32)                            # host arrays and a list of rows through the module
    rows = [nbrs[offs[i]:offs[i + 1]] for i in range(n)]
    assert np.array_equal(V().smooth_votes(v, rows, **hgates), want)
    assert np.array_equal(V().smooth_segment(v, (offs, nbrs), 133, 0.5, [86, 114, 115], **hgates), want_cls)
    into = np.empty((n, 134))
    assert V().smooth_votes(v, (offs, nbrs), out=into, **hgates) is into and np.array_equal(into, want)


def test_even_and_odd_iterations_land_in_votes_out():
    import torch
    n, (offs, nbrs), v, _, _, _ = _row_scene()
    ctx = _ctx()
    dv, do, db = _dev(v, offs, nbrs)
    st = torch.cuda.current_stream().cuda_stream
    for it in (1, 2, 3, 4):
        out = torch.full((n, 134), -7.0, dtype=torch.float64, device='cuda')
        torch.cuda.synchronize()
        ctx.smooth_votes_dev(dv.data_ptr(), f3d.VOTES_F64, n, 134, do.data_ptr(), db.data_ptr(), None, 0.0, None, f3d.F64, 0.0, 0.5, it,
                             out.data_ptr(), st)
        ctx.take_device_error(st)
        assert np.array_equal(_np(out), R.smooth(v, offs, nbrs, self_weight=0.5, iterations=it)), it
    assert np.array_equal(_np(dv), v)                                          # the input is never written


def test_c_entry_argument_errors():
    import torch
    n, (offs, nbrs), v, _, nrm, col = _row_scene()
    ctx = _ctx()
    with pytest.raises(ValueError, match='bad arguments'):
        ctx.smooth_votes(np.zeros((4, 257)), np.zeros(5, np.int64), np.zeros(0, np.int32))
    with pytest.raises(ValueError, match='bad arguments'):
        ctx.smooth_votes(v, offs, nbrs, iterations=0)
    with pytest.raises(ValueError, match='bad arguments'):
        ctx.smooth_votes(v, offs, nbrs, self_weight=-1.0)
    with pytest.raises(ValueError, match='bad arguments'):
        ctx.smooth_votes(v, offs, nbrs, normals=nrm, cos_angle=float('nan'))
    with pytest.raises(ValueError, match='bad arguments'):
        ctx.smooth_votes(v, offs, nbrs, colors=col, max_color_dist=-1.0)
    with pytest.raises(ValueError, match='overlaps'):
        ctx.smooth_votes(v, offs, nbrs, out=v)
    dv, do, db = _dev(v, offs, nbrs)
    with pytest.raises(ValueError, match='overlaps'):
        ctx.smooth_votes_dev(dv.data_ptr(), f3d.VOTES_F64, n, 134, do.data_ptr(), db.data_ptr(), None, 0.0, None, f3d.F64, 0.0, 1.0, 1,
                             dv.data_ptr() + 8 * 134, torch.cuda.current_stream().cuda_stream)
    with pytest.raises(IndexError, match='filter class'):
        ctx.smooth_segment(v, offs, nbrs, 133, 0.5, [134])
    with pytest.raises(ValueError, match='empty sequence'):
        ctx.smooth_segment(v[:, :1].copy(), offs, nbrs, 133, 0.5, None, True)
    assert ctx.smooth_votes(np.zeros((0, 5)), np.zeros(1, np.int64), np.zeros(0, np.int32)).shape == (0, 5)      # n == 0: a no-op
    assert ctx.smooth_segment(np.zeros((0, 5)), np.zeros(1, np.int64), np.zeros(0, np.int32), 4).shape == (0,)


def test_strict_context_after_reserve():
    import torch
    n, (offs, nbrs), v, vi, nrm, _ = _row_scene()
    dv, di, do, db, dn = _dev(v, vi, offs, nbrs, nrm)
    out = torch.empty((n, 134), dtype=torch.float64, device='cuda')
    cls = torch.empty(n, dtype=torch.int64, device='cuda')
    st = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()

    def votes(ctx, it):
        ctx.smooth_votes_dev(dv.data_ptr(), f3d.VOTES_F64, n, 134, do.data_ptr(), db.data_ptr(), dn.data_ptr(), 0.4, None, f3d.F64, 0.0, 1.0, it,
                             out.data_ptr(), st)

    def segment(ctx, it):
        ctx.smooth_segment_dev(di.data_ptr(), f3d.VOTES_F64, n, 134, do.data_ptr(), db.data_ptr(), dn.data_ptr(), 0.4, None, f3d.F64, 0.0, 1.0, it,
                               133, 0.5, None, False, cls.data_ptr(), st)

    ctx = f3d.Context(0)
    ctx.reserve_smooth(n, 134, 4)
    ctx.set_strict(True)
    before = ctx.alloc_count
    for it in (1, 2, 3, 4):
        votes(ctx, it)
        segment(ctx, it)
        ctx.take_device_error(st)
        assert np.array_equal(_np(out), R.smooth(v, offs, nbrs, normals=nrm, cos_angle=0.4, iterations=it))
        assert np.array_equal(_np(cls), R.smooth_segment(vi, offs, nbrs, 133, 0.5, normals=nrm, cos_angle=0.4, iterations=it))
    assert ctx.alloc_count == before
    ctx.close()
    fresh = f3d.Context(0)                                                     # without a reserve: one iteration needs no scratch,
    fresh.set_strict(True)
    votes(fresh, 1)
    segment(fresh, 1)
    fresh.take_device_error(st)
    with pytest.raises(MemoryError, match='strict context'):                   # more do, and nothing is allocated silently
        votes(fresh, 2)
    with pytest.raises(MemoryError, match='strict context'):
        segment(fresh, 2)
    fresh.reserve_smooth(n, 134, 2)                                            # one matrix: enough for 2 iterations, not for segment's 3
    votes(fresh, 2)
    segment(fresh, 2)
    votes(fresh, 5)
    with pytest.raises(MemoryError, match='strict context'):
        segment(fresh, 3)
    fresh.take_device_error(st)
    fresh.close()


# ------------------------------------------------------------------------------------------------ a bad index
@pytest.mark.parametrize('bad', ['n', -1], ids=['index_n', 'index_minus_1'])
def test_index_error_writes_nothing_and_the_next_call_succeeds(bad):
    import torch
    n, (offs, nbrs), v, vi, _, _ = _row_scene()
    wrong = nbrs.copy()
    wrong[len(wrong) // 2] = n if bad == 'n' else -1
    ctx = _ctx()
    into = np.full((n, 134), -7.0)
    with pytest.raises(IndexError, match='neighbour index'):
        ctx.smooth_votes(v, offs, wrong, iterations=2, out=into)
    assert (into == -7).all()
    with pytest.raises(IndexError, match='neighbour index'):
        ctx.smooth_segment(vi, offs, wrong, 133)
    dv, do, dw = _dev(v, offs, wrong)
    with pytest.raises(IndexError, match='neighbour index'):
        V().smooth_votes(dv, (do, dw))
    with pytest.raises(IndexError, match='neighbour index'):
        V().smooth_segment(dv, (do, dw), 133)
    out = torch.full((n, 134), -7.0, dtype=torch.float64, device='cuda')       # the device entries: the outputs keep their sentinel
    cls = torch.full((n,), -7, dtype=torch.int64, device='cuda')
    st = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    for it in (1, 2, 3):
        ctx.smooth_votes_dev(dv.data_ptr(), f3d.VOTES_F64, n, 134, do.data_ptr(), dw.data_ptr(), None, 0.0, None, f3d.F64, 0.0, 1.0, it,
                             out.data_ptr(), st)
        ctx.smooth_segment_dev(dv.data_ptr(), f3d.VOTES_F64, n, 134, do.data_ptr(), dw.data_ptr(), None, 0.0, None, f3d.F64, 0.0, 1.0, it, 133, 0.5,
                               None, False, cls.data_ptr(), st)
    torch.cuda.synchronize()
    assert (out == -7).all() and (cls == -7).all()
    with pytest.raises(IndexError, match='neighbour index'):
        ctx.take_device_error(st)
    ctx.take_device_error(st)                                                  # taken: the next read is clean
    assert np.array_equal(ctx.smooth_votes(v, offs, nbrs), R.smooth(v, offs, nbrs))
    down = offs.copy()                                                         # offsets that do not ascend are caught by the same check
    down[200] = down[201] + 3
    with pytest.raises(IndexError, match='offsets'):
        ctx.smooth_votes(v, down, nbrs)
    assert np.array_equal(ctx.smooth_votes(v, offs, nbrs), R.smooth(v, offs, nbrs))


# ------------------------------------------------------------------------------------------------ end to end
def test_sheet_end_to_end_smoothing_leaves_the_two_instances():
    from Fusion3DSeg.segUtils.cv import split_into_instances
    pts, votes, truth = R.noisy_sheet()
    far = R.sheet_far(pts)
    ctx = _ctx()
    adj = ctx.radius_graph(pts, R.SHEET_R)
    lens = np.diff(adj[0])
    assert 15 <= np.median(lens) <= 25
    classes = V().smooth_segment(votes, adj, R.NCLASSES, 0.5)
    assert np.array_equal(classes, R.smooth_segment(votes, *adj, R.NCLASSES, 0.5))
    _, ids, info, _ = split_into_instances(classes, adj, R.NCLASSES, list(R.SHEET_CLASSES), 50)
    kept = [r for r in info if r['isthing'] and r['category_id'] != R.NCLASSES]
    assert sorted(r['category_id'] for r in kept) == list(R.SHEET_CLASSES)     # exactly the two instances of the truth
    for r in kept:
        members = ids == r['id']
        assert (truth[members & far] == r['category_id']).all() and members[far & (truth == r['category_id'])].all()
    bucket = ~np.isin(ids, [r['id'] for r in kept])
    assert not (bucket & far).any()                                            # nothing in the small-cluster bucket beyond r of the boundary
    raw = ctx.segment_votes(votes, R.NCLASSES, 0.5)                            # the same votes unsmoothed
    _, ids0, info0, _ = split_into_instances(raw, adj, R.NCLASSES, list(R.SHEET_CLASSES), 50)
    kept0 = [r['id'] for r in info0 if r['isthing'] and r['category_id'] != R.NCLASSES]
    assert (~np.isin(ids0, kept0) & far).sum() > 200                           # islands and unseen points punch holes everywhere
    roots, roots0 = ctx.components_same_class(classes, *adj), ctx.components_same_class(raw, *adj)
    assert len(np.unique(roots0)) > len(np.unique(roots)) + 50


def test_corner_end_to_end_gate_stops_the_leak():
    pts, normals, votes, surface = R.corner()
    adj = _ctx().radius_graph(pts, 0.05)
    plain = V().smooth_votes(votes, adj)
    gated = V().smooth_votes(votes, adj, normals=normals, angle=30.0)
    assert np.array_equal(plain, R.smooth(votes, *adj)) and np.array_equal(gated, R.smooth(votes, *adj, normals=normals, cos_angle=COS30))
    assert R.corner_leaks(plain, surface) > 0 and R.corner_leaks(gated, surface) == 0
    cls = V().smooth_segment(votes, adj, R.NCLASSES, 0.5, normals=normals, angle=30.0)
    assert np.array_equal(cls, np.where(surface == 0, *R.CORNER_CLASSES))
