"""extract_planes on the GPU (f3d_extract_planes, csrc/f3d_planes.hip) against the restatement tests/planes_ref.py, for host arrays and
for device tensors: exact labels and counts on scenes that pass the margin condition, plane parameters within derived bounds, quads by
their properties, relabelling invariance, reproducibility, index errors, a strict context, and the chain into refinement.py."""
import functools
import math

import numpy as np
import pytest

import f3d
import planes_ref as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
MODES = pytest.mark.parametrize('on_device', [False, True], ids=['host', 'device'])
X, Y, Z = np.eye(3)


def PU():
    from Fusion3DSeg.segUtils import planeUtils
    return planeUtils


def _np(x):
    return x.cpu().numpy() if hasattr(x, 'cpu') else np.asarray(x)


def _dev(*arrays):
    import torch
    return tuple(None if a is None else torch.as_tensor(np.array(a), device='cuda') for a in arrays)


# ------------------------------------------------------------------------------------------------ scenes
def _tilted(nx, ny, degrees, origin):
    """A sheet in the plane that holds the y axis and is turned `degrees` about it, starting at `origin`."""
    a = math.radians(degrees)
    return R.sheet(nx, ny, 0.02, origin, (math.cos(a), 0.0, -math.sin(a)), Y)


@functools.lru_cache(maxsize=None)
def _scene(name):
    """(points, normals, (offsets, neighbours), keyword arguments) of a named scene; built once and never written."""
    rng = np.random.default_rng(sum(map(ord, name)))
    kw, radius, quiet = {}, 0.05, dict(sigma_p=0.0003, sigma_n=0.005)
    if name == 'room' or name == 'room32':
        pts, nrm, _ = R.room_corner(np.random.default_rng(1))
        if name == 'room32':
            pts = pts.astype(np.float32)
    elif name.startswith('prefix'):                       # the first N points of the shuffled room, on a graph of their own
        m = int(name[6:])
        pts, nrm, _ = R.room_corner(np.random.default_rng(1))
        pts, nrm, radius, kw = pts[:m].copy(), nrm[:m].copy(), 0.1, dict(min_points=3)
    elif name == 'sheet70':                               # 4900 members: two chunks of the plane sums
        pts, nrm, _ = R.noisy(*R.sheet(70, 70, 0.02, (0, 0, 0), X, Y), rng)
    elif name in R.EDGE_SHEETS:                           # 4095, 4096, 4097 members: a last chunk of 4095, none, 1
        pts, nrm = R.edge_sheet(name)
    elif name == 'long':                                  # 3 : 1, so that the in-plane axes are well separated
        pts, nrm, _ = R.noisy(*R.sheet(60, 20, 0.02, (0, 0, 0), X, (0, 0.8, 0.6)), rng)
    elif name == 'min_exact':                             # components of exactly min_points and of min_points - 1 members
        a, b = R.sheet(10, 5, 0.02, (0, 0, 0), X, Y), R.sheet(7, 7, 0.02, (1, 0, 0), X, Y)
        pts, nrm, _ = R.noisy(np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]]), rng, **quiet)
    elif name in ('sheets_half', 'sheets_3'):             # two parallel sheets 0.5 x offset / 3 x offset apart, half a cell askew
        gap = 0.005 if name == 'sheets_half' else 0.03
        a, b = R.sheet(20, 20, 0.02, (0, 0, 0), X, Y), R.sheet(20, 20, 0.02, (0.01, 0.01, gap), X, Y)
        pts, nrm, _ = R.noisy(np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]]), rng, **quiet)
    elif name in ('fold5', 'fold15'):                     # two faces that meet along the y axis at 5 / 15 degrees
        a, b = R.sheet(15, 20, 0.02, (-0.29, 0, 0), X, Y), _tilted(15, 20, float(name[4:]), (0.01, 0, 0))
        pts, nrm, _ = R.noisy(np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]]), rng, **quiet)
    elif name == 'many':                                  # 130 sheets of 9 points, 20 cm apart: more than 64 and than 128 planes
        parts = [R.sheet(3, 3, 0.02, (0.2 * (k % 13), 0.2 * (k // 13), 0.01 * k), X, Y) for k in range(130)]
        pts, nrm, _ = R.noisy(np.concatenate([p for p, _ in parts]), np.concatenate([q for _, q in parts]), rng, **quiet)
        kw = dict(min_points=5)
    elif name == 'stripped':                              # a 12 x 60 sheet whose middle has no core point: several attach rounds
        pts, nrm = R.sheet(12, 60, 0.02, (0, 0, 0), X, Y)
        middle = (pts[:, 1] > 0.2) & (pts[:, 1] < 1.0)
        pts, nrm, perm = R.noisy(pts, nrm, rng, **quiet)
        nrm[middle[perm]] = np.nan
    elif name == 'nocore':                                # no point has a finite normal: no plane
        pts, nrm, _ = R.noisy(*R.sheet(12, 12, 0.02, (0, 0, 0), X, Y), rng)
        nrm[:] = np.nan
    elif name == 'gaps':                                  # rows without self entries; far points whose rows are empty
        a = R.sheet(12, 12, 0.02, (0, 0, 0), X, Y)
        far = np.stack([np.arange(9) + 5.0, np.zeros(9), np.zeros(9)], axis=1)
        pts, nrm, _ = R.noisy(np.concatenate([a[0], far]), np.concatenate([a[1], np.tile(Z, (9, 1))]), rng)
    else:
        raise KeyError(name)
    offs, nbrs = R.radius_csr(pts.astype(np.float64), radius)
    if name == 'gaps':
        rows = np.repeat(np.arange(len(pts)), np.diff(offs))
        keep = nbrs != rows
        offs = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=len(pts)))]).astype(np.int64)
        nbrs = nbrs[keep]
        assert (np.diff(offs) == 0).sum() == 9
    for a in (pts, nrm, offs, nbrs):
        a.setflags(write=False)
    return pts, nrm, (offs, nbrs), kw


@functools.lru_cache(maxsize=None)
def _want(name, with_normals=True, **kw):
    pts, nrm, (offs, nbrs), skw = _scene(name)
    return R.extract(pts, offs, nbrs, nrm if with_normals else None, **{**skw, **kw})


def _run(name, on_device, with_normals=True, **kw):
    """PlaneSet of planeUtils.extract_planes on a scene, as NumPy arrays (after checking where the results live)."""
    pts, nrm, (offs, nbrs), skw = _scene(name)
    nrm = nrm if with_normals else None
    if on_device:
        pts, nrm, offs, nbrs = _dev(pts, nrm, offs, nbrs)
    got = PU().extract_planes(pts, (offs, nbrs), nrm, **{**skw, **kw})
    assert all(bool(getattr(a, 'is_cuda', False)) == on_device for a in got)
    return PU().PlaneSet(*[_np(a) for a in got])


def _same_labels(got, want):
    assert want.margin >= 1e-6, want.margin                                       # the scene is fit for an exact comparison
    assert got.labels.dtype == np.int32 and got.counts.dtype == np.int64
    assert np.array_equal(got.counts, want.counts), (got.counts, want.counts)
    assert np.array_equal(got.labels, want.labels), int((got.labels != want.labels).sum())
    assert got.planes.shape == (want.counts[0], 8) and got.corners.shape == (want.counts[0], 4, 3)


# ------------------------------------------------------------------------------------------------ exact labels and counts
GIVEN = ['room', 'room32', 'prefix1', 'prefix2', 'prefix3', 'prefix63', 'prefix64', 'prefix65', 'prefix257', 'gaps', 'nocore', 'min_exact',
         'sheets_half', 'sheets_3', 'fold5', 'fold15', 'sheet70', 'many', 'stripped']


@MODES
@pytest.mark.parametrize('name', GIVEN)
def test_labels_and_counts_with_normals(name, on_device):
    _same_labels(_run(name, on_device), _want(name))


def test_the_scenes_are_what_they_are_meant_to_be():
    """The restatement's verdicts on the scenes, so that the cases above test what their names say."""
    assert _want('room').counts.tolist()[:2] == [4, 4] and _want('room32').counts[0] == 4
    assert _want('nocore').counts.tolist() == [0, 0, 1, 0] and _want('prefix1').counts[0] == 0 and _want('prefix257').counts[0] >= 1
    assert _want('gaps').counts[0] == 1 and (_want('gaps').labels == -1).sum() == 9
    assert np.bincount(_want('min_exact').labels + 1).tolist() == [49, 50]
    assert _want('sheets_half').counts[0] == 1 and _want('sheets_3').counts[0] == 2
    assert _want('fold5').counts[0] == 1 and _want('fold15').counts[0] == 2
    assert len(_want('sheet70').members[0]) == 4900
    assert [len(_want(name).members[0]) for name in R.EDGE_SHEETS] == [4095, 4096, 4097]
    assert _want('many').counts.tolist()[:2] == [130, 130]
    assert _want('stripped').counts[2] >= 4 and (_want('stripped').labels >= 0).all()


@MODES
@pytest.mark.parametrize('max_rounds', [0, 1, 64])
def test_attach_rounds(max_rounds, on_device):
    want = _want('stripped', max_rounds=max_rounds)
    _same_labels(_run('stripped', on_device, max_rounds=max_rounds), want)
    assert want.counts[2] == min(max_rounds, _want('stripped').counts[2])
    if max_rounds < 64:
        assert (want.labels < 0).any()


@MODES
def test_max_planes_smaller_than_the_qualifying_components(on_device):
    import torch
    pts, nrm, (offs, nbrs), kw = _scene('many')
    want = _want('many', max_planes=70)
    assert want.counts.tolist()[:2] == [70, 130] and want.margin >= 1e-6
    args = (math.cos(math.radians(10.0)), 0.01, 0.01, 0.01, kw['min_points'], 64, 70)
    ctx = f3d.default_context()
    if on_device:
        dp, dn, do, db = _dev(pts, nrm, offs, nbrs)
        labels = torch.empty(len(pts), dtype=torch.int32, device='cuda')
        planes, corners = torch.empty((70, 8), dtype=torch.float64, device='cuda'), torch.empty((70, 4, 3), dtype=torch.float64, device='cuda')
        counts = torch.empty(4, dtype=torch.int64, device='cuda')
        st = torch.cuda.current_stream().cuda_stream
        torch.cuda.synchronize()
        ctx.extract_planes_dev(dp.data_ptr(), f3d.F64, len(pts), do.data_ptr(), db.data_ptr(), dn.data_ptr(), *args, labels.data_ptr(),
                               planes.data_ptr(), corners.data_ptr(), counts.data_ptr(), None, st)
        ctx.take_device_error(st)
        labels, planes, counts = _np(labels), _np(planes), _np(counts)
    else:
        labels, planes, _, counts = ctx.extract_planes(pts, offs, nbrs, nrm, *args)
    assert np.array_equal(counts, want.counts) and np.array_equal(labels, want.labels)
    assert len(planes) == 70 and np.isfinite(planes).all()


PCA = GIVEN + ['long']                                   # every scene: one that misses the margin condition shows as a failure of it


@MODES
@pytest.mark.parametrize('name', PCA)
def test_labels_and_counts_without_normals(name, on_device):
    _same_labels(_run(name, on_device, with_normals=False), _want(name, with_normals=False))


def test_computed_normals_are_returned():
    pts, _, (offs, nbrs), _ = _scene('long')
    want = _want('long', with_normals=False)
    out = f3d.default_context().extract_planes(pts, offs, nbrs, None, math.cos(math.radians(10.0)), 0.01, 0.01, 0.01, 50, 64, len(pts) // 50,
                                               want_normals=True)
    assert np.array_equal(out[0], want.labels)
    cosang = np.abs(np.einsum('ij,ij->i', out[4], want.normals))
    assert (cosang[want.core] > 1 - 1e-12).all() and np.array_equal(np.linalg.norm(out[4], axis=1) > 0.5, np.linalg.norm(want.normals, axis=1) > 0.5)


# ------------------------------------------------------------------------------------------------ plane parameters
def _angle(a, b):
    return math.atan2(np.linalg.norm(np.cross(a, b)), abs(float(a @ b)))


@MODES
@pytest.mark.parametrize('name,with_normals', [('room', True), ('room', False), ('sheet70', True), ('long', True), ('long', False), ('fold15', True)] +
                         [(name, True) for name in R.EDGE_SHEETS])
def test_plane_parameters(name, with_normals, on_device):
    pts = _scene(name)[0].astype(np.float64)
    want = _want(name, with_normals)
    got = _run(name, on_device, with_normals)
    _same_labels(got, want)
    for k in range(want.counts[0]):
        members = want.members[k]
        m = len(members)
        for a in range(3):                                                        # centroid: any-order float64 sum against fsum
            x = pts[members, a]
            exact = math.fsum(x.tolist())
            gamma = (m - 1) * U / (1 - (m - 1) * U)
            tol = gamma * math.fsum(np.abs(x).tolist()) / m * (1 + U) + 2 * U * abs(exact) / m + 5e-324
            assert abs(got.planes[k, 4 + a] - exact / m) <= tol, (k, a)
        lam0, lam1, lam2 = want.lam[k]
        bound = 64 * m * U * lam2 / (lam1 - lam0)
        assert _angle(got.planes[k, :3], want.planes[k, :3]) <= bound, (k, _angle(got.planes[k, :3], want.planes[k, :3]), bound)
        assert abs(np.linalg.norm(got.planes[k, :3]) - 1) <= 16 * U
        n = got.planes[k, :3]
        if with_normals:                                                          # towards the root's normal
            assert R.dot3(n, _scene(name)[1][members[0]]) >= 0
        else:                                                                     # the largest component is positive
            assert n[np.argmax(np.abs(n))] > 0
        u = got.corners[k, 1] - got.corners[k, 0]
        assert u[np.argmax(np.abs(u))] > 0
        assert abs(got.planes[k, 3] + R.dot3(n, got.planes[k, 4:7])) <= 4 * U * np.abs(got.planes[k, 4:7]).sum()
        final = pts[got.labels == k]
        res = (final - got.planes[k, 4:7]) @ n
        rms = math.sqrt(math.fsum((res * res).tolist()) / len(final))               # a sum of squares, and residuals good to 4 u |p - c|
        assert abs(got.planes[k, 7] - rms) <= (len(final) + 4) * U * rms + 8 * U * np.abs(final - got.planes[k, 4:7]).max()


# ------------------------------------------------------------------------------------------------ quads
@MODES
@pytest.mark.parametrize('name', ['room', 'long', 'many', 'fold15'])
def test_quads_by_their_properties(name, on_device):
    pts = _scene(name)[0].astype(np.float64)
    got = _run(name, on_device)
    assert len(got.planes) == _want(name).counts[0] > 0
    for k in range(len(got.planes)):
        n, c, q = got.planes[k, :3], got.planes[k, 4:7], got.corners[k]
        side_u, side_v = q[1] - q[0], q[3] - q[0]
        eu, ev = np.linalg.norm(side_u), np.linalg.norm(side_v)
        scale = np.abs(q).max() + eu + ev
        assert np.abs((q - c) @ n).max() <= 1e-12 * scale                          # the corners lie in the plane
        assert np.abs((q[0] + q[2]) - (q[1] + q[3])).max() <= 1e-12 * scale         # a parallelogram ...
        assert abs(side_u @ side_v) <= 1e-12 * scale * scale                        # ... with a right angle
        u, v = side_u / eu, side_v / ev
        a, b = (pts[got.labels == k] - q[0]) @ u, (pts[got.labels == k] - q[0]) @ v
        assert a.min() >= -1e-9 * eu and a.max() <= eu * (1 + 1e-9) and b.min() >= -1e-9 * ev and b.max() <= ev * (1 + 1e-9)
        assert abs(a.min()) <= 1e-9 * eu and abs(a.max() - eu) <= 1e-9 * eu         # every side is touched by a member
        assert abs(b.min()) <= 1e-9 * ev and abs(b.max() - ev) <= 1e-9 * ev


@MODES
def test_quad_of_an_elongated_sheet_equals_the_restatement(on_device):
    """On a 3 : 1 sheet lambda2 / (lambda2 - lambda1) is about 9 / 8, so the in-plane axes are determined to the bound the normal has
    (test_plane_parameters) and the corners, at most a diagonal from the centroid, to that angle times the diagonal."""
    want = _want('long')
    got = _run('long', on_device)
    _same_labels(got, want)
    m = len(want.members[0])
    lam0, lam1, lam2 = want.lam[0]
    angle = 64 * m * U * lam2 / min(lam1 - lam0, lam2 - lam1)
    diagonal = np.linalg.norm(want.corners[0, 2] - want.corners[0, 0])
    assert np.abs(got.corners - want.corners).max() <= angle * diagonal + 64 * U * np.abs(want.corners).max()
    sides = np.linalg.norm(got.corners[0, 1] - got.corners[0, 0]), np.linalg.norm(got.corners[0, 3] - got.corners[0, 0])
    assert 2.5 < sides[0] / sides[1] < 3.5                                         # corner 1 follows corner 0 along the long axis


# ------------------------------------------------------------------------------------------------ invariance, reproducibility
@MODES
def test_relabelling_invariance(on_device):
    pts, nrm, _, _ = _scene('room')
    perm = np.random.default_rng(5).permutation(len(pts))
    p2, n2 = np.ascontiguousarray(pts[perm]), np.ascontiguousarray(nrm[perm])
    offs, nbrs = R.radius_csr(p2, 0.05)
    assert R.extract(p2, offs, nbrs, n2).margin >= 1e-6
    base = _run('room', on_device)
    args = _dev(p2, offs, nbrs, n2) if on_device else (p2, offs, nbrs, n2)
    got = PU().extract_planes(args[0], (args[1], args[2]), args[3])
    labels = _np(got.labels)
    assert R.same_partition(labels, base.labels[perm])
    first = [int(np.flatnonzero(labels == k)[0]) for k in range(int(_np(got.counts)[0]))]
    assert first == sorted(first) and len(first) == 4                             # numbered by the new lowest indices


@MODES
@pytest.mark.parametrize('name,with_normals', [('room', True), ('room', False), ('stripped', True), ('sheet70', True)])
def test_two_calls_return_identical_bits(name, with_normals, on_device):
    a, b = _run(name, on_device, with_normals), _run(name, on_device, with_normals)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


# ------------------------------------------------------------------------------------------------ errors, strict context
@pytest.mark.parametrize('bad', ['n', -1], ids=['index_n', 'index_minus_1'])
def test_index_error_writes_nothing_and_the_next_call_succeeds(bad):
    import torch
    pts, nrm, (offs, nbrs), _ = _scene('room')
    wrong = nbrs.copy()
    wrong[len(wrong) // 2] = len(pts) if bad == 'n' else -1
    with pytest.raises(IndexError, match='neighbour index'):
        PU().extract_planes(pts, (offs, wrong), nrm)
    dp, dn, do, dw = _dev(pts, nrm, offs, wrong)
    with pytest.raises(IndexError, match='neighbour index'):
        PU().extract_planes(dp, (do, dw), dn)
    with pytest.raises(IndexError, match='neighbour index'):
        PU().extract_planes(dp, (do, dw), None)
    # the device entry itself: the outputs keep their sentinel, the sticky bit is taken once
    ctx = f3d.default_context()
    labels = torch.full((len(pts),), -7, dtype=torch.int32, device='cuda')
    planes = torch.full((72, 8), -7.0, dtype=torch.float64, device='cuda')
    corners = torch.full((72, 4, 3), -7.0, dtype=torch.float64, device='cuda')
    counts = torch.full((4,), -7, dtype=torch.int64, device='cuda')
    st = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    ctx.extract_planes_dev(dp.data_ptr(), f3d.F64, len(pts), do.data_ptr(), dw.data_ptr(), dn.data_ptr(), math.cos(math.radians(10.0)), 0.01,
                           0.01, 0.01, 50, 64, 72, labels.data_ptr(), planes.data_ptr(), corners.data_ptr(), counts.data_ptr(), None, st)
    torch.cuda.synchronize()
    assert (labels == -7).all() and (planes == -7).all() and (corners == -7).all() and (counts == -7).all()
    with pytest.raises(IndexError, match='neighbour index'):
        ctx.take_device_error(st)
    ctx.take_device_error(st)                                                   # taken: the next read is clean
    _same_labels(_run('room', False), _want('room'))
    _same_labels(_run('room', True), _want('room'))


def test_c_entry_argument_errors():
    pts, nrm, (offs, nbrs), _ = _scene('prefix65')
    ctx = f3d.default_context()
    for min_points, max_rounds, max_planes in [(2, 64, 10), (3, -1, 10), (3, 64, -1)]:
        with pytest.raises(ValueError, match='extract_planes'):
            ctx.extract_planes(pts, offs, nbrs, nrm, 0.98, 0.01, 0.01, 0.01, min_points, max_rounds, max_planes)
    labels, planes, corners, counts = ctx.extract_planes(pts[:0], offs[:1], nbrs[:0], None, 0.98, 0.01, 0.01, 0.01, 3, 64, 4)
    assert len(labels) == 0 and len(planes) == 0 and counts.tolist() == [0, 0, 0, 0]


def test_strict_context_after_reserve():
    import torch
    pts, nrm, (offs, nbrs), _ = _scene('room')
    n, mp = len(pts), len(pts) // 50
    want = _want('room')
    ctx = f3d.Context(0)
    ctx.reserve_planes(n)
    dp, dn, do, db = _dev(pts, nrm, offs, nbrs)
    labels = torch.empty(n, dtype=torch.int32, device='cuda')
    planes, corners = torch.empty((mp, 8), dtype=torch.float64, device='cuda'), torch.empty((mp, 4, 3), dtype=torch.float64, device='cuda')
    counts = torch.empty(4, dtype=torch.int64, device='cuda')
    st = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    ctx.set_strict(True)
    before = ctx.alloc_count
    args = (math.cos(math.radians(10.0)), 0.01, 0.01, 0.01, 50, 64, mp, labels.data_ptr(), planes.data_ptr(), corners.data_ptr(), counts.data_ptr())
    ctx.extract_planes_dev(dp.data_ptr(), f3d.F64, n, do.data_ptr(), db.data_ptr(), dn.data_ptr(), *args, None, st)
    ctx.extract_planes_dev(dp.data_ptr(), f3d.F64, n, do.data_ptr(), db.data_ptr(), None, *args, None, st)
    ctx.extract_planes_dev(dp.data_ptr(), f3d.F64, n, do.data_ptr(), db.data_ptr(), dn.data_ptr(), *args, None, st)
    ctx.take_device_error(st)
    assert ctx.alloc_count == before
    assert np.array_equal(_np(labels), want.labels) and np.array_equal(_np(counts), want.counts)
    ctx.close()
    small = f3d.Context(0)                                                      # a larger cloud than reserved: no silent allocation
    small.reserve_planes(16)
    small.set_strict(True)
    with pytest.raises(MemoryError, match='strict context'):
        small.extract_planes_dev(dp.data_ptr(), f3d.F64, n, do.data_ptr(), db.data_ptr(), dn.data_ptr(), *args, None, st)
    small.close()
    fresh = f3d.Context(0)                                                      # and without any reserve
    fresh.set_strict(True)
    with pytest.raises(MemoryError, match='strict context'):
        fresh.extract_planes_dev(dp.data_ptr(), f3d.F64, n, do.data_ptr(), db.data_ptr(), dn.data_ptr(), *args, None, st)
    fresh.close()


def test_strict_context_reserved_for_a_larger_cloud():
    """A reserve for N points serves every n <= N: the scratch layout of the smaller call, the sort's temporary storage included,
    lies inside the reserved buffer."""
    import torch
    ctx = f3d.Context(0)
    ctx.reserve_planes(5000)
    ctx.set_strict(True)
    before = ctx.alloc_count
    st = torch.cuda.current_stream().cuda_stream
    for name in ('sheet70', 'room', 'many', 'prefix257', 'prefix65', 'prefix1'):
        pts, nrm, (offs, nbrs), kw = _scene(name)
        n, min_points = len(pts), kw.get('min_points', 50)
        mp = n // min_points
        for with_normals in (True, False):
            want = _want(name, with_normals)
            dp, dn, do, db = _dev(pts, nrm if with_normals else None, offs, nbrs)
            labels = torch.empty(n, dtype=torch.int32, device='cuda')
            planes, corners = torch.empty((mp, 8), dtype=torch.float64, device='cuda'), torch.empty((mp, 4, 3), dtype=torch.float64, device='cuda')
            counts = torch.empty(4, dtype=torch.int64, device='cuda')
            torch.cuda.synchronize()
            ctx.extract_planes_dev(dp.data_ptr(), f3d.dtype_code(pts), n, do.data_ptr(), db.data_ptr(), None if dn is None else dn.data_ptr(),
                                   math.cos(math.radians(10.0)), 0.01, 0.01, 0.01, min_points, 64, mp, labels.data_ptr(), planes.data_ptr(),
                                   corners.data_ptr(), counts.data_ptr(), None, st)
            ctx.take_device_error(st)
            assert want.margin >= 1e-6
            assert np.array_equal(_np(labels), want.labels) and np.array_equal(_np(counts), want.counts), (name, with_normals)
    assert ctx.alloc_count == before
    ctx.close()


# ------------------------------------------------------------------------------------------------ end to end
def test_chain_into_depth_floodfill_point():
    """radius_graph -> extract_planes -> plane_table -> refinement.depth_floodfill_point on a wall with a panel set 4 cm into it: the
    flood from one picked panel point returns the panel."""
    from Fusion3DSeg.segUtils import refinement
    rng = np.random.default_rng(11)
    wall, _ = R.sheet(40, 40, 0.02, (0, 0, 0), X, Y)
    inset = (np.abs(wall[:, 0] - 0.39) < 0.1) & (np.abs(wall[:, 1] - 0.39) < 0.1)
    wall[inset, 2] -= 0.04
    pts = wall + 0.0005 * rng.standard_normal(wall.shape)
    nrm = np.tile(Z, (len(pts), 1))
    assert not inset[0] and inset.sum() == 100
    ctx = f3d.default_context()
    adj = ctx.radius_graph(pts, 0.05)
    planes = PU().extract_planes(pts, adj, nrm)
    assert planes.counts.tolist()[:2] == [2, 2] and np.array_equal(planes.labels == 1, inset)
    table, bounding = PU().plane_table(planes)
    vertex = np.hstack([pts, np.full((len(pts), 3), 0.5)])
    pick = int(np.flatnonzero(inset)[37])
    ids = np.zeros(len(pts), np.int64)
    ids[pick] = 7
    colors = np.zeros((len(pts), 3))
    colors[pick] = (1.0, 0.0, 0.0)
    out_ids, seg = refinement.depth_floodfill_point(table, vertex, [pts[0]], bounding, adj, None, depth_threshold=0.03, selected_point=[pick],
                                                    instance_id=ids, seg_colors=colors)
    assert np.array_equal(out_ids == 7, inset)
    assert np.array_equal((np.asarray(seg.colors) == (1.0, 0.0, 0.0)).all(axis=1), inset)
