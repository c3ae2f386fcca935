"""meshUtils on the GPU (f3d_mesh_*): bit-exact against the reference golden and, at the sizes where the kernels change path,
against the restatement tests/mesh_ref.py, for host arrays and for device tensors; reproducibility; clean_mesh against the
composition; index errors; a strict context."""
import functools

import numpy as np
import pytest

import f3d
import mesh_ref as R
from planes_ref import shaped_sum

pytestmark = pytest.mark.gpu

SCENES = ['some', 'none', 'all', 'odd', 'empty', 'corners']


def MU():
    from Fusion3DSeg.segUtils import meshUtils
    return meshUtils


def _np(x):
    return x.cpu().numpy() if hasattr(x, 'cpu') else x


def _dev(*arrays):
    import torch
    return tuple(torch.as_tensor(a, device='cuda') for a in arrays)


def _same(got, want):
    got = _np(got)
    assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), (got.dtype, got.shape, want.dtype, want.shape)


# ------------------------------------------------------------------------------------------------ golden scenes
@pytest.mark.parametrize('on_device', [False, True], ids=['host', 'device'])
@pytest.mark.parametrize('s', SCENES)
def test_bit_identical_to_reference_golden(golden, s, on_device):
    g = golden('mesh')
    verts, tris, mask = g[f'{s}_vertices'], g[f'{s}_triangles'], g[f'{s}_mask']
    before = tris.copy()
    a = _dev(verts, tris, mask) if on_device else (verts, tris, mask)
    vmap = MU().vertex_triangle_mapping(a[1], len(verts))
    offsets, tri, pos = vmap.csr
    _same(offsets, g[f'{s}_offsets']); _same(tri, g[f'{s}_tov'].astype(np.int32)); _same(pos, g[f'{s}_pov'].astype(np.int8))
    tov, pov = vmap
    assert tov == R.lists_of(g[f'{s}_offsets'], g[f'{s}_tov']) and pov == R.lists_of(g[f'{s}_offsets'], g[f'{s}_pov'])
    nr, rem, o2n = MU().remove_faces_by_vertices(len(verts), a[1], a[2])
    _same(nr, g[f'{s}_not_removed']); _same(rem, g[f'{s}_remaining']); _same(o2n, g[f'{s}_old2new'])
    kv, kt = MU().keep_faces_by_vertices(a[0], a[1], a[2])
    _same(kv, g[f'{s}_kept_vertices']); _same(kt, g[f'{s}_kept_triangles'])
    assert np.array_equal(_np(a[1]), before)                                   # the caller's triangles are left as they were
    if on_device:
        assert all(x.is_cuda for x in (offsets, tri, pos, nr, rem, o2n, kv, kt))


# ------------------------------------------------------------------------------------------------ shapes against the restatement
@functools.lru_cache(maxsize=None)
def _mesh(name):
    """(vertices, triangles, mask) of a named test mesh; built once."""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name.startswith('m'):                              # the first M faces of a shuffled 24 x 24 grid: clusters of many sizes
        m = int(name[1:])
        verts, tris = R.grid_mesh(24, 24, rng)
        tris = tris[rng.permutation(len(tris))][:m]
        return verts, tris, rng.random(len(verts)) < 0.1
    if name == 'grid':                                    # ~80k triangles, 40k vertices, shuffled, 5 % of the vertices masked
        verts, tris = R.grid_mesh(200, 200, rng)
        return verts, tris[rng.permutation(len(tris))], rng.random(len(verts)) < 0.05
    if name == 'grid32':                                  # the same in float32 / int32
        verts, tris, mask = _mesh('grid')
        return verts.astype(np.float32), tris.astype(np.int32), mask
    if name == 'strip':                                   # one cluster, a union chain across every block
        verts, tris = R.strip_mesh(70000, rng)
        return verts, tris, rng.random(len(verts)) < 0.001
    if name.startswith('strip'):                          # one cluster of exactly M triangles: the chunks of its area sum end at M
        verts, tris = R.strip_mesh(int(name[5:]), rng)
        return verts, tris, rng.random(len(verts)) < 0.001
    if name == 'two_strips':                              # clusters of 4096 and 4097 that share no vertex: the second one's first
        va, ta = R.strip_mesh(4096, rng)                  # chunk starts right behind the first one's only, full chunk
        vb, tb = R.strip_mesh(4097, rng)
        verts = np.concatenate([va, vb + (0.0, 5.0, 0.0)])
        return verts, np.concatenate([ta, tb + len(va)]), rng.random(len(verts)) < 0.001
    verts = rng.uniform(-1, 1, (12, 3))
    if name == 'fans':                                    # two fans that meet at vertex 0 only
        return verts, np.array(R.fan(0, [1, 2, 3, 4]) + R.fan(0, [5, 6, 7]), np.int64), np.arange(12) == 6
    if name == 'edge3':                                   # three triangles on the edge (0, 1)
        return verts, np.array([[0, 1, 2], [1, 0, 3], [4, 0, 1]], np.int64), np.arange(12) == 4
    if name == 'dups':                                    # duplicated faces and a (v, v, w) face
        return verts, np.array([[0, 1, 2], [5, 5, 6], [0, 1, 2], [2, 1, 0], [6, 7, 8], [9, 10, 11], [6, 5, 5]], np.int32), np.arange(12) == 9
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _want(name):
    """The restatement's results for a named mesh; computed once, shared, never modified."""
    verts, tris, mask = _mesh(name)
    out = {'vmap': R.vertex_map(tris, len(verts)), 'remove': R.remove_faces(len(verts), tris, mask), 'keep': R.keep_faces(verts, tris, mask),
           'clusters': R.clusters(verts, tris)}
    for group in out.values():
        for a in group:
            a.setflags(write=False)
    return out


def _check_clusters(got, want):
    cl, n, ca, ta = got
    wcl, wn, wca, wta = want
    _same(cl, wcl); _same(n, wn); _same(ta, wta)
    ca = _np(ca)
    assert ca.dtype == np.float64 and ca.shape == wca.shape
    err, bound = np.abs(ca - wca), R.area_bound(wn, wca)
    worst = int(np.argmax(err - bound)) if len(err) else -1
    assert np.all(err <= bound), (worst, ca[worst], wca[worst], int(wn[worst]))


def _run_all(verts, tris, mask):
    mu = MU()
    return (mu.vertex_triangle_mapping(tris, len(verts)).csr, mu.remove_faces_by_vertices(len(verts), tris, mask),
            mu.keep_faces_by_vertices(verts, tris, mask), mu.get_triangle_clusters((verts, tris), True))


CHUNK_EDGES = ['strip4095', 'strip4096', 'strip4097', 'strip8193', 'two_strips']        # around the 4096 members of a chunk
NAMES = ['m1', 'm2', 'm255', 'm256', 'm257', 'm1025', 'grid', 'grid32', 'strip', 'fans', 'edge3', 'dups'] + CHUNK_EDGES


@pytest.mark.parametrize('name', NAMES)
def test_matches_restatement_and_repeats(name):
    verts, tris, mask = _mesh(name)
    want = _want(name)
    first = _run_all(verts, tris, mask)
    for got, w in zip(first[0], want['vmap']):
        _same(got, w)
    for got, w in zip(first[1], want['remove']):
        _same(got, w)
    for got, w in zip(first[2], want['keep']):
        _same(got, w)
    _check_clusters(first[3], want['clusters'])
    second = _run_all(verts, tris, mask)                                        # two calls: identical bits, areas included
    for a, b in zip(first, second):
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()


@pytest.mark.parametrize('on_device', [False, True], ids=['host', 'device'])
@pytest.mark.parametrize('name', CHUNK_EDGES)
def test_cluster_sums_at_chunk_edges(name, on_device):
    """Clusters, sizes and triangle areas equal the restatement's bit for bit.  The restatement's cluster area is an fsum, which
    the library's sum is only close to (_check_clusters); its bits are those of the contract's shaped sum (chunks of 4096 members in
    ascending triangle index, planes_ref.shaped_sum) of the restatement's triangle areas."""
    verts, tris, _ = _mesh(name)
    wcl, wn, _, wta = _want(name)['clusters']
    assert wn.tolist() == ([4096, 4097] if name == 'two_strips' else [int(name[5:])])
    got = MU().get_triangle_clusters(_dev(verts, tris) if on_device else (verts, tris), True)
    assert all(bool(getattr(a, 'is_cuda', False)) == on_device for a in got)
    _check_clusters(got, _want(name)['clusters'])
    shaped = np.array([shaped_sum(wta[wcl == c]) for c in range(len(wn))])
    assert _np(got[2]).tobytes() == shaped.tobytes(), (_np(got[2]), shaped)


def test_known_cluster_counts():
    assert _want('fans')['clusters'][1].tolist() == [3, 2]
    assert _want('edge3')['clusters'][1].tolist() == [3]
    assert len(_want('strip')['clusters'][1]) == 1 and len(_want('grid')['clusters'][1]) == 1
    mu = MU()
    assert mu.get_triangle_clusters(_mesh('fans')[:2])[1].tolist() == [3, 2]
    assert mu.get_triangle_clusters(_mesh('edge3')[:2])[1].tolist() == [3]
    assert mu.get_triangle_clusters(_mesh('strip')[:2])[1].tolist() == [70000]


@pytest.mark.parametrize('name', ['m257', 'grid', 'grid32', 'dups'])
def test_device_tensors_equal_host_route(name):
    verts, tris, mask = _mesh(name)
    host = _run_all(verts, tris, mask)
    dev = _run_all(*_dev(verts, tris, mask))
    for a, b in zip(host, dev):
        for x, y in zip(a, b):
            assert y.is_cuda
            _same(y, x)


def test_triangle_mesh_object_and_masked_grid_clusters():
    """get_triangle_clusters takes get3DSeg's TriangleMesh; on the grid with 5 % of the vertices removed: one large cluster and
    a dozen fragments of 1 to 6 triangles."""
    from get3DSeg import TriangleMesh
    verts, tris, mask = _mesh('grid')
    _, t1, _ = R.remove_faces(len(verts), tris, mask)
    v1 = verts[~mask]
    want = R.clusters(v1, t1.astype(np.int32))
    assert len(want[1]) > 5 and want[1].max() > 100 * want[1].min()
    got = MU().get_triangle_clusters(TriangleMesh(v1, t1), True)
    _check_clusters(got, want)


# ------------------------------------------------------------------------------------------------ clean_mesh
@pytest.mark.parametrize('name', ['grid', 'grid32'])
def test_clean_mesh_equals_composition(name):
    mu = MU()
    verts, tris, mask = _mesh(name)
    want = R.ref_clean(verts, tris, mask, 50, 0.0)
    assert 0 < want[3].sum() < (~mask[tris].any(axis=1)).sum()                  # min_triangles = 50 drops some clusters, not all
    got = mu.clean_mesh(verts, tris, mask, 50)
    for g_, w in zip(got, want):
        _same(g_, w)
    referenced = np.zeros(len(verts), bool)
    referenced[tris[got[3]].reshape(-1)] = True
    assert np.array_equal(got[2], referenced)                                   # kept_vertex_mask = exactly the referenced vertices
    assert np.array_equal(got[0], verts[got[2]])
    # bit for bit the composition of the public functions, with an area threshold that bites as well
    areas = mu.get_triangle_clusters((verts[~mask], mu.remove_faces_by_vertices(len(verts), tris, mask)[1]))[2]
    min_area = float(np.median(areas))
    comp = R.clean_by_composition(mu.remove_faces_by_vertices, mu.get_triangle_clusters, verts, tris, mask, 2, min_area)
    got2 = mu.clean_mesh(verts, tris, mask, 2, min_area)
    assert 0 < comp[3].sum() < (~mask[tris].any(axis=1)).sum()                  # the area threshold drops some clusters, not all
    for g_, w in zip(got2, comp):
        _same(g_, w)
    dev = mu.clean_mesh(*_dev(verts, tris, mask), 50)                           # device tensors in, device tensors out
    for d, h in zip(dev, got):
        assert d.is_cuda
        _same(d, h)
    nomask = mu.clean_mesh(verts, tris)                                         # the defaults keep the whole (connected) grid
    _same(nomask[1], tris); _same(nomask[0], verts)
    assert nomask[2].all() and nomask[3].all()


# ------------------------------------------------------------------------------------------------ errors, strict context
@pytest.mark.parametrize('bad', [12, -1], ids=['index_V', 'index_minus_1'])
def test_index_error_writes_nothing_and_the_next_call_succeeds(bad):
    import torch
    mu = MU()
    verts, tris, mask = _mesh('dups')
    wrong = tris.copy()
    wrong[4, 1] = bad
    for fn in (lambda t, v, m: mu.vertex_triangle_mapping(t, len(v)), lambda t, v, m: mu.remove_faces_by_vertices(len(v), t, m),
               lambda t, v, m: mu.keep_faces_by_vertices(v, t, m), lambda t, v, m: mu.get_triangle_clusters((v, t)),
               lambda t, v, m: mu.clean_mesh(v, t, m)):
        with pytest.raises(IndexError):
            fn(wrong, verts, mask)
        with pytest.raises(IndexError):
            fn(*_dev(wrong), *_dev(verts, mask))
    # the device entry itself: the outputs keep their sentinel, counts[2] is set, the sticky bit is taken once
    ctx = f3d.default_context()
    dt, dm = _dev(wrong, mask)
    nr = torch.full((len(tris),), 7, dtype=torch.uint8, device='cuda')
    rem = torch.full((len(tris), 3), -5, dtype=torch.int32, device='cuda')
    o2n = torch.full((12,), -5, dtype=torch.int64, device='cuda')
    counts = torch.full((4,), -5, dtype=torch.int64, device='cuda')
    st = torch.cuda.current_stream().cuda_stream
    ctx.mesh_remove_faces_dev(dt.data_ptr(), f3d.I32, len(tris), 12, dm.data_ptr(), nr.data_ptr(), rem.data_ptr(), o2n.data_ptr(), counts.data_ptr(), st)
    torch.cuda.synchronize()
    assert counts.tolist() == [0, 0, 1, 0]
    assert (nr == 7).all() and (rem == -5).all() and (o2n == -5).all()
    with pytest.raises(IndexError, match='vertex index'):
        ctx.take_device_error(st)
    ctx.take_device_error(st)                                                   # taken: the next read is clean
    want = _want('dups')
    for got, w in zip(_run_all(verts, tris, mask)[1], want['remove']):
        _same(got, w)


def test_strict_context_after_reserve():
    import torch
    verts, tris, mask = _mesh('grid')
    nv, nt = len(verts), len(tris)
    ctx = f3d.Context(0)
    ctx.reserve_mesh(nv, nt)
    dv, dt, dm = _dev(verts, tris, mask)
    new_v = torch.empty((nv, 3), dtype=torch.float64, device='cuda')
    new_t = torch.empty((nt, 3), dtype=torch.int64, device='cuda')
    kv, kt = torch.zeros(nv, dtype=torch.bool, device='cuda'), torch.zeros(nt, dtype=torch.bool, device='cuda')
    offsets = torch.empty(nv + 1, dtype=torch.int64, device='cuda')
    tri, pos = torch.empty(3 * nt, dtype=torch.int32, device='cuda'), torch.empty(3 * nt, dtype=torch.int8, device='cuda')
    counts = torch.empty(4, dtype=torch.int64, device='cuda')
    st = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    ctx.set_strict(True)
    before = ctx.alloc_count
    ctx.mesh_vertex_map_dev(dt.data_ptr(), f3d.I64, nt, nv, offsets.data_ptr(), tri.data_ptr(), pos.data_ptr(), counts.data_ptr(), st)
    ctx.mesh_clean_dev(dv.data_ptr(), f3d.F64, nv, dt.data_ptr(), f3d.I64, nt, dm.data_ptr(), 50, 0.0, new_v.data_ptr(), new_t.data_ptr(),
                       kv.data_ptr(), kt.data_ptr(), counts.data_ptr(), st)
    ctx.take_device_error(st)
    assert ctx.alloc_count == before
    q, p = int(counts[0]), int(counts[1])
    want = R.ref_clean(verts, tris, mask, 50, 0.0)
    _same(new_v[:p], want[0]); _same(new_t[:q], want[1]); _same(kv, want[2]); _same(kt, want[3])
    for got, w in zip((offsets, tri, pos), _want('grid')['vmap']):
        _same(got, w)
    ctx.close()
    small = f3d.Context(0)                                                      # a larger mesh than reserved: no silent allocation
    small.reserve_mesh(16, 16)
    small.set_strict(True)
    with pytest.raises(MemoryError, match='strict context'):
        small.mesh_vertex_map_dev(dt.data_ptr(), f3d.I64, nt, nv, offsets.data_ptr(), tri.data_ptr(), pos.data_ptr(), counts.data_ptr(), st)
    small.close()
