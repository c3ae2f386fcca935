"""f3d.tensors on the GPU: the stream a ``*_dev`` call is handed (never the null handle, ordered both ways with the caller's
stream, also past an exception), the device CSR check, and PointCorrespondance on tensors from torch's default stream."""
import numpy as np
import pytest

import f3d
from f3d import tensors as T

pytestmark = pytest.mark.gpu

N = 4096
PP, NR = np.array([0.25, -0.5, 0.125]), np.array([0.6, -0.8, 0.3])


def _device():
    import torch
    ctx = f3d.default_context()
    return torch, ctx, torch.device('cuda', ctx.device)


def _points(torch, dev):
    """float64 [N, 3] made by kernels enqueued on the current stream just now: arange -> float64 -> arithmetic"""
    return (torch.arange(3 * N, device=dev).to(torch.float64) * 0.001 - 1.5).reshape(N, 3)


def _want(pts):
    """the kernel's expression in its operation order (built without FMA contraction): |((dx nx + dy ny) + dz nz)|"""
    p = pts.cpu().numpy()
    return np.abs(((p[:, 0] - PP[0]) * NR[0] + (p[:, 1] - PP[1]) * NR[1]) + (p[:, 2] - PP[2]) * NR[2])


def test_null_current_stream_gets_a_side_stream_ordered_both_ways():
    torch, ctx, dev = _device()
    assert torch.cuda.current_stream(dev).cuda_stream == 0
    pts = _points(torch, dev)
    out = torch.zeros(N, dtype=torch.float64, device=dev)
    with T.work_stream(dev) as work:
        assert work.cuda_stream != 0
        assert torch.cuda.current_stream(dev).cuda_stream == work.cuda_stream
        ctx.plane_distance_dev(pts.data_ptr(), N, PP, NR, out.data_ptr(), work.cuda_stream)
    assert torch.cuda.current_stream(dev).cuda_stream == 0
    got = out.cpu().numpy()                                              # a copy on the null stream, no synchronize before it
    assert np.array_equal(got, _want(pts)) and got.max() > 0.7           # not the zeros `out` held: point 0 lies 0.7377 off the plane


def test_non_null_current_stream_is_used_as_it_is(monkeypatch):
    torch, ctx, dev = _device()
    side, stream_type = torch.cuda.Stream(dev), torch.cuda.Stream

    def no_new_stream(*a, **k):
        if 'stream_id' not in k:                                         # (torch wraps an existing handle with stream_id=)
            raise AssertionError('work_stream made a stream although the current one is not the null stream')
        return stream_type(*a, **k)
    monkeypatch.setattr(torch.cuda, 'Stream', no_new_stream)
    with torch.cuda.stream(side):
        pts = _points(torch, dev)
        out = torch.zeros(N, dtype=torch.float64, device=dev)
        with T.work_stream(dev) as work:
            assert work.cuda_stream == side.cuda_stream != 0
            assert torch.cuda.current_stream(dev).cuda_stream == side.cuda_stream
            ctx.plane_distance_dev(pts.data_ptr(), N, PP, NR, out.data_ptr(), work.cuda_stream)
        assert torch.cuda.current_stream(dev).cuda_stream == side.cuda_stream
        got = out.cpu().numpy()
    assert np.array_equal(got, _want(pts))


def test_exception_in_the_block_propagates_after_the_join():
    torch, ctx, dev = _device()
    assert torch.cuda.current_stream(dev).cuda_stream == 0
    pts = _points(torch, dev)
    out = torch.zeros(N, dtype=torch.float64, device=dev)
    with pytest.raises(RuntimeError, match='raised by the test'):
        with T.work_stream(dev) as work:
            ctx.plane_distance_dev(pts.data_ptr(), N, PP, NR, out.data_ptr(), work.cuda_stream)
            raise RuntimeError('raised by the test')
    assert torch.cuda.current_stream(dev).cuda_stream == 0
    doubled = (out * 2).cpu().numpy()                                    # an op on the caller's stream sees the side stream's writes
    assert np.array_equal(doubled, _want(pts) * 2)


def test_device_csr_checks_the_pair():
    torch, ctx, dev = _device()
    offs = torch.tensor([0, 2, 2, 3], dtype=torch.int32, device=dev)
    nbrs = torch.tensor([1, 2, 0], dtype=torch.int64, device=dev)
    o, nb = T.device_csr((offs, nbrs), 3, dev, 'device values')
    assert o.dtype == torch.int64 and nb.dtype == torch.int32 and o.is_contiguous() and nb.is_contiguous()
    assert o.tolist() == [0, 2, 2, 3] and nb.tolist() == [1, 2, 0]
    host = (offs.cpu().numpy(), nbrs.cpu().numpy())
    for adj in (host, (offs.cpu(), nbrs.cpu()), (offs, host[1]), [offs, nbrs], (offs, nbrs, nbrs)):
        with pytest.raises(TypeError, match='^device values need a device CSR adjacency \\(offsets, neighbours\\)$'):
            T.device_csr(adj, 3, dev, 'device values')
    with pytest.raises(TypeError, match='^CVSegmentation: device classes need a device CSR adjacency'):
        T.device_csr(host, 3, dev, 'CVSegmentation: device classes')
    for adj, n in (((offs, nbrs), 2), ((offs, nbrs), 4), ((offs, nbrs[:2]), 3), ((offs.reshape(2, 2), nbrs), 3), ((offs[:1], nbrs), 0)):
        with pytest.raises(ValueError, match='^CSR adjacency: offsets must have n \\+ 1 entries ending at len\\(neighbours\\)$'):
            T.device_csr(adj, n, dev, 'device values')


def test_device_csr_rejects_a_pair_on_another_device():
    torch, ctx, dev = _device()
    if torch.cuda.device_count() < 2:
        pytest.skip('one device visible')
    other = torch.device('cuda', (dev.index + 1) % torch.cuda.device_count())
    offs = torch.tensor([0, 1, 2], dtype=torch.int64, device=other)
    nbrs = torch.tensor([1, 0], dtype=torch.int32, device=other)
    with pytest.raises(ValueError, match=f'^CSR adjacency must be on {dev}$'):
        T.device_csr((offs, nbrs), 2, dev, 'device values')
    from Fusion3DSeg.segUtils.cv import CVSegmentation
    with pytest.raises(ValueError, match=f'^CSR adjacency must be on {dev}$'):
        CVSegmentation(torch.zeros(2, dtype=torch.int64, device=dev), (offs, nbrs)).instance_seperate()


def test_point_correspondance_from_the_default_stream_equals_the_numpy_route():
    """The tensors are widened to float64 by a kernel on the null stream right before the radius query, which runs on the side
    stream: the CSR equals the host route's on the same values."""
    from Fusion3DSeg.segUtils.correspondance import PointCorrespondance
    torch, ctx, dev = _device()
    F, h, w = 2, 8, 8
    rng = np.random.default_rng(4)
    lattice = np.stack(np.meshgrid(*[np.arange(4) * 0.25] * 3, indexing='ij'), -1).reshape(-1, 3)
    sparse = lattice.astype(np.float16)                                  # 64 points, exact in float16
    dense = (np.round(rng.uniform(-0.4, 1.15, (F * h * w, 3)) * 64) / 64).astype(np.float32)
    assert np.array_equal(sparse.astype(np.float64), lattice) and len(sparse) == 64
    assert torch.cuda.current_stream(dev).cuda_stream == 0
    pc = PointCorrespondance(torch.from_numpy(sparse).to(dev), torch.from_numpy(dense).to(dev), 0.3, F, (h, w))
    assert torch.cuda.current_stream(dev).cuda_stream == 0
    host = PointCorrespondance(sparse, dense, 0.3, F, (h, w))
    offs, idx = (a.cpu().numpy() for a in pc.csr)                        # copies on the null stream
    assert pc.csr.offsets.is_cuda and offs.dtype == np.int64 and idx.dtype == np.int32
    assert np.array_equal(offs, host.csr.offsets) and np.array_equal(idx, host.csr.indices)
    lens = np.diff(offs)
    assert lens.min() == 0 and lens.max() > 1 and len(lens) == F * h * w
