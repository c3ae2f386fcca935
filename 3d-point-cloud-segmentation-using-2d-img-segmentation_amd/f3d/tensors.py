"""The hand-off from a NumPy array or a torch tensor to a ``Context`` call: which stream the library is given, which device
the tensors live on, the dtype codes of the C-ABI and the CSR adjacency checks.  torch is imported when a function needs it:
it is plumbing, not a requirement of the binding.
"""
from contextlib import contextmanager

import numpy as np

CSR_ADJACENCY = 'CSR adjacency: offsets must have n + 1 entries ending at len(neighbours)'


def on_device(a):
    """True for a torch tensor in device memory (False for NumPy arrays, CPU tensors and everything else)."""
    return getattr(a, 'is_cuda', False)


def torch_device(ctx, what):
    """(torch, the torch device of `ctx`), or F3DUnavailable when torch or a device is missing."""
    from f3d import F3DUnavailable
    try:
        import torch
    except ImportError:
        torch = None
    if torch is None or not torch.cuda.is_available():
        raise F3DUnavailable(f'{what} needs a HIP device; there is no CPU fallback')
    return torch, torch.device('cuda', ctx.device)


@contextmanager
def work_stream(device):
    """The torch stream whose handle a ``*_dev`` call is given, as torch's current stream for the block.

    The library reads the null handle (0) as "the context's own stream", and that stream is non-blocking: it is not ordered
    with torch's legacy default stream.  So the null handle is never handed over: when the caller's current stream is the
    default stream, the work goes to a side stream that waits for it, and the caller's stream waits for the side stream when
    the block ends, also when it ends with an exception.  Any other current stream is used as it is.  No host stall.

    Tensors the caller allocated before the block need no ``record_stream``: their memory belongs to the caller's stream's
    pool, so whatever reuses it is enqueued on that stream, after the wait."""
    import torch
    caller = torch.cuda.current_stream(device)
    work = caller
    if caller.cuda_stream == 0:
        work = torch.cuda.Stream(device)
        work.wait_stream(caller)
    try:
        with torch.cuda.stream(work):
            yield work
    finally:
        if work is not caller:
            caller.wait_stream(work)


def upload(a, dev):
    """A host array (a view table, a pose, a volume's zeros) as a tensor on `dev`, enqueued on the current stream with no host stall:
    it goes through pinned memory.  ``torch.from_numpy(a).to(dev)`` of a pageable array returns only when the copy is done, and the copy
    is ordered behind the stream's earlier work, so the host would wait for all of it.  torch's host allocator keeps the pinned block
    until the copy has run."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).pin_memory().to(dev, non_blocking=True)


def dtype_code(a):
    """f3d.F32 / f3d.F64 of a float32 / float64 array or tensor."""
    import f3d
    return f3d.F32 if a.dtype.itemsize == 4 else f3d.F64


def index_code(a):
    """f3d.I32 / f3d.I64 of an int32 / int64 array or tensor."""
    import f3d
    return f3d.I32 if a.dtype.itemsize == 4 else f3d.I64


def depth_code(depths):
    """F3D_DEPTH_F64 / F32 / U16 (0 / 1 / 2) of a float64 / float32 / uint16 depth array or tensor, TypeError for anything else."""
    name = str(depths.dtype).replace('torch.', '')
    if name not in ('float64', 'float32', 'uint16'):
        raise TypeError(f'depth frames must be uint16, float32 or float64, got {depths.dtype}')
    return {'float64': 0, 'float32': 1, 'uint16': 2}[name]


def host_csr(offsets, neighbours, n, message='offsets must have n+1 entries ending at len(neighbours)'):
    """(offsets int64 [n + 1], neighbours int32 [offsets[n]]) as contiguous NumPy arrays, checked: the kernels read every row
    the offsets name."""
    offs = np.ascontiguousarray(offsets, dtype=np.int64)
    nbrs = np.ascontiguousarray(neighbours, dtype=np.int32)
    if len(offs) != n + 1 or (n and offs[-1] != len(nbrs)):
        raise ValueError(message)
    return offs, nbrs


def device_csr(adj, n, dev, what):
    """host_csr for tensors on `dev`; `what` names the caller's device input in the TypeError.  One scalar readback."""
    import torch
    if not (isinstance(adj, tuple) and len(adj) == 2 and all(on_device(a) for a in adj)):
        raise TypeError(f'{what} need a device CSR adjacency (offsets, neighbours)')
    offs, nbrs = adj[0].to(torch.int64).contiguous(), adj[1].to(torch.int32).contiguous()
    if offs.device != dev or nbrs.device != dev:
        raise ValueError(f'CSR adjacency must be on {dev}')
    if offs.dim() != 1 or len(offs) != n + 1 or int(offs[-1]) != len(nbrs):
        raise ValueError(CSR_ADJACENCY)
    return offs, nbrs


def device_points(a, dev, name):
    """`a` as a contiguous float32 / float64 [N, 3] tensor on `dev` (other dtypes are widened to float64)."""
    import torch
    t = torch.as_tensor(a).to(dev)
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f'{name} must be [N, 3], got {tuple(t.shape)}')
    if t.dtype != torch.float32:
        t = t.to(torch.float64)
    return t.contiguous()
