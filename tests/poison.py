"""poisoned_empty(byte): for the duration of a `with` block, every array or tensor that numpy.empty, numpy.empty_like, torch.empty,
torch.empty_like or torch.Tensor.new_empty hands out has each of its bytes set to `byte`.  Fresh pages behind an uninitialised
allocation are zero in practice, and zero is what a forgotten initialisation usually wanted; under the block they hold 0xFF (-1, NaN,
the empty value of a min-key), 0x5A (large, positive, finite) or whatever else the caller asks for, so that an element the product
never writes shows in its result.

Test code: nothing in the product imports it.  Wrap the product call only, never the reference computation.  What it reaches is the
module attribute (`np.empty(...)`, `torch.empty(...)`, `t.new_empty(...)`) looked up at call time, which is how the product spells
every one of its allocations; a name bound earlier by `from numpy import empty` keeps the original."""
import contextlib

import numpy as np


def fill_array(a, byte):
    """Every byte of the ndarray `a` becomes `byte`, whatever its dtype, order or rank (object arrays are left as they are)."""
    if a.dtype.hasobject or a.size == 0:
        return a
    raw = np.frombuffer(bytes([byte]) * a.dtype.itemsize, dtype=f'V{a.dtype.itemsize}')[0]
    a.view(f'V{a.dtype.itemsize}')[...] = raw               # a view of the same item size exists for any strides, 0-d included
    return a


def fill_tensor(t, byte):
    """Every byte of the storage behind the fresh tensor `t` becomes `byte` (CPU or device; the fill is queued on the current stream)."""
    import torch
    if t.numel() == 0 or t.is_sparse or t.device.type == 'meta':
        return t
    torch.tensor([], dtype=torch.uint8, device=t.device).set_(t.untyped_storage()).fill_(byte)
    return t


@contextlib.contextmanager
def poisoned_empty(byte):
    if not 0 <= int(byte) <= 255:
        raise ValueError(f'byte {byte} outside [0, 255]')
    byte = int(byte)
    import torch
    np_empty, np_empty_like = np.empty, np.empty_like
    t_empty, t_empty_like, t_new_empty = torch.empty, torch.empty_like, torch.Tensor.new_empty

    def empty(*args, **kw):
        return fill_array(np_empty(*args, **kw), byte)

    def empty_like(*args, **kw):
        return fill_array(np_empty_like(*args, **kw), byte)

    def torch_empty(*args, **kw):
        if kw.get('out') is not None:                        # out=: the caller's tensor, resized; not a fresh allocation
            return t_empty(*args, **kw)
        return fill_tensor(t_empty(*args, **kw), byte)

    def torch_empty_like(*args, **kw):
        return fill_tensor(t_empty_like(*args, **kw), byte)

    def new_empty(self, *args, **kw):
        return fill_tensor(t_new_empty(self, *args, **kw), byte)

    np.empty, np.empty_like = empty, empty_like
    torch.empty, torch.empty_like, torch.Tensor.new_empty = torch_empty, torch_empty_like, new_empty
    try:
        yield
    finally:
        np.empty, np.empty_like = np_empty, np_empty_like
        torch.empty, torch.empty_like, torch.Tensor.new_empty = t_empty, t_empty_like, t_new_empty
