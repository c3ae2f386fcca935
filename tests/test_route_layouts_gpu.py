"""Every tensor route under equal-valued inputs of another layout or dtype (tests/route_cases.py): each tensor argument in turn is
replaced by a column slice of a wider tensor, by every second row of a doubled tensor, by a view at a storage offset that is not 16-byte
aligned, by a transposed-then-transposed-back copy, and by the other dtypes the route documents.  The result passes the case's check
against the same reference, or the route raises a TypeError / ValueError that names the argument; it never returns another answer.
Afterwards every tensor the test made holds the bits it held before, the padding around a view included, except the arguments a route
documents as updated in place.  The padding holds valid values (the argument's own, reversed), so a route that read it would be wrong,
not out of bounds."""
import numpy as np
import pytest

import f3d
import route_cases as R

pytestmark = pytest.mark.gpu


def variants(a, alt):
    """(label, host base array, function from the uploaded base to the tensor handed over) for the array `a`."""
    rev = a[::-1]
    if a.ndim >= 2:
        wide = np.concatenate([a, rev[..., :1]], axis=-1)
        yield 'column slice', wide, lambda t: t[..., :a.shape[-1]]
    else:
        yield 'column slice', np.stack([a, rev], axis=1), lambda t: t[:, 0]
    doubled = np.empty((2 * len(a),) + a.shape[1:], a.dtype)
    doubled[0::2], doubled[1::2] = a, rev
    yield 'every second row', doubled, lambda t: t[::2]
    flat = np.concatenate([a.reshape(-1)[:1], a.reshape(-1)])
    yield 'offset', flat, lambda t: t[1:].view(a.shape)
    if a.ndim == 2:
        yield 'transposed back', np.ascontiguousarray(a.T), lambda t: t.t()
    for dt in alt:
        yield np.dtype(dt).name, a.astype(dt), lambda t: t


@pytest.mark.parametrize('name', sorted(n for n, r in R.TABLE.items() if r.routes and not r.owned))      # (raycast: its tensors are the volume's)
def test_route_under_other_layouts(name):
    import torch
    dev = torch.device('cuda', f3d.default_context().device)
    r = R.TABLE[name]
    inputs, call, want, check, _ = R.prepared(name, R.SEED)
    passed = refused = 0
    for key, a in inputs.items():
        if key in r.owned:
            continue
        for label, base, view in variants(a, r.alt.get(key, ())):
            t = R.upload(inputs, dev)
            held = torch.from_numpy(np.array(base)).to(dev)
            t[key] = view(held)
            assert tuple(t[key].shape) == a.shape, (key, label)
            if label == 'offset':
                assert t[key].data_ptr() % 16 != 0, (key, label)
            try:
                got = R.to_host(call(t))
            except (TypeError, ValueError) as exc:
                word = r.names.get(key, key)
                assert word in str(exc), f'{name}: {key} as {label} was refused without naming it ({word}): {exc!r}'
                refused += 1
            else:
                torch.cuda.synchronize(dev)
                try:
                    check(got, want)
                except AssertionError as exc:
                    raise AssertionError(f'{name}: another answer for {key} as {label}') from exc
                passed += 1
            torch.cuda.synchronize(dev)
            for k, v in t.items():
                if k in r.inplace:
                    continue
                now = (held if k == key else v).cpu().numpy()
                before = base if k == key else inputs[k]
                assert now.tobytes() == np.ascontiguousarray(before).tobytes(), f'{name}: {k} was written ({key} as {label})'
    assert passed > 0, (passed, refused)
