"""Every tensor route under stalled streams (tests/route_cases.py, tests/stalled_streams.py).  The caller's stream C is made to sleep
100 ms; behind the sleep the inputs, which hold the decoy B, are overwritten with the scene A; the route is called at once, its results
are cloned on C, and the inputs are overwritten with B again, freed, and their memory refilled.  A kernel, copy or memset that the route
or the library puts on a stream that is not ordered behind C runs during the sleep and reads B; work that C is not made to wait for has
not run when C clones the results; a tensor freed while another stream still reads it is refilled under that stream's eyes.  Each of
them makes the clones fail the check against want(A), which the unstalled warm-up has just passed.  Every stream a route makes while the
lens is armed sleeps at its birth, and stateful routes have their streams and C put to sleep again between their steps."""
import numpy as np
import pytest

import f3d
import route_cases as R
import stalled_streams as S
from f3d import tensors as T

pytestmark = pytest.mark.gpu

PROBES = 8


def _device():
    import torch
    ctx = f3d.default_context()
    return torch, ctx, torch.device('cuda', ctx.device)


@pytest.fixture(scope='session')
def concurrency():
    """Proves once that the lens can see anything here: a kernel on a stream that is not ordered with the stalled caller's stream runs
    early and reads the decoy (fresh torch streams, probed once each), and the context's own stream and torch's null stream finish their
    work while a side stream sleeps.  -> the caller's side stream the per-case tests use and the counts.  If streams serialise on this
    machine, every test of the module fails here."""
    torch, ctx, dev = _device()
    cycles, probe_ms, took_ms = S.calibrate(dev.index)
    a, b = R.prepared('plane_distance', R.SEED)[0]['points'], R.prepared('plane_distance', R.OTHER_SEED)[0]['points']
    want_b = R._plane_dist(b)                                                # the kernel's own operation order: exact
    assert not np.array_equal(want_b, R._plane_dist(a))
    caller = torch.cuda.Stream(dev)
    src_a = torch.from_numpy(np.array(a)).to(dev)
    early = 0
    for _ in range(PROBES):
        fresh = torch.cuda.Stream(dev)
        x, out = torch.from_numpy(np.array(b)).to(dev), torch.zeros(R.N, dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)
        e = S.stall(caller)
        with torch.cuda.stream(caller):
            x.copy_(src_a)                                                   # behind the stall: a stream ordered with C reads A
        ctx.plane_distance_dev(x.data_ptr(), R.N, R.PP, R.NR, out.data_ptr(), fresh.cuda_stream)
        fresh.synchronize()
        still_stalled = not e.query()
        caller.synchronize()
        early += bool(still_stalled and np.array_equal(out.cpu().numpy(), want_b))
    own = null = 0
    pts = np.array(a)
    for _ in range(PROBES):
        side = torch.cuda.Stream(dev)
        torch.cuda.synchronize(dev)
        e = S.stall(side)
        ctx.rotate(pts, R.F.Q0)                                              # a host-pointer call: the context's own stream, drained
        own += not e.query()
        doubled = (src_a * 2).cpu()                                          # torch's null stream, drained by the copy
        null += not e.query()
        side.synchronize()
        assert np.array_equal(doubled.numpy(), pts * 2)
    found = dict(caller=caller, early=early, own=own, null=null, cycles=cycles, probe_ms=probe_ms, took_ms=took_ms)
    print(f'\nstalled-stream lens: {cycles} cycles stall {took_ms:.1f} ms (the probe of {S.PROBE_CYCLES} cycles took {probe_ms:.3f} ms); '
          f'{early} of {PROBES} fresh streams ran a kernel while the caller\'s stream slept, the context\'s own stream finished under '
          f'{own} of {PROBES} sleeping side streams and the null stream under {null}')
    if not (early and own and null):
        pytest.fail(f'streams serialise here: {early} of {PROBES} fresh streams ran early, the context\'s stream finished under {own} and the '
                    f'null stream under {null} of {PROBES} stalled side streams; this lens can see nothing on this machine')
    return found


def test_the_lens_sees_a_stray_stream(concurrency):
    c = concurrency
    assert c['early'] >= 1 and c['own'] >= 1 and c['null'] >= 1, f"{c['early']} of {PROBES} concurrent streams, own {c['own']}, null {c['null']}"
    assert S.LOW * S.STALL_MS <= c['took_ms'] <= S.HIGH * S.STALL_MS


def _mini_route(torch, ctx, dev, x, out, join, through_work_stream):
    """plane_distance on a stream of its own that waits for the caller's; `join`: the caller's stream waits for it afterwards."""
    if through_work_stream:
        with T.work_stream(dev) as work:
            ctx.plane_distance_dev(x.data_ptr(), R.N, R.PP, R.NR, out.data_ptr(), work.cuda_stream)
        return
    caller = torch.cuda.current_stream(dev)
    work = torch.cuda.Stream(dev)
    work.wait_stream(caller)
    ctx.plane_distance_dev(x.data_ptr(), R.N, R.PP, R.NR, out.data_ptr(), work.cuda_stream)
    if join:
        caller.wait_stream(work)


@pytest.mark.parametrize('kind', ['no join', 'join', 'work_stream'])
def test_canaries(concurrency, monkeypatch, kind):
    """A mini-route that waits for the caller but never joins back leaves the sentinel in the caller-side snapshot; the same with the
    join, and through f3d.tensors.work_stream from the null stream, gives the scene's distances."""
    torch, ctx, dev = _device()
    a, b = R.prepared('plane_distance', R.SEED)[0]['points'], R.prepared('plane_distance', R.OTHER_SEED)[0]['points']
    x, src_a = torch.from_numpy(np.array(b)).to(dev), torch.from_numpy(np.array(a)).to(dev)
    out = torch.full((R.N,), -1.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    factory = S.StalledFactory(monkeypatch).arm()
    caller = torch.cuda.default_stream(dev) if kind == 'work_stream' else concurrency['caller']
    with torch.cuda.stream(caller):
        e = S.stall(caller)
        x.copy_(src_a)
        _mini_route(torch, ctx, dev, x, out, kind == 'join', kind == 'work_stream')
        assert not e.query()
        snapshot = out.clone()
    factory.disarm()
    caller.synchronize()
    factory.synchronize()
    assert len(factory.made) == 1
    got = snapshot.cpu().numpy()
    if kind == 'no join':
        assert (got == -1.0).all(), int((got != -1.0).sum())                # the slip is seen
        assert np.array_equal(out.cpu().numpy(), R._plane_dist(a))           # (the work itself was right, only nobody waited for it)
    else:
        assert np.array_equal(got, R._plane_dist(a))


def _counted(monkeypatch, entries):
    counts = dict.fromkeys(entries, 0)
    for name in entries:
        inner = getattr(f3d.Context, name)

        def counting(self, *args, _inner=inner, _name=name, **kwargs):
            counts[_name] += 1
            return _inner(self, *args, **kwargs)
        monkeypatch.setattr(f3d.Context, name, counting)
    return counts


@pytest.mark.parametrize('mode', ['default', 'side'])
@pytest.mark.parametrize('name', sorted(R.TABLE))
def test_route_under_stalled_streams(concurrency, monkeypatch, name, mode):
    torch, ctx, dev = _device()
    r = R.TABLE[name]
    in_a, call, want_a, check_a, _ = R.prepared(name, R.SEED)
    in_b, call_b, want_b, check_b, _ = R.prepared(name, R.OTHER_SEED)
    caller = torch.cuda.default_stream(dev) if mode == 'default' else concurrency['caller']
    counts = _counted(monkeypatch, r.entries)
    with torch.cuda.stream(caller):
        # 1. warm-up, unstalled and synchronised: both seeds pass, so a later failure is an ordering failure; scratch and pools have grown
        for inputs, run, want, check in ((in_a, call, want_a, check_a), (in_b, call_b, want_b, check_b)):
            got = run(R.upload(inputs, dev))
            torch.cuda.synchronize(dev)
            check(R.to_host(got), want)
        assert all(counts.values()), f'{name} does not reach {[k for k, v in counts.items() if not v]}'
        del got
        # 2. the stalled run: no host synchronisation by the test between the stall and the snapshot
        t, src_a, src_b = R.upload(in_b, dev), R.upload(in_a, dev), R.upload(in_b, dev)
        shapes = [(tuple(v.shape), v.dtype) for v in t.values()]
        torch.cuda.synchronize(dev)
        factory = S.StalledFactory(monkeypatch).arm()
        e = S.stall(caller)
        for k in t:
            t[k].copy_(src_a[k])
        def between():                                                       # every stream the route made, and the caller's: on a side
            factory.stall_all()                                              #   stream work_stream makes none, the route works on C itself
            S.stall(caller)
        got = call(t, between) if r.stateful else call(t)
        still_stalled = not e.query()
        snapshot = R.clone_tree(got)
        for k in t:
            t[k].copy_(src_b[k])
        del t, got
        refill = [torch.full(shape, 1, dtype=dtype, device=dev) for shape, dtype in shapes]
        factory.disarm()
    # 3. the whole call was enqueued while the inputs still held the decoy
    if not r.syncs:
        assert still_stalled, f'{name} is not marked syncs, yet the {S.STALL_MS} ms stall had ended when it returned'
    # 4. the clones made on C hold what the scene's reference says
    caller.synchronize()
    factory.synchronize()
    check_a(R.to_host(snapshot), want_a)
    del refill
