#!/usr/bin/env python3
"""smooth_votes / smooth_segment at scan size: the box room of planes_stress.py at 1M and 4M points, its radius graph at r = 5 cm,
134 vote columns of random counts.

Variants: float64 and uint16 input; no gate and the normals gate at 30 degrees; smooth_votes and smooth_segment; one iteration, through
the _dev entries on device tensors.  Timing: HIP events around the call after a warm-up, the median of 10 calls, repeated three times
in this one process: the median of the three medians and their minimum and maximum are reported.  Per variant one JSON line with ms
per call, the algorithmic bytes computed from the shapes -- the contributing rows plus every point's own row read, the output written
(the matrix, or 8 B of class per point), the CSR, and for a gated variant the normals of every entry and of every point -- and
bytes/s; per size one line with the median and the maximum row length, so the skew is on record.

The one condition: in the same process the script times ``torch.sparse_csr_tensor(A + self_weight * I) @ votes`` in float64 on the
same graph and matrix, the only independent yardstick there is.  The ungated float64 smooth_votes call must not be slower; the script
says so and exits with status 1 when it is.  If this torch build cannot run that product on the device the script says that instead,
and no condition applies.

The kernel split (k_sm_check against k_smooth) comes from a run of its own:
``rocprofv3 --kernel-trace --stats -- python scripts/smooth_stress.py --once --points 1000000``.
"""
import argparse
import json
import math
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / '3d-point-cloud-segmentation-using-2d-img-segmentation_amd', ROOT / 'scripts'):
    sys.path.insert(0, str(p))

NCOLS, NCLASSES = 134, 133


def timed(fn, torch, calls, reps):
    """(median of the medians, min, max) in ms over `reps` repetitions of `calls` event-timed calls, after a warm-up."""
    fn(); torch.cuda.synchronize()
    medians = []
    for _ in range(reps):
        times = []
        for _ in range(calls):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record()
            torch.cuda.synchronize()
            times.append(a.elapsed_time(b))
        medians.append(statistics.median(times))
    return statistics.median(medians), min(medians), max(medians)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--points', type=int, nargs='*', default=[1_000_000, 4_000_000])
    ap.add_argument('--radius', type=float, default=0.05)
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--once', action='store_true', help='one call per variant after a warm-up: the target of a kernel trace')
    args = ap.parse_args()
    calls, reps = (1, 1) if args.once else (args.calls, args.reps)
    import torch
    import f3d
    from planes_stress import device_graph, room
    ctx = f3d.default_context(0)
    cos30 = math.cos(math.radians(30.0))
    missed = False
    with torch.cuda.stream(torch.cuda.Stream()):                      # a stream of the caller's own: no side-stream hand-off per call
        st = torch.cuda.current_stream().cuda_stream
        for want in args.points:
            pts, nrm, spacing = room(want)
            n = len(pts)
            x, nd = torch.as_tensor(pts, device='cuda'), torch.as_tensor(nrm, device='cuda')
            (offs, nbrs), _, _ = device_graph(ctx, torch, x, args.radius, 1)
            e = len(nbrs)
            lens = offs[1:] - offs[:-1]
            rows = torch.repeat_interleave(torch.arange(n, device='cuda'), lens)
            cols = nbrs.to(torch.int64)
            others = rows != cols
            dots = ((nd[rows, 0] * nd[cols, 0] + nd[rows, 1] * nd[cols, 1]) + nd[rows, 2] * nd[cols, 2]).abs()
            contributing = {'none': int(others.sum()), 'normals': int((others & (dots >= cos30)).sum())}
            del dots
            meta = {'points': n, 'spacing': round(spacing, 5), 'radius': args.radius, 'entries': e,
                    'row_median': int(lens.median()), 'row_max': int(lens.max())}
            print(json.dumps({'stage': 'graph', **meta}), flush=True)
            gen = torch.Generator(device='cuda').manual_seed(5)
            v64 = torch.randint(0, 9, (n, NCOLS), device='cuda', generator=gen).to(torch.float64)
            v16 = v64.to(torch.int16)                                  # uint16 counts as int16 bits
            out = torch.empty((n, NCOLS), dtype=torch.float64, device='cuda')
            cls = torch.empty(n, dtype=torch.int64, device='cuda')
            base_ms = {}
            for vname, v, vtype, width in (('float64', v64, f3d.VOTES_F64, 8), ('uint16', v16, f3d.VOTES_U16, 2)):
                for gate in ('none', 'normals'):
                    nptr = nd.data_ptr() if gate == 'normals' else None
                    for entry in ('smooth_votes', 'smooth_segment'):
                        if entry == 'smooth_votes':
                            fn = lambda: ctx.smooth_votes_dev(v.data_ptr(), vtype, n, NCOLS, offs.data_ptr(), nbrs.data_ptr(), nptr, cos30, None,
                                                              f3d.F64, 0.0, 1.0, 1, out.data_ptr(), st)
                            written = n * NCOLS * 8
                        else:
                            fn = lambda: ctx.smooth_segment_dev(v.data_ptr(), vtype, n, NCOLS, offs.data_ptr(), nbrs.data_ptr(), nptr, cos30, None,
                                                                f3d.F64, 0.0, 1.0, 1, NCLASSES, 0.5, None, False, cls.data_ptr(), st)
                            written = n * 8
                        ms, lo, hi = timed(fn, torch, calls, reps)
                        ctx.take_device_error(st)
                        nbytes = (contributing[gate] + n) * NCOLS * width + written + (n + 1) * 8 + e * 4 + \
                                 ((e + n) * 24 if gate == 'normals' else 0)
                        base_ms[(vname, gate, entry)] = ms
                        print(json.dumps({'stage': entry, 'input': vname, 'gate': gate, 'ms': round(ms, 3), 'ms_min': round(lo, 3),
                                          'ms_max': round(hi, 3), 'contributing_rows': contributing[gate], 'bytes': nbytes,
                                          'TBps': round(nbytes / ms / 1e9, 3), **meta}), flush=True)
            # the yardstick: the same sum as a generic sparse product (the row's own entry carries self_weight = 1)
            try:
                a = torch.sparse_csr_tensor(offs, cols, torch.ones(e, dtype=torch.float64, device='cuda'), size=(n, n))
                ref = None

                def product():
                    nonlocal ref
                    ref = a @ v64
                ms, lo, hi = timed(product, torch, calls, reps)
            except Exception as exc:                                   # this torch build has no such product on the device
                print(json.dumps({'stage': 'torch_csr_matmul', 'unavailable': f'{type(exc).__name__}: {exc}'[:300], **meta}), flush=True)
                continue
            ctx.smooth_votes_dev(v64.data_ptr(), f3d.VOTES_F64, n, NCOLS, offs.data_ptr(), nbrs.data_ptr(), None, 0.0, None, f3d.F64, 0.0, 1.0, 1,
                                 out.data_ptr(), st)
            ctx.take_device_error(st)
            same = bool(torch.equal(out, ref))                         # integer counts: both sums are exact
            mine = base_ms[('float64', 'none', 'smooth_votes')]
            ok = mine <= ms
            missed |= not ok
            print(json.dumps({'stage': 'torch_csr_matmul', 'ms': round(ms, 3), 'ms_min': round(lo, 3), 'ms_max': round(hi, 3),
                              'smooth_votes_ms': round(mine, 3), 'equal': same, 'condition': 'met' if ok else 'missed', **meta}), flush=True)
            del a, ref
    return 1 if missed else 0


if __name__ == '__main__':
    sys.exit(main())
