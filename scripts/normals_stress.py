#!/usr/bin/env python3
"""Surface normals of depth frames (f3d_estimate_normals_batch_dev): ms per batch (HIP events, after a warm-up) and points/s for
256 frames x 256x192 and 64 frames x 480x640, each with and without 10 % zero-depth pixels; the host oracle's seconds per frame
(tests/normals_ref.py, scipy cKDTree + NumPy eigh, one core); the VGPR / scratch use of the kernels from the compiler's
resource-usage remarks.  Synthetic scene: a wall at 2.5 m and a floor 1.2 m below the camera, focal length 210 px at 256x192
(scaled with the width), depth in uint16 millimetres with 1 mm noise."""
import argparse
import json
import os
import re
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
PKG = ROOT / '3d-point-cloud-segmentation-using-2d-img-segmentation_amd'
sys.path.insert(0, str(PKG))
sys.path.insert(0, str(ROOT / 'tests'))
import f3d                     # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--repeats', type=int, default=5)
ap.add_argument('--radius', type=float, default=0.05)
ap.add_argument('--max-nn', type=int, default=30)
ap.add_argument('--no-oracle', action='store_true')
ap.add_argument('--no-regs', action='store_true')
args = ap.parse_args()


def scene(F, h, w, dropout, seed=0):
    rng = np.random.default_rng(seed)
    f = 210.0 * w / 256
    K = np.array([[f, 0.0, w / 2], [0.0, f, h / 2], [0.0, 0.0, 1.0]])
    v = np.arange(h, dtype=np.float64)[:, None] + np.zeros((1, w))
    with np.errstate(divide='ignore'):
        floor = np.where(v > h / 2 + 0.5, f * 1.2 / (v - h / 2), np.inf)
    d = np.minimum(2.5, floor)
    depth = np.empty((F, h, w), np.uint16)
    for j in range(F):
        mm = np.round(d * 1000 + rng.normal(0, 1.0, d.shape)).astype(np.uint16)
        if dropout:
            mm[rng.random(mm.shape) < dropout] = 0
        depth[j] = mm
    q = np.tile([1.0, 0.0, 0.0, 0.0], (F, 1))
    t = np.stack([[0.01 * j, 0.0, 0.0] for j in range(F)])
    return K, depth, q, t


def regs():
    """VGPR / AGPR / scratch of the kernels of f3d_normals.hip (compiled for gfx950 with the library's flags)."""
    csrc = PKG / 'csrc'
    cmd = [os.environ.get('HIPCC', '/opt/rocm/bin/hipcc'), '-O3', '-std=c++17', '--offload-arch=gfx950', '-ffp-contract=off', '-fno-fast-math',
           '-fPIC', f'-I{ROOT / "include"}', f'-I{csrc}', '-c', '--cuda-device-only', '-Rpass-analysis=kernel-resource-usage',
           str(csrc / 'f3d_normals.hip'), '-o', os.devnull]
    text = subprocess.run(cmd, capture_output=True, text=True).stderr
    out, name = {}, None
    for line in text.splitlines():
        m = re.search(r'Function Name: (\S+)', line)
        if m:
            name = m.group(1) if 'k_nrm' in m.group(1) else None
            if name:
                short = re.search(r'(k_nrm_\w+?)(ILi(\d+)E)?E', name)
                name = short.group(1) + (f'<{short.group(3)}>' if short.group(3) else '')
                out[name] = {}
            continue
        if name:
            for key, label in (('VGPRs', 'vgpr'), ('AGPRs', 'agpr'), ('ScratchSize [bytes/lane]', 'scratch'), ('Occupancy [waves/SIMD]', 'occupancy')):
                m = re.search(re.escape(key) + r': (\d+)', line)
                if m:
                    out[name][label] = int(m.group(1))
    return out


def main():
    import torch
    dev = torch.device('cuda', 0)
    ctx = f3d.default_context(0)
    results = []
    for F, h, w in ((256, 192, 256), (64, 480, 640)):
        for dropout in (0.0, 0.1):
            K, depth, q, t = scene(F, h, w, dropout)
            n = h * w
            d = torch.from_numpy(depth.view(np.int16)).to(dev)
            pts = torch.empty((F, n, 3), dtype=torch.float64, device=dev)
            nrm = torch.empty((F, n, 3), dtype=torch.float64, device=dev)
            s = torch.cuda.Stream(dev)                    # not the null stream: its handle would select the context's own stream
            s.wait_stream(torch.cuda.current_stream(dev))
            ctx.unproject_depth_batch_dev(d.data_ptr(), 2, F, h, w, K, q, t, pts.data_ptr(), 1000.0, s.cuda_stream)
            ms = []
            for r in range(args.repeats + 1):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                ctx.estimate_normals_batch_dev(pts.data_ptr(), F, n, t, nrm.data_ptr(), args.radius, args.max_nn, True, stream=s.cuda_stream)
                e1.record(s)
                e1.synchronize()
                if r:
                    ms.append(e0.elapsed_time(e1))
            torch.cuda.synchronize(dev)
            first = nrm[0].cpu().numpy()
            res = {'frames': F, 'h': h, 'w': w, 'dropout': dropout, 'points': F * n, 'ms_per_batch_median': float(np.median(ms)),
                   'ms_per_batch_min': float(np.min(ms)), 'points_per_s': F * n / (np.median(ms) / 1e3),
                   'unit_rows': int((np.abs(np.linalg.norm(first, axis=1) - 1) < 1e-14).sum())}
            if not args.no_oracle and h == 192:
                import normals_ref as R
                p0 = pts[0].cpu().numpy()
                t0 = time.perf_counter()
                want = R.surface_normal_estimation(p0, t[0], args.radius, args.max_nn)
                res['oracle_s_per_frame'] = time.perf_counter() - t0
                res['oracle_sign_agree'] = float(np.mean(np.einsum('ij,ij->i', want, first) > 0.999999))
            print(json.dumps(res), flush=True)
            results.append(res)
            del d, pts, nrm
            torch.cuda.empty_cache()
    if not args.no_regs:
        print(json.dumps({'kernel_resources': regs()}), flush=True)


if __name__ == '__main__':
    main()
