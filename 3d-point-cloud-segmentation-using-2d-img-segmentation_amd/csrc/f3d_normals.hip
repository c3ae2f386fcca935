// Surface normals of depth frames: Open3D's PointCloud::EstimateNormals(KDTreeSearchParamHybrid(radius, max_nn)) followed by
// the camera-facing flip of RTAB2Cache.surface_normal_estimation (RTAB_utils/ios_rtab.py:236-248), for F frames of n points at once.
//
// The radius graph's grid (f3d_graph.hip), with the frame folded into the cell key so that one sort serves the whole batch:
//   bbox               : f3d_launch_graph_bbox over all F * n points (the caller's one readback: grid + non-finite check)
//   k_nrm_keys         : key = (frame, cz, cy, cx) packed into <= 64 bits, idx = f * n + i
//   rocprim radix sort : (key, idx) -> cell order; stable, so indices ascend inside a cell
//   k_nrm_gather       : sorted float64 copy (candidate loops read it contiguously)
//   k_nrm_query<K>     : one thread per point, in cell order.  No per-cell table: frame f owns sorted positions [f n, (f + 1) n), and
//                        the three cells (cx - 1 .. cx + 1) of one (dy, dz) row are consecutive keys, so each of the 9 rows is one
//                        contiguous range found by two binary searches.  Memory is bounded by the number of points, not the extent.
// Selection keeps the max_nn smallest (d2, j) in a sorted register array of K >= max_nn slots, updated by a compile-time-unrolled
// insertion network (no runtime-indexed arrays: they would live in scratch).  The first max_nn slots are the answer.
// A zero-depth cluster (every dropout pixel unprojects to the camera centre) sits in one cell: the own cell is scanned first, in
// ascending index, and once max_nn candidates at d2 == 0 are kept nothing later in that cell can enter -- the scan stops there.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include <rocprim/device/device_radix_sort.hpp>
#include "f3d.h"
#include "f3d_kernels.h"
#include "f3d_eigen.h"

#pragma clang fp contract(off)

namespace {

constexpr int NB = 128;

__device__ __forceinline__ uint64_t pack_key(const f3d_nrmgrid& g, uint64_t f, int cx, int cy, int cz) {
    return (f << g.shift[3]) | ((uint64_t)cz << g.shift[2]) | ((uint64_t)cy << g.shift[1]) | (uint64_t)cx;
}

__global__ __launch_bounds__(256) void k_nrm_keys(const double* __restrict__ xyz, int64_t n, int64_t total, f3d_nrmgrid g,
                                                   uint64_t* __restrict__ keys, uint32_t* __restrict__ idx) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        int cx, cy, cz;
        f3d_cell_of(g, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], cx, cy, cz);
        keys[i] = pack_key(g, (uint64_t)(i / n), cx, cy, cz);
        idx[i] = (uint32_t)i;
    }
}

__global__ __launch_bounds__(256) void k_nrm_gather(const double* __restrict__ xyz, int64_t total, const uint32_t* __restrict__ perm,
                                                     double* __restrict__ sorted) {
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < total; j += (int64_t)gridDim.x * 256) {
        const int64_t i = perm[j];
        sorted[3 * j] = xyz[3 * i]; sorted[3 * j + 1] = xyz[3 * i + 1]; sorted[3 * j + 2] = xyz[3 * i + 2];
    }
}

// first position in [a, b) whose key is >= k
__device__ __forceinline__ int64_t lower_bound(const uint64_t* __restrict__ keys, int64_t a, int64_t b, uint64_t k) {
    while (a < b) {
        const int64_t m = a + ((b - a) >> 1);
        if (keys[m] < k) a = m + 1; else b = m;
    }
    return a;
}

// selection: topk<K> (f3d_kernels.h)
template <int K>
__global__ __launch_bounds__(NB) void k_nrm_query(const double* __restrict__ xyz, const double* __restrict__ sorted,
                                                   const uint64_t* __restrict__ skeys, const uint32_t* __restrict__ perm, int64_t n,
                                                   int64_t total, f3d_nrmgrid g, double r2, int max_nn, const double* __restrict__ cams,
                                                   int orient, double* __restrict__ normals, int32_t* __restrict__ counts,
                                                   int32_t* __restrict__ nbrs) {
    for (int64_t j = (int64_t)blockIdx.x * NB + threadIdx.x; j < total; j += (int64_t)gridDim.x * NB) {
        const double px = sorted[3 * j], py = sorted[3 * j + 1], pz = sorted[3 * j + 2];
        const int64_t gi = perm[j];
        const int64_t f = gi / n, base = f * n;
        int cx, cy, cz;
        f3d_cell_of(g, px, py, pz, cx, cy, cz);
        const uint64_t own = pack_key(g, (uint64_t)f, cx, cy, cz);
        const int64_t flo = base, fhi = base + n;                  // frame f's sorted positions
        topk<K> top;
        top.init();
        int64_t inside = 0;                                       // candidates with d2 < r2 that were visited
        int zeros = 0;
        const int64_t oa = lower_bound(skeys, flo, fhi, own), ob = lower_bound(skeys, oa, fhi, own + 1);
        // r = -1: the own cell; r = 0 .. 8: the (dz, dy) rows, the middle one without the own cell (two pieces).  One candidate
        // loop for all of them: a single copy of the insertion network in the code.
#pragma nounroll
        for (int r = -1; r < 9; ++r) {
            int64_t a = oa, b = ob, a2 = 0, b2 = 0;
            if (r >= 0) {
                const int dz = r / 3 - 1, dy = r % 3 - 1, z = cz + dz, y = cy + dy;
                if (z < 0 || z >= g.dim[2] || y < 0 || y >= g.dim[1]) continue;
                const uint64_t klo = pack_key(g, (uint64_t)f, max(cx - 1, 0), y, z), khi = pack_key(g, (uint64_t)f, min(cx + 1, g.dim[0] - 1), y, z);
                a = lower_bound(skeys, flo, fhi, klo);
                b = lower_bound(skeys, a, fhi, khi + 1);
                if (dz == 0 && dy == 0) { a2 = ob; b2 = b; b = oa; }
            }
#pragma nounroll
            for (int64_t k = a;; ++k) {
                if (k >= b) {
                    if (a2 >= b2) break;
                    k = a2; b = b2; a2 = b2;
                }
                const double t0 = px - sorted[3 * k], t1 = py - sorted[3 * k + 1], t2 = pz - sorted[3 * k + 2];
                const double d2 = (t0 * t0 + t1 * t1) + t2 * t2;
                if (d2 < r2) {
                    ++inside;
                    top.insert(d2, (int)((int64_t)perm[k] - base));
                    // own cell in ascending index: after max_nn candidates at distance 0 nothing later in it can be kept
                    if (r < 0 && d2 == 0.0 && ++zeros >= max_nn) break;
                }
            }
        }
        const int kept = inside < max_nn ? (int)inside : max_nn;
        if (counts) counts[gi] = kept;
        if (nbrs) {
            int32_t* row = nbrs + gi * max_nn;
#pragma unroll
            for (int s = 0; s < K; ++s)
                if (s < max_nn) row[s] = s < kept ? top.j[s] : -1;
        }
        double nx = 0.0, ny = 0.0, nz = 1.0;
        if (kept >= 3) {
            // Open3D's cumulants over the kept set, in (d2, j) order; degenerate when every kept point is bit-identical to the first
            const double* q0 = xyz + 3 * (base + top.j[0]);
            const double x0 = q0[0], y0 = q0[1], z0 = q0[2];
            double s0 = 0, s1 = 0, s2 = 0, s00 = 0, s01 = 0, s02 = 0, s11 = 0, s12 = 0, s22 = 0;
            bool same = true;
#pragma unroll
            for (int s = 0; s < K; ++s) {
                if (s < kept) {
                    const double* q = xyz + 3 * (base + top.j[s]);
                    const double x = q[0], y = q[1], z = q[2];
                    same = same && __double_as_longlong(x) == __double_as_longlong(x0) && __double_as_longlong(y) == __double_as_longlong(y0) &&
                           __double_as_longlong(z) == __double_as_longlong(z0);
                    s0 += x; s1 += y; s2 += z;
                    s00 += x * x; s01 += x * y; s02 += x * z; s11 += y * y; s12 += y * z; s22 += z * z;
                }
            }
            if (!same) {
                const double m = (double)kept;
                s0 /= m; s1 /= m; s2 /= m; s00 /= m; s01 /= m; s02 /= m; s11 /= m; s12 /= m; s22 /= m;
                const double c00 = s00 - s0 * s0, c01 = s01 - s0 * s1, c02 = s02 - s0 * s2;
                const double c11 = s11 - s1 * s1, c12 = s12 - s1 * s2, c22 = s22 - s2 * s2;
                if (c00 != 0.0 || c01 != 0.0 || c02 != 0.0 || c11 != 0.0 || c12 != 0.0 || c22 != 0.0) {   // a vanishing covariance: (0, 0, 1)
                    double w[3], V[9];
                    jacobi3(c00, c01, c02, c11, c12, c22, w, V);
                    const int e = (w[1] < w[0]) ? (w[2] < w[1] ? 2 : 1) : (w[2] < w[0] ? 2 : 0);
                    const double vx = e == 0 ? V[0] : e == 1 ? V[1] : V[2];
                    const double vy = e == 0 ? V[3] : e == 1 ? V[4] : V[5];
                    const double vz = e == 0 ? V[6] : e == 1 ? V[7] : V[8];
                    const double len = sqrt((vx * vx + vy * vy) + vz * vz);
                    nx = vx / len; ny = vy / len; nz = vz / len;
                }
            }
        }
        if (orient) {
            // ios_rtab.py:242-246: direction = (p - c) / norm(p - c); flipped when dot(n, direction) > 0 (NaN for p == c: kept)
            const double dx = px - cams[3 * f], dy = py - cams[3 * f + 1], dz = pz - cams[3 * f + 2];
            const double mag = sqrt((dx * dx + dy * dy) + dz * dz);
            const double ux = dx / mag, uy = dy / mag, uz = dz / mag;
            if ((nx * ux + ny * uy) + nz * uz > 0.0) { nx = -nx; ny = -ny; nz = -nz; }
        }
        normals[3 * gi] = nx; normals[3 * gi + 1] = ny; normals[3 * gi + 2] = nz;
    }
}

struct nrm_layout { size_t keys_a, keys_b, idx_a, perm, sorted, temp, total; };

nrm_layout layout_for(int64_t total, size_t temp_bytes) {
    nrm_layout L;
    f3d_carve c;
    L.keys_a = c.take((size_t)total * 8); L.keys_b = c.take((size_t)total * 8); L.idx_a = c.take((size_t)total * 4); L.perm = c.take((size_t)total * 4);
    L.sorted = c.take((size_t)total * 24); L.temp = c.take(temp_bytes);
    L.total = c.off;
    return L;
}

size_t temp_bytes_for(int64_t total) {
    size_t a = 0;
    (void)rocprim::radix_sort_pairs(nullptr, a, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, (size_t)total, 0u, 64u);
    return a + 256;
}

}  // namespace

size_t f3d_normals_scratch_bytes(int64_t total) { return layout_for(total, temp_bytes_for(total)).total; }

// enqueue only: the grid was chosen by the caller from the bounding box; cams: device [F, 3] (unread when orient == 0)
hipError_t f3d_launch_normals(const double* xyz, int nframes, int64_t n, const f3d_nrmgrid& g, double r2, int max_nn, const double* cams,
                              int orient, void* scratch, double* normals, int32_t* counts, int32_t* nbrs, hipStream_t s) {
    const int64_t total = (int64_t)nframes * n;
    const size_t tb = temp_bytes_for(total);
    const nrm_layout L = layout_for(total, tb);
    char* base = (char*)scratch;
    uint64_t *ka = (uint64_t*)(base + L.keys_a), *kb = (uint64_t*)(base + L.keys_b);
    uint32_t *ia = (uint32_t*)(base + L.idx_a), *perm = (uint32_t*)(base + L.perm);
    double* sorted = (double*)(base + L.sorted);
    hipLaunchKernelGGL(k_nrm_keys, dim3(f3d_grid_for(total, 256, 65536)), dim3(256), 0, s, xyz, n, total, g, ka, ia);
    size_t t = tb;
    hipError_t e = rocprim::radix_sort_pairs(base + L.temp, t, ka, kb, ia, perm, (size_t)total, 0u, (unsigned)g.key_bits, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_nrm_gather, dim3(f3d_grid_for(total, 256, 65536)), dim3(256), 0, s, xyz, total, perm, sorted);
    const dim3 gr(f3d_grid_for(total, NB, 65536)), b(NB);
    if (max_nn <= 8)
        hipLaunchKernelGGL(k_nrm_query<8>, gr, b, 0, s, xyz, sorted, kb, perm, n, total, g, r2, max_nn, cams, orient, normals, counts, nbrs);
    else if (max_nn <= 32)
        hipLaunchKernelGGL(k_nrm_query<32>, gr, b, 0, s, xyz, sorted, kb, perm, n, total, g, r2, max_nn, cams, orient, normals, counts, nbrs);
    else
        hipLaunchKernelGGL(k_nrm_query<F3D_NORMALS_MAX_NN>, gr, b, 0, s, xyz, sorted, kb, perm, n, total, g, r2, max_nn, cams, orient, normals,
                           counts, nbrs);
    return hipGetLastError();
}
