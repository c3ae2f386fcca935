// The per-frame bookkeeping of Fusion.fuse (Fusion3DSeg/fusion.py) on a device-resident cloud: what Fusion.fuse_device runs
// between the projection of the cloud (k_project_view) and the patch kernels of f3d_patch.hip, so that no per-point or per-pixel
// array goes back to the host.
//
//   k_fu_hit_flags / scan / k_fu_hits : order-preserving compaction of the in-frustum flags -> hit ids, uv [2,m], their rows
//   k_fu_seed_update                  : the matches of a frame applied in place to the resident rows ids[k]
//   k_fu_lookup                       : uv2pt[p] = ids[owner[p]], taken pixels leave the free mask
//   k_fu_check                        : free pixels left, and whether one of them fails its own test (sequential fallback)
//   k_fu_prio                         : prio[order[i]] = i of the host's shuffle
//   k_fu_seed_flags / scan / k_fu_seed_rows / k_fu_seed_lookup / k_fu_seed_count : patch_downsample's new seeds appended in
//                                       visiting order at base + rank, their pixels' lookups, the new cloud count
//
// Means and normalisation are written as fusion.py reads them (the library builds with -ffp-contract=off):
//   matched seed  (ordered member sum + seed row) / (n + 1),  new seed  ordered member sum / n,
//   normal / sqrt(v.dot(v)) with the dot in the host BLAS's order (F3D_NORM_PLAIN / F3D_NORM_FMA), or left unnormalised for
//   the host (F3D_NORM_HOST).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <rocprim/device/device_scan.hpp>
#include "f3d.h"
#include "f3d_kernels.h"

namespace {

constexpr int FB = 256;

// nsum / np.linalg.norm(nsum) of a 1-D vector: sqrt(v.dot(v)), the dot in `mode`'s order
__device__ __forceinline__ void normalise(double v[3], int mode) {
    if (mode == F3D_NORM_HOST) return;
    double dd;
    if (mode == F3D_NORM_FMA) dd = __fma_rn(v[2], v[2], __fma_rn(v[1], v[1], v[0] * v[0]));
    else dd = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
    const double nr = sqrt(dd);
    v[0] = v[0] / nr; v[1] = v[1] / nr; v[2] = v[2] / nr;
}

// sums `value` over the block into *out (one atomic per block)
__device__ __forceinline__ void block_add(unsigned long long value, unsigned long long* out) {
    __shared__ unsigned long long part[FB / 64];
    for (int o = 32; o > 0; o >>= 1) value += __shfl_down(value, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = value;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
        for (int k = 0; k < FB / 64; ++k) t += part[k];
        if (t) atomicAdd(out, t);
    }
}

// ---- hits: flags[i] = inside[i] for the rows of the cloud (rows at or beyond *count are spare capacity), flags[n] = 0
__global__ __launch_bounds__(FB) void k_fu_hit_flags(const uint8_t* __restrict__ inside, int64_t n, const int64_t* __restrict__ count,
                                                      int32_t* __restrict__ flags) {
    const int64_t live = *count;
    for (int64_t i = (int64_t)blockIdx.x * FB + threadIdx.x; i <= n; i += (int64_t)gridDim.x * FB)
        flags[i] = (i < n && i < live && inside[i]) ? 1 : 0;
}

__global__ __launch_bounds__(FB) void k_fu_hits(const int32_t* __restrict__ flags, const int32_t* __restrict__ offs, int64_t n,
                                                 const int32_t* __restrict__ uv_all, const double* __restrict__ pts, const double* __restrict__ nrm,
                                                 int32_t* __restrict__ ids, int32_t* __restrict__ uv, double* __restrict__ hit_pts,
                                                 double* __restrict__ hit_nrm) {
    const int64_t m = offs[n];
    for (int64_t i = (int64_t)blockIdx.x * FB + threadIdx.x; i < n; i += (int64_t)gridDim.x * FB) {
        if (!flags[i]) continue;
        const int64_t r = offs[i];
        ids[r] = (int32_t)i;
        uv[r] = uv_all[i];
        uv[m + r] = uv_all[n + i];
        for (int c = 0; c < 3; ++c) { hit_pts[3 * r + c] = pts[3 * i + c]; hit_nrm[3 * r + c] = nrm[3 * i + c]; }
    }
}

// stats[0] = hits, stats[1] = valid pixels of the frame (pre-zeroed), stats[2] = cloud rows
__global__ __launch_bounds__(FB) void k_fu_hit_stats(const int32_t* __restrict__ offs, int64_t n, const int64_t* __restrict__ count,
                                                      const uint8_t* __restrict__ valid, int64_t npx, int64_t* __restrict__ stats) {
    unsigned long long mine = 0;
    for (int64_t p = (int64_t)blockIdx.x * FB + threadIdx.x; p < npx; p += (int64_t)gridDim.x * FB) mine += valid[p] != 0;
    block_add(mine, (unsigned long long*)&stats[1]);
    if (blockIdx.x == 0 && threadIdx.x == 0) { stats[0] = offs[n]; stats[2] = *count; }
}

// ---- the matches of one frame (fusion.py, Fusion.fuse: x_pts[seeds] = (sums + x_pts) / (n + 1), ...)
__global__ __launch_bounds__(FB) void k_fu_seed_update(const int32_t* __restrict__ ids, int64_t m, const double* __restrict__ sums,
                                                        const int32_t* __restrict__ counts, int mode, double* __restrict__ pts,
                                                        double* __restrict__ nrm, double* __restrict__ clr, int64_t* __restrict__ nmerges,
                                                        uint32_t* __restrict__ occ) {
    for (int64_t k = (int64_t)blockIdx.x * FB + threadIdx.x; k < m; k += (int64_t)gridDim.x * FB) {
        const int n = counts[k];
        if (n == 0) continue;
        const int64_t row = ids[k];
        const double denom = (double)((int64_t)n + 1);
        const double* s = sums + 9 * k;
        double v[3];
        for (int c = 0; c < 3; ++c) {
            pts[3 * row + c] = (s[c] + pts[3 * row + c]) / denom;
            clr[3 * row + c] = (s[6 + c] + clr[3 * row + c]) / denom;
            v[c] = (s[3 + c] + nrm[3 * row + c]) / denom;
        }
        normalise(v, mode);
        for (int c = 0; c < 3; ++c) nrm[3 * row + c] = v[c];
        nmerges[row] += n;
        occ[row] += 1u;
    }
}

__global__ __launch_bounds__(FB) void k_fu_lookup(const int32_t* __restrict__ owner, const int32_t* __restrict__ ids, int64_t npx,
                                                   int32_t* __restrict__ uv2pt, uint8_t* __restrict__ free_px) {
    for (int64_t p = (int64_t)blockIdx.x * FB + threadIdx.x; p < npx; p += (int64_t)gridDim.x * FB) {
        const int o = owner[p];
        uv2pt[p] = o >= 0 ? ids[o] : -1;
        if (o >= 0) free_px[p] = 0;
    }
}

// ---- patch_downsample's guard (fusion.py): own_cos = einsum('ij,ij->i', normals, normals), usable = own_cos > min_cosine and a
// finite point; a free pixel that is not usable sends the frame down the sequential path.  stats[0] = free pixels, stats[1] = flag
__global__ __launch_bounds__(FB) void k_fu_check(const uint8_t* __restrict__ free_px, const double* __restrict__ pts, const double* __restrict__ nrm,
                                                  int64_t npx, double radius, double min_cosine, int64_t* __restrict__ stats) {
    unsigned long long nfree = 0;
    bool bad = blockIdx.x == 0 && threadIdx.x == 0 && !(radius > 0);        // patch_downsample's `not (max_distance > 0)`
    for (int64_t p = (int64_t)blockIdx.x * FB + threadIdx.x; p < npx; p += (int64_t)gridDim.x * FB) {
        if (!free_px[p]) continue;
        ++nfree;
        const double n0 = nrm[3 * p], n1 = nrm[3 * p + 1], n2 = nrm[3 * p + 2];
        const double own = (n0 * n0 + n1 * n1) + n2 * n2;
        const bool finite = isfinite(pts[3 * p]) && isfinite(pts[3 * p + 1]) && isfinite(pts[3 * p + 2]);
        if (!(own > min_cosine) || !finite) bad = true;
    }
    if (bad) atomicOr((unsigned long long*)&stats[1], 1ull);
    block_add(nfree, (unsigned long long*)&stats[0]);
}

__global__ __launch_bounds__(FB) void k_fu_prio(const int64_t* __restrict__ order, int64_t npx, int32_t* __restrict__ prio) {
    for (int64_t i = (int64_t)blockIdx.x * FB + threadIdx.x; i < npx; i += (int64_t)gridDim.x * FB) {
        const int64_t p = order[i];
        if (p >= 0 && p < npx) prio[p] = (int32_t)i;
    }
}

// ---- new seeds: rank in visiting order = exclusive scan of "the pixel visited at position i is a seed"
__global__ __launch_bounds__(FB) void k_fu_seed_flags(const int32_t* __restrict__ owner, const int32_t* __restrict__ prio, int64_t npx,
                                                       int32_t* __restrict__ flags) {
    for (int64_t p = (int64_t)blockIdx.x * FB + threadIdx.x; p <= npx; p += (int64_t)gridDim.x * FB) {
        if (p == npx) { flags[npx] = 0; continue; }
        const int32_t at = prio[p];
        if (at >= 0 && at < npx) flags[at] = owner[p] == (int32_t)p ? 1 : 0;
    }
}

__global__ __launch_bounds__(FB) void k_fu_seed_rows(const int32_t* __restrict__ owner, const int32_t* __restrict__ prio,
                                                      const int32_t* __restrict__ rank, const double* __restrict__ sums,
                                                      const int32_t* __restrict__ counts, int64_t npx, int mode, const int64_t* __restrict__ count,
                                                      int64_t cap, double* __restrict__ pts, double* __restrict__ nrm, double* __restrict__ clr,
                                                      int64_t* __restrict__ nmerges, uint32_t* __restrict__ occ) {
    const int64_t base = *count;
    for (int64_t p = (int64_t)blockIdx.x * FB + threadIdx.x; p < npx; p += (int64_t)gridDim.x * FB) {
        if (owner[p] != (int32_t)p) continue;
        const int64_t row = base + rank[prio[p]];
        if (row >= cap) continue;                                            // the caller reserves count + h*w rows
        const int n = counts[p];
        const double denom = (double)(int64_t)n;
        const double* s = sums + 9 * p;
        double v[3];
        for (int c = 0; c < 3; ++c) {
            pts[3 * row + c] = s[c] / denom;
            clr[3 * row + c] = s[6 + c] / denom;
            v[c] = s[3 + c] / denom;
        }
        normalise(v, mode);
        for (int c = 0; c < 3; ++c) nrm[3 * row + c] = v[c];
        nmerges[row] = n;
        occ[row] = 1u;
    }
}

__global__ __launch_bounds__(FB) void k_fu_seed_lookup(const int32_t* __restrict__ owner, const int32_t* __restrict__ prio,
                                                        const int32_t* __restrict__ rank, int64_t npx, const int64_t* __restrict__ count,
                                                        int32_t* __restrict__ uv2pt, uint8_t* __restrict__ free_px) {
    const int64_t base = *count;
    for (int64_t p = (int64_t)blockIdx.x * FB + threadIdx.x; p < npx; p += (int64_t)gridDim.x * FB) {
        const int o = owner[p];
        if (o < 0) continue;
        uv2pt[p] = (int32_t)(base + rank[prio[o]]);
        free_px[p] = 0;
    }
}

__global__ void k_fu_seed_count(const int32_t* __restrict__ rank, int64_t npx, int64_t* __restrict__ count) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *count += rank[npx];
}

size_t scan_temp(int64_t n) {
    size_t b = 0;
    (void)rocprim::exclusive_scan(nullptr, b, (int32_t*)nullptr, (int32_t*)nullptr, (int32_t)0, (size_t)n + 1, rocprim::plus<int32_t>());
    return b + 256;
}

// compaction of n + 1 flags: the flags, their exclusive scan, the scan's temporary storage
struct compact_layout { size_t flags, scan, temp, temp_bytes, total; };

compact_layout layout_for(int64_t n) {
    compact_layout L;
    f3d_carve c;
    L.flags = c.take((size_t)(n + 1) * 4); L.scan = c.take((size_t)(n + 1) * 4);
    L.temp_bytes = scan_temp(n); L.temp = c.take(L.temp_bytes);
    L.total = c.off;
    return L;
}

}  // namespace

size_t f3d_fusion_scratch_bytes(int64_t n) { return layout_for(n).total; }

hipError_t f3d_launch_fusion_hits(const uint8_t* inside, const int32_t* uv_all, int64_t n, const int64_t* count, const double* pts,
                                  const double* nrm, const uint8_t* valid, int64_t npx, int32_t* ids, int32_t* uv, double* hit_pts,
                                  double* hit_nrm, int64_t* stats, void* scratch, hipStream_t s) {
    const compact_layout L = layout_for(n);
    char* base = (char*)scratch;
    int32_t *flags = (int32_t*)(base + L.flags), *offs = (int32_t*)(base + L.scan);
    hipError_t e = hipMemsetAsync(stats, 0, 3 * sizeof(int64_t), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_fu_hit_flags, dim3(f3d_grid_for(n + 1, FB, 8192)), dim3(FB), 0, s, inside, n, count, flags);
    size_t t = L.temp_bytes;
    e = rocprim::exclusive_scan(base + L.temp, t, flags, offs, (int32_t)0, (size_t)n + 1, rocprim::plus<int32_t>(), s);
    if (e != hipSuccess) return e;
    if (n > 0) hipLaunchKernelGGL(k_fu_hits, dim3(f3d_grid_for(n, FB, 8192)), dim3(FB), 0, s, flags, offs, n, uv_all, pts, nrm, ids, uv, hit_pts, hit_nrm);
    hipLaunchKernelGGL(k_fu_hit_stats, dim3(f3d_grid_for(npx, FB, 8192)), dim3(FB), 0, s, offs, n, count, valid, npx, stats);
    return hipGetLastError();
}

hipError_t f3d_launch_fusion_seed_update(const int32_t* ids, int64_t m, const double* sums, const int32_t* counts, int mode, double* pts,
                                         double* nrm, double* clr, int64_t* nmerges, uint32_t* occ, hipStream_t s) {
    if (m <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_fu_seed_update, dim3(f3d_grid_for(m, FB, 8192)), dim3(FB), 0, s, ids, m, sums, counts, mode, pts, nrm, clr, nmerges, occ);
    return hipGetLastError();
}

hipError_t f3d_launch_fusion_lookup(const int32_t* owner, const int32_t* ids, int64_t npx, int32_t* uv2pt, uint8_t* free_px, hipStream_t s) {
    if (npx <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_fu_lookup, dim3(f3d_grid_for(npx, FB, 8192)), dim3(FB), 0, s, owner, ids, npx, uv2pt, free_px);
    return hipGetLastError();
}

hipError_t f3d_launch_fusion_check(const uint8_t* free_px, const double* pts, const double* nrm, int64_t npx, double radius,
                                   double min_cosine, int64_t* stats, hipStream_t s) {
    hipError_t e = hipMemsetAsync(stats, 0, 2 * sizeof(int64_t), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_fu_check, dim3(f3d_grid_for(npx, FB, 8192)), dim3(FB), 0, s, free_px, pts, nrm, npx, radius, min_cosine, stats);
    return hipGetLastError();
}

hipError_t f3d_launch_fusion_prio(const int64_t* order, int64_t npx, int32_t* prio, hipStream_t s) {
    if (npx <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_fu_prio, dim3(f3d_grid_for(npx, FB, 8192)), dim3(FB), 0, s, order, npx, prio);
    return hipGetLastError();
}

hipError_t f3d_launch_fusion_new_seeds(const int32_t* owner, const int32_t* prio, const double* sums, const int32_t* counts, int64_t npx,
                                       int mode, int64_t* count, int64_t cap, double* pts, double* nrm, double* clr, int64_t* nmerges,
                                       uint32_t* occ, int32_t* uv2pt, uint8_t* free_px, void* scratch, hipStream_t s) {
    if (npx <= 0) return hipSuccess;
    const compact_layout L = layout_for(npx);
    char* base = (char*)scratch;
    int32_t *flags = (int32_t*)(base + L.flags), *rank = (int32_t*)(base + L.scan);
    const dim3 g(f3d_grid_for(npx, FB, 8192)), b(FB);
    hipLaunchKernelGGL(k_fu_seed_flags, dim3(f3d_grid_for(npx + 1, FB, 8192)), b, 0, s, owner, prio, npx, flags);
    size_t t = L.temp_bytes;
    hipError_t e = rocprim::exclusive_scan(base + L.temp, t, flags, rank, (int32_t)0, (size_t)npx + 1, rocprim::plus<int32_t>(), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_fu_seed_rows, g, b, 0, s, owner, prio, rank, sums, counts, npx, mode, (const int64_t*)count, cap, pts, nrm, clr,
                       nmerges, occ);
    hipLaunchKernelGGL(k_fu_seed_lookup, g, b, 0, s, owner, prio, rank, npx, (const int64_t*)count, uv2pt, free_px);
    hipLaunchKernelGGL(k_fu_seed_count, dim3(1), dim3(64), 0, s, rank, npx, count);
    return hipGetLastError();
}
