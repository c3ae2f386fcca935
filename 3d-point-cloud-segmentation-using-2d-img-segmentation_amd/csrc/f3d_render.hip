// Point-splat z-buffer of a posed cloud (include/f3d.h "occlusion-aware forward voting"): per-view depth keys, the lookups made
// from them, and the forward vote restricted to the samples near the front surface of their pixel.
//
// A sample is a (point, view) pair that passes the canonical arithmetic of k_project_view (f3d_math.h: 5 planes, projection,
// floor) and lands in the image with a normal positive float32 depth.  Its key (float32 depth bits << 32 | point index) is a
// monotone unsigned integer, so the z-buffer is one 64-bit atomicMin per covered cell and the result is the same whatever the
// order of the threads: nearest depth first, lowest index on ties.
#include <hip/hip_runtime.h>
#include <float.h>
#include <stdint.h>
#include "f3d.h"
#include "f3d_math.h"
#include "f3d_kernels.h"

#pragma clang fp contract(off)

namespace {

#define F3D_ZKEY_EMPTY (~0ull)

__global__ __launch_bounds__(F3D_BLOCK) void k_zkey_fill(unsigned long long* __restrict__ zkey, size_t cells) {
    for (size_t i = (size_t)blockIdx.x * F3D_BLOCK + threadIdx.x; i < cells; i += (size_t)gridDim.x * F3D_BLOCK) zkey[i] = F3D_ZKEY_EMPTY;
}

// One thread per point, blockIdx.y = view of the pass (the view record is wave-uniform: scalar loads).  A cell is read before the
// atomic and the atomic skipped when the cell already holds a smaller key: under contention most samples lose, and min is
// idempotent.  The read is an agent-scope atomic load (L2): a stale larger value would only cost a needless atomic, never a result.
// counts (STATS only): {samples, cells covered, atomics issued}.
template <typename T, bool STATS>
__global__ __launch_bounds__(F3D_BLOCK) void k_zsplat(const T* __restrict__ xyz, int64_t n, const f3d_view* __restrict__ views, int h, int w,
                                                       int splat, unsigned long long* __restrict__ zkey, unsigned long long* __restrict__ counts) {
    const f3d_view& vw = views[blockIdx.y];
    unsigned long long* plane = zkey + (size_t)blockIdx.y * h * w;
    unsigned long long nsamples = 0, ncells = 0, natomics = 0;
    for (int64_t i = (int64_t)blockIdx.x * F3D_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * F3D_BLOCK) {
        int u, v;
        float z32;
        if (!f3d_sample(vw, f3d_load_p3(xyz, i), h, w, u, v, z32)) continue;
        const unsigned long long key = (unsigned long long)__float_as_uint(z32) << 32 | (unsigned long long)(uint32_t)i;
        const int r0 = max(v - splat, 0), r1 = min(v + splat, h - 1), c0 = max(u - splat, 0), c1 = min(u + splat, w - 1);
        if (STATS) { ++nsamples; ncells += (unsigned long long)(r1 - r0 + 1) * (c1 - c0 + 1); }
        for (int r = r0; r <= r1; ++r) {
            unsigned long long* row = plane + (size_t)r * w;
            for (int c = c0; c <= c1; ++c) {
                if (__hip_atomic_load(row + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= key) continue;
                __hip_atomic_fetch_min(row + c, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (STATS) ++natomics;
            }
        }
    }
    if (STATS) {
        if (nsamples) atomicAdd(counts, nsamples);
        if (ncells) atomicAdd(counts + 1, ncells);
        if (natomics) atomicAdd(counts + 2, natomics);
    }
}

// keys -> the lookups: depth = the winning z32 (+inf for an empty cell), uv2pt = the winning index (-1)
__global__ __launch_bounds__(F3D_BLOCK) void k_zkey_unpack(const unsigned long long* __restrict__ zkey, size_t cells, float* __restrict__ depth,
                                                            int32_t* __restrict__ uv2pt, const int* __restrict__ skip) {
    if (skip && *skip) return;
    for (size_t i = (size_t)blockIdx.x * F3D_BLOCK + threadIdx.x; i < cells; i += (size_t)gridDim.x * F3D_BLOCK) {
        const unsigned long long key = zkey[i];
        const bool empty = key == F3D_ZKEY_EMPTY;
        if (depth) depth[i] = empty ? INFINITY : __uint_as_float((uint32_t)(key >> 32));
        if (uv2pt) uv2pt[i] = empty ? -1 : (int32_t)(uint32_t)key;
    }
}

// One thread per point, looping over the views of the pass (uniform index: scalar loads of the record).  The thread owns its vote
// row: plain float64 read-modify-writes, exact counts.  masks = the plane of the pass's first view.  MESH: the keys are a mesh's
// (f3d_raster.hip), so the sample's own cell may be empty -- nothing in front of it, +inf -- and *mesh_flag set means a bad mesh.
template <typename T, bool MESH>
__global__ __launch_bounds__(F3D_BLOCK) void k_vote_visible(const T* __restrict__ xyz, int64_t n, const f3d_view* __restrict__ views, int nv,
                                                             const uint8_t* __restrict__ masks, int h, int w,
                                                             const unsigned long long* __restrict__ zkey, double depth_tol,
                                                             double* __restrict__ votes, int ncols, const int* __restrict__ mesh_flag,
                                                             int* __restrict__ err) {
    if (MESH && *mesh_flag) return;
    const size_t hw = (size_t)h * w;
    for (int64_t i = (int64_t)blockIdx.x * F3D_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * F3D_BLOCK) {
        const f3d_p3 p = f3d_load_p3(xyz, i);
        double* row = votes + (size_t)i * ncols;
        for (int j = 0; j < nv; ++j) {
            int u, v;
            float z32;
            if (!f3d_sample(views[j], p, h, w, u, v, z32)) continue;
            const size_t cell = (size_t)j * hw + (size_t)v * w + u;
            const unsigned long long key = zkey[cell];
            const float zmin32 = MESH && key == F3D_ZKEY_EMPTY ? INFINITY : __uint_as_float((uint32_t)(key >> 32));   // !MESH: never empty, this sample covers the cell
            if (!((double)z32 <= (double)zmin32 + depth_tol)) continue;
            const int label = masks[cell];
            if (label >= ncols) { atomicOr(err, F3D_DEVERR_ZVOTE); continue; }      // the reference's IndexError (voting.py:98)
            row[label] += 1.0;
        }
    }
}

}  // namespace

hipError_t f3d_launch_zkey_fill(unsigned long long* zkey, size_t cells, hipStream_t s) {
    if (!cells) return hipSuccess;
    hipLaunchKernelGGL(k_zkey_fill, dim3(f3d_grid_for((int64_t)cells, F3D_BLOCK, F3D_GRID_CAP)), dim3(F3D_BLOCK), 0, s, zkey, cells);
    return hipGetLastError();
}

hipError_t f3d_launch_zsplat(const void* xyz, int dtype, int64_t n, const f3d_view* views_dev, int nv, int h, int w, int splat,
                             unsigned long long* zkey, unsigned long long* counts, hipStream_t s) {
    if (n <= 0 || nv <= 0) return hipSuccess;
    const int cap = (F3D_GRID_CAP + nv - 1) / nv;
    const dim3 g(f3d_grid_for(n, F3D_BLOCK, cap < 64 ? 64 : cap), nv), b(F3D_BLOCK);
#define F3D_ZS(T, S) hipLaunchKernelGGL((k_zsplat<T, S>), g, b, 0, s, (const T*)xyz, n, views_dev, h, w, splat, zkey, counts)
    if (dtype == F3D_F64) { if (counts) F3D_ZS(double, true); else F3D_ZS(double, false); }
    else { if (counts) F3D_ZS(float, true); else F3D_ZS(float, false); }
#undef F3D_ZS
    return hipGetLastError();
}

hipError_t f3d_launch_zkey_unpack(const unsigned long long* zkey, size_t cells, float* depth, int32_t* uv2pt, const int* skip, hipStream_t s) {
    if (!cells || (!depth && !uv2pt)) return hipSuccess;
    hipLaunchKernelGGL(k_zkey_unpack, dim3(f3d_grid_for((int64_t)cells, F3D_BLOCK, F3D_GRID_CAP)), dim3(F3D_BLOCK), 0, s, zkey, cells, depth, uv2pt, skip);
    return hipGetLastError();
}

hipError_t f3d_launch_vote_visible(const void* xyz, int dtype, int64_t n, const f3d_view* views_dev, int nv, const uint8_t* masks, int h, int w,
                                   const unsigned long long* zkey, double depth_tol, double* votes, int ncols, const int* mesh_flag, int* err,
                                   hipStream_t s) {
    if (n <= 0 || nv <= 0) return hipSuccess;
    const dim3 g(f3d_grid_for(n, F3D_BLOCK, F3D_GRID_CAP)), b(F3D_BLOCK);
#define F3D_VV(T, M) hipLaunchKernelGGL((k_vote_visible<T, M>), g, b, 0, s, (const T*)xyz, n, views_dev, nv, masks, h, w, zkey, depth_tol, votes, ncols, mesh_flag, err)
    if (dtype == F3D_F64) { if (mesh_flag) F3D_VV(double, true); else F3D_VV(double, false); }
    else { if (mesh_flag) F3D_VV(float, true); else F3D_VV(float, false); }
#undef F3D_VV
    return hipGetLastError();
}
