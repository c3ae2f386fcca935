// Region growing of segUtils/refinement.py (reference :70-400, the four nested floodfill_* functions) and the distance to the
// wall plane that two of them grow over.
//
// One flood is a FIFO breadth-first search whose acceptance test is a running mean carried over the whole flood: a serial chain
// in queue order.  One workgroup runs it, level by level, as k_color_grow (f3d_color.hip) does:
//   * the threads stage the level's queue entries and their values in LDS, a chunk at a time (the first level is the caller's
//     seed list and may be the whole instance: any number of chunks);
//   * lane 0 runs the recurrence in queue order, in the values' dtype, operation for operation as NumPy evaluates it: an entry
//     with |sma - value| > threshold in any channel (compared in float64) is skipped; otherwise it EXPANDS, and unless it is a
//     given seed it is also ACCEPTED: npts += 1, sma = sma + (value - sma) / npts, appended to the cluster;
//   * the threads expand: every neighbour that was never enqueued keeps the minimum of (position of the discoverer among the
//     entries that expand << 32 | position in the discoverer's row) (64-bit atomicMin), and a block scan places the children in
//     that order, which is the reference's FIFO order.
// The key counts the entries that expand, not the accepted ones: a given seed that passes the test enqueues its neighbours
// without being accepted, so the two differ on the first level of the *_dl variants.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "f3d.h"
#include "f3d_kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int GT = 1024;                 // threads of the one workgroup
constexpr int CHUNK = GT;                // queue entries staged in LDS per step of the serial lane
constexpr int IB = 256;

__global__ __launch_bounds__(IB) void k_grow_init(int64_t n, int32_t* __restrict__ inq, unsigned long long* __restrict__ best,
                                                  int64_t* __restrict__ count) {
    for (int64_t i = (int64_t)blockIdx.x * IB + threadIdx.x; i < n; i += (int64_t)gridDim.x * IB) {
        inq[i] = 0;
        best[i] = ~0ull;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *count = 0;
}

template <typename T, int C>
__global__ __launch_bounds__(GT) void k_region_grow(const T* __restrict__ values, int64_t n, const int64_t* __restrict__ offs,
                                                    const int32_t* __restrict__ nbrs, const int64_t* __restrict__ seeds, int64_t nseeds,
                                                    f3d_grow_args a, int32_t* inq, unsigned long long* best, int32_t* qa, int32_t* qb,
                                                    int32_t* xq, int64_t* __restrict__ cluster, int64_t* count, int* err) {
    __shared__ T val[CHUNK * C];
    __shared__ int32_t idx[CHUNK];
    __shared__ int lds[GT];
    __shared__ int s_nq, s_ne, s_bad;
    const int t = threadIdx.x;
    if (t == 0) s_bad = 0;
    __syncthreads();
    // the first queue: the seeds in the caller's order.  A seed out of range, or one that is listed twice (the queue, and with
    // it `cluster`, is sized for every point being enqueued once), is an error and nothing runs.
    int bad = 0;
    for (int64_t k = t; k < nseeds; k += GT) {
        const int64_t v = seeds[k];
        if (v < 0 || v >= n) { bad = 1; continue; }
        if (atomicExch(inq + v, 1) != 0) bad = 1;
        qa[k] = (int32_t)v;
    }
    if (bad) atomicOr(&s_bad, 1);
    if (t == 0) s_nq = (int)nseeds;
    __syncthreads();
    if (s_bad) { if (t == 0) atomicOr(err, F3D_DEVERR_GROW); return; }
    // lane 0 only: the running mean, its point count, and the cluster's length
    T sma[C];
    for (int c = 0; c < C; ++c) sma[c] = (T)a.sma0[c];
    int64_t npts = a.npts0, nc = 0;
    int32_t *q = qa, *qn = qb;
    for (int level = 1; s_nq > 0 && level != a.max_level; ++level) {
        const int nq = s_nq;
        const bool given = level == 1 && a.seeds_given;
        if (t == 0) s_ne = 0;
        // the test and the recurrence, in queue order
        for (int c0 = 0; c0 < nq; c0 += CHUNK) {
            const int m = min(CHUNK, nq - c0);
            if (t < m) {
                const int32_t v = q[c0 + t];
                idx[t] = v;
                for (int c = 0; c < C; ++c) val[t * C + c] = values[(int64_t)v * C + c];
            }
            __syncthreads();
            if (t == 0) {
                int ne = s_ne;
                for (int i = 0; i < m; ++i) {
                    T x[C];
                    bool skip = false;
                    for (int c = 0; c < C; ++c) {
                        x[c] = val[i * C + c];
                        const T d = sma[c] - x[c];
                        skip |= (double)(d < 0 ? -d : d) > a.thr[c];
                    }
                    if (skip) continue;
                    const int32_t v = idx[i];
                    if (!given) {
                        npts += 1;
                        const T den = (T)npts;
                        for (int c = 0; c < C; ++c) sma[c] = sma[c] + (x[c] - sma[c]) / den;
                        cluster[nc++] = v;
                    }
                    xq[ne++] = v;
                }
                s_ne = ne;
            }
            __syncthreads();
        }
        const int ne = s_ne;
        if (level + 1 == a.max_level) break;                               // children would be skipped unseen
        // expand: minimum (expanding position, row position) per neighbour that was never enqueued
        f3d_flood_expand<GT>(xq, ne, offs, nbrs, n, best, err, F3D_DEVERR_GROW, [&](int64_t j) { return inq[j] == 0; });
        __syncthreads();
        // place the children in (expanding position, row position) order
        const int carry = f3d_flood_place<GT>(xq, ne, offs, nbrs, n, best, qn, lds, [&](int64_t j) { inq[j] = 1; });
        if (t == 0) s_nq = carry;
        int32_t* tmp = q; q = qn; qn = tmp;
        __syncthreads();
    }
    if (t == 0) *count = nc;
}

__global__ __launch_bounds__(IB) void k_plane_distance(const double* __restrict__ pts, int64_t n, double px, double py, double pz, double nx,
                                                       double ny, double nz, double* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * IB + threadIdx.x; i < n; i += (int64_t)gridDim.x * IB) {
        const double d = ((pts[i * 3] - px) * nx + (pts[i * 3 + 1] - py) * ny) + (pts[i * 3 + 2] - pz) * nz;
        out[i] = fabs(d);
    }
}

struct grow_layout { size_t inq, best, qa, qb, xq, total; };

grow_layout grow_layout_for(int64_t n) {
    const size_t n4 = (size_t)(n < 1 ? 1 : n) * 4;
    f3d_carve c;                                                         // (a braced list is evaluated left to right)
    return {c.take(n4), c.take(n4 * 2), c.take(n4), c.take(n4), c.take(n4), c.off};
}

}  // namespace

size_t f3d_grow_scratch_bytes(int64_t n) { return grow_layout_for(n).total; }

hipError_t f3d_launch_region_grow(const void* values, int dtype, int nchan, int64_t n, const int64_t* offs, const int32_t* nbrs,
                                  const int64_t* seeds, int64_t nseeds, const f3d_grow_args& a, void* scratch, int64_t* cluster,
                                  int64_t* count_dev, int* err, hipStream_t s) {
    if (n <= 0 || n > F3D_GROW_MAX_POINTS || nseeds < 0 || nseeds > n || !(nchan == 3 || (nchan == 1 && dtype == F3D_F64)))
        return hipErrorInvalidValue;
    const grow_layout L = grow_layout_for(n);
    char* base = (char*)scratch;
    int32_t *inq = (int32_t*)(base + L.inq), *qa = (int32_t*)(base + L.qa), *qb = (int32_t*)(base + L.qb), *xq = (int32_t*)(base + L.xq);
    unsigned long long* best = (unsigned long long*)(base + L.best);
    hipLaunchKernelGGL(k_grow_init, dim3(f3d_grid_for(n, IB, 16384)), dim3(IB), 0, s, n, inq, best, count_dev);
    if (nseeds == 0) return hipGetLastError();
#define F3D_GROW(T, C)                                                                                                                   \
    hipLaunchKernelGGL((k_region_grow<T, C>), dim3(1), dim3(GT), 0, s, (const T*)values, n, offs, nbrs, seeds, nseeds, a, inq, best, qa, \
                       qb, xq, cluster, count_dev, err)
    if (nchan == 1) F3D_GROW(double, 1);
    else if (dtype == F3D_F64) F3D_GROW(double, 3);
    else F3D_GROW(float, 3);
#undef F3D_GROW
    return hipGetLastError();
}

hipError_t f3d_launch_plane_distance(const double* pts, int64_t n, const double pp[3], const double nr[3], double* out, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_plane_distance, dim3(f3d_grid_for(n, IB, F3D_GRID_CAP)), dim3(IB), 0, s, pts, n, pp[0], pp[1], pp[2], nr[0], nr[1],
                       nr[2], out);
    return hipGetLastError();
}
