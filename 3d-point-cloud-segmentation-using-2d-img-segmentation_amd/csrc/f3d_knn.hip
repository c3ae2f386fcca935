// Hybrid k-nearest search (at most k nearest within r: Open3D's KDTreeSearchParamHybrid, sklearn's query cut at a radius) and the
// label transfer built on it.  No reference counterpart: the contract is in include/f3d.h (f3d_knn_query, f3d_transfer_labels).
//
// The data cloud's grid is the radius graph's (f3d_launch_graph_grid: cell edge a hair above r, stable cell sort, cell table, sorted
// float64 copy); the candidate walk and its distance test are f3d_grid_walk_d2 (f3d_kernels.h), which hands over the squared
// distance it has just computed.
//   k_knn_flag         : streaming pre-pass, raises the flag word when a query is NaN / infinite (read back with the cloud's box)
//   k_knn_query<T, K>  : one thread per query, in the caller's order.  Keeps the K >= k smallest (d2, caller-order data index) in
//                        topk<K>, a sorted register array with a compile-time-unrolled insertion network (no runtime-indexed private
//                        arrays: they would live in scratch memory); K = 1 is a plain running minimum.  Writes idx / dist2 / counts.
//   k_knn_labels<T, K> : the same walk and selection, then the plurality over the kept set in registers (K * K unrolled compares,
//                        labels gathered as labels[perm[k]]).  Writes out / support only: no [n, k] table exists in memory.
// The key is total (no two data points share an index), so the kept set and its order depend on neither the cell order nor the
// launch shape.  A query outside the reach box cannot match anything and skips the walk.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include <type_traits>
#include "f3d.h"
#include "f3d_kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int KB = 128;

template <int K>
struct knn_keep : topk<K> {};

// K = 1: the running minimum of (d2, index)
template <>
struct knn_keep<1> {
    double d[1];
    int j[1];
    __device__ __forceinline__ void init() { d[0] = INFINITY; j[0] = 0x7fffffff; }
    __device__ __forceinline__ void insert(double dn, int jn) {
        if (dn < d[0] || (dn == d[0] && jn < j[0])) { d[0] = dn; j[0] = jn; }
    }
};

template <typename T>
__global__ __launch_bounds__(256) void k_knn_flag(const T* __restrict__ q, int64_t n, unsigned* __restrict__ flag) {
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < 3 * n; i += (int64_t)gridDim.x * 256) bad = bad || !f3d_finite((double)q[i]);
    if (bad) atomicOr(flag, 1u);
}

// the kept set of query i in `top`; -> its size c = min(k, matches within the radius)
template <typename T, int K>
__device__ __forceinline__ int knn_select(const T* __restrict__ q, int64_t i, const f3d_gridview& gv, const f3d_gridsearch& gs, int k,
                                          knn_keep<K>& top) {
    const double px = (double)q[3 * i], py = (double)q[3 * i + 1], pz = (double)q[3 * i + 2];
    top.init();
    int inside = 0;                                                                // matches visited (at most m < 2^31)
    if (f3d_in_box(gs.reach, px, py, pz))
        f3d_grid_walk_d2(gv, gs.g, px, py, pz, gs.r2, [&](int s, double d) {
            ++inside;
            top.insert(d, (int)gv.perm[s]);
            return false;
        });
    return min(inside, k);
}

template <typename T, int K>
__global__ __launch_bounds__(KB) void k_knn_query(const T* __restrict__ q, int64_t n, int k, const double* __restrict__ sorted,
                                                   const uint32_t* __restrict__ perm, const int2* __restrict__ cells, f3d_gridsearch gs,
                                                   int32_t* __restrict__ idx, double* __restrict__ dist2, int32_t* __restrict__ counts) {
    const f3d_gridview gv = {sorted, perm, cells};
    for (int64_t i = (int64_t)blockIdx.x * KB + threadIdx.x; i < n; i += (int64_t)gridDim.x * KB) {
        knn_keep<K> top;
        const int c = knn_select<T, K>(q, i, gv, gs, k, top);
        int32_t* irow = idx + i * k;
        double* drow = dist2 ? dist2 + i * k : nullptr;
#pragma unroll
        for (int s = 0; s < K; ++s) {
            if (s < k) {
                irow[s] = s < c ? top.j[s] : -1;
                if (drow) drow[s] = s < c ? top.d[s] : INFINITY;
            }
        }
        if (counts) counts[i] = c;
    }
}

template <typename T, int K>
__global__ __launch_bounds__(KB) void k_knn_labels(const T* __restrict__ q, int64_t n, int k, const double* __restrict__ sorted,
                                                    const uint32_t* __restrict__ perm, const int2* __restrict__ cells, f3d_gridsearch gs,
                                                    const int64_t* __restrict__ labels, int64_t fill, int64_t* __restrict__ out,
                                                    int32_t* __restrict__ support) {
    const f3d_gridview gv = {sorted, perm, cells};
    for (int64_t i = (int64_t)blockIdx.x * KB + threadIdx.x; i < n; i += (int64_t)gridDim.x * KB) {
        knn_keep<K> top;
        const int c = knn_select<T, K>(q, i, gv, gs, k, top);
        int64_t lab[K];
#pragma unroll
        for (int s = 0; s < K; ++s) lab[s] = s < c ? labels[top.j[s]] : 0;        // (no label is read for an empty slot)
        // plurality: the label with the most occurrences; the scan ascends and replaces on a strictly larger count only, so among
        // equal counts the label whose first occurrence comes earliest in the row wins
        int best = 0;
        int64_t win = fill;
#pragma unroll
        for (int s = 0; s < K; ++s) {
            int cnt = 0;
#pragma unroll
            for (int t = 0; t < K; ++t) cnt += (t < c && lab[t] == lab[s]) ? 1 : 0;
            if (s < c && cnt > best) { best = cnt; win = lab[s]; }
        }
        out[i] = win;
        if (support) support[i] = best;
    }
}

int knn_grid(int64_t n) { return f3d_grid_for(n, KB, 16384); }

// the smallest instantiated K >= k
template <typename F>
void for_k(int k, F f) {
    if (k <= 1) f(std::integral_constant<int, 1>());
    else if (k <= 4) f(std::integral_constant<int, 4>());
    else if (k <= 8) f(std::integral_constant<int, 8>());
    else if (k <= 16) f(std::integral_constant<int, 16>());
    else f(std::integral_constant<int, 32>());
}

}  // namespace

hipError_t f3d_launch_knn_flag(const void* queries, int qdtype, int64_t n, unsigned* flag, hipStream_t s) {
    const dim3 gr(f3d_grid_for(3 * n, 256, 8192)), b(256);
    if (qdtype == F3D_F64) hipLaunchKernelGGL(k_knn_flag<double>, gr, b, 0, s, (const double*)queries, n, flag);
    else hipLaunchKernelGGL(k_knn_flag<float>, gr, b, 0, s, (const float*)queries, n, flag);
    return hipGetLastError();
}

hipError_t f3d_launch_knn_query(const void* queries, int qdtype, int64_t n, int k, const f3d_gridview& gv, const f3d_gridsearch& gs,
                                int32_t* idx, double* dist2, int32_t* counts, hipStream_t s) {
    if (k < 1 || k > F3D_KNN_MAX_K) return hipErrorInvalidValue;
    const dim3 gr(knn_grid(n)), b(KB);
    for_k(k, [&](auto kc) {
        constexpr int K = decltype(kc)::value;
        if (qdtype == F3D_F64)
            hipLaunchKernelGGL((k_knn_query<double, K>), gr, b, 0, s, (const double*)queries, n, k, gv.sorted, gv.perm, gv.cells, gs, idx, dist2,
                               counts);
        else
            hipLaunchKernelGGL((k_knn_query<float, K>), gr, b, 0, s, (const float*)queries, n, k, gv.sorted, gv.perm, gv.cells, gs, idx, dist2,
                               counts);
    });
    return hipGetLastError();
}

hipError_t f3d_launch_knn_labels(const void* queries, int qdtype, int64_t n, int k, const f3d_gridview& gv, const f3d_gridsearch& gs,
                                 const int64_t* labels, int64_t fill, int64_t* out, int32_t* support, hipStream_t s) {
    if (k < 1 || k > F3D_KNN_MAX_K) return hipErrorInvalidValue;
    const dim3 gr(knn_grid(n)), b(KB);
    for_k(k, [&](auto kc) {
        constexpr int K = decltype(kc)::value;
        if (qdtype == F3D_F64)
            hipLaunchKernelGGL((k_knn_labels<double, K>), gr, b, 0, s, (const double*)queries, n, k, gv.sorted, gv.perm, gv.cells, gs, labels, fill,
                               out, support);
        else
            hipLaunchKernelGGL((k_knn_labels<float, K>), gr, b, 0, s, (const float*)queries, n, k, gv.sorted, gv.perm, gv.cells, gs, labels, fill,
                               out, support);
    });
    return hipGetLastError();
}
