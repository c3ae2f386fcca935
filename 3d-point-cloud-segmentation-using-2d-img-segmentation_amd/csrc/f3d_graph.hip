// (f)#1 adjacency: sklearn.neighbors.KDTree(points).query_radius(points, r=2*ds_radius) of fusion.py:374-375 as a CSR graph.
//
// A uniform grid of cell edge >= r replaces the tree: every neighbour of a point lies in the 27 cells around its own.
//   k_graph_bbox      : finite bounding box of the whole cloud + count of non-finite coordinates (sklearn rejects those)
//   k_graph_keys      : key[i] = linear cell id, idx[i] = i
//   rocprim radix sort: (key, idx) -> cell order (stable: indices ascend inside a cell)
//   k_graph_cells     : [first, last) position of every non-empty cell in the sorted order
//   k_graph_gather    : sorted float64 copy of the cloud (candidate loops read it contiguously)
//   k_graph_scan<0>   : neighbours per point -> counts[orig] ; rocprim exclusive scan -> offsets[n + 1]
//   k_graph_scan<1>   : same walk, writes the neighbours' caller-order indices at offsets[orig]
// The walk and its distance test are f3d_grid_walk (f3d_kernels.h).  The order inside a row is (cell, index) instead of the tree's
// traversal order, which sklearn does not specify either.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cstring>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include "f3d.h"
#include "f3d_kernels.h"

namespace {

constexpr int GB = 256;

struct gbox { double lo[3], hi[3]; unsigned long long bad; };

template <typename T>
__global__ __launch_bounds__(GB) void k_graph_bbox(const T* __restrict__ xyz, int64_t n, gbox* __restrict__ partial) {
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    unsigned long long bad = 0;
    for (int64_t i = (int64_t)blockIdx.x * GB + threadIdx.x; i < n; i += (int64_t)gridDim.x * GB) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double x = (double)xyz[3 * i + c];
            if (f3d_finite(x)) { lo[c] = fmin(lo[c], x); hi[c] = fmax(hi[c], x); } else ++bad;
        }
    }
    __shared__ gbox sh[GB / 64];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double a = lo[c], b = hi[c];
        for (int off = 32; off >= 1; off >>= 1) { a = fmin(a, __shfl_xor(a, off, 64)); b = fmax(b, __shfl_xor(b, off, 64)); }
        if ((threadIdx.x & 63) == 0) { sh[threadIdx.x >> 6].lo[c] = a; sh[threadIdx.x >> 6].hi[c] = b; }
    }
    for (int off = 32; off >= 1; off >>= 1) bad += __shfl_xor(bad, off, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6].bad = bad;
    __syncthreads();
    if (threadIdx.x == 0) {
        gbox o = sh[0];
        for (int w = 1; w < GB / 64; ++w) {
            for (int c = 0; c < 3; ++c) { o.lo[c] = fmin(o.lo[c], sh[w].lo[c]); o.hi[c] = fmax(o.hi[c], sh[w].hi[c]); }
            o.bad += sh[w].bad;
        }
        partial[blockIdx.x] = o;
    }
}

template <typename T>
__global__ __launch_bounds__(GB) void k_graph_keys(const T* __restrict__ xyz, int64_t n, f3d_graphgrid g, uint32_t* __restrict__ keys,
                                                    uint32_t* __restrict__ idx) {
    for (int64_t i = (int64_t)blockIdx.x * GB + threadIdx.x; i < n; i += (int64_t)gridDim.x * GB) {
        int cx, cy, cz;
        f3d_cell_of(g, (double)xyz[3 * i], (double)xyz[3 * i + 1], (double)xyz[3 * i + 2], cx, cy, cz);
        keys[i] = (uint32_t)((cz * g.dim[1] + cy) * g.dim[0] + cx);
        idx[i] = (uint32_t)i;
    }
}

__global__ __launch_bounds__(GB) void k_graph_cells(const uint32_t* __restrict__ keys, int64_t n, int2* __restrict__ cells) {
    for (int64_t j = (int64_t)blockIdx.x * GB + threadIdx.x; j < n; j += (int64_t)gridDim.x * GB) {
        const uint32_t k = keys[j];
        if (j == 0 || keys[j - 1] != k) cells[k].x = (int)j;
        if (j == n - 1 || keys[j + 1] != k) cells[k].y = (int)j + 1;
    }
}

template <typename T>
__global__ __launch_bounds__(GB) void k_graph_gather(const T* __restrict__ xyz, int64_t n, const uint32_t* __restrict__ perm,
                                                      double* __restrict__ sorted) {
    for (int64_t j = (int64_t)blockIdx.x * GB + threadIdx.x; j < n; j += (int64_t)gridDim.x * GB) {
        const int64_t i = perm[j];
        sorted[3 * j] = (double)xyz[3 * i]; sorted[3 * j + 1] = (double)xyz[3 * i + 1]; sorted[3 * j + 2] = (double)xyz[3 * i + 2];
    }
}

// one thread per point, in cell order (a wave's threads walk nearly the same candidate ranges)
template <bool FILL>
__global__ __launch_bounds__(GB) void k_graph_scan(const double* __restrict__ sorted, int64_t n, const uint32_t* __restrict__ perm,
                                                    const int2* __restrict__ cells, f3d_gridsearch gs, int64_t* __restrict__ offsets,
                                                    int32_t* __restrict__ nbrs) {
    const f3d_gridview gv = {sorted, perm, cells};
    for (int64_t j = (int64_t)blockIdx.x * GB + threadIdx.x; j < n; j += (int64_t)gridDim.x * GB) {
        const int64_t orig = perm[j];
        int64_t out = FILL ? offsets[orig] : 0;
        f3d_grid_walk(gv, gs.g, sorted[3 * j], sorted[3 * j + 1], sorted[3 * j + 2], gs.r2, [&](int k) {
            if (FILL) nbrs[out] = (int32_t)perm[k];
            ++out;
            return false;
        });
        if (!FILL) offsets[orig] = out;
    }
}

struct graph_layout { size_t keys_a, keys_b, idx_a, perm, sorted, cells, bbox, temp, total; };

graph_layout layout_for(int64_t n, int64_t ncells, size_t temp_bytes) {
    graph_layout L;
    f3d_carve c;
    L.keys_a = c.take((size_t)n * 4); L.keys_b = c.take((size_t)n * 4); L.idx_a = c.take((size_t)n * 4); L.perm = c.take((size_t)n * 4);
    L.sorted = c.take((size_t)n * 24); L.cells = c.take((size_t)ncells * 8); L.bbox = c.take(sizeof(gbox) * 1024); L.temp = c.take(temp_bytes);
    L.total = c.off;
    return L;
}

// rocprim's temporary storage: the cell sort of `nsort` points and the scan of `nscan` + 1 offsets share it
size_t temp_bytes_for(int64_t nsort, int64_t nscan) {
    size_t a = 0, b = 0;
    (void)rocprim::radix_sort_pairs(nullptr, a, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, (size_t)nsort, 0u, 32u);
    (void)rocprim::exclusive_scan(nullptr, b, (int64_t*)nullptr, (int64_t*)nullptr, (int64_t)0, (size_t)nscan + 1, rocprim::plus<int64_t>());
    return (a > b ? a : b) + 256;
}

f3d_gridview view_of(const void* scratch, const graph_layout& L) {
    const char* base = (const char*)scratch;
    return {(const double*)(base + L.sorted), (const uint32_t*)(base + L.perm), (const int2*)(base + L.cells)};
}

}  // namespace

size_t f3d_graph_bbox_bytes(void) { return sizeof(gbox) * 1024; }

// stage 1 of the count pass: bounding box partials (the host reduces <= 1024 of them and chooses the grid)
hipError_t f3d_launch_graph_bbox(const void* xyz, int dtype, int64_t n, void* partial, int* nblocks, hipStream_t s) {
    const int b = f3d_grid_for(n, GB, 1024);
    *nblocks = b;
    if (dtype == F3D_F64) hipLaunchKernelGGL(k_graph_bbox<double>, dim3(b), dim3(GB), 0, s, (const double*)xyz, n, (gbox*)partial);
    else hipLaunchKernelGGL(k_graph_bbox<float>, dim3(b), dim3(GB), 0, s, (const float*)xyz, n, (gbox*)partial);
    return hipGetLastError();
}

int f3d_graph_reduce_bbox(const void* partial_host, int nblocks, double lo[3], double hi[3]) {
    const gbox* p = (const gbox*)partial_host;
    unsigned long long bad = 0;
    for (int c = 0; c < 3; ++c) { lo[c] = INFINITY; hi[c] = -INFINITY; }
    for (int b = 0; b < nblocks; ++b) {
        for (int c = 0; c < 3; ++c) { lo[c] = fmin(lo[c], p[b].lo[c]); hi[c] = fmax(hi[c], p[b].hi[c]); }
        bad += p[b].bad;
    }
    return bad ? 1 : 0;
}

size_t f3d_graph_scratch_bytes(int64_t n, int64_t ncells) { return layout_for(n, ncells, temp_bytes_for(n, n)).total; }

// the grid itself, shared by the radius graph and the radius query: cell keys, stable sort by cell, cell table, sorted float64 copy
static hipError_t build_grid(const void* xyz, int dtype, int64_t n, const f3d_graphgrid& g, const graph_layout& L, size_t tb, char* base,
                             hipStream_t s) {
    const int64_t ncells = f3d_ncells(g);
    uint32_t *ka = (uint32_t*)(base + L.keys_a), *kb = (uint32_t*)(base + L.keys_b), *ia = (uint32_t*)(base + L.idx_a), *perm = (uint32_t*)(base + L.perm);
    double* sorted = (double*)(base + L.sorted);
    int2* cells = (int2*)(base + L.cells);
    const dim3 gr(f3d_grid_for(n, GB, 8192)), b(GB);
    if (dtype == F3D_F64) hipLaunchKernelGGL(k_graph_keys<double>, gr, b, 0, s, (const double*)xyz, n, g, ka, ia);
    else hipLaunchKernelGGL(k_graph_keys<float>, gr, b, 0, s, (const float*)xyz, n, g, ka, ia);
    unsigned bits = 1; while (bits < 32 && ((int64_t)1 << bits) < ncells) ++bits;
    size_t t = tb;
    hipError_t e = rocprim::radix_sort_pairs(base + L.temp, t, ka, kb, ia, perm, (size_t)n, 0u, bits, s);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(cells, 0, (size_t)ncells * 8, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_graph_cells, gr, b, 0, s, kb, n, cells);
    if (dtype == F3D_F64) hipLaunchKernelGGL(k_graph_gather<double>, gr, b, 0, s, (const double*)xyz, n, perm, sorted);
    else hipLaunchKernelGGL(k_graph_gather<float>, gr, b, 0, s, (const float*)xyz, n, perm, sorted);
    return hipGetLastError();
}

// the grid alone, for searches that keep no CSR (f3d_pointvote.hip): scratch holds f3d_graph_scratch_bytes(n, ncells)
hipError_t f3d_launch_graph_grid(const void* xyz, int dtype, int64_t n, const f3d_graphgrid& g, void* scratch, f3d_gridview* view,
                                 hipStream_t s) {
    const size_t tb = temp_bytes_for(n, n);
    const graph_layout L = layout_for(n, f3d_ncells(g), tb);
    *view = view_of(scratch, L);
    return build_grid(xyz, dtype, n, g, L, tb, (char*)scratch, s);
}

// count pass after the grid is known: sort by cell, cell table, sorted copy, neighbour counts, exclusive scan into offsets[n + 1]
hipError_t f3d_launch_graph_count(const void* xyz, int dtype, int64_t n, const f3d_gridsearch& gs, void* scratch, int64_t* offsets,
                                  hipStream_t s) {
    const size_t tb = temp_bytes_for(n, n);
    const graph_layout L = layout_for(n, f3d_ncells(gs.g), tb);
    char* base = (char*)scratch;
    hipError_t e = build_grid(xyz, dtype, n, gs.g, L, tb, base, s);
    if (e != hipSuccess) return e;
    const f3d_gridview gv = view_of(scratch, L);
    hipLaunchKernelGGL(k_graph_scan<false>, dim3(f3d_grid_for(n, GB, 8192)), dim3(GB), 0, s, gv.sorted, n, gv.perm, gv.cells, gs, offsets,
                       (int32_t*)nullptr);
    e = hipMemsetAsync(offsets + n, 0, 8, s);
    if (e != hipSuccess) return e;
    size_t t = tb;
    e = rocprim::exclusive_scan(base + L.temp, t, offsets, offsets, (int64_t)0, (size_t)n + 1, rocprim::plus<int64_t>(), s);
    if (e != hipSuccess) return e;
    return hipGetLastError();
}

// fill pass: the scratch still holds the grid of the count pass
hipError_t f3d_launch_graph_fill(int64_t n, const f3d_gridsearch& gs, const void* scratch, const int64_t* offsets, int32_t* nbrs,
                                 hipStream_t s) {
    const f3d_gridview gv = view_of(scratch, layout_for(n, f3d_ncells(gs.g), temp_bytes_for(n, n)));
    hipLaunchKernelGGL(k_graph_scan<true>, dim3(f3d_grid_for(n, GB, 8192)), dim3(GB), 0, s, gv.sorted, n, gv.perm, gv.cells, gs,
                       const_cast<int64_t*>(offsets), nbrs);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Bipartite form: KDTree(data).query_radius(queries, r) inverted to one row per query, rows in ascending data index.
//   the data's grid is built as above (build_grid); one thread per query point, in the caller's order
//   k_query_scan<0>   : matches per query -> offsets[q]; non-finite queries raise a flag (sklearn rejects them)
//   rocprim exclusive scan -> offsets[n + 1]
//   k_query_scan<1>   : same walk, writes the matches' caller-order data indices; the cell walk leaves <= 27 ascending runs, which
//                       the thread sorts in place when the row is short, else it lists the row for k_query_sort_long
//   k_query_sort_long : one block per listed row, a bitonic network in LDS (or in place in global memory past the LDS capacity)
// A query outside the reach box (f3d_gridsearch) cannot match anything and skips the walk.
namespace {

constexpr int QRY_SHORT = 32;           // rows up to this length are sorted by their own thread (insertion sort)
constexpr int QRY_LDS = 8192;           // longest row k_query_sort_long sorts in LDS (32 KiB)

struct query_layout { graph_layout grid; size_t words, longrows, total; };

// words: [0] nnz (copied from offsets[n]), [1] bit 0 = a query is NaN / infinite, [2] number of rows listed for k_query_sort_long
query_layout query_layout_for(int64_t m, int64_t n, int64_t ncells, size_t temp_bytes) {
    query_layout Q;
    Q.grid = layout_for(m, ncells, temp_bytes);
    f3d_carve c;
    c.off = Q.grid.total;
    Q.words = c.take(64); Q.longrows = c.take((size_t)n * 4);
    Q.total = c.off;
    return Q;
}

template <typename T, bool FILL>
__global__ __launch_bounds__(GB) void k_query_scan(const T* __restrict__ q, int64_t n, const double* __restrict__ sorted,
                                                    const uint32_t* __restrict__ perm, const int2* __restrict__ cells, f3d_gridsearch gs,
                                                    int64_t* __restrict__ offsets, int32_t* __restrict__ nbrs,
                                                    unsigned long long* __restrict__ words, int32_t* __restrict__ longrows) {
    const f3d_gridview gv = {sorted, perm, cells};
    for (int64_t i = (int64_t)blockIdx.x * GB + threadIdx.x; i < n; i += (int64_t)gridDim.x * GB) {
        const double px = (double)q[3 * i], py = (double)q[3 * i + 1], pz = (double)q[3 * i + 2];
        const int64_t start = FILL ? offsets[i] : 0, end = FILL ? offsets[i + 1] : 0;
        int64_t out = start;
        if (!FILL && !f3d_finite(px, py, pz)) atomicOr(&words[1], 1ull);
        if (f3d_in_box(gs.reach, px, py, pz))
            f3d_grid_walk(gv, gs.g, px, py, pz, gs.r2, [&](int k) {
                if (FILL && out < end) nbrs[out] = (int32_t)perm[k];               // (queries changed since the count: never past the row)
                ++out;
                return false;
            });
        if (FILL) out = min(out, end);
        if (!FILL) {
            offsets[i] = out;
        } else if (out - start > QRY_SHORT) {
            longrows[atomicAdd((unsigned long long*)&words[2], 1ull)] = (int32_t)i;
        } else {
            for (int64_t a = start + 1; a < out; ++a) {                             // the row was just written: it is in this CU's cache
                const int32_t v = nbrs[a];
                int64_t b = a;
                for (; b > start && nbrs[b - 1] > v; --b) nbrs[b] = nbrs[b - 1];
                nbrs[b] = v;
            }
        }
    }
}

// Ascending bitonic network on a[0, len) padded to p (a power of two) with virtual +inf: every comparator puts the smaller value at the
// lower position (the first stage of each merge compares mirrored positions), so a comparator whose upper element lies past len is a no-op.
// I: int in LDS, int64_t for rows sorted in place in global memory (their padded length may pass 2^30).
template <typename I>
__device__ void bitonic_sort(int32_t* a, I len, I p) {
    for (I k = 2; k <= p; k <<= 1) {
        for (I j = k >> 1; j >= 1; j >>= 1) {
            for (I t = threadIdx.x; t < (p >> 1); t += GB) {
                const I lo = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const I hi = (j == (k >> 1)) ? (lo ^ (k - 1)) : lo + j;
                if (hi < len) {
                    const int32_t x = a[lo], y = a[hi];
                    if (y < x) { a[lo] = y; a[hi] = x; }
                }
            }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(GB) void k_query_sort_long(const int64_t* __restrict__ offsets, int32_t* __restrict__ nbrs,
                                                         const unsigned long long* __restrict__ words, const int32_t* __restrict__ longrows) {
    __shared__ int32_t sh[QRY_LDS];
    const int64_t count = (int64_t)words[2];
    for (int64_t r = blockIdx.x; r < count; r += gridDim.x) {
        const int64_t row = longrows[r];
        const int64_t start = offsets[row];
        const int64_t len = offsets[row + 1] - start;
        int64_t p = 1;
        while (p < len) p <<= 1;
        int32_t* a = nbrs + start;
        if (p <= QRY_LDS) {
            for (int t = threadIdx.x; t < (int)len; t += GB) sh[t] = a[t];
            __syncthreads();
            bitonic_sort<int>(sh, (int)len, (int)p);
            for (int t = threadIdx.x; t < (int)len; t += GB) a[t] = sh[t];
        } else {
            bitonic_sort<int64_t>(a, len, p);                                      // one block: its barriers order the global accesses
        }
        __syncthreads();
    }
}

}  // namespace

size_t f3d_query_scratch_bytes(int64_t m, int64_t n, int64_t ncells) {
    return query_layout_for(m, n, ncells, temp_bytes_for(m, n)).total;
}

hipError_t f3d_launch_query_count(const void* data, int ddtype, int64_t m, const void* queries, int qdtype, int64_t n, const f3d_gridsearch& gs,
                                  void* scratch, int64_t* offsets, int64_t* words_host, hipStream_t s) {
    const size_t tb = temp_bytes_for(m, n);
    const query_layout Q = query_layout_for(m, n, f3d_ncells(gs.g), tb);
    char* base = (char*)scratch;
    unsigned long long* words = (unsigned long long*)(base + Q.words);
    hipError_t e = hipMemsetAsync(words, 0, 64, s);
    if (e != hipSuccess) return e;
    if ((e = build_grid(data, ddtype, m, gs.g, Q.grid, tb, base, s)) != hipSuccess) return e;
    const f3d_gridview gv = view_of(scratch, Q.grid);
    const dim3 gr(f3d_grid_for(n, GB, 8192)), b(GB);
    if (qdtype == F3D_F64)
        hipLaunchKernelGGL((k_query_scan<double, false>), gr, b, 0, s, (const double*)queries, n, gv.sorted, gv.perm, gv.cells, gs, offsets,
                           (int32_t*)nullptr, words, (int32_t*)nullptr);
    else
        hipLaunchKernelGGL((k_query_scan<float, false>), gr, b, 0, s, (const float*)queries, n, gv.sorted, gv.perm, gv.cells, gs, offsets,
                           (int32_t*)nullptr, words, (int32_t*)nullptr);
    if ((e = hipMemsetAsync(offsets + n, 0, 8, s)) != hipSuccess) return e;
    size_t t = tb;
    e = rocprim::exclusive_scan(base + Q.grid.temp, t, offsets, offsets, (int64_t)0, (size_t)n + 1, rocprim::plus<int64_t>(), s);
    if (e != hipSuccess) return e;
    if ((e = hipMemcpyAsync(words, offsets + n, 8, hipMemcpyDeviceToDevice, s)) != hipSuccess) return e;
    return hipMemcpyAsync(words_host, words, 16, hipMemcpyDeviceToHost, s);     // the caller synchronises
}

hipError_t f3d_launch_query_fill(const void* queries, int qdtype, int64_t m, int64_t n, const f3d_gridsearch& gs, void* scratch,
                                 const int64_t* offsets, int32_t* nbrs, hipStream_t s) {
    const query_layout Q = query_layout_for(m, n, f3d_ncells(gs.g), temp_bytes_for(m, n));
    char* base = (char*)scratch;
    unsigned long long* words = (unsigned long long*)(base + Q.words);
    int32_t* longrows = (int32_t*)(base + Q.longrows);
    hipError_t e = hipMemsetAsync(words + 2, 0, 8, s);
    if (e != hipSuccess) return e;
    const f3d_gridview gv = view_of(scratch, Q.grid);
    int64_t* offs = const_cast<int64_t*>(offsets);                              // (read only in the fill pass)
    const dim3 gr(f3d_grid_for(n, GB, 8192)), b(GB);
    if (qdtype == F3D_F64)
        hipLaunchKernelGGL((k_query_scan<double, true>), gr, b, 0, s, (const double*)queries, n, gv.sorted, gv.perm, gv.cells, gs, offs, nbrs,
                           words, longrows);
    else
        hipLaunchKernelGGL((k_query_scan<float, true>), gr, b, 0, s, (const float*)queries, n, gv.sorted, gv.perm, gv.cells, gs, offs, nbrs,
                           words, longrows);
    hipLaunchKernelGGL(k_query_sort_long, dim3(2048), b, 0, s, offsets, nbrs, words, longrows);
    return hipGetLastError();
}
