// Same-class connected components for split_into_instances (reference segUtils/cv.py:425-440, 473-499).
//
// The reference flood-fills from the lowest remaining point index through neighbours of the same class.  On a
// symmetric adjacency (the only producer, KDTree.query_radius at fusion.py:369-377, is symmetric) the cluster of a
// seed is its connected component in the graph restricted to same-class edges, and "lowest remaining index" is the
// component's minimum index.  That is what this file computes: a lock-free union-find where the larger root is
// always linked under the smaller one (so every component ends rooted at its minimum index), one pass over the
// CSR edges, then a compression pass.  The union-find itself (f3d_find_root, f3d_uf_link) lives in f3d_kernels.h.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include "f3d.h"
#include "f3d_kernels.h"

namespace {

constexpr int CB = 256;

__global__ __launch_bounds__(CB) void k_cc_init(int32_t* __restrict__ parent, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * CB + threadIdx.x; i < n; i += (int64_t)gridDim.x * CB) parent[i] = (int32_t)i;
}

__global__ __launch_bounds__(CB) void k_cc_hook(const int64_t* __restrict__ classes, int64_t n, const int64_t* __restrict__ offs,
                                                const int32_t* __restrict__ nbrs, int32_t* parent, int* __restrict__ err, int errbit) {
    for (int64_t i = (int64_t)blockIdx.x * CB + threadIdx.x; i < n; i += (int64_t)gridDim.x * CB) {
        const int64_t ci = classes[i];
        for (int64_t e = offs[i]; e < offs[i + 1]; ++e) {
            const int64_t j = nbrs[e];
            if (j < 0 || j >= n) { atomicOr(err, errbit); continue; }
            if (j == i || classes[j] != ci) continue;
            f3d_uf_link(parent, (int32_t)i, (int32_t)j);
        }
    }
}

__global__ __launch_bounds__(CB) void k_cc_compress(const int32_t* parent, int64_t n, int64_t* __restrict__ root) {
    for (int64_t i = (int64_t)blockIdx.x * CB + threadIdx.x; i < n; i += (int64_t)gridDim.x * CB) {
        root[i] = f3d_uf_root(parent, (int32_t)i);
    }
}

}  // namespace

hipError_t f3d_launch_components(const int64_t* classes, int64_t n, const int64_t* offs, const int32_t* nbrs, int32_t* parent,
                                 int64_t* root, int* err, hipStream_t s, int errbit) {
    if (n <= 0) return hipSuccess;
    if (n > 0x7fffffffLL) return hipErrorInvalidValue;
    const dim3 g((unsigned)f3d_grid_for(n, CB, 16384)), b(CB);
    hipLaunchKernelGGL(k_cc_init, g, b, 0, s, parent, n);
    hipLaunchKernelGGL(k_cc_hook, g, b, 0, s, classes, n, offs, nbrs, parent, err, errbit);
    hipLaunchKernelGGL(k_cc_compress, g, b, 0, s, parent, n, root);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Ordered same-class flood of CVSegmentation.instance_seperate (reference segUtils/cv.py:52-89, 309-365).
//
// The reference floods each cluster with a FIFO queue from its lowest index; different-class neighbours are enqueued but
// not expanded.  On a symmetric adjacency with no duplicate entries the queue's pop order restricted to the cluster is a
// level-by-level order in which v's parent is the cluster point with the smallest position that has v in its row, and
// siblings follow their position in that row.  So every cluster gets a slot range [base, base + size) of one `order`
// array (clusters numbered by the rank of their class in the processing list, then by ascending seed: a radix sort of
// (rank, root) keys) and all clusters are flooded together, one level per round:
//   k_fo_expand : each frontier node offers (slot << 32 | row position) to every unvisited same-class neighbour (atomicMin)
//   k_fo_count  : children per frontier node (neighbours whose minimum names it) + per-block sums; first / last frontier
//                 entry of every cluster
//   k_fo_top    : one block scans the block sums; the total is the next frontier's length (it stays on the device)
//   k_fo_apply  : exclusive scan of the children counts over the frontier (frontier order = slot order, cluster by cluster)
//   k_fo_place  : children take the slots after their cluster's frontier, in (parent slot, row position) order
// The result depends on nothing but the minima, never on thread timing.  The host reads the frontier length back every
// FO_CHUNK levels; the kernels of a round with an empty frontier exit at once.  Boundary (cv.py:81-83): cluster point u
// is flagged when a different-class neighbour q has no point of u's cluster with a smaller slot in its row (q's first
// discoverer is u).  A boundary point belongs to its own cluster, so one byte per point holds every cluster's boundary.
namespace {

constexpr int FO_GRID = 1024;            // blocks of the per-level kernels (each owns a contiguous share of the frontier)
constexpr int FO_CHUNK = 8;              // levels enqueued between two readbacks of the frontier length

struct fo_words { int32_t nf[2]; int32_t levels; int32_t pad; };

__device__ __forceinline__ int fo_rank(int64_t c, const int64_t* __restrict__ inst, int k) {
    for (int r = 0; r < k; ++r) if (inst[r] == c) return r;
    return -1;
}

__global__ __launch_bounds__(CB) void k_fo_keys(const int64_t* __restrict__ classes, int64_t n, const int64_t* __restrict__ root,
                                                const int64_t* __restrict__ inst, int k, uint64_t* __restrict__ keys) {
    for (int64_t i = (int64_t)blockIdx.x * CB + threadIdx.x; i < n; i += (int64_t)gridDim.x * CB) {
        const int r = fo_rank(classes[i], inst, k);
        keys[i] = r < 0 ? ~0ull : ((uint64_t)r << 32 | (uint64_t)root[i]);
    }
}

__global__ __launch_bounds__(CB) void k_fo_heads(const uint64_t* __restrict__ sk, int64_t n, int32_t* __restrict__ head) {
    for (int64_t i = (int64_t)blockIdx.x * CB + threadIdx.x; i <= n; i += (int64_t)gridDim.x * CB)
        head[i] = (i < n && sk[i] != ~0ull && (i == 0 || sk[i - 1] != sk[i])) ? 1 : 0;
}

// seeds: slot = first position of the cluster's run in the sorted keys; frontier 0 = the seeds in cluster order
__global__ __launch_bounds__(CB) void k_fo_seeds(const uint64_t* __restrict__ sk, int64_t n, const int32_t* __restrict__ cid,
                                                 int64_t* __restrict__ coffs, int64_t* __restrict__ order, int32_t* __restrict__ slot,
                                                 int32_t* __restrict__ F, int32_t* __restrict__ FC, fo_words* w) {
    for (int64_t i = (int64_t)blockIdx.x * CB + threadIdx.x; i < n; i += (int64_t)gridDim.x * CB) {
        const uint64_t key = sk[i];
        if (key == ~0ull) continue;
        if (i == 0 || sk[i - 1] != key) {
            const int32_t c = cid[i];
            const int32_t seed = (int32_t)(key & 0xffffffffull);
            coffs[c] = i; F[c] = (int32_t)i; FC[c] = c;
            order[i] = seed; slot[seed] = (int32_t)i;
        }
        if (i == n - 1 || sk[i + 1] == ~0ull) {          // last clustered position: totals
            coffs[cid[n]] = i + 1;
            w->nf[0] = cid[n];
        }
    }
}

__device__ __forceinline__ void fo_range(int nf, int& lo, int& hi) {
    const int per = (nf + (int)gridDim.x - 1) / (int)gridDim.x;
    lo = min(nf, (int)blockIdx.x * per); hi = min(nf, lo + per);
}

__global__ __launch_bounds__(CB) void k_fo_expand(const int64_t* __restrict__ classes, int64_t n, const int64_t* __restrict__ offs,
                                                  const int32_t* __restrict__ nbrs, const int64_t* __restrict__ order,
                                                  const int32_t* __restrict__ slot, const int32_t* __restrict__ F, const fo_words* w, int cur,
                                                  unsigned long long* best, int* __restrict__ err, int errbit) {
    const int nf = w->nf[cur];
    for (int i = blockIdx.x * CB + threadIdx.x; i < nf; i += gridDim.x * CB) {
        const int32_t s = F[i];
        const int64_t u = order[s];
        const int64_t cu = classes[u];
        const int64_t e0 = offs[u], e1 = offs[u + 1];
        for (int64_t e = e0; e < e1; ++e) {
            const int64_t j = nbrs[e];
            if (j < 0 || j >= n) { atomicOr(err, errbit); continue; }
            if (classes[j] != cu || slot[j] >= 0) continue;
            atomicMin(best + j, (unsigned long long)s << 32 | (unsigned long long)(e - e0));
        }
    }
}

__device__ __forceinline__ int fo_children(const int64_t* __restrict__ offs, const int32_t* __restrict__ nbrs, int64_t n, int64_t u,
                                           int32_t s, const unsigned long long* best) {
    int c = 0;
    const int64_t e0 = offs[u], e1 = offs[u + 1];
    for (int64_t e = e0; e < e1; ++e) {
        const int64_t j = nbrs[e];
        if (j < 0 || j >= n) continue;
        if (best[j] == ((unsigned long long)s << 32 | (unsigned long long)(e - e0))) ++c;
    }
    return c;
}

__global__ __launch_bounds__(CB) void k_fo_count(int64_t n, const int64_t* __restrict__ offs, const int32_t* __restrict__ nbrs,
                                                 const int64_t* __restrict__ order, const int32_t* __restrict__ F,
                                                 const int32_t* __restrict__ FC, const fo_words* w, int cur, const unsigned long long* best,
                                                 int32_t* __restrict__ cnt, int32_t* __restrict__ part, int32_t* __restrict__ i0,
                                                 int32_t* __restrict__ i1) {
    __shared__ int lds[CB];
    const int nf = w->nf[cur];
    if (nf == 0) return;
    int lo, hi;
    fo_range(nf, lo, hi);
    int sum = 0;
    for (int i = lo + (int)threadIdx.x; i < hi; i += CB) {
        const int32_t s = F[i];
        const int c = fo_children(offs, nbrs, n, order[s], s, best);
        cnt[i] = c;
        sum += c;
        const int32_t C = FC[i];
        if (i == 0 || FC[i - 1] != C) i0[C] = i;
        if (i == nf - 1 || FC[i + 1] != C) i1[C] = i;
    }
    int ex, tot;
    f3d_block_scan<CB>(sum, lds, ex, tot);
    if (threadIdx.x == 0) part[blockIdx.x] = tot;
}

// one block of CB threads scans the FO_GRID block sums (FO_GRID / CB per thread)
__global__ __launch_bounds__(CB) void k_fo_top(int32_t* __restrict__ part, fo_words* w, int cur) {
    __shared__ int lds[CB];
    if (w->nf[cur] == 0) { if (threadIdx.x == 0) w->nf[cur ^ 1] = 0; return; }
    constexpr int PER = FO_GRID / CB;
    int v[PER], sum = 0;
    for (int k = 0; k < PER; ++k) { v[k] = part[threadIdx.x * PER + k]; sum += v[k]; }
    int run, tot;
    f3d_block_scan<CB>(sum, lds, run, tot);
    for (int k = 0; k < PER; ++k) { part[threadIdx.x * PER + k] = run; run += v[k]; }
    if (threadIdx.x == 0) { w->nf[cur ^ 1] = tot; w->levels += 1; }
}

__global__ __launch_bounds__(CB) void k_fo_apply(const int32_t* __restrict__ cnt, const int32_t* __restrict__ part, const fo_words* w, int cur,
                                                 int32_t* __restrict__ gx) {
    __shared__ int lds[CB];
    const int nf = w->nf[cur];
    if (nf == 0) return;
    int lo, hi;
    fo_range(nf, lo, hi);
    int carry = part[blockIdx.x];
    for (int b = lo; b < hi; b += CB) {
        const int i = b + (int)threadIdx.x;
        const int v = i < hi ? cnt[i] : 0;
        int ex, tot;
        f3d_block_scan<CB>(v, lds, ex, tot);
        if (i < hi) gx[i] = carry + ex;
        carry += tot;
    }
}

__global__ __launch_bounds__(CB) void k_fo_place(int64_t n, const int64_t* __restrict__ offs, const int32_t* __restrict__ nbrs,
                                                 int64_t* __restrict__ order, int32_t* __restrict__ slot, const int32_t* __restrict__ F,
                                                 const int32_t* __restrict__ FC, const fo_words* w, int cur, const unsigned long long* best,
                                                 const int32_t* __restrict__ gx, const int32_t* __restrict__ i0, const int32_t* __restrict__ i1,
                                                 int32_t* __restrict__ F2, int32_t* __restrict__ FC2) {
    const int nf = w->nf[cur];
    for (int i = blockIdx.x * CB + threadIdx.x; i < nf; i += gridDim.x * CB) {
        const int32_t s = F[i], C = FC[i];
        const int64_t u = order[s];
        int32_t pos = F[i1[C]] + 1 + (gx[i] - gx[i0[C]]);       // after the cluster's frontier, behind its earlier siblings
        int32_t q = gx[i];
        const int64_t e0 = offs[u], e1 = offs[u + 1];
        for (int64_t e = e0; e < e1; ++e) {
            const int64_t j = nbrs[e];
            if (j < 0 || j >= n) continue;
            if (best[j] != ((unsigned long long)s << 32 | (unsigned long long)(e - e0))) continue;
            order[pos] = j; slot[j] = pos;
            F2[q] = pos; FC2[q] = C;
            ++pos; ++q;
        }
    }
}

__global__ __launch_bounds__(CB) void k_fo_boundary(const int64_t* __restrict__ classes, int64_t n, const int64_t* __restrict__ offs,
                                                    const int32_t* __restrict__ nbrs, const int64_t* __restrict__ root,
                                                    const int32_t* __restrict__ slot, uint8_t* __restrict__ flags) {
    for (int64_t u = (int64_t)blockIdx.x * CB + threadIdx.x; u < n; u += (int64_t)gridDim.x * CB) {
        const int32_t su = slot[u];
        uint8_t f = 0;
        if (su >= 0) {
            const int64_t cu = classes[u], ru = root[u];
            for (int64_t e = offs[u]; e < offs[u + 1] && !f; ++e) {
                const int64_t q = nbrs[e];
                if (q < 0 || q >= n || classes[q] == cu) continue;
                bool first = true;                                  // no point of u's cluster before u has q in its row
                for (int64_t g = offs[q]; g < offs[q + 1]; ++g) {
                    const int64_t x = nbrs[g];
                    if (x < 0 || x >= n || root[x] != ru) continue;
                    const int32_t sx = slot[x];
                    if (sx >= 0 && sx < su) { first = false; break; }
                }
                if (first) f = 1;
            }
        }
        flags[u] = f;
    }
}

struct fo_layout { size_t parent, keys_a, keys_b, cid, slot, f[2], fc[2], cnt, gx, i0, i1, part, words, temp, total; size_t temp_bytes; };

fo_layout fo_layout_for(int64_t n) {
    fo_layout L;
    size_t a = 0, b = 0;
    (void)rocprim::radix_sort_keys(nullptr, a, (uint64_t*)nullptr, (uint64_t*)nullptr, (size_t)n, 0u, 64u);
    (void)rocprim::exclusive_scan(nullptr, b, (int32_t*)nullptr, (int32_t*)nullptr, (int32_t)0, (size_t)n + 1, rocprim::plus<int32_t>());
    L.temp_bytes = (a > b ? a : b) + 256;
    f3d_carve c;
    const size_t n4 = (size_t)n * 4, n8 = (size_t)n * 8;
    L.parent = c.take(n4); L.keys_a = c.take(n8); L.keys_b = c.take(n8); L.cid = c.take(n4 + 4); L.slot = c.take(n4);
    L.f[0] = c.take(n4); L.f[1] = c.take(n4); L.fc[0] = c.take(n4); L.fc[1] = c.take(n4);
    L.cnt = c.take(n4); L.gx = c.take(n4); L.i0 = c.take(n4); L.i1 = c.take(n4);
    L.part = c.take(FO_GRID * 4); L.words = c.take(sizeof(fo_words)); L.temp = c.take(L.temp_bytes);
    L.total = c.off;
    return L;
}

}  // namespace

size_t f3d_flood_scratch_bytes(int64_t n) { return fo_layout_for(n < 1 ? 1 : n).total; }

hipError_t f3d_launch_flood_order(const int64_t* classes, int64_t n, const int64_t* offs, const int32_t* nbrs, const int64_t* inst, int k,
                                  int64_t* root, int64_t* order, int64_t* coffs, uint8_t* flags, void* scratch, int* err, int64_t stats[4],
                                  hipStream_t s) {
    for (int q = 0; q < 4; ++q) stats[q] = 0;
    if (n <= 0) return hipSuccess;
    if (n > 0x7fffffffLL || k < 0 || k > 0x7fffffff) return hipErrorInvalidValue;
    const fo_layout L = fo_layout_for(n);
    char* base = (char*)scratch;
    int32_t* parent = (int32_t*)(base + L.parent);
    uint64_t *ka = (uint64_t*)(base + L.keys_a), *kb = (uint64_t*)(base + L.keys_b);
    int32_t* cid = (int32_t*)(base + L.cid);
    int32_t* slot = (int32_t*)(base + L.slot);
    int32_t *F[2] = {(int32_t*)(base + L.f[0]), (int32_t*)(base + L.f[1])}, *FC[2] = {(int32_t*)(base + L.fc[0]), (int32_t*)(base + L.fc[1])};
    int32_t *cnt = (int32_t*)(base + L.cnt), *gx = (int32_t*)(base + L.gx), *i0 = (int32_t*)(base + L.i0), *i1 = (int32_t*)(base + L.i1);
    int32_t* part = (int32_t*)(base + L.part);
    fo_words* w = (fo_words*)(base + L.words);
    unsigned long long* best = (unsigned long long*)ka;     // the unsorted keys are dead once the sort has run
    const dim3 g((unsigned)f3d_grid_for(n + 1, CB, 16384)), b(CB), gl(FO_GRID);

    F3D_TRY(f3d_launch_components(classes, n, offs, nbrs, parent, root, err, s, F3D_DEVERR_FLOOD));
    hipLaunchKernelGGL(k_fo_keys, g, b, 0, s, classes, n, root, inst, k, ka);
    const unsigned bits = 32 + (unsigned)f3d_bits_for((int64_t)k + 1, 0);          // k + 1 ranks above the 32 root bits
    size_t tb = L.temp_bytes;
    F3D_TRY(rocprim::radix_sort_keys(base + L.temp, tb, ka, kb, (size_t)n, 0u, bits, s));
    hipLaunchKernelGGL(k_fo_heads, g, b, 0, s, kb, n, cid);
    tb = L.temp_bytes;
    F3D_TRY(rocprim::exclusive_scan(base + L.temp, tb, cid, cid, (int32_t)0, (size_t)n + 1, rocprim::plus<int32_t>(), s));
    F3D_TRY(hipMemsetAsync(w, 0, sizeof(fo_words), s));
    F3D_TRY(hipMemsetAsync(slot, 0xff, (size_t)n * 4, s));
    F3D_TRY(hipMemsetAsync(order, 0xff, (size_t)n * 8, s));
    F3D_TRY(hipMemsetAsync(coffs, 0, 8, s));
    hipLaunchKernelGGL(k_fo_seeds, g, b, 0, s, kb, n, cid, coffs, order, slot, F[0], FC[0], w);
    F3D_TRY(hipMemsetAsync(best, 0xff, (size_t)n * 8, s));

    fo_words hw;
    int cur = 0;
    for (;;) {
        for (int lv = 0; lv < FO_CHUNK; ++lv, cur ^= 1) {
            hipLaunchKernelGGL(k_fo_expand, gl, b, 0, s, classes, n, offs, nbrs, order, slot, F[cur], w, cur, best, err, F3D_DEVERR_FLOOD);
            hipLaunchKernelGGL(k_fo_count, gl, b, 0, s, n, offs, nbrs, order, F[cur], FC[cur], w, cur, best, cnt, part, i0, i1);
            hipLaunchKernelGGL(k_fo_top, dim3(1), b, 0, s, part, w, cur);
            hipLaunchKernelGGL(k_fo_apply, gl, b, 0, s, cnt, part, w, cur, gx);
            hipLaunchKernelGGL(k_fo_place, gl, b, 0, s, n, offs, nbrs, order, slot, F[cur], FC[cur], w, cur, best, gx, i0, i1, F[cur ^ 1],
                               FC[cur ^ 1]);
        }
        F3D_TRY(hipGetLastError());
        F3D_TRY(hipMemcpyAsync(&hw, w, sizeof(hw), hipMemcpyDeviceToHost, s));
        F3D_TRY(hipStreamSynchronize(s));
        ++stats[3];
        if (hw.nf[cur] == 0) break;
        if (stats[3] * FO_CHUNK > n + 2 * FO_CHUNK) return hipErrorUnknown;   // every level places a point: cannot happen
    }
    hipLaunchKernelGGL(k_fo_boundary, g, b, 0, s, classes, n, offs, nbrs, root, slot, flags);
    int32_t mh = 0;
    int64_t lh = 0;
    F3D_TRY(hipMemcpyAsync(&mh, cid + n, 4, hipMemcpyDeviceToHost, s));
    F3D_TRY(hipStreamSynchronize(s));
    if (mh > 0) F3D_TRY(hipMemcpyAsync(&lh, coffs + mh, 8, hipMemcpyDeviceToHost, s));
    F3D_TRY(hipStreamSynchronize(s));
    stats[0] = mh; stats[1] = lh; stats[2] = hw.levels;
    return hipGetLastError();
}
