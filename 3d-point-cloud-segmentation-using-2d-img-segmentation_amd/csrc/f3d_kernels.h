// Internal interface between the C-ABI layer (f3d_ctx.cpp, f3d_capi.cpp) and the kernel sources (f3d_*.hip), and the launch helpers they share.
#pragma once
#include <hip/hip_runtime.h>
#include <float.h>
#include <stdint.h>
#include <atomic>
#include "f3d.h"
#include "f3d_math.h"

// sticky device error word of a context: one bit per operation, so that an IndexError recorded by one operation is
// neither blamed on nor silently skips another one that shares the context
#define F3D_DEVERR_FUSE 1                  // project_vote_argmax: a sampled label > nclasses (voting.py:98)
#define F3D_DEVERR_VOTE 2                  // vote_uv2pt: point index or label out of bounds (voting.py:98)
#define F3D_DEVERR_CC 4                    // components_same_class: neighbour index out of bounds
#define F3D_DEVERR_FLOOD 8                 // flood_order: neighbour index out of bounds
#define F3D_DEVERR_COLOR 16                // color_segment: neighbour or seed index out of bounds
#define F3D_DEVERR_QUADS 32                // door_window_quads: triangle vertex index out of bounds
#define F3D_DEVERR_GROW 64                 // region_grow: seed or neighbour index out of bounds, or a repeated seed
#define F3D_DEVERR_PVOTE 128               // point_vote_frames: a pixel with a neighbour carries a label > nclasses (voting.py:257)
#define F3D_DEVERR_MESH 256                // meshUtils: triangle vertex index outside [0, nv)
#define F3D_DEVERR_ZVOTE 512               // vote_visible: a visible sample's label >= ncols (voting.py:98)
#define F3D_DEVERR_PLANES 1024             // extract_planes: neighbour index outside [0, n)
#define F3D_DEVERR_RASTER 2048             // mesh z-buffer: triangle vertex index outside [0, nv)
#define F3D_DEVERR_SMOOTH 4096             // smooth_votes / smooth_segment: neighbour index outside [0, n), or offsets not ascending
#define F3D_DEVERR_LIFT 8192               // lift_overlaps / lift_instances: an instance id > max_ids or a lookup >= npoints
#define F3D_DEVERR_ALL 16383
#define F3D_PLANES_PER_LAUNCH 16
#define F3D_OBB_MAX_BOXES 4096
#define F3D_SORT_MAX_CELLS 32767            // + 1 overflow cell = 2^15 keys -> 16 key bits sorted
#define F3D_BLOCK 256                       // threads per block of the f3d_kernels.hip / f3d_fuse.hip kernels
#define F3D_GRID_CAP (256 * 8 * 4)          // their usual grid cap: 256 CUs x 8 blocks, x4 so that tails stay short

// f3d_debug_grid_cap (test hook), one per process: blocks > 0 is a further upper bound of every f3d_grid_for, 0 = off.  calls counts the
// f3d_grid_for calls made while it is on, lowered those whose grid it made smaller.  Relaxed atomics: launchers run on any host thread.
struct f3d_grid_debug { std::atomic<int> blocks{0}; std::atomic<long long> calls{0}, lowered{0}; };
inline f3d_grid_debug f3d_grid_debug_state;
inline int f3d_grid_debug_cap() { return f3d_grid_debug_state.blocks.load(std::memory_order_relaxed); }

// blocks of a grid-stride launch over n items, per_block items per block: ceil(n / per_block) clamped to [1, cap].  Every kernel launched
// with this grid walks its items with a gridDim.x stride, so no result depends on the value: the debug cap may lower it further (never
// below 1, never above what it would have been) to drive a small input through many passes per block.
inline int f3d_grid_for(int64_t n, int per_block, int cap) {
    int64_t g = (n + per_block - 1) / per_block;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    const int dbg = f3d_grid_debug_cap();
    if (dbg > 0) {
        f3d_grid_debug_state.calls.fetch_add(1, std::memory_order_relaxed);
        if (g > dbg) { g = dbg; f3d_grid_debug_state.lowered.fetch_add(1, std::memory_order_relaxed); }
    }
    return (int)g;
}

// returns a failed HIP call's error from the enclosing function
#define F3D_TRY(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return e_; } while (0)

// bits of a radix key: the smallest b >= min_bits with 2^b >= v, i.e. rounded up, 2^b itself needs b bits (v = number of key
// values, so keys 0 .. m take f3d_bits_for(m + 1, ..)); min_bits = 1 where a sort must order at least one bit
inline int f3d_bits_for(int64_t v, int min_bits) { int b = min_bits; while (((int64_t)1 << b) < v) ++b; return b; }

// offsets of the pieces of a scratch buffer: each piece starts on a 256-byte boundary; `off` ends as the total size
struct f3d_carve {
    size_t off = 0;
    size_t take(size_t bytes) { const size_t at = off; off += (bytes + 255) & ~(size_t)255; return at; }
};

// inclusive-to-exclusive scan of one int / uint32 per thread over a workgroup of NT threads (lds: NT of them): ex = sum of the values
// of the threads before this one, tot = the workgroup's sum.  Every thread of the workgroup must call it.
template <int NT, typename T>
__device__ __forceinline__ void f3d_block_scan(T v, T* lds, T& ex, T& tot) {
    const int t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
    for (int d = 1; d < NT; d <<= 1) {
        const T x = t >= d ? lds[t - d] : 0;
        __syncthreads();
        lds[t] += x;
        __syncthreads();
    }
    ex = lds[t] - v;
    tot = lds[NT - 1];
    __syncthreads();
}

// Lock-free union-find over int32 parents (f3d_cc.hip, f3d_mesh.hip, f3d_planes.hip): the larger root is always linked under the smaller one, so
// every component ends rooted at its minimum index.  Parent reads are agent-scope relaxed atomic loads (served by L2): a CU's L1
// is not coherent with other CUs' atomics, and the CAS return value -- always current -- drives the retry.
__device__ __forceinline__ int32_t f3d_uf_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int32_t f3d_find_root(int32_t* parent, int32_t x) {
    for (;;) {
        const int32_t p = f3d_uf_load(parent + x);
        if (p == x) return x;
        const int32_t gp = f3d_uf_load(parent + p);
        if (gp != p) __hip_atomic_store(parent + x, gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // path halving (any ancestor is valid)
        x = p;
    }
}

// the root of x by a read-only walk (after the links: compression passes, nothing is written)
__device__ __forceinline__ int32_t f3d_uf_root(const int32_t* parent, int32_t x) {
    for (;;) { const int32_t p = f3d_uf_load(parent + x); if (p == x) return x; x = p; }
}

// joins the components of a and b
__device__ __forceinline__ void f3d_uf_link(int32_t* parent, int32_t a, int32_t b) {
    for (;;) {
        a = f3d_find_root(parent, a); b = f3d_find_root(parent, b);
        if (a == b) break;
        if (a < b) { const int32_t t = a; a = b; b = t; }            // a = larger root, goes under b
        const int32_t old = atomicCAS(parent + a, a, b);
        if (old == a) break;
        a = old;                                                     // someone else linked a first: continue from there
    }
}

// doubles -> unsigned integers of the same order (min / max by integer atomics; exact in any order)
__device__ __forceinline__ unsigned long long f3d_ord_enc(double x) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(x);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double f3d_ord_dec(unsigned long long u) {
    return __longlong_as_double((long long)((u >> 63) ? (u & 0x7fffffffffffffffull) : ~u));
}

// One level of an ordered FIFO flood run by one workgroup of NT threads (f3d_color.hip, f3d_refine.hip).  `list[0..cnt)` are the
// level's expanding points in queue order.  A child's key is (position of its discoverer in `list` << 32 | position in the
// discoverer's row); the smallest key over all discoverers is the reference's FIFO position.  best[j] = ~0 between levels.
__device__ __forceinline__ unsigned long long f3d_child_key(int expander, int64_t row_pos) {
    return (unsigned long long)expander << 32 | (unsigned long long)row_pos;
}

// expand: every neighbour j with open(j) keeps its smallest key; a neighbour outside [0, n) sets `errbit`.  The caller
// synchronises the workgroup before f3d_flood_place.
template <int NT, typename Open>
__device__ __forceinline__ void f3d_flood_expand(const int32_t* list, int cnt, const int64_t* __restrict__ offs,
                                                 const int32_t* __restrict__ nbrs, int64_t n, unsigned long long* best, int* err, int errbit,
                                                 Open open) {
    for (int i = threadIdx.x; i < cnt; i += NT) {
        const int64_t v = list[i];
        const int64_t e0 = offs[v], e1 = offs[v + 1];
        for (int64_t e = e0; e < e1; ++e) {
            const int64_t j = nbrs[e];
            if (j < 0 || j >= n) { atomicOr(err, errbit); continue; }
            if (!open(j)) continue;
            atomicMin(best + j, f3d_child_key(i, e - e0));
        }
    }
}

// place: the children in key order into qn (a block scan of the per-expander counts, NT expanders at a time); mark(j) records
// that j is enqueued, best[j] is reset.  Every thread of the workgroup must call it.  -> the number of children
template <int NT, typename Mark>
__device__ __forceinline__ int f3d_flood_place(const int32_t* list, int cnt, const int64_t* __restrict__ offs,
                                               const int32_t* __restrict__ nbrs, int64_t n, unsigned long long* best, int32_t* qn, int* lds,
                                               Mark mark) {
    const int t = threadIdx.x;
    int carry = 0;
    for (int b = 0; b < cnt; b += NT) {
        const int i = b + t;
        int c = 0;
        int64_t e0 = 0, e1 = 0;
        if (i < cnt) {
            const int64_t v = list[i];
            e0 = offs[v]; e1 = offs[v + 1];
            for (int64_t e = e0; e < e1; ++e) {
                const int64_t j = nbrs[e];
                if (j < 0 || j >= n) continue;
                if (best[j] == f3d_child_key(i, e - e0)) ++c;
            }
        }
        int ex, tot;
        f3d_block_scan<NT>(c, lds, ex, tot);
        if (i < cnt) {
            int pos = carry + ex;
            for (int64_t e = e0; e < e1; ++e) {
                const int64_t j = nbrs[e];
                if (j < 0 || j >= n) continue;
                if (best[j] != f3d_child_key(i, e - e0)) continue;
                qn[pos++] = (int32_t)j;
                mark(j);
                best[j] = ~0ull;
            }
        }
        carry += tot;
    }
    return carry;
}

struct f3d_cellgrid {                      // device-resident description of the cell-sort grid
    double lo[3];
    double inv_cell[3];
    int dim[3];                            // cells per axis = 1 << bits[c]
    int bits[3];                           // key bits given to each axis
    int ncells;                            // key space (last key: non-finite points)
};

struct f3d_graphgrid {                     // uniform grid of the radius graph (by-value kernel argument)
    double lo[3];
    double inv_cell;                       // 1 / cell edge; the edge is a hair above the query radius
    int dim[3];
    int pad;
};

struct f3d_nrmgrid {                       // cell grid of the normal estimation (by-value kernel argument)
    double lo[3];                          // bounding box corner of the whole batch
    double inv_cell;                       // 1 / cell edge; the edge is a hair above the query radius
    int dim[3];                            // cells per axis, dim[c] <= 1 << (shift[c + 1] - shift[c])
    int shift[4];                          // key = frame << shift[3] | cz << shift[2] | cy << shift[1] | cx  (shift[0] = 0)
    int key_bits;                          // bits the radix sort orders (<= 63: key + 1 never wraps)
};

// cell of a point in a neighbour grid (f3d_graphgrid, f3d_nrmgrid)
template <typename G>
__device__ __forceinline__ void f3d_cell_of(const G& g, double x, double y, double z, int& cx, int& cy, int& cz) {
    // clamped: rounding at the upper faces of the box must not leave the grid
    cx = min(g.dim[0] - 1, max(0, (int)floor((x - g.lo[0]) * g.inv_cell)));
    cy = min(g.dim[1] - 1, max(0, (int)floor((y - g.lo[1]) * g.inv_cell)));
    cz = min(g.dim[2] - 1, max(0, (int)floor((z - g.lo[2]) * g.inv_cell)));
}

// a built f3d_graphgrid (f3d_launch_graph_grid): cell-sorted float64 copy, caller-order index of every sorted point, [first, last) of every cell
struct f3d_gridview { const double* sorted; const uint32_t* perm; const int2* cells; };
struct f3d_box { double lo[3], hi[3]; };
// what a radius search over a built grid needs besides the view: the grid, the cloud's box grown by one cell (a point outside it is
// more than one cell, hence more than r, from every cloud point) and the reduced radius r * r (-1: nothing matches)
struct f3d_gridsearch { f3d_graphgrid g; f3d_box reach; double r2; };
inline int64_t f3d_ncells(const f3d_graphgrid& g) { return (int64_t)g.dim[0] * g.dim[1] * g.dim[2]; }

// (false for NaN as well)
__device__ __forceinline__ bool f3d_in_box(const f3d_box& b, double x, double y, double z) {
    return x >= b.lo[0] && x <= b.hi[0] && y >= b.lo[1] && y <= b.hi[1] && z >= b.lo[2] && z <= b.hi[2];
}
// neither NaN nor infinite (sklearn rejects such coordinates)
__device__ __forceinline__ bool f3d_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }
__device__ __forceinline__ bool f3d_finite(double x, double y, double z) { return f3d_finite(x) && f3d_finite(y) && f3d_finite(z); }

// The radius search of the radius graph, the radius query, the point vote and the k-nearest search: hit(k, d) for every sorted point k
// of the grid with d = |p - sorted[k]|^2 <= r2, until hit returns true (-> true: it did).  The cell edge is above r, so every match lies in the <= 27 cells around p's own;
// they are visited dz outer, dy, dx inner, each cell's points in ascending k.  p may lie up to one cell outside the grid (f3d_in_box
// of the reach box): f3d_cell_of clamps its cell, which never moves two points more than one cell apart, and every candidate still
// gets the exact test.  That test is the leaf test of sklearn's KDTree, operation for operation (sklearn/metrics/_dist_metrics:
// euclidean_rdist accumulates tmp * tmp over the 3 coordinates left to right; query_radius compares it with r * r, inclusive).
template <typename Hit>
__device__ __forceinline__ bool f3d_grid_walk_d2(const f3d_gridview& gv, const f3d_graphgrid& g, double px, double py, double pz, double r2,
                                                 Hit hit) {
    int cx, cy, cz;
    f3d_cell_of(g, px, py, pz, cx, cy, cz);
    bool stop = false;                                                             // (a flag, not a return: it folds away when hit is constant)
    for (int dz = -1; dz <= 1 && !stop; ++dz) {
        const int z = cz + dz;
        if (z < 0 || z >= g.dim[2]) continue;
        for (int dy = -1; dy <= 1 && !stop; ++dy) {
            const int y = cy + dy;
            if (y < 0 || y >= g.dim[1]) continue;
            for (int dx = -1; dx <= 1 && !stop; ++dx) {
                const int x = cx + dx;
                if (x < 0 || x >= g.dim[0]) continue;
                const int2 range = gv.cells[(z * g.dim[1] + y) * g.dim[0] + x];
                for (int k = range.x; k < range.y; ++k) {
                    const double t0 = px - gv.sorted[3 * (int64_t)k], t1 = py - gv.sorted[3 * (int64_t)k + 1], t2 = pz - gv.sorted[3 * (int64_t)k + 2];
                    const double d = (t0 * t0 + t1 * t1) + t2 * t2;                // euclidean_rdist, left to right
                    if (d <= r2 && hit(k, d)) { stop = true; break; }
                }
            }
        }
    }
    return stop;
}

// the same search for callers that need the position only: hit(k)
template <typename Hit>
__device__ __forceinline__ bool f3d_grid_walk(const f3d_gridview& gv, const f3d_graphgrid& g, double px, double py, double pz, double r2,
                                              Hit hit) {
    return f3d_grid_walk_d2(gv, g, px, py, pz, r2, [&](int k, double) { return hit(k); });
}

// the K smallest (d2, j) seen so far, ascending; empty slots are (+inf, INT_MAX)
template <int K>
struct topk {
    double d[K];
    int j[K];
    __device__ __forceinline__ void init() {
#pragma unroll
        for (int s = 0; s < K; ++s) { d[s] = INFINITY; j[s] = 0x7fffffff; }
    }
    __device__ __forceinline__ static bool less(double da, int ja, double db, int jb) { return da < db || (da == db && ja < jb); }
    __device__ __forceinline__ void insert(double dn, int jn) {
        if (!less(dn, jn, d[K - 1], j[K - 1])) return;
        d[K - 1] = dn; j[K - 1] = jn;                        // replaces the worst, then sinks to its place
#pragma unroll
        for (int s = K - 1; s >= 1; --s) {
            const bool sw = less(d[s], j[s], d[s - 1], j[s - 1]);
            const double da = d[s - 1], db = d[s];
            const int ja = j[s - 1], jb = j[s];
            d[s - 1] = sw ? db : da; d[s] = sw ? da : db;
            j[s - 1] = sw ? jb : ja; j[s] = sw ? ja : jb;
        }
    }
};

struct f3d_plane_args {                    // by-value kernel argument of k_inside_polyhedra
    int m;
    int accumulate;                        // 1: AND into the existing `inside` bytes (chained launches)
    double pt[F3D_PLANES_PER_LAUNCH][3];
    double n[F3D_PLANES_PER_LAUNCH][3];
};

struct f3d_filter_args {                   // filter_classes of VotingSegmentation.segment
    int nfilter;                           // 0 = no filter
    int cls[8];                            // the list itself when nfilter <= 8 (unused slots = -1)
    const int* cls_dev;                    // device copy of the list when nfilter > 8
    const int* cls_host;                   // host copy of the whole list (the context's staging array; NULL when nfilter == 0)
};

// k-th entry of filter_classes: short lists travel in the kernarg, long ones in device memory
__device__ __forceinline__ int f3d_filter_at(const f3d_filter_args& flt, int k) {
    return (flt.nfilter <= 8) ? flt.cls[k & 7] : flt.cls_dev[k];
}

// device-resident code book of the fused path's vote bins (built per call by k_mask_presence + k_code_lut, f3d_fuse.hip)
struct f3d_codebook {
    uint8_t lut[256];                      // label -> bin code (0 = no sample / absent label, 1 = rejected label, ...)
    uint8_t inv[256];                      // bin code -> label (must follow lut directly: the kernels stage both with one copy)
    uint16_t cmin[256];                    // (must follow inv directly) cmin[t]: votes below which max / t < threshold (k_threshold_table)
    int ncodes, words, book, pad;          // bins in use, histogram dwords per thread = (ncodes + 3) / 4, 1 presence / 2 filter book,
                                           // pad = 1: the book states that no label above nclasses occurs in the masks (presence book only)
    unsigned presence[8];                  // bit l: label l occurs in the masks
};

hipError_t f3d_launch_clear_error_bits(int* err, int bits, hipStream_t s);
hipError_t f3d_launch_rotate(const double* xyz, int64_t n, const double q[4], double* out, hipStream_t s);
hipError_t f3d_launch_unproject_depth(const void* depth, int depth_type, int h, int w, const double K[9], double scale,
                                      const double q[4], const double t[3], double* out, hipStream_t s);
hipError_t f3d_launch_project_view(const void* xyz, int dtype, int64_t n, const f3d_view& vw, int32_t* uv, uint8_t* inside,
                                   hipStream_t s);
hipError_t f3d_launch_inside_polyhedra(const void* xyz, int dtype, int64_t n, const f3d_plane_args& pa, uint8_t* inside,
                                       hipStream_t s);
#define F3D_CODE_MAX_NCLASSES 253            // labels 0..nclasses + "rejected" + "no sample" must fit the 256 byte codes
// The SLOT_TODO scratch of a fused call: 4 counters (first list, second list, the exact kernel's list of a call
// with more than 255 views, the wave-tiles k_fuse took out of their view loops early); two index lists of n entries (fast kernel -> float64 tier -> exact kernel); then per parked slot of
// the first list the open-view masks (ngroups words of 64 views) and, behind all of those, the parked bins (park_stride dwords each).
struct f3d_fuse_todo {
    size_t bytes, list2_off, umask_off, park_off;      // of the whole block; byte offsets (the counters and the first list have fixed ones)
    int park_slots, park_stride, ngroups;
    static unsigned int* counters(void* base) { return reinterpret_cast<unsigned int*>(base); }
    static int32_t* list(void* base) { return reinterpret_cast<int32_t*>(reinterpret_cast<char*>(base) + 4 * sizeof(unsigned int)); }
    int32_t* list2(void* base) const { return reinterpret_cast<int32_t*>(reinterpret_cast<char*>(base) + list2_off); }
    unsigned long long* umask(void* base) const { return reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(base) + umask_off); }
    uint32_t* park(void* base) const { return reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(base) + park_off); }
};
f3d_fuse_todo f3d_fuse_todo_layout(int64_t n, int nviews, int nclasses);   // (reads F3D_DEBUG_PARK_SLOTS: once per C-ABI call, handed down)
size_t f3d_fuse_tables_bytes(int nviews);
size_t f3d_fuse_carry_bytes(int64_t n, int nclasses);
// One fused launch.  perm (device, may be NULL): caller-order index of sorted point i.  gather = false: xyz is already the sorted copy;
// gather = true: xyz is the caller's cloud and the kernel reads point perm[i].  cmasks: the coded, tiled copy of masks (read by the fast
// kernel), or NULL when nclasses > F3D_CODE_MAX_NCLASSES -- the exact kernel then labels every point from the raw masks.  carry == NULL:
// one launch over all views (v0, v1 ignored).  Otherwise the views [v0, v1) of a view-chunked call: `carry` holds f3d_fuse_carry_bytes
// of scratch that survives from the chunk with v0 == 0 to the one with v1 == nviews; chunks ascending without gaps; no vote output.
// xyz_keep (may be NULL; first chunk with gather only): receives the cloud in perm order -- the caller passes it as xyz from then on.
// Blocks of a k_fuse instance a CU holds at a time, by (kernel, dynamic LDS bytes): asked of the runtime once and kept by the context
// (the deal of tiles to blocks is sized by it, f3d_fuse_deal.h).  Zero-initialised = empty.
struct f3d_fuse_occupancy {
    struct entry { const void* kernel; size_t lds; int blocks_per_cu; } e[32];
    int n, cus;
};
struct f3d_fuse_job {
    const void* xyz; int dtype; int64_t n; const int32_t* perm; bool gather;        // the cloud
    const f3d_view* views_dev; int nviews, v0, v1;                                  // the views
    const uint8_t *masks, *cmasks; int h, w;                                        // their masks
    int nclasses; f3d_filter_args flt; double threshold;                            // the vote rule
    int64_t* classes; uint16_t* votes; int* err;                                    // outputs (votes may be NULL)
    void* todo; f3d_fuse_todo lay;                                                  // scratch: the todo block and its layout,
    const f3d_codebook* cb; void* tables; uint32_t* carry; void* xyz_keep;          //   the code book, f3d_fuse_tables_bytes(nviews), ...
    hipStream_t stream;
    bool filled;                                                                    // the label fill has been done (a rider of the cell sort)
    f3d_fuse_occupancy* occ;                                                        // the context's cache (NULL: the stated blocks per CU are assumed)
};
hipError_t f3d_launch_fuse(const f3d_fuse_job& job);
// Before f3d_launch_fuse, on any stream that is joined into its stream: the threshold table of the code book (segment_point) and the
// transposed tables of the job's views [v0, v1); v0 == 0 zeroes the deferred lists' counters.  with_book: an extra block builds the code book
hipError_t f3d_launch_fuse_setup(const f3d_fuse_job& job, f3d_codebook* cb, bool with_book);
// the one-shot call: presence -> [setup + book in one launch] -> job.masks coded into `coded` (f3d_coded_masks_bytes)
hipError_t f3d_launch_code_masks_with_setup(const f3d_fuse_job& job, uint8_t* coded, f3d_codebook* cb);
hipError_t f3d_launch_mask_presence(const uint8_t* src, int64_t nbytes, f3d_codebook* cb, hipStream_t s);
hipError_t f3d_launch_presence_bytes(f3d_codebook* cb, uint8_t* bytes256, bool to_bytes, hipStream_t s);
hipError_t f3d_launch_code_book(f3d_codebook* cb, int nclasses, const f3d_filter_args& flt, bool want_votes, hipStream_t s);
// masks [V,H,W] row-major labels -> 8x8-pixel tiles of vote-bin codes (any H, W) with the book as it stands; dst holds f3d_coded_masks_bytes()
hipError_t f3d_launch_code_planes(const uint8_t* src, uint8_t* dst, int nviews, int h, int w, const f3d_codebook* cb, hipStream_t s);
size_t f3d_coded_masks_bytes(int nviews, int h, int w);
// audit of the fast projection (tests only): for every (point, view) pair inside the frustum counts
// stats[0] pairs, stats[1] pairs sent to the exact fallback, stats[2] accepted pairs whose floor differs from the
// canonical path (must stay 0), stats[3] pairs rejected/accepted by the f32 cull that the exact test contradicts (0)
hipError_t f3d_launch_fastpath_audit(const void* xyz, int dtype, int64_t n, const f3d_view* views_dev, int nviews, int w, int h,
                                     unsigned long long* stats_dev, hipStream_t s);
// cell sort (f3d_sort.hip): perm (and sorted_xyz unless NULL) receive the cloud in grid-cell order; scratch >= f3d_sort_scratch_bytes(n)
size_t f3d_sort_scratch_bytes(int64_t n);
// riders (internal, f3d_fuse_blocks.h; NULL = none): streaming work of the fused call that depends on nothing the sort produces and runs
// as extra blocks of the sort's launches -- label presence beside pass 1, the label fill beside the high-byte histogram (a small cloud:
// beside pass 1), k_fuse_setup with the book inside the second scan's launch, mask coding beside pass 2.  Ordering between them comes
// from the launches alone.
struct f3d_sort_riders;
hipError_t f3d_launch_cell_sort(const void* xyz, int dtype, int64_t n, void* sorted_xyz, int32_t* perm, void* scratch, hipStream_t s,
                                const f3d_sort_riders* riders = nullptr);
// Block b of a launch of `grid` blocks of which `extra` are riders, spread evenly through the grid (blocks are dispatched in index order:
// riders at the end would start when the host kernel's own work is nearly over).  The riders before block b number floor(b * extra / grid);
// b is a rider when that count steps at b + 1.  index: the rider's number 0..extra-1, or the host kernel's own block number 0..grid-extra-1.
struct f3d_block_role { bool rider; int index; };
__host__ __device__ inline f3d_block_role f3d_rider_role(unsigned b, unsigned grid, unsigned extra) {
    const unsigned before = (unsigned)(((unsigned long long)b * extra) / grid);
    const unsigned upto = (unsigned)(((unsigned long long)(b + 1) * extra) / grid);
    f3d_block_role r;
    r.rider = upto != before;
    r.index = r.rider ? (int)before : (int)(b - before);
    return r;
}
// Which run of a sorted tile a position lies in, without a byte per position (pass 1 of the cell sort, f3d_sort.hip: its record carries
// the OTHER byte of the key).  The tile's keys stand in runs of equal digit value; a run is known by its rank among the non-empty runs.
//   starts[w]  64-bit word w of a bitmap over the tile's positions: bit p & 63 of word p >> 6 is set when a run starts at position p
//   before[w]  the runs that start in front of word w's first position (before[0] = 0)
// The owner of a non-empty run (start, count, rank) sets the run's bit and writes rank + 1 to before[w] of every word w whose first
// position comes after the run's start and no later than one past the run's end: the run that holds position 64 w - 1 is the last one
// that starts in front of word w.  f3d_run_span_of gives the bit and that range of words (first > last: none; nwords = words of the tile,
// no entry beyond it is ever read); f3d_run_at turns a position's word, its `before` entry and its bit number into the rank of its run.
struct f3d_run_span { unsigned word, bit, first, last; };
__host__ __device__ inline f3d_run_span f3d_run_span_of(unsigned start, unsigned count, unsigned nwords) {
    f3d_run_span s;
    s.word = start >> 6; s.bit = start & 63u;
    s.first = (start >> 6) + 1u;
    s.last = (start + count) >> 6;
    if (s.last > nwords - 1u) s.last = nwords - 1u;
    return s;
}
__host__ __device__ inline unsigned f3d_run_at(unsigned long long word, unsigned before, unsigned bit) {
    return before + (unsigned)__builtin_popcountll(word & ((2ull << bit) - 1ull)) - 1u;      // (bit 63: 2 << 63 wraps to 0, - 1 = all ones)
}
// the one-shot call that sorts and codes: the cell sort carrying the work of f3d_launch_code_masks_with_setup and the label fill as
// riders (f3d_fuse.hip).  Sets job.filled; the caller sets job.cmasks = coded and must not call f3d_launch_code_masks_with_setup.
hipError_t f3d_launch_cell_sort_with_riders(f3d_fuse_job& job, uint8_t* coded, f3d_codebook* cb, int32_t* perm, void* sort_scratch);
// same-class connected components (f3d_cc.hip): root[i] = smallest index of i's component; parent = int32 [n] scratch
hipError_t f3d_launch_components(const int64_t* classes, int64_t n, const int64_t* offs, const int32_t* nbrs, int32_t* parent,
                                 int64_t* root, int* err, hipStream_t s, int errbit = F3D_DEVERR_CC);
// ordered same-class flood of CVSegmentation.instance_seperate (f3d_cc.hip): the clusters of the classes inst[0..k) (processing order)
// concatenated in the reference's pop order.  root [n]; order [n] (first stats[1] used, the rest -1); coffs [n + 1] (first stats[0] + 1
// used); flags [n] boundary points.  Synchronises the stream (the frontier length is read back every few levels); stats (host) =
// {clusters, points in clusters, levels, readbacks}.  scratch: f3d_flood_scratch_bytes(n)
size_t f3d_flood_scratch_bytes(int64_t n);
hipError_t f3d_launch_flood_order(const int64_t* classes, int64_t n, const int64_t* offs, const int32_t* nbrs, const int64_t* inst, int k,
                                  int64_t* root, int64_t* order, int64_t* coffs, uint8_t* flags, void* scratch, int* err, int64_t stats[4],
                                  hipStream_t s);
// running-mean colour growing of CVSegmentation.color_segment (f3d_color.hip): one workgroup for the whole seed list; ids [n] in/out;
// seeds device [nseeds]; colors [n, 3] of `dtype`; stats_dev (device int64) += accepted points.  scratch: f3d_color_scratch_bytes(n)
struct f3d_color_args {
    double thr[3];
    int max_level;                         // <= 0: no level limit (the reference's `level == max_level` never holds)
    int nneutral;
    int64_t neutral[F3D_COLOR_MAX_NEUTRAL];
};
size_t f3d_color_scratch_bytes(int64_t n);
hipError_t f3d_launch_color_segment(const void* colors, int dtype, int64_t n, const int64_t* offs, const int32_t* nbrs, int64_t* ids,
                                    const int64_t* seeds, int64_t nseeds, const f3d_color_args& a, void* scratch, int64_t* stats_dev, int* err,
                                    hipStream_t s);
// region growing of segUtils/refinement.py (f3d_refine.hip): one workgroup, one flood.  values [n, nchan] of `dtype`; seeds device
// [nseeds] = the first queue; cluster device int64 [n] receives the accepted points in acceptance order, *count_dev their number.
// scratch: f3d_grow_scratch_bytes(n)
struct f3d_grow_args {
    double thr[3];
    double sma0[3];                        // running mean at the start (exactly representable in the values' dtype)
    int64_t npts0;                         // points the mean counts at the start
    int max_level;                         // <= 0: no level limit
    int seeds_given;                       // 1: the seeds are tested and expanded but neither accepted nor averaged in
};
#define F3D_GROW_MAX_POINTS (0x7fffffffLL - 2048)   // the kernel's int chunk counters step by 1024 past a level's length
size_t f3d_grow_scratch_bytes(int64_t n);
hipError_t f3d_launch_region_grow(const void* values, int dtype, int nchan, int64_t n, const int64_t* offs, const int32_t* nbrs,
                                  const int64_t* seeds, int64_t nseeds, const f3d_grow_args& a, void* scratch, int64_t* cluster,
                                  int64_t* count_dev, int* err, hipStream_t s);
// out[i] = |((x - px) * nx + (y - py) * ny) + (z - pz) * nz| (f3d_refine.hip), float64 points [n, 3]
hipError_t f3d_launch_plane_distance(const double* pts, int64_t n, const double pp[3], const double nr[3], double* out, hipStream_t s);
// radius graph (f3d_graph.hip): KDTree.query_radius(points, r) as CSR.  bbox partials -> host picks the grid -> count pass
// (offsets[n + 1], exclusive scan) -> fill pass; `scratch` (f3d_graph_scratch_bytes) carries the grid between the passes
size_t f3d_graph_bbox_bytes(void);
hipError_t f3d_launch_graph_bbox(const void* xyz, int dtype, int64_t n, void* partial, int* nblocks, hipStream_t s);
int f3d_graph_reduce_bbox(const void* partial_host, int nblocks, double lo[3], double hi[3]);      // 1: non-finite coordinates seen
size_t f3d_graph_scratch_bytes(int64_t n, int64_t ncells);
hipError_t f3d_launch_graph_count(const void* xyz, int dtype, int64_t n, const f3d_gridsearch& gs, void* scratch, int64_t* offsets,
                                  hipStream_t s);
hipError_t f3d_launch_graph_fill(int64_t n, const f3d_gridsearch& gs, const void* scratch, const int64_t* offsets, int32_t* nbrs,
                                 hipStream_t s);
// the grid of the radius graph on its own, for searches that keep no CSR
hipError_t f3d_launch_graph_grid(const void* xyz, int dtype, int64_t n, const f3d_graphgrid& g, void* scratch, f3d_gridview* view,
                                 hipStream_t s);
// radius query (f3d_graph.hip): KDTree(data).query_radius(queries, r) inverted, one row per query in ascending data index.  Grid over
// the m data points (from the f3d_launch_graph_bbox partials).  The count pass enqueues the readback of words_host[0] = nnz and
// words_host[1] = 1 if a query is NaN / infinite (the caller synchronises); the fill pass needs the same queries and the scratch
// (f3d_query_scratch_bytes) of the count pass
size_t f3d_query_scratch_bytes(int64_t m, int64_t n, int64_t ncells);
hipError_t f3d_launch_query_count(const void* data, int ddtype, int64_t m, const void* queries, int qdtype, int64_t n, const f3d_gridsearch& gs,
                                  void* scratch, int64_t* offsets, int64_t* words_host, hipStream_t s);
hipError_t f3d_launch_query_fill(const void* queries, int qdtype, int64_t m, int64_t n, const f3d_gridsearch& gs, void* scratch,
                                 const int64_t* offsets, int32_t* nbrs, hipStream_t s);
// hybrid k-nearest search and label transfer (f3d_knn.hip): per query the <= k data points within the radius that are smallest under
// (d2, caller-order data index), over a grid built by f3d_launch_graph_grid.  K_MAX bounds k; flag: device word, bit 0 raised by
// f3d_launch_knn_flag when a query is NaN / infinite (cleared by the caller).  Enqueue only; every offset is 64-bit.
#define F3D_KNN_MAX_K 32
hipError_t f3d_launch_knn_flag(const void* queries, int qdtype, int64_t n, unsigned* flag, hipStream_t s);
hipError_t f3d_launch_knn_query(const void* queries, int qdtype, int64_t n, int k, const f3d_gridview& gv, const f3d_gridsearch& gs,
                                int32_t* idx, double* dist2 /* may be NULL */, int32_t* counts /* may be NULL */, hipStream_t s);
hipError_t f3d_launch_knn_labels(const void* queries, int qdtype, int64_t n, int k, const f3d_gridview& gv, const f3d_gridsearch& gs,
                                 const int64_t* labels, int64_t fill, int64_t* out, int32_t* support /* may be NULL */, hipStream_t s);

// surface normals (f3d_normals.hip): F frames of n float64 points, grid chosen on the host from the f3d_launch_graph_bbox partials;
// cams device [F, 3].  Enqueue only.  scratch: f3d_normals_scratch_bytes(F * n)
size_t f3d_normals_scratch_bytes(int64_t total);
hipError_t f3d_launch_normals(const double* xyz, int nframes, int64_t n, const f3d_nrmgrid& g, double r2, int max_nn, const double* cams,
                              int orient, void* scratch, double* normals, int32_t* counts, int32_t* nbrs, hipStream_t s);
// a5 patch matching (f3d_patch.hip): owner[p] = first seed (lowest index) whose window covers free pixel p and accepts it, -1 if none
size_t f3d_patch_scratch_bytes(int h, int w, int64_t m);
hipError_t f3d_launch_patch_owner(const int32_t* uv, int64_t m, int h, int w, int half, double radius, double min_cosine,
                                  const double* seed_pts, const double* seed_nrm, const double* q_pts, const double* q_nrm,
                                  const uint8_t* free_px, int32_t* owner, void* scratch, hipStream_t s);
hipError_t f3d_launch_patch_seeds(const double* pts, const double* nrm, const int32_t* prio, const uint8_t* free_px, int h, int w, int half,
                                  double radius, double min_cosine, int32_t* status, int32_t* owner, int32_t* counter, int* rounds,
                                  hipStream_t s);
// ordered per-seed sums of the rows of up to three [h*w, 3] arrays over the pixels each seed owns (uv != NULL: seeds of Fusion.fuse at
// their projections, m of them; uv == NULL: the self-owning pixels of patch_downsample, m = h*w); sums [m, 9], counts [m]
hipError_t f3d_launch_patch_sums(const int32_t* owner, const int32_t* uv, int64_t m, int h, int w, int half, const double* rows_a,
                                 const double* rows_b, const double* rows_c, double* sums, int32_t* counts, hipStream_t s);
// the per-frame steps of Fusion.fuse_device on a device-resident cloud (f3d_fusion.hip); scratch: f3d_fusion_scratch_bytes(n) for a
// compaction of n flags (hits: n = cloud rows, new seeds: n = h*w)
size_t f3d_fusion_scratch_bytes(int64_t n);
hipError_t f3d_launch_fusion_hits(const uint8_t* inside, const int32_t* uv_all, int64_t n, const int64_t* count, const double* pts,
                                  const double* nrm, const uint8_t* valid, int64_t npx, int32_t* ids, int32_t* uv, double* hit_pts,
                                  double* hit_nrm, int64_t* stats, void* scratch, hipStream_t s);
hipError_t f3d_launch_fusion_seed_update(const int32_t* ids, int64_t m, const double* sums, const int32_t* counts, int mode, double* pts,
                                         double* nrm, double* clr, int64_t* nmerges, uint32_t* occ, hipStream_t s);
hipError_t f3d_launch_fusion_lookup(const int32_t* owner, const int32_t* ids, int64_t npx, int32_t* uv2pt, uint8_t* free_px, hipStream_t s);
hipError_t f3d_launch_fusion_check(const uint8_t* free_px, const double* pts, const double* nrm, int64_t npx, double radius,
                                   double min_cosine, int64_t* stats, hipStream_t s);
hipError_t f3d_launch_fusion_prio(const int64_t* order, int64_t npx, int32_t* prio, hipStream_t s);
hipError_t f3d_launch_fusion_new_seeds(const int32_t* owner, const int32_t* prio, const double* sums, const int32_t* counts, int64_t npx,
                                       int mode, int64_t* count, int64_t cap, double* pts, double* nrm, double* clr, int64_t* nmerges,
                                       uint32_t* occ, int32_t* uv2pt, uint8_t* free_px, void* scratch, hipStream_t s);
// a12: remaining intersections.py primitives (f3d_geom.hip), device pointers
hipError_t f3d_launch_ray_x_lines(const double o[3], const double d[3], const double* starts, const double* ends, int64_t n, double* pts,
                                  uint8_t* within, hipStream_t s);
hipError_t f3d_launch_rays_x_plane(const double pp[3], const double pn[3], const double* origins, const double* dirs, int64_t n, double* pts,
                                   uint8_t* valid, hipStream_t s);
hipError_t f3d_launch_lines_x_planes(const double* lo, const double* le, int64_t n, const double* pps, const double* pns, int m, int bmode,
                                     double* pts, uint8_t* valid, hipStream_t s);
hipError_t f3d_launch_point_inside_polygon(const double* points, int64_t n, const double* verts, int m, uint8_t* inside, uint8_t* within,
                                           hipStream_t s);
hipError_t f3d_launch_points_plane_projection(const double* points, int64_t n, const double pp[3], const double nr[3], double* out, hipStream_t s);
hipError_t f3d_launch_unit_difference(const double* a, const double* b, int64_t n, double* out, hipStream_t s);
hipError_t f3d_launch_segment_votes(const double* votes, int64_t npts, int ncols, int nclasses, double threshold,
                                    const f3d_filter_args& flt, int64_t* classes, hipStream_t s);
// PointVotingSegmentation.segment: the total is the last column, the unfiltered candidates are the columns before it.  neg: bit k =
// filter_classes[k] was given as a negative index; the remap then writes the class as given (NumPy stores cls_ itself), flt holds
// the column it reads
struct f3d_negmask { uint32_t w[F3D_MAX_FILTER / 32]; };
hipError_t f3d_launch_segment_votes_lastcol(const double* votes, int64_t npts, int ncols, int nclasses, double threshold,
                                            const f3d_filter_args& flt, const f3d_negmask& neg, int64_t* classes, hipStream_t s);
hipError_t f3d_launch_vote_uv2pt(const int32_t* uv2pt, const uint8_t* mask, int64_t hw, double* votes, int64_t npts, int ncols,
                                 unsigned long long* table, uint64_t table_slots, int* err, hipStream_t s);
// batched vote: frames [frame0, frame0 + nframes) of a call; table slots carry `gen` (< 16383), first_bad = device int (INT_MAX = none)
hipError_t f3d_launch_vote_uv2pt_batch(const int32_t* luts, const uint8_t* masks, int nframes, int h, int w, double* votes, int64_t npts,
                                       int ncols, unsigned long long* table, uint64_t table_slots, unsigned gen, int frame0, int* first_bad,
                                       int* err, hipStream_t s);
hipError_t f3d_launch_sem_to_mask(const float* sem, int nimg, int c, int64_t hw, float conf, int low_label, uint8_t* mask, hipStream_t s);
// aabb: float [6 * b] of device scratch (the boxes' padded float32 bounds, filled by the launch); cells: f3d_obb_cells_bytes() of
// 8-byte aligned device scratch (the cell table of a call with 8 .. 64 boxes; NULL: every point visits every box)
size_t f3d_obb_cells_bytes();
hipError_t f3d_launch_points_in_obb(const void* xyz, int dtype, int64_t n, const f3d_obb* boxes_dev, int b, float* aabb, void* cells, uint32_t* bits,
                                    uint8_t* cooc, hipStream_t s);
hipError_t f3d_launch_unproject_depth_batch(const void* depth, int depth_type, int nframes, int h, int w, const double K[9], double scale,
                                            const double* q_host, const double* t_host, double* out, hipStream_t s);
hipError_t f3d_launch_relabel(int64_t* ids, int64_t n, int64_t from, int64_t to, unsigned long long* count, hipStream_t s);

// merge_bb support (f3d_obb.hip): grouping of the points by instance id, extreme members along 26 directions, inner-hull filter
#define F3D_OBB_NDIR 26
size_t f3d_group_scratch_bytes(int64_t n, int64_t nids);
hipError_t f3d_launch_group_by_id(const int64_t* ids, int64_t n, int64_t nids, int32_t* order, uint32_t* sorted_keys, int64_t* starts,
                                  void* scratch, hipStream_t s);
hipError_t f3d_launch_obb_extremes(const void* xyz, int dtype, int64_t n, const int32_t* order, const uint32_t* sorted_keys, int64_t nseg,
                                   unsigned long long* table, int32_t* extremes, hipStream_t s);
hipError_t f3d_launch_obb_hull_filter(const void* xyz, int dtype, int64_t n, const int32_t* order, const uint32_t* sorted_keys,
                                      const int64_t* starts, int64_t nseg, const int32_t* fstart, const double* facets, const double* margin,
                                      int32_t* cand, int32_t* cand_count, hipStream_t s);
// the box fit on the device (f3d_hull.hip) and the all-device candidate pipeline (f3d_obb.hip)
#define F3D_OBB_SMALL_FACETS 48              // a triangulated hull of 26 points has at most 2 * 26 - 4 facets
hipError_t f3d_launch_obb_fit(const double* pts, const int64_t* start, int nfit, double* boxes, int32_t* status, uint8_t* isvert, int32_t* vlist,
                              int32_t* nvert, hipStream_t s);
hipError_t f3d_launch_obb_small_hulls(const void* xyz, int dtype, const int32_t* extremes, const int64_t* starts, int64_t nids, int min_members,
                                      double* gathered, uint8_t* isvert, double* facets, int32_t* nfacets, double* margin, hipStream_t s);
size_t f3d_obb_candidates_scratch_bytes(int64_t n, int64_t nids);
hipError_t f3d_launch_obb_candidates(const void* xyz, int dtype, int64_t n, const int32_t* order, const uint32_t* sorted_keys, const int64_t* starts,
                                     int64_t nids, int min_members, unsigned long long* table, void* scratch, int32_t* cand, int64_t* cand_start,
                                     hipStream_t s);
hipError_t f3d_launch_gather_points(const void* xyz, int dtype, const int32_t* idx, int64_t count, double* out, hipStream_t s);
// door / window quads of door_window_bbox.generate_mesh (f3d_quads.hip): pts float64 [n, 3], ids int64 [n], inst int64 [k] (device),
// verts float64 [nv, 3], tris int64 [nt, 3]; quads float64 [k, 4, 3], status / tri int32 [k], normals float64 [nt, 3] (may be NULL).
// Enqueue only.  scratch: f3d_quads_scratch_bytes(n, k, nt)
size_t f3d_quads_scratch_bytes(int64_t n, int k, int64_t nt);
hipError_t f3d_launch_door_window_quads(const double* pts, int64_t n, const int64_t* ids, const int64_t* inst, int k, const double* verts,
                                        int64_t nv, const int64_t* tris, int64_t nt, double* quads, int32_t* status, int32_t* tri,
                                        double* normals, void* scratch, int* err, hipStream_t s);

// fused radius search + frame vote of PointVotingSegmentation.vote (f3d_pointvote.hip).  words: device int[4] = {a label >= ncols
// exists, first frame with a non-finite query coordinate, first frame whose pixel with such a label has a neighbour, spare};
// "none" = F3D_PVOTE_NONE.  bits: the per-frame (point, label) sets, f3d_pvote_bits_bytes(m, ncols, group) bytes.
#define F3D_PVOTE_NONE 0x7f7f7f7f
#define F3D_PVOTE_MAX_GROUP 64               // frames one vote launch covers at most
#define F3D_PVOTE_BITS_BUDGET ((size_t)256 << 20)
int f3d_pvote_words_per_point(int ncols);
int f3d_pvote_group(int64_t m, int ncols);   // frames per vote launch: the bitsets of a group fit the budget (at least 1 frame)
size_t f3d_pvote_bits_bytes(int64_t m, int ncols, int group);
hipError_t f3d_launch_pvote_prepass(const void* queries, int qdtype, const uint8_t* masks, int64_t nframes, int64_t hw, int ncols, int* words,
                                    hipStream_t s);
hipError_t f3d_launch_pvote_validate(const void* queries, int qdtype, const uint8_t* masks, int64_t nframes, int64_t hw, int ncols,
                                     const f3d_gridview& gv, const f3d_gridsearch& gs, int* words, hipStream_t s);
hipError_t f3d_launch_pvote_frames(const void* queries, int qdtype, const uint8_t* masks, int64_t nframes, int64_t hw, int64_t m, int ncols,
                                   const f3d_gridview& gv, const f3d_gridsearch& gs, double* votes, uint32_t* bits, int group,
                                   const int* words, const int* err, hipStream_t s);
hipError_t f3d_launch_pvote_flag(const int* words, int limit, int* err, hipStream_t s);

// meshUtils (f3d_mesh.hip): triangles [nt, 3] of `itype` (F3D_I64 / F3D_I32), vertices [nv, 3] of `vdtype`.  counts: device int64[4] =
// {first size, second size, 1 when a vertex index is outside [0, nv) (then nothing else is written and `errbit` is set), spare}.
// Enqueue only.  scratch: f3d_mesh_scratch_bytes(nv, nt) for every entry
size_t f3d_mesh_scratch_bytes(int64_t nv, int64_t nt);
hipError_t f3d_launch_mesh_vertex_map(const void* tris, int itype, int64_t nt, int64_t nv, int64_t* offsets, int32_t* tri, int8_t* pos,
                                      void* scratch, int64_t* counts, int* err, hipStream_t s);
hipError_t f3d_launch_mesh_remove_faces(const void* tris, int itype, int64_t nt, int64_t nv, const uint8_t* mask, uint8_t* not_removed,
                                        void* remaining, int64_t* old2new, void* scratch, int64_t* counts, int* err, hipStream_t s);
hipError_t f3d_launch_mesh_keep_faces(const void* verts, int vdtype, int64_t nv, const void* tris, int itype, int64_t nt, const uint8_t* mask,
                                      void* out_verts, void* out_tris, void* scratch, int64_t* counts, int* err, hipStream_t s);
hipError_t f3d_launch_mesh_clusters(const void* verts, int vdtype, int64_t nv, const void* tris, int itype, int64_t nt, int32_t* clusters,
                                    int64_t* cluster_n, double* cluster_area, double* tri_area, void* scratch, int64_t* counts, int* err,
                                    hipStream_t s);
hipError_t f3d_launch_mesh_clean(const void* verts, int vdtype, int64_t nv, const void* tris, int itype, int64_t nt, const uint8_t* remove_mask,
                                 int64_t min_triangles, double min_area, void* new_verts, void* new_tris, uint8_t* kept_v, uint8_t* kept_t,
                                 void* scratch, int64_t* counts, int* err, hipStream_t s);
// face frames and the face graph (f3d_mesh.hip, include/f3d.h f3d_mesh_face_frames / f3d_mesh_face_graph): normals / centroids float64
// [nt, 3], areas float64 [nt] (the last two may be NULL; no scratch).  The graph: counts = {nnz, non-manifold edges, bad index, boundary
// edges}; verts may be NULL without a gate; neighbours (room for cap entries, may be NULL) is written only when nnz <= cap.
// scratch: f3d_face_graph_scratch_bytes(nt), whatever nv is
size_t f3d_face_graph_scratch_bytes(int64_t nt);
hipError_t f3d_launch_mesh_face_frames(const void* verts, int vdtype, int64_t nv, const void* tris, int itype, int64_t nt, double* normals,
                                       double* centroids, double* areas, int64_t* counts, int* err, hipStream_t s);
hipError_t f3d_launch_mesh_face_graph(const void* verts, int vdtype, int64_t nv, const void* tris, int itype, int64_t nt, int gate,
                                      double cos_crease, int64_t* offsets, int32_t* neighbours, int64_t cap, void* scratch, int64_t* counts,
                                      int* err, hipStream_t s);

// the sample of point p in view vw, if it has one: pixel (u, v) inside the w x h image, float32 depth z32 in [FLT_MIN, inf)
// (shared by f3d_render.hip and f3d_features.hip; f3d_math.h carries #pragma clang fp contract(off))
__device__ __forceinline__ bool f3d_sample(const f3d_view& vw, f3d_p3 p, int h, int w, int& u, int& v, float& z32) {
    if (!f3d_inside_view(vw, p)) return false;                             // a4 first: most pairs end here
    const f3d_p3 hp = f3d_project_h(vw.K, vw.qinv, vw.t, p);
    u = f3d_floor_to_i32(hp.x / hp.z);
    v = f3d_floor_to_i32(hp.y / hp.z);
    z32 = (float)hp.z;                                                     // round to nearest even
    return u >= 0 && u < w && v >= 0 && v < h && z32 >= FLT_MIN && z32 < INFINITY;   // (NaN fails both depth tests)
}

// point-splat z-buffer and the visibility-tested forward vote (f3d_render.hip).  zkey: uint64 [nv, h, w] depth keys of the nv views of
// a pass (views_dev / masks point at the pass's first view); counts (device uint64 [3], may be NULL) += {samples, cells covered,
// atomics issued}.  Enqueue only.
hipError_t f3d_launch_zkey_fill(unsigned long long* zkey, size_t cells, hipStream_t s);
hipError_t f3d_launch_zsplat(const void* xyz, int dtype, int64_t n, const f3d_view* views_dev, int nv, int h, int w, int splat,
                             unsigned long long* zkey, unsigned long long* counts, hipStream_t s);
// skip (device int, may be NULL): nothing is written when it is set (the mesh entries' bad-index flag).
hipError_t f3d_launch_zkey_unpack(const unsigned long long* zkey, size_t cells, float* depth, int32_t* uv2pt, const int* skip, hipStream_t s);
// mesh_flag == NULL: the keys are a splat of this very cloud (a sample's cell is never empty).  Otherwise they are a mesh's: an empty
// cell counts as +inf, and nothing is written when *mesh_flag is set.
hipError_t f3d_launch_vote_visible(const void* xyz, int dtype, int64_t n, const f3d_view* views_dev, int nv, const uint8_t* masks, int h, int w,
                                   const unsigned long long* zkey, double depth_tol, double* votes, int ncols, const int* mesh_flag, int* err,
                                   hipStream_t s);

// triangle rasteriser into the same keys (f3d_raster.hip).  scratch: f3d_raster_scratch_bytes(capacity of the deferral list), laid out
// by f3d_raster_scratch_layout: a bad-index flag, the list's counter, 4 tier counters, the list.  f3d_launch_raster_check clears the
// first three, flags a corner outside [0, nv) (F3D_DEVERR_RASTER) and zeroes straddling (may be NULL); every later launch returns at
// once under the flag.  f3d_launch_raster rasterises the pass's nv views [view0, view0 + nv) of views_dev into zkey [nv, h, w] (filled
// by f3d_launch_zkey_fill) and adds to straddling[view0 ..]; list_cap <= the capacity the scratch was sized for; stats: count the pairs.
struct f3d_raster_entry { int32_t view, tri, u0, v0, u1, v1; };
struct f3d_raster_scratch { size_t flag, count, stats, entries, bytes; };
#define F3D_RASTER_LIST_CAP (1u << 16)
inline f3d_raster_scratch f3d_raster_scratch_layout(unsigned list_cap) {
    f3d_carve c;
    f3d_raster_scratch l;
    l.flag = c.take(sizeof(int)); l.count = c.take(sizeof(unsigned)); l.stats = c.take(4 * sizeof(unsigned long long));
    l.entries = c.take((size_t)list_cap * sizeof(f3d_raster_entry));
    l.bytes = c.off;
    return l;
}
size_t f3d_raster_scratch_bytes(unsigned list_cap);
hipError_t f3d_launch_raster_check(const void* tris, int itype, int64_t nt, int64_t nv, void* scratch, int nviews, long long* straddling, int* err,
                                   hipStream_t s);
hipError_t f3d_launch_raster(const void* verts, int vdtype, const void* tris, int itype, int64_t nt, const f3d_view* views_dev, int view0, int nv,
                             int h, int w, double z_far, unsigned long long* zkey, long long* straddling, void* scratch, unsigned list_cap,
                             bool stats, hipStream_t s);

// TSDF reconstruction (f3d_tsdf.hip; the contract is in include/f3d.h).  Device pointers, lo on the host.  Enqueue only.  The count
// pass leaves the voxel codes, the cell ranks and the quad offsets in `scratch` (f3d_tsdf_scratch_bytes(nx * ny * nz)) for the fill pass
// and enqueues the readback of counts_host = {active cells, quads} (the caller synchronises).  grid_cap > 0: at most that many blocks
// per launch (a test forces the grid-stride passes at a small size; no result depends on it).
size_t f3d_tsdf_scratch_bytes(int64_t nvoxels);
hipError_t f3d_launch_tsdf_integrate(float* tsdf, float* weight, int nx, int ny, int nz, const double lo[3], double vs, double trunc, double max_weight,
                                     const void* depth, int depth_type, int nframes, int h, int w, double depth_scale, double max_depth,
                                     const f3d_view* views_dev, int grid_cap, hipStream_t s);
hipError_t f3d_launch_tsdf_count(const float* tsdf, const float* weight, int nx, int ny, int nz, float min_weight, void* scratch,
                                 unsigned long long* counts_host, int grid_cap, hipStream_t s);
hipError_t f3d_launch_tsdf_fill(const float* tsdf, int nx, int ny, int nz, const double lo[3], double vs, const void* scratch, double* verts,
                                int32_t* tris, int grid_cap, hipStream_t s);
// the same with colour: color float32 [nz, ny, nx, 4] (16-byte aligned), rgb uint8 [F, hc, wc, 3]; the vertex colours of a counted
// volume read the codes, the active cells and the ranks of `scratch` (colored may be NULL)
hipError_t f3d_launch_tsdf_integrate_color(float* tsdf, float* weight, float* color, int nx, int ny, int nz, const double lo[3], double vs, double trunc,
                                           double max_weight, const void* depth, int depth_type, const uint8_t* rgb, int nframes, int h, int w,
                                           int hc, int wc, double depth_scale, double max_depth, const f3d_view* views_dev, int grid_cap,
                                           hipStream_t s);
hipError_t f3d_launch_tsdf_vert_colors(const float* tsdf, const float* color, int nx, int ny, int nz, const void* scratch, uint8_t* rgb,
                                       uint8_t* colored, int grid_cap, hipStream_t s);

// Registration (f3d_icp.hip; the contract is in include/f3d.h).  Device pointers; lo, K, qn / q and t on the host.  Enqueue only.
// The raycast takes the quaternion already normalised (qn).  grid_cap as for the TSDF launches.
hipError_t f3d_launch_tsdf_raycast(const float* tsdf, const float* weight, int nx, int ny, int nz, const double lo[3], double vs, float min_weight,
                                   const double K[9], const double qn[4], const double t[3], int h, int w, double near, double step, int nsteps,
                                   double* vertex, double* normal, double* depth, int grid_cap, hipStream_t s);
// the source frame, the model maps and the model camera of an ICP call.  scratch: f3d_icp_scratch_bytes(h * w); it holds the chunk
// sums, the pose between the rounds and the lost flag.  sums [29], pose_out [7], stats [iterations, 3] and status (may be NULL) are device
// pointers.
struct f3d_icp_args {
    const void* depth; int depth_type, h, w;
    const double* K;
    double depth_scale, max_depth;
    const double* model_vertex; const double* model_normal;
    int hm, wm;
    const f3d_view* model_view;
    double max_dist;
};
size_t f3d_icp_scratch_bytes(int64_t npixels);
hipError_t f3d_launch_icp_sums(const f3d_icp_args& a, const double q[4], const double t[3], void* scratch, double* sums, hipStream_t s);
hipError_t f3d_launch_icp(const f3d_icp_args& a, const double q[4], const double t[3], int iterations, int min_pairs, void* scratch,
                          double* pose_out, double* stats, int32_t* status, hipStream_t s);
// The same with colour.  The raycast: color the state [nz, ny, nx, 4] (16-byte aligned), rgb [h*w, 3] and intensity [h*w] two more
// optional outputs.  ICP: the model's intensity map [hm*wm], the source colour image [hc, wc_img, 3] and the weight of the photometric
// system; scratch: f3d_icp_color_scratch_bytes(h * w), whose chunk rows are 58 wide; sums [58], stats [iterations, 5].
hipError_t f3d_launch_tsdf_raycast_color(const float* tsdf, const float* weight, const float* color, int nx, int ny, int nz, const double lo[3],
                                         double vs, float min_weight, const double K[9], const double qn[4], const double t[3], int h, int w,
                                         double near, double step, int nsteps, double* vertex, double* normal, double* depth, double* rgb,
                                         double* intensity, int grid_cap, hipStream_t s);
struct f3d_icp_color_args {
    const double* model_intensity;
    const uint8_t* rgb; int hc, wc_img;
    double color_weight;
};
size_t f3d_icp_color_scratch_bytes(int64_t npixels);
hipError_t f3d_launch_icp_color_sums(const f3d_icp_args& a, const f3d_icp_color_args& c, const double q[4], const double t[3], void* scratch,
                                     double* sums, hipStream_t s);
hipError_t f3d_launch_icp_color(const f3d_icp_args& a, const f3d_icp_color_args& c, const double q[4], const double t[3], int iterations,
                                int min_pairs, void* scratch, double* pose_out, double* stats, int32_t* status, hipStream_t s);
// Coarse-to-fine.  One pyramid step of a depth frame (out [h/2 * w/2], metres) and of model maps (the outputs [hm/2 * wm/2, 3] and
// [hm/2 * wm/2]; intensity and intensity_out both NULL = no intensity map); no scratch.  The rounds of f3d_launch_icp /
// f3d_launch_icp_color over nlevels host records whose pointers are device pointers (rgb NULL = depth only); scratch: that of the
// level with the most source pixels, f3d_icp_scratch_bytes / f3d_icp_color_scratch_bytes of that count; stats [sum of iterations, 3 or 5].
hipError_t f3d_launch_depth_half(const void* depth, int depth_type, int h, int w, double depth_scale, double max_depth, double gate, double* out,
                                 hipStream_t s);
hipError_t f3d_launch_maps_half(const double* vertex, const double* normal, const double* intensity, int hm, int wm, const f3d_view* view, double gate,
                                double* vertex_out, double* normal_out, double* intensity_out, hipStream_t s);
hipError_t f3d_launch_icp_levels(const f3d_icp_level* levels, int nlevels, double max_depth, const double q[4], const double t[3], const uint8_t* rgb,
                                 int hc, int wc_img, double color_weight, void* scratch, double* pose_out, double* stats, int32_t* status,
                                 hipStream_t s);
// Cloud to cloud.  The source cloud [n, 3] of source_dtype, the target's built grid (f3d_launch_graph_grid) with its search, the target's
// normals float64 [m, 3] in the caller's order (read in F3D_CLOUD_ICP_PLANE mode only) and the mode.  scratch: f3d_icp_scratch_bytes(n);
// sums [29], pairs int32 [n] (may be NULL), pose_out, stats and status as for f3d_launch_icp.  n = 0 is fine: zero sums.
struct f3d_cloud_icp_args {
    const void* source; int source_dtype; int64_t n;
    f3d_gridview gv; f3d_gridsearch gs;
    const double* normals;
    int mode;
};
hipError_t f3d_launch_cloud_icp_sums(const f3d_cloud_icp_args& a, const double q[4], const double t[3], void* scratch, double* sums, int32_t* pairs,
                                     hipStream_t s);
hipError_t f3d_launch_cloud_icp(const f3d_cloud_icp_args& a, const double q[4], const double t[3], int iterations, int min_pairs, void* scratch,
                                double* pose_out, double* stats, int32_t* status, hipStream_t s);

// plane table of a cloud over its adjacency (f3d_planes.hip).  Device pointers (counts int64 [4] too); normals (may be NULL: PCA of the
// rows) and normals_out (may be NULL; written in PCA mode only) float64 [n, 3].  n >= 1.  Enqueues on `s` and synchronises it every few
// attach rounds.  A neighbour outside [0, n) sets F3D_DEVERR_PLANES and nothing is written.  scratch: f3d_planes_scratch_bytes(n)
struct f3d_planes_args { double cos_angle, offset, dist, max_variation; int64_t min_points, max_rounds, max_planes; };
size_t f3d_planes_scratch_bytes(int64_t n);
hipError_t f3d_launch_extract_planes(const void* xyz, int dtype, int64_t n, const int64_t* offs, const int32_t* nbrs,
                                     const double* normals, const f3d_planes_args& a, int32_t* labels, double* planes, double* corners,
                                     int64_t* counts, double* normals_out, void* scratch, int* err, hipStream_t s);

// neighbour-summed vote rows over a CSR adjacency (f3d_smooth.hip; the contract is in include/f3d.h).  Device pointers.  A gate
// exists iff its array is not NULL; lim2 = max_color_dist * max_color_dist.  f3d_launch_smooth_check goes first: a neighbour outside
// [0, n) or offsets that do not ascend from >= 0 set F3D_DEVERR_SMOOTH, under which every f3d_launch_smooth returns at once.
// f3d_launch_smooth is ONE iteration: votes (F3D_VOTES_F64 / F3D_VOTES_U16) -> out float64 [n, ncols] (seg NULL), or -> classes with the
// rules of f3d_launch_segment_votes(_lastcol) applied to the smoothed row, which is not written (seg given; flt.cls_dev holds the list).
struct f3d_smooth_gates { const double* normals; double cos_angle; const void* colors; int cdtype; double lim2; };
struct f3d_smooth_seg { int nclasses; double threshold; f3d_filter_args flt; f3d_negmask neg; int lastcol; };
hipError_t f3d_launch_smooth_check(int64_t n, const int64_t* offs, const int32_t* nbrs, int* err, hipStream_t s);
hipError_t f3d_launch_smooth(const void* votes, int vtype, int64_t n, int ncols, const int64_t* offs, const int32_t* nbrs,
                             const f3d_smooth_gates& g, double self_weight, double* out, const f3d_smooth_seg* seg, int64_t* classes,
                             const int* err, hipStream_t s);

// mask lifting (f3d_lift.hip; the contract is in include/f3d.h).  Device pointers.  f3d_launch_lift_incidence enqueues the incidence
// (rows, sizes, seen); f3d_launch_lift_merge then runs the pair table of `slots` entries (a power of two) and, with `instances`, the merge,
// the vote and the renumbering, or else the sorted pairs when at most `cap` of them exist.  It synchronises the stream for its one
// readback: stats = {distinct pairs, instances kept, instances before min_points, incidences, pair occurrences, table overflowed, bad
// input}.  After an overflow it is called again with a larger table (the incidence stays).  Bad input sets F3D_DEVERR_LIFT and nothing
// is written.  scratch: f3d_lift_scratch_bytes(F * HW, N, F * K); table: f3d_lift_table_bytes(slots, cap) (cap 0 with `instances`)
#define F3D_LIFT_NSTATS 7
struct f3d_lift_job {
    const int32_t* luts; const uint16_t* inst; int nframes; int64_t hw, npoints; int max_ids;               // the frames
    bool instances; double ratio; int64_t min_overlap, min_points; const int32_t* seg_classes;            // the merge rule (seg_classes may be NULL)
    uint16_t* seen; int32_t* sizes;                                                                         // incidence outputs (either may be NULL)
    int32_t *pairs, *counts; int64_t cap;                                                                   // overlaps outputs
    int32_t* ids; uint16_t* support; int32_t* seg2inst; int64_t* inst_points;                               // instances outputs
    void *scratch, *table; uint64_t slots; int* err; hipStream_t stream;
};
size_t f3d_lift_scratch_bytes(int64_t pixels, int64_t npoints, int64_t nseg);
size_t f3d_lift_table_bytes(uint64_t slots, int64_t cap);
hipError_t f3d_launch_lift_incidence(const f3d_lift_job& j);
hipError_t f3d_launch_lift_merge(const f3d_lift_job& j, int64_t stats[F3D_LIFT_NSTATS]);

// feature fusion (f3d_features.hip; the contract is in include/f3d.h).  views_dev, feats and zkey point at the first view of a pass of
// nv views; zkey: the splat keys of the same cloud for those views, or NULL when every sample is visible (depth_tol = +inf).  The
// launcher picks the group shape from d and ftype.  Enqueue only, no scratch.
hipError_t f3d_launch_fuse_features(const void* xyz, int dtype, int64_t n, const f3d_view* views_dev, int nv, int h, int w, const void* feats,
                                    int ftype, int hf, int wf, int d, const unsigned long long* zkey, double depth_tol, float* sums,
                                    int32_t* counts, hipStream_t s);
hipError_t f3d_launch_features_finalize(const float* sums, const int32_t* counts, int64_t n, int d, int normalize, float* out, hipStream_t s);
