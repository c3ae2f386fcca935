// Triangle-mesh z-buffer of a posed mesh (include/f3d.h "triangle-mesh z-buffer renders"): the rasteriser into the depth keys of
// f3d_render.hip.  A fragment's key is (float32 depth bits << 32 | triangle index), a cell keeps the minimum, so the buffers are the
// same whatever the order of the threads, the launch shape or the tier that handled a triangle.
//
// Nothing is kept per vertex: every (triangle, view) pair projects its own three corners (tri_setup) and every candidate pixel of its
// bounding box is evaluated directly from that setup (tri_sample) -- no incremental stepping, whose rounding would depend on the walk.
// Three tiers share those two functions and differ only in who walks the box:
//   small   (<= RASTER_SMALL cells)  the lane that set the pair up walks it alone;
//   medium  (<= RASTER_HUGE cells)   the wave takes its medium lanes one by one (ballot, broadcast of the triangle index), all 64
//                                    lanes repeat the setup and stride over the box together;
//   huge    (more)                   the pair goes to a list of fixed capacity in context scratch (one atomic per wave), and
//                                    k_raster_huge deals (entry, 64 x 64 screen tile) pairs to blocks.  A pair that finds the list
//                                    full is rasterised in place by the medium path.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>
#include "f3d.h"
#include "f3d_math.h"
#include "f3d_kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int RASTER_SMALL = 64;            // cells of a box one lane walks alone: one wave's worth of pixels
constexpr int RASTER_HUGE = 64 * 64;        // above: deferred to the tile kernel
constexpr int RASTER_TILE = 64;             // edge of a screen tile of the tile kernel (a block takes 16 cells per thread)
constexpr double RASTER_XY_MAX = 1073741824.0;   // 2^30

// One directed edge i -> j of a triangle, evaluated on the canonical (lower index -> higher index) form so that the two triangles
// sharing it compute the same bits: e = dx * (sy - y) - dy * (sx - x) with (x, y) the lower-index end; the directed value is -e when
// flip (i > j, xor a negative winding).
struct tri_edge { double x, y, dx, dy; bool flip; };

struct tri_setup {
    tri_edge e01, e12, e20;
    double iza, izb, izc;
    int u0, u1, v0, v1;                     // candidate box, clamped to the image (empty when u0 > u1 or v0 > v1)
};

struct tri_vertex { double x, y, iz; bool ok; };

__device__ __forceinline__ int64_t corner_at(const void* __restrict__ tris, int itype, int64_t s) {
    return itype == F3D_I32 ? (int64_t)reinterpret_cast<const int32_t*>(tris)[s] : reinterpret_cast<const int64_t*>(tris)[s];
}

__device__ __forceinline__ f3d_p3 vertex_at(const void* __restrict__ verts, int vdtype, int64_t i) {
    return vdtype == F3D_F64 ? f3d_load_p3(reinterpret_cast<const double*>(verts), i) : f3d_load_p3(reinterpret_cast<const float*>(verts), i);
}

__device__ __forceinline__ tri_vertex project_vertex(const f3d_view& vw, f3d_p3 p) {
    const f3d_p3 hp = f3d_project_h(vw.K, vw.qinv, vw.t, p);
    tri_vertex r;
    r.x = hp.x / hp.z;
    r.y = hp.y / hp.z;
    r.iz = 1.0 / hp.z;
    const float z32 = (float)hp.z;
    r.ok = z32 >= FLT_MIN && z32 < INFINITY && fabs(r.x) <= RASTER_XY_MAX && fabs(r.y) <= RASTER_XY_MAX;   // (NaN fails every test)
    return r;
}

__device__ __forceinline__ tri_edge make_edge(const tri_vertex& a, int64_t ia, const tri_vertex& b, int64_t ib, bool neg) {
    const bool fwd = ia < ib;
    tri_edge e;
    e.x = fwd ? a.x : b.x;
    e.y = fwd ? a.y : b.y;
    e.dx = (fwd ? b.x : a.x) - e.x;
    e.dy = (fwd ? b.y : a.y) - e.y;
    e.flip = fwd == neg;                    // i > j flips, a negative winding flips again
    return e;
}

__device__ __forceinline__ double edge_value(const tri_edge& e, double sx, double sy) {
    const double v = e.dx * (sy - e.y) - e.dy * (sx - e.x);
    return e.flip ? -v : v;
}

// 0: not rasterised, 1: straddles the camera plane (some but not all corners eligible), 2: set up
__device__ __forceinline__ int tri_set_up(const f3d_view& vw, const void* __restrict__ verts, int vdtype, const void* __restrict__ tris,
                                          int itype, int64_t t, int h, int w, tri_setup& T) {
    const int64_t ia = corner_at(tris, itype, 3 * t), ib = corner_at(tris, itype, 3 * t + 1), ic = corner_at(tris, itype, 3 * t + 2);
    const tri_vertex a = project_vertex(vw, vertex_at(verts, vdtype, ia));
    const tri_vertex b = project_vertex(vw, vertex_at(verts, vdtype, ib));
    const tri_vertex c = project_vertex(vw, vertex_at(verts, vdtype, ic));
    const int nok = (int)a.ok + (int)b.ok + (int)c.ok;
    if (nok != 3) return nok ? 1 : 0;
    if (ia == ib || ib == ic || ia == ic) return 0;
    const double A = (b.x - a.x) * (c.y - a.y) - (b.y - a.y) * (c.x - a.x);
    if (!(fabs(A) < INFINITY) || A == 0.0) return 0;
    const bool neg = A < 0.0;
    T.e01 = make_edge(a, ia, b, ib, neg);
    T.e12 = make_edge(b, ib, c, ic, neg);
    T.e20 = make_edge(c, ic, a, ia, neg);
    T.iza = a.iz; T.izb = b.iz; T.izc = c.iz;
    // candidates: floor(min) - 1 .. floor(max) + 1, clamped (|x|, |y| <= 2^30: the floors fit an int)
    const int fx0 = (int)floor(fmin(fmin(a.x, b.x), c.x)), fx1 = (int)floor(fmax(fmax(a.x, b.x), c.x));
    const int fy0 = (int)floor(fmin(fmin(a.y, b.y), c.y)), fy1 = (int)floor(fmax(fmax(a.y, b.y), c.y));
    T.u0 = max(fx0 - 1, 0); T.u1 = min(fx1 + 1, w - 1);
    T.v0 = max(fy0 - 1, 0); T.v1 = min(fy1 + 1, h - 1);
    return 2;
}

__device__ __forceinline__ int64_t box_cells(const tri_setup& T) {
    return T.u0 > T.u1 || T.v0 > T.v1 ? 0 : (int64_t)(T.u1 - T.u0 + 1) * (T.v1 - T.v0 + 1);
}

// the fragment of the set-up triangle at pixel (u, v), if it has one
__device__ __forceinline__ bool tri_sample(const tri_setup& T, int u, int v, double z_far, float& z32) {
    const double sx = (double)u + 0.5, sy = (double)v + 0.5;
    const double E01 = edge_value(T.e01, sx, sy), E12 = edge_value(T.e12, sx, sy), E20 = edge_value(T.e20, sx, sy);
    if (!(E01 >= 0.0 && E12 >= 0.0 && E20 >= 0.0)) return false;
    const double s = (E12 + E20) + E01;
    if (!(s > 0.0)) return false;
    const double z = s / ((E12 * T.iza + E20 * T.izb) + E01 * T.izc);
    z32 = (float)z;
    return z32 >= FLT_MIN && z32 < INFINITY && z <= z_far;
}

// load, then atomicMin only when the key would win (k_zsplat's skip: min is idempotent, a stale read costs one needless atomic)
__device__ __forceinline__ void put_key(unsigned long long* cell, float z32, uint32_t t) {
    const unsigned long long key = (unsigned long long)__float_as_uint(z32) << 32 | (unsigned long long)t;
    if (__hip_atomic_load(cell, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= key) return;
    __hip_atomic_fetch_min(cell, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// cells k0, k0 + step, ... of the box of T, row-major
__device__ __forceinline__ void walk_box(const tri_setup& T, int k0, int step, unsigned long long* plane, int w, double z_far, uint32_t t) {
    const int bw = T.u1 - T.u0 + 1;
    const int n = (int)box_cells(T);                                       // <= h * w <= 2^30 (checked by the entries)
    for (int k = k0; k < n; k += step) {
        const int r = k / bw, c = k - r * bw;
        float z32;
        if (tri_sample(T, T.u0 + c, T.v0 + r, z_far, z32)) put_key(plane + (size_t)(T.v0 + r) * w + (size_t)(T.u0 + c), z32, t);
    }
}

// flag[0] = 1 and the error bit when a corner is outside [0, nv); every kernel below returns at once when it is set
__global__ __launch_bounds__(F3D_BLOCK) void k_raster_check(const void* __restrict__ tris, int itype, int64_t n3, int64_t nv, int* flag, int* err) {
    bool bad = false;
    for (int64_t s = (int64_t)blockIdx.x * F3D_BLOCK + threadIdx.x; s < n3; s += (int64_t)gridDim.x * F3D_BLOCK) {
        const int64_t v = corner_at(tris, itype, s);
        bad |= (v < 0) | (v >= nv);
    }
    if (bad) { *flag = 1; atomicOr(err, F3D_DEVERR_RASTER); }
}

__global__ __launch_bounds__(F3D_BLOCK) void k_raster_zero(long long* __restrict__ straddling, int n, const int* __restrict__ flag) {
    if (*flag) return;
    for (int i = blockIdx.x * F3D_BLOCK + threadIdx.x; i < n; i += gridDim.x * F3D_BLOCK) straddling[i] = 0;
}

// blockIdx.y = view of the pass (the record is wave-uniform: scalar loads); a thread sets up triangle t of that view.  The loop is
// uniform over the block (every lane reaches the ballots).  stats (STATS only): pairs handled {small, medium, huge, overflow}.
template <bool STATS>
__global__ __launch_bounds__(F3D_BLOCK) void k_raster(const void* __restrict__ verts, int vdtype, const void* __restrict__ tris, int itype, int64_t nt,
                                                       const f3d_view* __restrict__ views, int view0, int h, int w, double z_far,
                                                       unsigned long long* __restrict__ zkey, long long* __restrict__ straddling,
                                                       f3d_raster_entry* __restrict__ list, unsigned* __restrict__ list_count, unsigned list_cap,
                                                       unsigned long long* __restrict__ stats, const int* __restrict__ flag) {
    if (*flag) return;
    const f3d_view& vw = views[blockIdx.y];
    unsigned long long* plane = zkey + (size_t)blockIdx.y * h * w;
    const int lane = threadIdx.x & 63;
    unsigned nstraddle = 0, nsmall = 0, nmedium = 0, nhuge = 0, nover = 0;
    for (int64_t base = (int64_t)blockIdx.x * F3D_BLOCK; base < nt; base += (int64_t)gridDim.x * F3D_BLOCK) {
        const int64_t t = base + threadIdx.x;
        tri_setup T;
        const int state = t < nt ? tri_set_up(vw, verts, vdtype, tris, itype, t, h, w, T) : 0;
        nstraddle += state == 1;
        const int64_t cells = state == 2 ? box_cells(T) : 0;
        bool medium = cells > RASTER_SMALL && cells <= RASTER_HUGE;
        const bool huge = cells > RASTER_HUGE;
        if (cells > 0 && cells <= RASTER_SMALL) {
            walk_box(T, 0, 1, plane, w, z_far, (uint32_t)t);
            if (STATS) ++nsmall;
        }
        // huge: one counter bump per wave; the lanes past the capacity fall back to the medium path
        const unsigned long long hmask = __ballot(huge);
        if (hmask) {
            const int leader = __ffsll((long long)hmask) - 1;
            unsigned first = 0;
            if (lane == leader) first = atomicAdd(list_count, (unsigned)__popcll(hmask));
            first = __shfl(first, leader, 64);
            if (huge) {
                const unsigned slot = first + (unsigned)__popcll(hmask & ((1ull << lane) - 1ull));
                if (slot < list_cap) {
                    f3d_raster_entry e;
                    e.view = view0 + (int)blockIdx.y; e.tri = (int32_t)t; e.u0 = T.u0; e.v0 = T.v0; e.u1 = T.u1; e.v1 = T.v1;
                    list[slot] = e;
                    if (STATS) ++nhuge;
                } else {
                    medium = true;
                    if (STATS) ++nover;
                }
            }
        }
        if (STATS && medium && !huge) ++nmedium;
        // medium: the wave takes its lanes' boxes one by one
        unsigned long long mmask = __ballot(medium);
        while (mmask) {
            const int src = __ffsll((long long)mmask) - 1;
            mmask &= mmask - 1;
            const int64_t tm = base + (threadIdx.x & ~63) + src;            // that lane's triangle: wave-uniform
            tri_setup M;
            if (tri_set_up(vw, verts, vdtype, tris, itype, tm, h, w, M) == 2) walk_box(M, lane, 64, plane, w, z_far, (uint32_t)tm);
        }
    }
    if (straddling && nstraddle) atomicAdd((unsigned long long*)(straddling + view0 + blockIdx.y), (unsigned long long)nstraddle);
    if (STATS) {
        if (nsmall) atomicAdd(stats, (unsigned long long)nsmall);
        if (nmedium) atomicAdd(stats + 1, (unsigned long long)nmedium);
        if (nhuge) atomicAdd(stats + 2, (unsigned long long)nhuge);
        if (nover) atomicAdd(stats + 3, (unsigned long long)nover);
    }
}

// A block takes (entry, screen tile) pairs, entry-major; the entry's box rejects the tiles it does not touch before any arithmetic.
// Every thread repeats the setup (uniform over the block) and takes the tile's cells threadIdx.x, + 256, ...: 4 rows of 64 per step.
__global__ __launch_bounds__(F3D_BLOCK) void k_raster_huge(const void* __restrict__ verts, int vdtype, const void* __restrict__ tris, int itype,
                                                            const f3d_view* __restrict__ views, int view0, int h, int w, double z_far,
                                                            unsigned long long* __restrict__ zkey, const f3d_raster_entry* __restrict__ list,
                                                            const unsigned* __restrict__ list_count, unsigned list_cap, const int* __restrict__ flag) {
    if (*flag) return;
    const unsigned n = min(*list_count, list_cap);
    const int tx = (w + RASTER_TILE - 1) / RASTER_TILE, ty = (h + RASTER_TILE - 1) / RASTER_TILE;
    const int64_t tiles = (int64_t)tx * ty;
    for (int64_t pair = blockIdx.x; pair < (int64_t)n * tiles; pair += gridDim.x) {
        const int64_t ei = pair / tiles;
        const int tile = (int)(pair - ei * tiles);
        const f3d_raster_entry e = list[ei];
        const int c0 = (tile % tx) * RASTER_TILE, r0 = (tile / tx) * RASTER_TILE;
        if (e.u1 < c0 || e.u0 >= c0 + RASTER_TILE || e.v1 < r0 || e.v0 >= r0 + RASTER_TILE) continue;
        tri_setup T;
        if (tri_set_up(views[e.view - view0], verts, vdtype, tris, itype, e.tri, h, w, T) != 2) continue;
        unsigned long long* plane = zkey + (size_t)(e.view - view0) * h * w;
        for (int k = threadIdx.x; k < RASTER_TILE * RASTER_TILE; k += F3D_BLOCK) {
            const int r = r0 + k / RASTER_TILE, c = c0 + (k & (RASTER_TILE - 1));
            if (r < T.v0 || r > T.v1 || c < T.u0 || c > T.u1) continue;
            float z32;
            if (tri_sample(T, c, r, z_far, z32)) put_key(plane + (size_t)r * w + (size_t)c, z32, (uint32_t)e.tri);
        }
    }
}

}  // namespace

size_t f3d_raster_scratch_bytes(unsigned list_cap) { return f3d_raster_scratch_layout(list_cap).bytes; }

hipError_t f3d_launch_raster_check(const void* tris, int itype, int64_t nt, int64_t nv, void* scratch, int nviews, long long* straddling, int* err,
                                   hipStream_t s) {
    const f3d_raster_scratch lay = f3d_raster_scratch_layout(0);
    char* base = (char*)scratch;
    hipError_t e = hipMemsetAsync(base, 0, lay.entries, s);                                   // flag, list counter, stats
    if (e != hipSuccess) return e;
    if (nt > 0) hipLaunchKernelGGL(k_raster_check, dim3(f3d_grid_for(3 * nt, F3D_BLOCK, F3D_GRID_CAP)), dim3(F3D_BLOCK), 0, s, tris, itype, 3 * nt, nv,
                                   (int*)(base + lay.flag), err);
    if (straddling && nviews > 0)
        hipLaunchKernelGGL(k_raster_zero, dim3(f3d_grid_for(nviews, F3D_BLOCK, F3D_GRID_CAP)), dim3(F3D_BLOCK), 0, s, straddling, nviews, (const int*)(base + lay.flag));
    return hipGetLastError();
}

hipError_t f3d_launch_raster(const void* verts, int vdtype, const void* tris, int itype, int64_t nt, const f3d_view* views_dev, int view0, int nv,
                             int h, int w, double z_far, unsigned long long* zkey, long long* straddling, void* scratch, unsigned list_cap,
                             bool stats, hipStream_t s) {
    if (nt <= 0 || nv <= 0) return hipSuccess;
    const f3d_raster_scratch lay = f3d_raster_scratch_layout(list_cap);
    char* base = (char*)scratch;
    const int* flag = (const int*)(base + lay.flag);
    unsigned* count = (unsigned*)(base + lay.count);
    unsigned long long* st = (unsigned long long*)(base + lay.stats);
    f3d_raster_entry* list = (f3d_raster_entry*)(base + lay.entries);
    for (int c0 = 0; c0 < nv; c0 += 65535) {                                                  // blockIdx.y = view: at most 65535 per launch
        const int nc = nv - c0 < 65535 ? nv - c0 : 65535;
        const f3d_view* views = views_dev + view0 + c0;
        unsigned long long* keys = zkey + (size_t)c0 * h * w;
        hipError_t e = hipMemsetAsync(count, 0, sizeof(unsigned), s);                         // the list of these views
        if (e != hipSuccess) return e;
        const int cap = (F3D_GRID_CAP + nc - 1) / nc;
        const dim3 g(f3d_grid_for(nt, F3D_BLOCK, cap < 64 ? 64 : cap), nc), b(F3D_BLOCK);
        if (stats)
            hipLaunchKernelGGL(k_raster<true>, g, b, 0, s, verts, vdtype, tris, itype, nt, views, view0 + c0, h, w, z_far, keys, straddling, list, count,
                               list_cap, st, flag);
        else
            hipLaunchKernelGGL(k_raster<false>, g, b, 0, s, verts, vdtype, tris, itype, nt, views, view0 + c0, h, w, z_far, keys, straddling, list, count,
                               list_cap, st, flag);
        hipLaunchKernelGGL(k_raster_huge, dim3(F3D_GRID_CAP / 4), dim3(F3D_BLOCK), 0, s, verts, vdtype, tris, itype, views, view0 + c0, h, w, z_far, keys,
                           list, count, list_cap, flag);
    }
    return hipGetLastError();
}
