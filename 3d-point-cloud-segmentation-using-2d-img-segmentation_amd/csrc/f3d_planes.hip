// Plane table of a cloud over its adjacency (include/f3d.h f3d_extract_planes) on gfx950: the producer of the PlaneswithPoints /
// BoundingPoints tables that segUtils/refinement.py consumes.  No reference counterpart (the reference ran a binary it does not ship).
//
//   k_pl_check   : a neighbour index outside [0, n) raises words->bad and the error bit; every later kernel then returns at once;
//   k_pl_core    : core flag and normal of every point (the caller's normal, or the PCA of the point's row: mean and centred second
//                  moments added in row order by one thread, jacobi3);
//   k_pl_union   : the smooth edges between core points, joined with f3d_uf_link (a root is its component's lowest index);
//   k_pl_roots / k_pl_flags / scan / k_pl_labels : components of at least min_points members, numbered by ascending root;
//   k_pl_group_keys + f3d_group_pairs : the members of every plane in ascending index;
//   k_pl_chunk_sums / k_pl_fit : per plane the centroid, then the centred second moments, as the fixed-shape sums of f3d_groups.h
//                  (chunks of 4096 members, lane-strided wave sums, xor butterfly), jacobi3 -> normal, in-plane axes;
//   k_pl_inliers : members farther than dist from their plane become -1 (the plane is not refitted);
//   k_pl_attach / k_pl_round_end : synchronous rounds over two label buffers; the changed flag stays on the device and the host reads
//                  {done, rounds} back every ATTACH_CHUNK rounds;
//   group again (final members) -> k_pl_chunk_sums (squared residuals) -> rms; k_pl_extents: order-preserving 64-bit atomicMin / atomicMax,
//                  after a reduction among the lanes of a wave that share a plane (k_pl_roots counts the same way);
//   k_pl_finish  : the plane rows, the quads, the counts.
// Every dot product is (a0*b0 + a1*b1) + a2*b2 (f3d_dot3), no contraction, no float atomics: two calls return the same bits.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <rocprim/device/device_scan.hpp>
#include "f3d.h"
#include "f3d_kernels.h"
#include "f3d_groups.h"
#include "f3d_math.h"
#include "f3d_eigen.h"

#pragma clang fp contract(off)

namespace {

constexpr int PB = 256;
constexpr int PGRID = 8192;
constexpr int SUM_CHUNK = 4096;            // members per chunk of a plane's sums
constexpr int SUM_SHIFT = 12;              // log2(SUM_CHUNK)
constexpr int WAVE_GROUPS = 8;             // distinct roots / planes of a wave that are reduced among its lanes before the atomic
constexpr int ATTACH_CHUNK = 4;            // attach rounds enqueued between two readbacks of {done, rounds}

#define PL_LOOP(i, n) for (int64_t i = (int64_t)blockIdx.x * PB + threadIdx.x; i < (n); i += (int64_t)gridDim.x * PB)

struct pl_words { int32_t bad, done, rounds, changed; };

__device__ __forceinline__ f3d_p3 ldp(const void* __restrict__ xyz, int dtype, int64_t i) {
    return dtype == F3D_F64 ? f3d_load_p3(reinterpret_cast<const double*>(xyz), i) : f3d_load_p3(reinterpret_cast<const float*>(xyz), i);
}

// planes written: the qualifying components (scan[n]) cut at max_planes
__device__ __forceinline__ int64_t planes_written(const uint32_t* __restrict__ scan, int64_t n, int64_t max_planes) {
    const int64_t q = (int64_t)scan[n];
    return q < max_planes ? q : max_planes;
}

// index of the smallest of w[0..3) (ties: the lowest index), and of the largest of the other two (ties: the lowest index)
__device__ __forceinline__ void eig_order(const double w[3], int& k0, int& k2) {
    k0 = 0;
    if (w[1] < w[k0]) k0 = 1;
    if (w[2] < w[k0]) k0 = 2;
    const int a = k0 == 0 ? 1 : 0, b = k0 == 2 ? 1 : 2;
    k2 = w[b] > w[a] ? b : a;
}

// the largest component (ties: the lowest axis) made positive
__device__ __forceinline__ void sign_largest(double v[3]) {
    int a = 0;
    if (fabs(v[1]) > fabs(v[a])) a = 1;
    if (fabs(v[2]) > fabs(v[a])) a = 2;
    if (v[a] < 0.0) { v[0] = -v[0]; v[1] = -v[1]; v[2] = -v[2]; }
}

__global__ __launch_bounds__(PB) void k_pl_check(int64_t n, const int64_t* __restrict__ offs, const int32_t* __restrict__ nbrs, pl_words* w, int* err) {
    bool bad = false;
    PL_LOOP(i, n) {
        for (int64_t e = offs[i]; e < offs[i + 1]; ++e) {
            const int64_t j = nbrs[e];
            bad |= (j < 0) | (j >= n);
        }
    }
    if (bad) { w->bad = 1; atomicOr(err, F3D_DEVERR_PLANES); }
}

// core[i], nrm[i] (written only in PCA mode: with normals given nrm IS the caller's array), parent[i] = i, cnt[i] = 0
__global__ __launch_bounds__(PB) void k_pl_core(const void* __restrict__ xyz, int dtype, int64_t n, const int64_t* __restrict__ offs,
                                                const int32_t* __restrict__ nbrs, const double* __restrict__ normals_in, double max_variation,
                                                const pl_words* w, uint8_t* __restrict__ core, double* __restrict__ nrm,
                                                int32_t* __restrict__ parent, int32_t* __restrict__ cnt) {
    if (w->bad) return;
    PL_LOOP(i, n) {
        parent[i] = (int32_t)i;
        cnt[i] = 0;
        const int64_t e0 = offs[i], e1 = offs[i + 1];
        int64_t others = 0;
        for (int64_t e = e0; e < e1; ++e) others += nbrs[e] != (int32_t)i;
        bool is_core = others >= 2;
        if (normals_in) {
            is_core = is_core && f3d_finite(normals_in[3 * i], normals_in[3 * i + 1], normals_in[3 * i + 2]);
        } else {
            double nx = 0.0, ny = 0.0, nz = 0.0;
            if (is_core) {
                const f3d_p3 p = ldp(xyz, dtype, i);
                const double m = (double)(others + 1);
                double sx = p.x, sy = p.y, sz = p.z;                       // the point itself, then its row in row order
                for (int64_t e = e0; e < e1; ++e) {
                    const int32_t j = nbrs[e];
                    if (j == (int32_t)i) continue;
                    const f3d_p3 q = ldp(xyz, dtype, j);
                    sx = sx + q.x; sy = sy + q.y; sz = sz + q.z;
                }
                const double cx = sx / m, cy = sy / m, cz = sz / m;
                double dx = p.x - cx, dy = p.y - cy, dz = p.z - cz;
                double a00 = dx * dx, a01 = dx * dy, a02 = dx * dz, a11 = dy * dy, a12 = dy * dz, a22 = dz * dz;
                for (int64_t e = e0; e < e1; ++e) {
                    const int32_t j = nbrs[e];
                    if (j == (int32_t)i) continue;
                    const f3d_p3 q = ldp(xyz, dtype, j);
                    dx = q.x - cx; dy = q.y - cy; dz = q.z - cz;
                    a00 = a00 + dx * dx; a01 = a01 + dx * dy; a02 = a02 + dx * dz;
                    a11 = a11 + dy * dy; a12 = a12 + dy * dz; a22 = a22 + dz * dz;
                }
                double ev[3], V[9];
                jacobi3(a00, a01, a02, a11, a12, a22, ev, V);
                int k0, k2;
                eig_order(ev, k0, k2);
                const int k1 = 3 - k0 - k2;
                const double tr = (ev[k0] + ev[k1]) + ev[k2];
                is_core = tr > 0.0 && ev[k0] / tr <= max_variation;
                nx = V[k0]; ny = V[3 + k0]; nz = V[6 + k0];
            }
            nrm[3 * i] = nx; nrm[3 * i + 1] = ny; nrm[3 * i + 2] = nz;
        }
        core[i] = is_core;
    }
}

// the smooth-edge test of core points i and j: the same bits from either end
__device__ __forceinline__ bool smooth_edge(const f3d_p3& pi, const f3d_p3& pj, const double* __restrict__ ni, const double* __restrict__ nj,
                                            double cos_angle, double offset) {
    if (!(fabs(f3d_dot3(ni[0], ni[1], ni[2], nj[0], nj[1], nj[2])) >= cos_angle)) return false;
    const double d0 = pj.x - pi.x, d1 = pj.y - pi.y, d2 = pj.z - pi.z;
    const double oi = fabs(f3d_dot3(d0, d1, d2, ni[0], ni[1], ni[2])), oj = fabs(f3d_dot3(d0, d1, d2, nj[0], nj[1], nj[2]));
    return fmax(oi, oj) <= offset;
}

__global__ __launch_bounds__(PB) void k_pl_union(const void* __restrict__ xyz, int dtype, int64_t n, const int64_t* __restrict__ offs,
                                                 const int32_t* __restrict__ nbrs, const uint8_t* __restrict__ core,
                                                 const double* __restrict__ nrm, double cos_angle, double offset, const pl_words* w,
                                                 int32_t* parent) {
    if (w->bad) return;
    PL_LOOP(i, n) {
        if (!core[i]) continue;
        const f3d_p3 pi = ldp(xyz, dtype, i);
        const double ni[3] = {nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2]};
        for (int64_t e = offs[i]; e < offs[i + 1]; ++e) {
            const int64_t j = nbrs[e];
            if (j <= i || !core[j]) continue;                            // the relation is symmetric: the lower end links
            if (smooth_edge(pi, ldp(xyz, dtype, j), ni, nrm + 3 * j, cos_angle, offset)) f3d_uf_link(parent, (int32_t)i, (int32_t)j);
        }
    }
}

// root[i] = lowest index of core point i's component (-1 for a point that is not core); cnt[root] = its core members
__global__ __launch_bounds__(PB) void k_pl_roots(const int32_t* parent, int64_t n, const uint8_t* __restrict__ core, const pl_words* w,
                                                 int32_t* __restrict__ root, int32_t* cnt) {
    if (w->bad) return;
    const int lane = threadIdx.x & 63;
    for (int64_t w0 = (int64_t)blockIdx.x * PB + threadIdx.x - lane; w0 < n; w0 += (int64_t)gridDim.x * PB) {
        const int64_t i = w0 + lane;
        int32_t x = -1;
        if (i < n) {
            if (core[i]) x = f3d_uf_root(parent, (int32_t)i);
            root[i] = x;
        }
        // the lanes of the wave that share a root count themselves with one atomic (a room has a few large planes)
        unsigned long long todo = __ballot(x >= 0);
        for (int it = 0; todo && it < WAVE_GROUPS; ++it) {
            const int src = __ffsll((long long)todo) - 1;
            const int32_t r = __shfl(x, src);
            const unsigned long long peers = __ballot(x == r);
            todo &= ~peers;
            if (lane == src) atomicAdd(cnt + r, (int32_t)__popcll(peers));
            if (x == r) x = -1;
        }
        if (x >= 0) atomicAdd(cnt + x, 1);                               // more than WAVE_GROUPS roots in the wave: one by one
    }
}

// flags[r] = r is the root of a component with at least min_points core members; flags[n] = 0
__global__ __launch_bounds__(PB) void k_pl_flags(const int32_t* __restrict__ root, const int32_t* __restrict__ cnt, int64_t n, int64_t min_points,
                                                 const pl_words* w, uint32_t* __restrict__ flags) {
    if (w->bad) return;
    PL_LOOP(i, n + 1) flags[i] = i < n && root[i] == (int32_t)i && (int64_t)cnt[i] >= min_points;
}

// labels[i] = the plane of core point i (-1: none, or a plane past max_planes)
__global__ __launch_bounds__(PB) void k_pl_labels(const int32_t* __restrict__ root, const uint32_t* __restrict__ scan, int64_t n,
                                                  int64_t max_planes, const pl_words* w, int32_t* __restrict__ labels) {
    if (w->bad) return;
    const int64_t P = planes_written(scan, n, max_planes);
    PL_LOOP(i, n) {
        const int32_t r = root[i];
        int32_t l = -1;
        if (r >= 0 && scan[r + 1] != scan[r] && (int64_t)scan[r] < P) l = (int32_t)scan[r];
        labels[i] = l;
    }
}

// ---- group: the members of every plane in ascending point index -----------------------------------------------------------------
__global__ __launch_bounds__(PB) void k_pl_group_keys(const int32_t* __restrict__ labels, int64_t n, const uint32_t* __restrict__ scan,
                                                      int64_t max_planes, const pl_words* w, uint32_t* __restrict__ keys,
                                                      uint32_t* __restrict__ vals) {
    if (w->bad) return;
    const int64_t P = planes_written(scan, n, max_planes);
    PL_LOOP(i, n) {
        const int32_t l = labels[i];
        keys[i] = l >= 0 ? (uint32_t)l : (uint32_t)P;
        vals[i] = (uint32_t)i;
    }
}

// what a member adds to its plane's sums
//   SUM_MEAN: x, y, z;  SUM_MOMENTS: the 6 products of (p - c);  SUM_RESIDUAL: ((p - c) . n)^2
enum { SUM_MEAN = 0, SUM_MOMENTS = 1, SUM_RESIDUAL = 2 };
__device__ __forceinline__ int sum_terms(int mode) { return mode == SUM_MEAN ? 3 : mode == SUM_MOMENTS ? 6 : 1; }

__device__ __forceinline__ double sum_term(int mode, int k, const f3d_p3& p, const double* __restrict__ fr) {
    if (mode == SUM_MEAN) return k == 0 ? p.x : k == 1 ? p.y : p.z;
    const double dx = p.x - fr[0], dy = p.y - fr[1], dz = p.z - fr[2];
    if (mode == SUM_RESIDUAL) { const double r = f3d_dot3(dx, dy, dz, fr[3], fr[4], fr[5]); return r * r; }
    return k == 0 ? dx * dx : k == 1 ? dx * dy : k == 2 ? dx * dz : k == 3 ? dy * dy : k == 4 ? dy * dz : dz * dz;
}

// frame of a plane, 12 doubles: centroid, normal, u, v
#define PL_FRAME 12

// The chunk of SUM_CHUNK consecutive members of plane c that starts at grouped position q owns slot (q >> SUM_SHIFT) + c of `partial`
// (6 doubles each): slots grow with the chunk inside a plane and from a plane to the next, so no two chunks share one.  Every chunk is
// summed term by term.
__global__ __launch_bounds__(PB) void k_pl_chunk_sums(const void* __restrict__ xyz, int dtype, int64_t n, int mode,
                                                      const uint32_t* __restrict__ order, const uint32_t* __restrict__ skeys,
                                                      const int64_t* __restrict__ starts, const uint32_t* __restrict__ scan, int64_t max_planes,
                                                      const double* __restrict__ frames, const pl_words* w, double* __restrict__ partial) {
    if (w->bad) return;
    const int lane = threadIdx.x & 63;
    const int nterms = sum_terms(mode);
    f3d_chunk_heads<SUM_CHUNK, PB>(skeys, starts, n, planes_written(scan, n, max_planes), [&](int64_t q, int64_t len, int64_t c) {
        const double* fr = frames + PL_FRAME * c;
        for (int k = 0; k < nterms; ++k) {
            const double sum = f3d_wave_sum(len, lane, [&](int64_t i) { return sum_term(mode, k, ldp(xyz, dtype, (int64_t)order[q + i]), fr); });
            if (lane == 0) partial[6 * ((q >> SUM_SHIFT) + c) + k] = sum;
        }
    });
}

// one wave per plane: the sum of the plane's chunk sums, term by term, then
//   SUM_MEAN    : frames[c].centroid = sums / members
//   SUM_MOMENTS : jacobi3 of the moment sums -> normal (smallest eigenvalue), u (largest), v = normal x u, with their signs
//   SUM_RESIDUAL: rms[c] = sqrt(sum / members) (NaN for a plane without members)
__global__ __launch_bounds__(PB) void k_pl_fit(int64_t n, int mode, const int64_t* __restrict__ starts, const uint32_t* __restrict__ scan,
                                               int64_t max_planes, const double* __restrict__ partial, const double* __restrict__ nrm,
                                               int have_normals, const uint32_t* __restrict__ order, const pl_words* w,
                                               double* __restrict__ frames, double* __restrict__ rms) {
    if (w->bad) return;
    const int lane = threadIdx.x & 63;
    const int nterms = sum_terms(mode);
    f3d_group_waves<PB>(starts, planes_written(scan, n, max_planes), [&](int64_t c, int64_t b, int64_t e) {
        double s[6] = {0, 0, 0, 0, 0, 0};
        for (int k = 0; k < nterms; ++k)
            s[k] = f3d_chunks_sum<SUM_CHUNK>(b, e, lane, [&](int64_t q) { return partial[6 * ((q >> SUM_SHIFT) + c) + k]; });
        if (lane != 0) return;
        double* fr = frames + PL_FRAME * c;
        const double m = (double)(e - b);
        if (mode == SUM_MEAN) {
            fr[0] = s[0] / m; fr[1] = s[1] / m; fr[2] = s[2] / m;
        } else if (mode == SUM_RESIDUAL) {
            rms[c] = sqrt(s[0] / m);
        } else {
            double ev[3], V[9];
            jacobi3(s[0], s[1], s[2], s[3], s[4], s[5], ev, V);
            int k0, k2;
            eig_order(ev, k0, k2);
            double nv[3] = {V[k0], V[3 + k0], V[6 + k0]}, u[3] = {V[k2], V[3 + k2], V[6 + k2]};
            if (have_normals) {                                          // the root is the plane's first member
                const double* nr = nrm + 3 * (int64_t)order[b];
                if (f3d_dot3(nv[0], nv[1], nv[2], nr[0], nr[1], nr[2]) < 0.0) { nv[0] = -nv[0]; nv[1] = -nv[1]; nv[2] = -nv[2]; }
            } else {
                sign_largest(nv);
            }
            sign_largest(u);
            fr[3] = nv[0]; fr[4] = nv[1]; fr[5] = nv[2];
            fr[6] = u[0]; fr[7] = u[1]; fr[8] = u[2];
            fr[9] = nv[1] * u[2] - nv[2] * u[1]; fr[10] = nv[2] * u[0] - nv[0] * u[2]; fr[11] = nv[0] * u[1] - nv[1] * u[0];
        }
    });
}

// |(p - c) . n| of point p to the plane with frame fr
__device__ __forceinline__ double plane_dist(const f3d_p3& p, const double* __restrict__ fr) {
    return fabs(f3d_dot3(p.x - fr[0], p.y - fr[1], p.z - fr[2], fr[3], fr[4], fr[5]));
}

__global__ __launch_bounds__(PB) void k_pl_inliers(const void* __restrict__ xyz, int dtype, int64_t n, const double* __restrict__ frames,
                                                   double dist, const pl_words* w, int32_t* __restrict__ labels) {
    if (w->bad) return;
    PL_LOOP(i, n) {
        const int32_t l = labels[i];
        if (l >= 0 && plane_dist(ldp(xyz, dtype, i), frames + PL_FRAME * (int64_t)l) > dist) labels[i] = -1;
    }
}

// one synchronous round: cur = the labels at the end of the previous round, nxt = at the end of this one
__global__ __launch_bounds__(PB) void k_pl_attach(const void* __restrict__ xyz, int dtype, int64_t n, const int64_t* __restrict__ offs,
                                                  const int32_t* __restrict__ nbrs, const double* __restrict__ frames, double dist,
                                                  const int32_t* __restrict__ cur, int32_t* __restrict__ nxt, pl_words* w) {
    if (w->bad | w->done) return;
    bool changed = false;
    PL_LOOP(i, n) {
        int32_t l = cur[i];
        if (l < 0) {
            const f3d_p3 p = ldp(xyz, dtype, i);
            int32_t best = 0x7fffffff;
            for (int64_t e = offs[i]; e < offs[i + 1]; ++e) {
                const int32_t c = cur[nbrs[e]];
                if (c >= 0 && c < best && plane_dist(p, frames + PL_FRAME * (int64_t)c) <= dist) best = c;
            }
            if (best != 0x7fffffff) { l = best; changed = true; }
        }
        nxt[i] = l;
    }
    if (changed) w->changed = 1;
}

// closes a round: counts it, and ends the rounds when it changed nothing
__global__ void k_pl_round_end(pl_words* w) {
    if (w->bad | w->done) return;
    w->rounds += 1;
    if (!w->changed) w->done = 1;
    w->changed = 0;
}

// ext[4c ..] = {min a, max a, min b, max b} of a = (p - c) . u, b = (p - c) . v over the final members, order-encoded
__global__ __launch_bounds__(PB) void k_pl_ext_init(int64_t n, const uint32_t* __restrict__ scan, int64_t max_planes, const pl_words* w,
                                                    unsigned long long* __restrict__ ext) {
    if (w->bad) return;
    const int64_t P = planes_written(scan, n, max_planes);
    PL_LOOP(k, 4 * P) ext[k] = (k & 1) ? 0ull : ~0ull;
}

__global__ __launch_bounds__(PB) void k_pl_extents(const void* __restrict__ xyz, int dtype, int64_t n, const int32_t* __restrict__ labels,
                                                   const double* __restrict__ frames, const pl_words* w, unsigned long long* ext) {
    if (w->bad) return;
    const int lane = threadIdx.x & 63;
    for (int64_t w0 = (int64_t)blockIdx.x * PB + threadIdx.x - lane; w0 < n; w0 += (int64_t)gridDim.x * PB) {
        const int64_t i = w0 + lane;
        int32_t l = i < n ? labels[i] : -1;
        unsigned long long a = 0, b = 0;
        if (l >= 0) {
            const double* fr = frames + PL_FRAME * (int64_t)l;
            const f3d_p3 p = ldp(xyz, dtype, i);
            const double dx = p.x - fr[0], dy = p.y - fr[1], dz = p.z - fr[2];
            a = f3d_ord_enc(f3d_dot3(dx, dy, dz, fr[6], fr[7], fr[8]));
            b = f3d_ord_enc(f3d_dot3(dx, dy, dz, fr[9], fr[10], fr[11]));
        }
        // the lanes of the wave that share a plane meet in a butterfly first: integer minima and maxima, the same bits in any order
        unsigned long long todo = __ballot(l >= 0);
        for (int it = 0; todo && it < WAVE_GROUPS; ++it) {
            const int src = __ffsll((long long)todo) - 1;
            const int32_t lk = __shfl(l, src);
            const bool mine = l == lk;
            todo &= ~__ballot(mine);
            unsigned long long an = mine ? a : ~0ull, ax = mine ? a : 0ull, bn = mine ? b : ~0ull, bx = mine ? b : 0ull;
            for (int off = 32; off > 0; off >>= 1) {
                const unsigned long long t0 = __shfl_xor(an, off), t1 = __shfl_xor(ax, off), t2 = __shfl_xor(bn, off), t3 = __shfl_xor(bx, off);
                an = t0 < an ? t0 : an; ax = t1 > ax ? t1 : ax; bn = t2 < bn ? t2 : bn; bx = t3 > bx ? t3 : bx;
            }
            if (lane == src) {
                atomicMin(&ext[4 * (int64_t)lk], an); atomicMax(&ext[4 * (int64_t)lk + 1], ax);
                atomicMin(&ext[4 * (int64_t)lk + 2], bn); atomicMax(&ext[4 * (int64_t)lk + 3], bx);
            }
            if (mine) l = -1;
        }
        if (l >= 0) {                                                    // more than WAVE_GROUPS planes in the wave: one by one
            atomicMin(&ext[4 * (int64_t)l], a); atomicMax(&ext[4 * (int64_t)l + 1], a);
            atomicMin(&ext[4 * (int64_t)l + 2], b); atomicMax(&ext[4 * (int64_t)l + 3], b);
        }
    }
}

// the label buffer of the last round into the caller's array, when that is the other one
__global__ __launch_bounds__(PB) void k_pl_copy_labels(const int32_t* __restrict__ from, int64_t n, const pl_words* w, int32_t* __restrict__ to) {
    if (w->bad) return;
    PL_LOOP(i, n) to[i] = from[i];
}

// planes [max_planes, 8], corners [max_planes, 4, 3] (rows past the planes written are zero), counts [4]
__global__ __launch_bounds__(PB) void k_pl_finish(int64_t n, const uint32_t* __restrict__ scan, int64_t max_planes, const double* __restrict__ frames,
                                                  const double* __restrict__ rms, const unsigned long long* __restrict__ ext,
                                                  const int64_t* __restrict__ starts, const pl_words* w, double* __restrict__ planes,
                                                  double* __restrict__ corners, int64_t* __restrict__ counts) {
    if (w->bad) return;
    const int64_t P = planes_written(scan, n, max_planes);
    PL_LOOP(c, max_planes) {
        double* pr = planes + 8 * c;
        double* cr = corners + 12 * c;
        if (c >= P) {
            for (int k = 0; k < 8; ++k) pr[k] = 0.0;
            for (int k = 0; k < 12; ++k) cr[k] = 0.0;
            continue;
        }
        const double* fr = frames + PL_FRAME * c;
        pr[0] = fr[3]; pr[1] = fr[4]; pr[2] = fr[5];
        pr[3] = -f3d_dot3(fr[3], fr[4], fr[5], fr[0], fr[1], fr[2]);
        pr[4] = fr[0]; pr[5] = fr[1]; pr[6] = fr[2];
        pr[7] = rms[c];
        const bool any = starts[c + 1] > starts[c];
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        const double a0 = any ? f3d_ord_dec(ext[4 * c]) : nan, a1 = any ? f3d_ord_dec(ext[4 * c + 1]) : nan;
        const double b0 = any ? f3d_ord_dec(ext[4 * c + 2]) : nan, b1 = any ? f3d_ord_dec(ext[4 * c + 3]) : nan;
        const double ca[4] = {a0, a1, a1, a0}, cb[4] = {b0, b0, b1, b1};
        for (int q = 0; q < 4; ++q)
            for (int k = 0; k < 3; ++k) cr[3 * q + k] = (fr[k] + ca[q] * fr[6 + k]) + cb[q] * fr[9 + k];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        counts[0] = P; counts[1] = (int64_t)scan[n]; counts[2] = (int64_t)w->rounds; counts[3] = starts[P];
    }
}

struct planes_layout {
    size_t words, core, nrm, parent, root, cnt, flags, labels_b, keys_a, keys_b, vals_a, vals_b, starts, partial, frames, rms, ext, temp, total;
    size_t temp_bytes;
};

planes_layout planes_layout_for(int64_t n) {
    if (n < 1) n = 1;
    const size_t np = (size_t)(n / 3 + 1);                 // min_points >= 3: at most n / 3 planes
    planes_layout L;
    size_t a = f3d_group_temp_bytes(n), b = 0;
    (void)rocprim::exclusive_scan(nullptr, b, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t)0, (size_t)n + 1, rocprim::plus<uint32_t>());
    L.temp_bytes = (a > b ? a : b) + 256;
    f3d_carve k;
    L.words = k.take(sizeof(pl_words));
    L.core = k.take((size_t)n); L.nrm = k.take((size_t)n * 24);
    L.parent = k.take((size_t)n * 4); L.root = k.take((size_t)n * 4); L.cnt = k.take((size_t)n * 4);
    L.flags = k.take(((size_t)n + 1) * 4); L.labels_b = k.take((size_t)n * 4);
    L.keys_a = k.take((size_t)n * 4); L.keys_b = k.take((size_t)n * 4); L.vals_a = k.take((size_t)n * 4); L.vals_b = k.take((size_t)n * 4);
    L.starts = k.take((np + 1) * 8);
    L.partial = k.take((((size_t)n >> SUM_SHIFT) + np + 1) * 48);
    L.frames = k.take(np * PL_FRAME * 8); L.rms = k.take(np * 8); L.ext = k.take(np * 32);
    L.temp = k.take(L.temp_bytes);
    L.total = k.off;
    return L;
}

dim3 grid_of(int64_t n) { return dim3(f3d_grid_for(n, PB, PGRID)); }

}  // namespace

size_t f3d_planes_scratch_bytes(int64_t n) { return planes_layout_for(n).total; }

hipError_t f3d_launch_extract_planes(const void* xyz, int dtype, int64_t n, const int64_t* offs, const int32_t* nbrs,
                                     const double* normals, const f3d_planes_args& a, int32_t* labels, double* planes, double* corners,
                                     int64_t* counts, double* normals_out, void* scratch, int* err, hipStream_t s) {
    if (n < 1 || n > 0x7fffffffLL || a.min_points < 3 || a.max_planes < 0 || a.max_rounds < 0) return hipErrorInvalidValue;
    const planes_layout L = planes_layout_for(n);
    char* base = reinterpret_cast<char*>(scratch);
    pl_words* w = reinterpret_cast<pl_words*>(base + L.words);
    uint8_t* core = reinterpret_cast<uint8_t*>(base + L.core);
    // the normals the kernels read: the caller's, or the computed ones (in the caller's output array when there is one)
    double* nrm_w = normals ? nullptr : (normals_out ? normals_out : reinterpret_cast<double*>(base + L.nrm));
    const double* nrm = normals ? normals : nrm_w;
    int32_t *parent = reinterpret_cast<int32_t*>(base + L.parent), *root = reinterpret_cast<int32_t*>(base + L.root),
            *cnt = reinterpret_cast<int32_t*>(base + L.cnt), *labels_b = reinterpret_cast<int32_t*>(base + L.labels_b);
    uint32_t *flags = reinterpret_cast<uint32_t*>(base + L.flags), *ka = reinterpret_cast<uint32_t*>(base + L.keys_a),
             *kb = reinterpret_cast<uint32_t*>(base + L.keys_b), *va = reinterpret_cast<uint32_t*>(base + L.vals_a),
             *vb = reinterpret_cast<uint32_t*>(base + L.vals_b);
    int64_t* starts = reinterpret_cast<int64_t*>(base + L.starts);
    double *partial = reinterpret_cast<double*>(base + L.partial), *frames = reinterpret_cast<double*>(base + L.frames),
           *rms = reinterpret_cast<double*>(base + L.rms);
    unsigned long long* ext = reinterpret_cast<unsigned long long*>(base + L.ext);
    const dim3 g(grid_of(n + 1)), b(PB), gw(f3d_grid_for(n / 3 + 1, PB / 64, PGRID));
    const int64_t mp = a.max_planes;
    const int key_bits = f3d_bits_for(n / 3 + 2, 1);

    F3D_TRY(hipMemsetAsync(w, 0, sizeof(pl_words), s));
    hipLaunchKernelGGL(k_pl_check, g, b, 0, s, n, offs, nbrs, w, err);
    hipLaunchKernelGGL(k_pl_core, g, b, 0, s, xyz, dtype, n, offs, nbrs, normals, a.max_variation, w, core, nrm_w, parent, cnt);
    hipLaunchKernelGGL(k_pl_union, g, b, 0, s, xyz, dtype, n, offs, nbrs, core, nrm, a.cos_angle, a.offset, w, parent);
    hipLaunchKernelGGL(k_pl_roots, g, b, 0, s, parent, n, core, w, root, cnt);
    hipLaunchKernelGGL(k_pl_flags, g, b, 0, s, root, cnt, n, a.min_points, w, flags);
    F3D_TRY(hipGetLastError());
    size_t tb = L.temp_bytes;
    F3D_TRY(rocprim::exclusive_scan(base + L.temp, tb, flags, flags, (uint32_t)0, (size_t)n + 1, rocprim::plus<uint32_t>(), s));
    hipLaunchKernelGGL(k_pl_labels, g, b, 0, s, root, flags, n, mp, w, labels);

    // the members of every plane in ascending index, then centroid and moments
    auto group = [&](const int32_t* lab) -> hipError_t {
        hipLaunchKernelGGL(k_pl_group_keys, g, b, 0, s, lab, n, flags, mp, w, ka, va);
        F3D_TRY(hipGetLastError());
        return f3d_group_pairs(ka, kb, va, vb, n, key_bits, base + L.temp, L.temp_bytes, mp, flags + n, &w->bad, starts, s);
    };
    auto sums = [&](int mode) -> hipError_t {
        hipLaunchKernelGGL(k_pl_chunk_sums, g, b, 0, s, xyz, dtype, n, mode, vb, kb, starts, flags, mp, frames, w, partial);
        hipLaunchKernelGGL(k_pl_fit, gw, b, 0, s, n, mode, starts, flags, mp, partial, nrm, normals ? 1 : 0, vb, w, frames, rms);
        return hipGetLastError();
    };
    F3D_TRY(group(labels));
    F3D_TRY(sums(SUM_MEAN));
    F3D_TRY(sums(SUM_MOMENTS));
    hipLaunchKernelGGL(k_pl_inliers, g, b, 0, s, xyz, dtype, n, frames, a.dist, w, labels);
    F3D_TRY(hipGetLastError());

    // attach: round t reads buf[t & 1] and writes buf[~t & 1]
    int32_t* buf[2] = {labels, labels_b};
    pl_words hw = {0, 0, 0, 0};
    for (int64_t t = 0; t < a.max_rounds;) {
        for (int q = 0; q < ATTACH_CHUNK && t < a.max_rounds; ++q, ++t) {
            hipLaunchKernelGGL(k_pl_attach, g, b, 0, s, xyz, dtype, n, offs, nbrs, frames, a.dist, buf[t & 1], buf[(t & 1) ^ 1], w);
            hipLaunchKernelGGL(k_pl_round_end, dim3(1), dim3(1), 0, s, w);
        }
        F3D_TRY(hipGetLastError());
        F3D_TRY(hipMemcpyAsync(&hw, w, sizeof(hw), hipMemcpyDeviceToHost, s));
        F3D_TRY(hipStreamSynchronize(s));
        if (hw.bad || hw.done) break;
    }
    const int32_t* fin = buf[hw.rounds & 1];
    if (fin != labels) hipLaunchKernelGGL(k_pl_copy_labels, g, b, 0, s, fin, n, w, labels);

    // final members: residuals, extents, the rows
    F3D_TRY(group(labels));
    F3D_TRY(sums(SUM_RESIDUAL));
    hipLaunchKernelGGL(k_pl_ext_init, g, b, 0, s, n, flags, mp, w, ext);
    hipLaunchKernelGGL(k_pl_extents, g, b, 0, s, xyz, dtype, n, labels, frames, w, ext);
    hipLaunchKernelGGL(k_pl_finish, grid_of(mp > 0 ? mp : 1), b, 0, s, n, flags, mp, frames, rms, ext, starts, w, planes, corners, counts);
    return hipGetLastError();
}
