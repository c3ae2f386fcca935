// Feature fusion (include/f3d.h "feature fusion"): per-point sums of per-pixel feature rows over the views that see the point, and
// the mean / unit-length rows made from them.
//
// The samples and the visibility rule are those of f3d_vote_visible (f3d_sample, the splat keys of the same cloud); what differs is
// the payload: a contiguous row of d channels per visible sample instead of a byte.  A group of G lanes owns a point and keeps its
// row of sums in registers, lane g holding the 16-byte slices g, g + G, ... of the row.  The group projects G views at a time, one per
// lane, ballots the visible ones and walks the set bits in ascending order: the cell index is broadcast, every lane loads its
// slices of that feature row and adds them.  Per point the adds therefore happen in ascending view order, one float32 add per
// channel and sample, whatever the launch shape or the pass size: the result is fixed bit for bit.  No atomics.
#include <hip/hip_runtime.h>
#include <float.h>
#include <stdint.h>
#include "f3d.h"
#include "f3d_math.h"
#include "f3d_kernels.h"

#pragma clang fp contract(off)

namespace {

typedef _Float16 f3d_h8 __attribute__((ext_vector_type(8)));
typedef float f3d_f4 __attribute__((ext_vector_type(4)));

// a 16-byte slice of a feature row: E channels
template <typename F> struct feat_slice;
template <> struct feat_slice<_Float16> { static constexpr int E = 8; typedef f3d_h8 vec; };
template <> struct feat_slice<float> { static constexpr int E = 4; typedef f3d_f4 vec; };

// a view record in LDS: 712 bytes apart, so that the lanes of a group (one record each) spread over the banks (704 B = 176 dwords
// would put 16 lanes on one bank of a ds_read_b64)
struct view_slot { f3d_view v; double pad; };
#define F3D_VIEW_DOUBLES ((int)(sizeof(f3d_view) / 8))

__device__ __forceinline__ void stage_views(view_slot* lv, const f3d_view* __restrict__ views, int nc) {
    const double* src = (const double*)views;
    double* dst = (double*)lv;
    for (int k = threadIdx.x; k < nc * F3D_VIEW_DOUBLES; k += F3D_BLOCK)
        dst[(k / F3D_VIEW_DOUBLES) * (F3D_VIEW_DOUBLES + 1) + k % F3D_VIEW_DOUBLES] = src[k];
}

// acc += the slices of one feature row.  A 16-byte aligned row is read in 16-byte loads, all of a lane's slices requested before the
// first add; a slice the row ends in (d not a multiple of E) and every slice of an unaligned row go channel by channel.
template <typename F, int G, int S>
__device__ __forceinline__ void add_row(float (&acc)[S][feat_slice<F>::E], const F* __restrict__ row, int d, int gl) {
    constexpr int E = feat_slice<F>::E;
    typedef typename feat_slice<F>::vec vec;
    if (((uintptr_t)row & 15) == 0) {
        vec x[S];
#pragma unroll
        for (int k = 0; k < S; ++k) {
            const int c0 = (gl + k * G) * E;
            if (c0 + E <= d) x[k] = *(const vec*)(row + c0);
        }
#pragma unroll
        for (int k = 0; k < S; ++k) {
            const int c0 = (gl + k * G) * E;
            if (c0 + E <= d) {
#pragma unroll
                for (int e = 0; e < E; ++e) acc[k][e] = acc[k][e] + (float)x[k][e];
            } else {
#pragma unroll
                for (int e = 0; e < E; ++e)
                    if (c0 + e < d) acc[k][e] = acc[k][e] + (float)row[c0 + e];
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < S; ++k) {
            const int c0 = (gl + k * G) * E;
            if (c0 + E <= d) {
                F x[E];
#pragma unroll
                for (int e = 0; e < E; ++e) x[e] = row[c0 + e];
#pragma unroll
                for (int e = 0; e < E; ++e) acc[k][e] = acc[k][e] + (float)x[e];
            } else {
#pragma unroll
                for (int e = 0; e < E; ++e)
                    if (c0 + e < d) acc[k][e] = acc[k][e] + (float)row[c0 + e];
            }
        }
    }
}

// the group's row of sums <-> registers, with the same split: float4 where the row is 16-byte aligned and the slice is whole
template <int G, int S, int E, bool STORE>
__device__ __forceinline__ void move_sums(float (&acc)[S][E], float* row, int d, int gl) {
    const bool al = ((uintptr_t)row & 15) == 0;
#pragma unroll
    for (int k = 0; k < S; ++k) {
        const int c0 = (gl + k * G) * E;
        if (al && c0 + E <= d) {
#pragma unroll
            for (int q = 0; q < E / 4; ++q) {
                f3d_f4* p = (f3d_f4*)(row + c0 + 4 * q);
                if (STORE) {
                    f3d_f4 x;
                    x[0] = acc[k][4 * q]; x[1] = acc[k][4 * q + 1]; x[2] = acc[k][4 * q + 2]; x[3] = acc[k][4 * q + 3];
                    *p = x;
                } else {
                    const f3d_f4 x = *p;
                    acc[k][4 * q] = x[0]; acc[k][4 * q + 1] = x[1]; acc[k][4 * q + 2] = x[2]; acc[k][4 * q + 3] = x[3];
                }
            }
        } else {
#pragma unroll
            for (int e = 0; e < E; ++e)
                if (c0 + e < d) {
                    if (STORE) row[c0 + e] = acc[k][e]; else acc[k][e] = row[c0 + e];
                }
        }
    }
}

// the feature pixel vf * wf + uf of the visible sample of point p in view vw, -1 without one.  plane: the view's depth keys, NULL = every
// sample is visible
__device__ __forceinline__ int sample_pixel(const f3d_view& vw, f3d_p3 p, int h, int w, int hf, int wf, const unsigned long long* __restrict__ plane,
                                            double depth_tol) {
    int u, v;
    float z32;
    if (!f3d_sample(vw, p, h, w, u, v, z32)) return -1;
    if (plane) {
        const unsigned long long key = plane[(size_t)v * w + u];
        const float zmin32 = __uint_as_float((uint32_t)(key >> 32));            // never empty: this sample covers the cell
        if (!((double)z32 <= (double)zmin32 + depth_tol)) return -1;
    }
    return (int)((int64_t)v * hf / h) * wf + (int)((int64_t)u * wf / w);
}

// T: the cloud's type, F: the features' type, G lanes per point (a power of two <= 64), S 16-byte slices per lane (> 1 only with
// G = 64).  A block works on F3D_BLOCK / G points at a time (a tile) and walks the tiles with the grid's stride.  The view records of
// the pass are staged in LDS, C at a time: once per block when the pass has at most C views, otherwise per tile.  zkey == NULL:
// every sample is visible (depth_tol = +inf).  A point without a visible sample in the pass is neither read nor written.
template <typename T, typename F, int G, int S>
__global__ __launch_bounds__(F3D_BLOCK) void k_fuse_features(const T* __restrict__ xyz, int64_t n, const f3d_view* __restrict__ views, int nv,
                                                              int h, int w, const F* __restrict__ feats, int hf, int wf, int d,
                                                              const unsigned long long* __restrict__ zkey, double depth_tol,
                                                              float* __restrict__ sums, int32_t* __restrict__ counts) {
    constexpr int E = feat_slice<F>::E, C = G < 32 ? 32 : G, PPB = F3D_BLOCK / G;
    __shared__ view_slot lv[C];
    const int lane = threadIdx.x & 63, gl = threadIdx.x & (G - 1), gbase = lane & ~(G - 1);
    const unsigned long long gmask = (G == 64 ? ~0ull : (1ull << (G & 63)) - 1) << gbase;
    const size_t hw = (size_t)h * w, fcells = (size_t)hf * wf;
    const bool once = nv <= C;
    if (once) {
        stage_views(lv, views, nv);
        __syncthreads();
    }
    const int64_t ntiles = (n + PPB - 1) / PPB;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {     // (block-uniform: the barriers below are reached by all)
        const int64_t i = tile * PPB + threadIdx.x / G;
        const bool live = i < n;
        f3d_p3 p;
        p.x = p.y = p.z = 0.0;
        if (live) p = f3d_load_p3(xyz, i);
        float acc[S][E];
        bool touched = false;
        int cnt = 0;
        for (int j0 = 0; j0 < nv; j0 += C) {
            const int nc = nv - j0 < C ? nv - j0 : C;
            if (!once) {
                __syncthreads();
                stage_views(lv, views + j0, nc);
                __syncthreads();
            }
            for (int k0 = 0; k0 < nc; k0 += G) {
                const int k = k0 + gl;
                int pf = -1;                                                 // this lane's view: the feature pixel of a visible sample
                if (live && k < nc) pf = sample_pixel(lv[k].v, p, h, w, hf, wf, zkey ? zkey + (size_t)(j0 + k) * hw : nullptr, depth_tol);
                unsigned long long m = __ballot(pf >= 0) & gmask;            // the same in every lane of the group
                if (m && !touched) {
                    move_sums<G, S, E, false>(acc, sums + (size_t)i * d, d, gl);
                    touched = true;
                }
                cnt += __popcll(m);
                while (m) {                                                  // ascending views
                    const int src = __ffsll((long long)m) - 1;
                    m &= m - 1;
                    const int cell = __shfl(pf, src, 64);
                    const size_t j = (size_t)(j0 + k0 + (src - gbase));
                    add_row<F, G, S>(acc, feats + (j * fcells + (size_t)cell) * d, d, gl);
                }
            }
        }
        if (touched) {
            move_sums<G, S, E, true>(acc, sums + (size_t)i * d, d, gl);
            if (gl == 0) counts[i] += cnt;
        }
    }
}

// The same for a pass of so few views that a group would leave most of its lanes idle while it projects (2 nv <= G).  The group's lanes
// then project R = G / P consecutive points at once, P = the power of two >= nv lanes each, and the group gathers for those points one
// after the other: per point still one read and one write of its sums, the adds in ascending view order.
template <typename T, typename F, int G, int S>
__global__ __launch_bounds__(F3D_BLOCK) void k_fuse_features_few(const T* __restrict__ xyz, int64_t n, const f3d_view* __restrict__ views, int nv,
                                                                  int P, int h, int w, const F* __restrict__ feats, int hf, int wf, int d,
                                                                  const unsigned long long* __restrict__ zkey, double depth_tol,
                                                                  float* __restrict__ sums, int32_t* __restrict__ counts) {
    constexpr int E = feat_slice<F>::E, PPB = F3D_BLOCK / G;
    __shared__ view_slot lv[32];                                                // nv <= G / 2 <= 32
    const int lane = threadIdx.x & 63, gl = threadIdx.x & (G - 1), gbase = lane & ~(G - 1);
    const int R = G / P, sub = gl / P, pl = gl & (P - 1);
    const size_t hw = (size_t)h * w, fcells = (size_t)hf * wf;
    stage_views(lv, views, nv);
    __syncthreads();
    const int64_t per_tile = (int64_t)PPB * R, ntiles = (n + per_tile - 1) / per_tile;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t i0 = tile * per_tile + (int64_t)(threadIdx.x / G) * R;    // the group's first point
        int pf = -1;
        if (i0 + sub < n && pl < nv)
            pf = sample_pixel(lv[pl].v, f3d_load_p3(xyz, i0 + sub), h, w, hf, wf, zkey ? zkey + (size_t)pl * hw : nullptr, depth_tol);
        const unsigned long long ball = __ballot(pf >= 0);
        for (int r = 0; r < R; ++r) {
            const int first = gbase + r * P;                                    // the lanes that projected point i0 + r
            unsigned m = (unsigned)(ball >> first) & (unsigned)((1ull << P) - 1);
            if (!m) continue;                                                   // (the same in every lane of the group)
            float* row = sums + (size_t)(i0 + r) * d;
            float acc[S][E];
            move_sums<G, S, E, false>(acc, row, d, gl);
            const int cnt = __popc(m);
            while (m) {                                                         // ascending views
                const int j = __ffs((int)m) - 1;
                m &= m - 1;
                const int cell = __shfl(pf, first + j, 64);
                add_row<F, G, S>(acc, feats + ((size_t)j * fcells + (size_t)cell) * d, d, gl);
            }
            move_sums<G, S, E, true>(acc, row, d, gl);
            if (gl == 0) counts[i0 + r] += cnt;
        }
    }
}

// g lanes per point (a power of two <= 64), lane c of the group takes channels c, c + g, ...  The mean is formed in float64 and
// rounded once: for two float32 operands that is the correctly rounded float32 quotient (53 >= 2 * 24 + 2).  The butterfly leaves the
// same float64 sum of squares in every lane of the group.  out may be sums: a lane writes only what it alone read.
__global__ __launch_bounds__(F3D_BLOCK) void k_features_finalize(const float* sums, const int32_t* __restrict__ counts, int64_t n, int d, int g,
                                                                  int normalize, float* out) {
    const int ppb = F3D_BLOCK / g, gl = threadIdx.x & (g - 1);
    const int64_t ntiles = (n + ppb - 1) / ppb;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t i = tile * ppb + threadIdx.x / g;
        const bool live = i < n;
        const int cnt = live ? counts[i] : 0;
        const double den = (double)(float)cnt;
        const float* row = sums + (size_t)(live ? i : 0) * d;
        float* orow = out + (size_t)(live ? i : 0) * d;
        double s = 0.0;
        if (normalize && cnt > 0)
            for (int c = gl; c < d; c += g) {
                const double m = (double)(float)((double)row[c] / den);
                s = s + m * m;
            }
        for (int o = g >> 1; o >= 1; o >>= 1) s = s + __shfl_xor(s, o, 64);
        if (!live) continue;
        const double len = sqrt(s);
        for (int c = gl; c < d; c += g) {
            float m = 0.f;
            if (cnt > 0) {
                m = (float)((double)row[c] / den);
                if (normalize) m = s == 0.0 ? 0.f : (float)((double)m / len);
            }
            orow[c] = m;
        }
    }
}

// (G, S) of a row of d channels in slices of E: the smallest power of two G with G * E >= d, at most 64, then the smallest power of
// two S with 64 * S * E >= d
inline void group_shape(int d, int E, int& G, int& S) {
    const int slices = (d + E - 1) / E;
    G = 1; S = 1;
    while (G < 64 && G < slices) G <<= 1;
    while (G * S < slices) S <<= 1;
}

template <typename T, typename F>
hipError_t launch_fuse(const void* xyz, int64_t n, const f3d_view* views_dev, int nv, int h, int w, const void* feats, int hf, int wf, int d,
                       const unsigned long long* zkey, double depth_tol, float* sums, int32_t* counts, hipStream_t s) {
    int G, S;
    group_shape(d, feat_slice<F>::E, G, S);
    int P = 1;                                                                  // few views: P lanes project a point (k_fuse_features_few)
    while (P < nv) P <<= 1;
#define F3D_FF(GG, SS) do { \
        const dim3 b(F3D_BLOCK); \
        if constexpr (GG > 1) \
            if (2 * nv <= GG) { \
                const int64_t per_tile = (int64_t)(F3D_BLOCK / GG) * (GG / P); \
                hipLaunchKernelGGL((k_fuse_features_few<T, F, GG, SS>), dim3(f3d_grid_for((n + per_tile - 1) / per_tile, 1, F3D_GRID_CAP)), b, 0, s, \
                                   (const T*)xyz, n, views_dev, nv, P, h, w, (const F*)feats, hf, wf, d, zkey, depth_tol, sums, counts); \
                return hipGetLastError(); \
            } \
        hipLaunchKernelGGL((k_fuse_features<T, F, GG, SS>), dim3(f3d_grid_for((n + F3D_BLOCK / GG - 1) / (F3D_BLOCK / GG), 1, F3D_GRID_CAP)), b, 0, s, \
                           (const T*)xyz, n, views_dev, nv, h, w, (const F*)feats, hf, wf, d, zkey, depth_tol, sums, counts); \
        return hipGetLastError(); } while (0)
    switch (G * 100 + S) {
        case 101: F3D_FF(1, 1);
        case 201: F3D_FF(2, 1);
        case 401: F3D_FF(4, 1);
        case 801: F3D_FF(8, 1);
        case 1601: F3D_FF(16, 1);
        case 3201: F3D_FF(32, 1);
        case 6401: F3D_FF(64, 1);
        case 6402: F3D_FF(64, 2);
        case 6404: F3D_FF(64, 4);
        case 6408: F3D_FF(64, 8);
        case 6416: if constexpr (feat_slice<F>::E == 4) F3D_FF(64, 16);                // (d <= 4096: float32 rows only)
    }
#undef F3D_FF
    return hipErrorInvalidValue;
}

}  // namespace

hipError_t f3d_launch_fuse_features(const void* xyz, int dtype, int64_t n, const f3d_view* views_dev, int nv, int h, int w, const void* feats,
                                    int ftype, int hf, int wf, int d, const unsigned long long* zkey, double depth_tol, float* sums,
                                    int32_t* counts, hipStream_t s) {
    if (n <= 0 || nv <= 0) return hipSuccess;
    if (d < 1 || d > 4096) return hipErrorInvalidValue;
#define F3D_FL(T, F) launch_fuse<T, F>(xyz, n, views_dev, nv, h, w, feats, hf, wf, d, zkey, depth_tol, sums, counts, s)
    if (dtype == F3D_F64) return ftype == F3D_FEAT_F16 ? F3D_FL(double, _Float16) : F3D_FL(double, float);
    return ftype == F3D_FEAT_F16 ? F3D_FL(float, _Float16) : F3D_FL(float, float);
#undef F3D_FL
}

hipError_t f3d_launch_features_finalize(const float* sums, const int32_t* counts, int64_t n, int d, int normalize, float* out, hipStream_t s) {
    if (n <= 0 || d <= 0) return hipSuccess;
    int g = 1;
    while (g < 64 && g < d) g <<= 1;
    const int ppb = F3D_BLOCK / g;
    hipLaunchKernelGGL(k_features_finalize, dim3(f3d_grid_for((n + ppb - 1) / ppb, 1, F3D_GRID_CAP)), dim3(F3D_BLOCK), 0, s, sums, counts, n, d, g,
                       normalize, out);
    return hipGetLastError();
}
