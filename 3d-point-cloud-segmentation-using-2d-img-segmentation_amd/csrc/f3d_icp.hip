// Registration (include/f3d.h "registration"): model maps of a TSDF volume by ray casting, and projective point-to-plane ICP of a depth
// frame against such maps.  The contract there is restated operation for operation in tests/icp_ref.py; everything that decides a
// result is float64 without contraction, in the order written.
//
//   k_tsdf_raycast  one thread per pixel, a wavefront = one 8 x 8 pixel tile (neighbouring rays touch neighbouring voxels), no LDS.  The
//                   per-ray constants (origin, direction, the sample range) are hoisted; the eight taps of a sample are loaded as four
//                   pairs adjacent in x.  The march starts and ends where a slab test of the ray against the box of valid sample
//                   positions, widened by a margin that dwarfs every rounding, says so: every sample it skips fails the index rule of
//                   the contract, so no bit of the output depends on it.
//   k_icp_terms     one wave per chunk of F3D_ICP_CHUNK source pixels: lane l takes the pixels l, l + 64, .. of the chunk in ascending
//                   order with the 29 accumulators in registers (f3d_wave_sum's lane order), the xor butterfly follows, lane 0 stores
//                   the chunk row.
//   k_icp_solve     one block: its waves take the 29 totals in turn (f3d_wave_sum over the chunk sums); after the barrier thread 0 does
//                   the 6 x 6 Cholesky solve and writes the pose and the stats row.  Two launches per round, no host round trip: the pose
//                   and the lost flag live in device memory, both kernels read them.
// Colour (f3d_tsdf_raycast_color, f3d_icp_color_sums, f3d_icp_color) is the COLOR = true instantiation of the three kernels; the
// depth-only ones carry none of its arguments and none of its code:
//   k_tsdf_raycast<true>  after the hit is settled, the colour state's eight corners around V, lerped like F.
//   k_icp_terms<T, true>  a second sweep over the chunk recomputes each pixel and accumulates the 29 photometric terms, so that no more
//                         than 29 accumulators are live at a time; a chunk row is 58 wide, the geometric sums first.
//   k_icp_solve<true>     58 totals; A = A_g + color_weight * A_c; a stats row of 5.
// Coarse-to-fine (f3d_depth_half, f3d_maps_half, f3d_icp_levels): two kernels that halve a depth frame and a set of model maps, and a
// launcher that runs the rounds above over a list of levels.  It adds no arithmetic to a round: k_icp_terms and k_icp_solve are used
// as they are.
//   k_depth_half<T>       one thread per output pixel, grid-stride; the 2 x 2 block's four samples in registers; no LDS, no atomics.
//   k_maps_half<INTENSITY> the same over the model maps: a block row's two map rows are 48 contiguous bytes, which the compiler
//                         fetches with three 16-byte loads (global memory needs no 16-byte alignment for them).
// Cloud to cloud (f3d_cloud_icp_sums, f3d_cloud_icp): the source is an unordered cloud and its partner the nearest target point, found
// in the target's radius grid (f3d_launch_graph_grid, built once per call by the C-ABI layer) with f3d_grid_walk_d2.
//   k_cloud_icp_terms<T, MODE>  k_icp_terms' wave per chunk, lane order, butterfly and chunk row.  A lane transforms its point, walks the
//                         <= 27 cells around it keeping the running (d2, index) minimum, and forms the terms of the pair: no pair list is
//                         kept in memory.  MODE is point-to-plane (the target's normals) or point-to-point (three unit-axis rows per pair,
//                         their zero products left out).  k_icp_solve follows unchanged.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "f3d.h"
#include "f3d_math.h"
#include "f3d_kernels.h"
#include "f3d_groups.h"

#pragma clang fp contract(off)

namespace {

constexpr int NS = F3D_ICP_NSUMS;
constexpr int NSC = F3D_ICP_NSUMS_COLOR;
constexpr int ICP_WAVES = F3D_BLOCK / 64;                  // chunks a block of k_icp_terms takes per pass: one per wave

template <typename T> struct raw_depth;
template <> struct raw_depth<double> { static __device__ __forceinline__ double at(const double* d, int64_t i) { return d[i]; } };
template <> struct raw_depth<float> { static __device__ __forceinline__ double at(const float* d, int64_t i) { return (double)d[i]; } };
template <> struct raw_depth<uint16_t> { static __device__ __forceinline__ double at(const uint16_t* d, int64_t i) { return (double)d[i]; } };

struct ray_volume {
    const float* tsdf; const float* weight;
    int nx, ny, nz;
    double lo[3], vs;
    float min_weight;
};

// F(P) of the contract: false = the sample is invalid
__device__ __forceinline__ bool sample(const ray_volume& g, double px, double py, double pz, double& F) {
    const double gx = (px - g.lo[0]) / g.vs - 0.5, gy = (py - g.lo[1]) / g.vs - 0.5, gz = (pz - g.lo[2]) / g.vs - 0.5;
    const double ix = floor(gx), iy = floor(gy), iz = floor(gz);
    if (!(ix >= 0.0 && ix <= (double)(g.nx - 2) && iy >= 0.0 && iy <= (double)(g.ny - 2) && iz >= 0.0 && iz <= (double)(g.nz - 2))) return false;
    const double fx = gx - ix, fy = gy - iy, fz = gz - iz;
    const int64_t sy = g.nx, sz = (int64_t)g.nx * g.ny;
    const int64_t at = ((int64_t)iz * g.ny + (int64_t)iy) * g.nx + (int64_t)ix;
    const float* W = g.weight + at;
    bool seen = true;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int64_t o = (c & 1) * sy + (c >> 1) * sz;
        seen = seen & (W[o] >= g.min_weight) & (W[o + 1] >= g.min_weight);
    }
    if (!seen) return false;
    const float* S = g.tsdf + at;
    double cjk[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {                           // c = j + 2 k: the pair (T0jk, T1jk), lerped along x
        const int64_t o = (c & 1) * sy + (c >> 1) * sz;
        const double t0 = (double)S[o], t1 = (double)S[o + 1];
        cjk[c] = t0 + fx * (t1 - t0);
    }
    const double c0 = cjk[0] + fy * (cjk[1] - cjk[0]), c1 = cjk[2] + fy * (cjk[3] - cjk[2]);
    F = c0 + fz * (c1 - c0);
    return true;
}

// The samples k of [0, nsteps) that can be valid lie in [k0, k1): outside it P_a(s_k) misses the box of valid positions
// [lo + 0.5 vs, lo + (n - 0.5) vs) on some axis by more than a voxel, a step and 1e-6 of the operand magnitudes, nine decimal orders
// above the rounding of either evaluation.  Anything not finite leaves the whole range to the samples.
__device__ __forceinline__ void sample_range(const ray_volume& g, const double t[3], const double dw[3], double near, double step, int nsteps,
                                             int& k0, int& k1) {
    k0 = 0; k1 = nsteps;
    double s0 = -INFINITY, s1 = INFINITY;
    const int n[3] = {g.nx, g.ny, g.nz};
    const double far = near + (double)nsteps * step;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double bmin = g.lo[a], bmax = g.lo[a] + (double)n[a] * g.vs;
        const double reach = fabs(dw[a]) * (fabs(near) + fabs(far));
        const double m = g.vs + 1e-6 * (((fabs(bmin) + fabs(bmax)) + fabs(t[a])) + reach);
        if (!(m < INFINITY)) return;
        const double a0 = (bmin - m) - t[a], a1 = (bmax + m) - t[a];
        if (reach < m * 1e-3) {                                                   // the ray moves far less than the margin along this axis
            if (a0 > m || a1 < -m) { k1 = 0; return; }                            // and starts more than a margin outside the widened slab
            continue;
        }
        const double u0 = a0 / dw[a], u1 = a1 / dw[a];
        if (!(u0 == u0 && u1 == u1)) return;
        s0 = fmax(s0, fmin(u0, u1)); s1 = fmin(s1, fmax(u0, u1));
    }
    if (!(s0 <= s1)) { k1 = 0; return; }
    const double f0 = floor((s0 - near) / step) - 2.0, f1 = ceil((s1 - near) / step) + 3.0;
    if (!(f0 == f0 && f1 == f1)) return;
    if (f0 > 0.0) k0 = f0 < (double)nsteps ? (int)f0 : nsteps;
    if (f1 < (double)nsteps) k1 = f1 > 0.0 ? (int)f1 : 0;
}

struct ray_camera { double fx, fy, cx, cy, qn[4], t[3]; };

// the colour arguments of k_tsdf_raycast<true>: the state (r, g, b, wc) per voxel and the two colour outputs (each may be NULL); the
// depth-only instantiation carries none
template <bool COLOR> struct ray_color_io {};
template <> struct ray_color_io<true> { const float4* color; double* rgb; double* intensity; };

__device__ __forceinline__ double intensity_of(double r, double g, double b) { return ((0.299 * r + 0.587 * g) + 0.114 * b) / 255.0; }

// the colour sample of the contract at V: false = invalid (V outside the index rule, or a corner without colour)
__device__ __forceinline__ bool sample_color(const ray_volume& g, const float4* __restrict__ color, const double V[3], double rgb[3]) {
    const double gx = (V[0] - g.lo[0]) / g.vs - 0.5, gy = (V[1] - g.lo[1]) / g.vs - 0.5, gz = (V[2] - g.lo[2]) / g.vs - 0.5;
    const double ix = floor(gx), iy = floor(gy), iz = floor(gz);
    if (!(ix >= 0.0 && ix <= (double)(g.nx - 2) && iy >= 0.0 && iy <= (double)(g.ny - 2) && iz >= 0.0 && iz <= (double)(g.nz - 2))) return false;
    const double fx = gx - ix, fy = gy - iy, fz = gz - iz;
    const int64_t sy = g.nx, sz = (int64_t)g.nx * g.ny;
    const float4* C = color + (((int64_t)iz * g.ny + (int64_t)iy) * g.nx + (int64_t)ix);
    double cjk[4][3];
    bool seen = true;
#pragma unroll
    for (int c = 0; c < 4; ++c) {                           // c = j + 2 k: the pair (C0jk, C1jk), lerped along x
        const int64_t o = (c & 1) * sy + (c >> 1) * sz;
        const float4 c0 = C[o], c1 = C[o + 1];
        seen = seen & (c0.w > 0.f) & (c1.w > 0.f);
        cjk[c][0] = (double)c0.x + fx * ((double)c1.x - (double)c0.x);
        cjk[c][1] = (double)c0.y + fx * ((double)c1.y - (double)c0.y);
        cjk[c][2] = (double)c0.z + fx * ((double)c1.z - (double)c0.z);
    }
    if (!seen) return false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double c0 = cjk[0][a] + fy * (cjk[1][a] - cjk[0][a]), c1 = cjk[2][a] + fy * (cjk[3][a] - cjk[2][a]);
        rgb[a] = c0 + fz * (c1 - c0);
    }
    return true;
}

template <bool COLOR>
__global__ __launch_bounds__(F3D_BLOCK) void k_tsdf_raycast(ray_volume g, ray_camera cam, int h, int w, double near, double step, int nsteps,
                                                             double* __restrict__ vertex, double* __restrict__ normal, double* __restrict__ depth,
                                                             ray_color_io<COLOR> cio) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tx = (w + 7) >> 3, ty = (h + 7) >> 3;
    const int64_t ntiles = (int64_t)tx * ty;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    for (int64_t tile = (int64_t)blockIdx.x * (F3D_BLOCK / 64) + wave; tile < ntiles; tile += (int64_t)gridDim.x * (F3D_BLOCK / 64)) {
        const int u = (int)(tile % tx) * 8 + (lane & 7), v = (int)(tile / tx) * 8 + (lane >> 3);
        if (u >= w || v >= h) continue;
        f3d_p3 dc;
        dc.x = (((double)u + 0.5) - cam.cx) / cam.fx;
        dc.y = (((double)v + 0.5) - cam.cy) / cam.fy;
        dc.z = 1.0;
        const f3d_p3 d = f3d_rotate(cam.qn, dc);
        const double dw[3] = {d.x, d.y, d.z};
        int k0, k1;
        sample_range(g, cam.t, dw, near, step, nsteps, k0, k1);
        bool hit = false, prev_ok = false;
        double F_prev = 0.0, s_star = 0.0;
        for (int k = k0; k < k1; ++k) {
            const double s = near + (double)k * step;
            double F = 0.0;
            const bool valid = sample(g, cam.t[0] + s * dw[0], cam.t[1] + s * dw[1], cam.t[2] + s * dw[2], F);
            if (valid && F < 0.0) {
                if (prev_ok) {                                                  // then k >= 1: the sample before is the one that set prev_ok
                    const double s_prev = near + (double)(k - 1) * step;
                    s_star = s_prev + step * (F_prev / (F_prev - F));
                    hit = true;
                }
                break;
            }
            prev_ok = valid && F >= 0.0;
            F_prev = F;
        }
        double V[3] = {nan, nan, nan}, N[3] = {nan, nan, nan}, z = 0.0;
        if (hit) {
            const double P[3] = {cam.t[0] + s_star * dw[0], cam.t[1] + s_star * dw[1], cam.t[2] + s_star * dw[2]};
            double G[3];
            bool ok = true;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                double Fp = 0.0, Fm = 0.0;
                ok = ok && sample(g, P[0] + (a == 0 ? g.vs : 0.0), P[1] + (a == 1 ? g.vs : 0.0), P[2] + (a == 2 ? g.vs : 0.0), Fp);
                ok = ok && sample(g, P[0] - (a == 0 ? g.vs : 0.0), P[1] - (a == 1 ? g.vs : 0.0), P[2] - (a == 2 ? g.vs : 0.0), Fm);
                G[a] = Fp - Fm;
            }
            if (ok) {
                const double len = sqrt((G[0] * G[0] + G[1] * G[1]) + G[2] * G[2]);
                if (len > 0.0 && len < INFINITY) {
#pragma unroll
                    for (int a = 0; a < 3; ++a) { V[a] = P[a]; N[a] = G[a] / len; }
                    z = s_star;
                }
            }
        }
        const int64_t i = (int64_t)v * w + u;
        if (vertex) { vertex[3 * i] = V[0]; vertex[3 * i + 1] = V[1]; vertex[3 * i + 2] = V[2]; }
        if (normal) { normal[3 * i] = N[0]; normal[3 * i + 1] = N[1]; normal[3 * i + 2] = N[2]; }
        if (depth) depth[i] = z;
        if constexpr (COLOR) {
            double C[3] = {nan, nan, nan}, I = nan;
            if (V[0] == V[0]) {                                                 // a hit: its vertex is finite
                double S[3];
                if (sample_color(g, cio.color, V, S)) {
                    C[0] = S[0]; C[1] = S[1]; C[2] = S[2];
                    I = intensity_of(S[0], S[1], S[2]);
                }
            }
            if (cio.rgb) { cio.rgb[3 * i] = C[0]; cio.rgb[3 * i + 1] = C[1]; cio.rgb[3 * i + 2] = C[2]; }
            if (cio.intensity) cio.intensity[i] = I;
        }
    }
}

// ---- ICP -------------------------------------------------------------------------------------------------------------------
struct icp_frame {
    const void* depth;
    int h, w;
    double fx, fy, cx, cy, depth_scale, max_depth;
    const double* model_vertex; const double* model_normal;
    int hm, wm;
    const f3d_view* model_view;
    double max_dist2;
};

// the colour arguments of k_icp_terms<T, true>: the model's intensity map [hm*wm] (NaN = missing) and the source colour image
// [hc, wc, 3]; the depth-only instantiations carry none
template <bool COLOR> struct icp_color_io {};
template <> struct icp_color_io<true> { const double* model_intensity; const uint8_t* rgb; int hc, wc; };

// what the photometric pair of a pixel needs from its geometric steps
struct icp_seen { f3d_p3 pr; double x, y, h2; int u, v; };

__device__ __forceinline__ void normalised(const double q[4], double qn[4]) {
    const double len = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
    qn[0] = q[0] / len; qn[1] = q[1] / len; qn[2] = q[2] / len; qn[3] = q[3] / len;
}

// the pose of a call, from its kernel arguments into device memory, and the lost flag cleared
__global__ void k_icp_init(double* __restrict__ pose, int* __restrict__ lost, double q0, double q1, double q2, double q3, double t0, double t1, double t2) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        pose[0] = q0; pose[1] = q1; pose[2] = q2; pose[3] = q3; pose[4] = t0; pose[5] = t1; pose[6] = t2;
        *lost = 0;
    }
}

// the 29 terms of source pixel i at the pose (qn, t), added to acc; false = the pixel contributes 0.0 to every sum
template <typename T, bool SEEN>
__device__ __forceinline__ bool icp_pixel(const icp_frame& f, const double qn[4], const double t[3], int64_t i, double J[6], double& r, icp_seen& seen) {
    const double d = raw_depth<T>::at((const T*)f.depth, i) / f.depth_scale;
    if (!(d > 0.0 && d <= f.max_depth)) return false;
    const int v = (int)(i / f.w), u = (int)(i - (int64_t)v * f.w);
    f3d_p3 c;
    c.x = (((double)u + 0.5) - f.cx) * (d / f.fx);
    c.y = (((double)v + 0.5) - f.cy) * (d / f.fy);
    c.z = d;
    const f3d_p3 pr = f3d_rotate(qn, c);
    f3d_p3 p;
    p.x = pr.x + t[0]; p.y = pr.y + t[1]; p.z = pr.z + t[2];
    const f3d_view& mv = *f.model_view;
    const f3d_p3 hp = f3d_project_h(mv.K, mv.qinv, mv.t, p);
    if (!(hp.z > 0.0)) return false;
    const double x = hp.x / hp.z, y = hp.y / hp.z;
    if (!(x >= 0.0 && x < (double)f.wm && y >= 0.0 && y < (double)f.hm)) return false;
    const int um = (int)floor(x), vm = (int)floor(y);
    const int64_t at = 3 * ((int64_t)vm * f.wm + um);
    const double V0 = f.model_vertex[at], V1 = f.model_vertex[at + 1], V2 = f.model_vertex[at + 2];
    const double N0 = f.model_normal[at], N1 = f.model_normal[at + 1], N2 = f.model_normal[at + 2];
    if (!(fabs(V0) < INFINITY && fabs(V1) < INFINITY && fabs(V2) < INFINITY && fabs(N0) < INFINITY && fabs(N1) < INFINITY && fabs(N2) < INFINITY))
        return false;
    const double e0 = p.x - V0, e1 = p.y - V1, e2 = p.z - V2;
    if (!((e0 * e0 + e1 * e1) + e2 * e2 <= f.max_dist2)) return false;
    r = f3d_dot3(N0, N1, N2, e0, e1, e2);
    J[0] = pr.y * N2 - pr.z * N1;
    J[1] = pr.z * N0 - pr.x * N2;
    J[2] = pr.x * N1 - pr.y * N0;
    J[3] = N0; J[4] = N1; J[5] = N2;
    if constexpr (SEEN) { seen.pr = pr; seen.x = x; seen.y = y; seen.h2 = hp.z; seen.u = u; seen.v = v; }
    return true;
}

// the photometric pair of a pixel that passed step 5: false = it has none
__device__ __forceinline__ bool icp_color_pair(const icp_frame& f, const icp_color_io<true>& c, const icp_seen& p, double J[6], double& r) {
    const double a = p.x - 0.5, b = p.y - 0.5;
    const double i0 = floor(a), j0 = floor(b);
    if (!(i0 >= 0.0 && i0 <= (double)(f.wm - 2) && j0 >= 0.0 && j0 <= (double)(f.hm - 2))) return false;
    const double fa = a - i0, fb = b - j0;
    const double* I = c.model_intensity + ((int64_t)j0 * f.wm + (int64_t)i0);
    const double I00 = I[0], I10 = I[1], I01 = I[f.wm], I11 = I[f.wm + 1];
    if (!(fabs(I00) < INFINITY && fabs(I10) < INFINITY && fabs(I01) < INFINITY && fabs(I11) < INFINITY)) return false;
    const int64_t uc = (int64_t)p.u * c.wc / f.w, vc = (int64_t)p.v * c.hc / f.h;
    const uint8_t* pix = c.rgb + (vc * c.wc + uc) * 3;
    const double Is = intensity_of((double)pix[0], (double)pix[1], (double)pix[2]);
    const double top = I00 + fa * (I10 - I00), bot = I01 + fa * (I11 - I01);
    const double Im = top + fb * (bot - top);
    const double dx0 = I10 - I00, dx1 = I11 - I01;
    const double gx = dx0 + fb * (dx1 - dx0), gy = bot - top;
    r = Im - Is;
    const f3d_view& mv = *f.model_view;
    f3d_p3 gc;
    gc.x = (gx * (mv.K[0] - p.x * mv.K[6]) + gy * (mv.K[3] - p.y * mv.K[6])) / p.h2;
    gc.y = (gx * (mv.K[1] - p.x * mv.K[7]) + gy * (mv.K[4] - p.y * mv.K[7])) / p.h2;
    gc.z = (gx * (mv.K[2] - p.x * mv.K[8]) + gy * (mv.K[5] - p.y * mv.K[8])) / p.h2;
    const double qc[4] = {mv.qinv[0], -mv.qinv[1], -mv.qinv[2], -mv.qinv[3]};
    const f3d_p3 gw = f3d_rotate(qc, gc);
    J[0] = p.pr.y * gw.z - p.pr.z * gw.y;
    J[1] = p.pr.z * gw.x - p.pr.x * gw.z;
    J[2] = p.pr.x * gw.y - p.pr.y * gw.x;
    J[3] = gw.x; J[4] = gw.y; J[5] = gw.z;
    return true;
}

template <typename T, bool COLOR>
__global__ __launch_bounds__(F3D_BLOCK) void k_icp_terms(icp_frame f, const double* __restrict__ pose, const int* __restrict__ lost,
                                                          int64_t npix, int64_t nchunks, double* __restrict__ chunks, icp_color_io<COLOR> cio) {
    if (*lost) return;
    constexpr int ROW = COLOR ? NSC : NS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double qn[4];
    normalised(pose, qn);
    const double t[3] = {pose[4], pose[5], pose[6]};
    for (int64_t chunk = (int64_t)blockIdx.x * ICP_WAVES + wave; chunk < nchunks; chunk += (int64_t)gridDim.x * ICP_WAVES) {
        const int64_t first = chunk * F3D_ICP_CHUNK;
        const int64_t count = npix - first < F3D_ICP_CHUNK ? npix - first : (int64_t)F3D_ICP_CHUNK;
        double acc[NS];
#pragma unroll
        for (int j = 0; j < NS; ++j) acc[j] = 0.0;
        for (int64_t i = lane; i < count; i += 64) {
            double J[6], r;
            icp_seen seen;
            if (!icp_pixel<T, false>(f, qn, t, first + i, J, r, seen)) continue;   // + 0.0 leaves an accumulator as it is (none is ever -0.0)
            int j = 0;
#pragma unroll
            for (int a = 0; a < 6; ++a)
#pragma unroll
                for (int b = a; b < 6; ++b) { acc[j] = acc[j] + J[a] * J[b]; ++j; }
#pragma unroll
            for (int a = 0; a < 6; ++a) acc[21 + a] = acc[21 + a] + J[a] * r;
            acc[27] = acc[27] + r * r;
            acc[28] = acc[28] + 1.0;
        }
#pragma unroll
        for (int j = 0; j < NS; ++j)
            for (int off = 32; off > 0; off >>= 1) acc[j] = acc[j] + __shfl_xor(acc[j], off);
        if (lane == 0) {
#pragma unroll
            for (int j = 0; j < NS; ++j) chunks[chunk * ROW + j] = acc[j];
        }
        if constexpr (COLOR) {                                                  // the second sweep: the same pixels, their photometric pairs
#pragma unroll
            for (int j = 0; j < NS; ++j) acc[j] = 0.0;
            for (int64_t i = lane; i < count; i += 64) {
                double J[6], r;
                icp_seen seen;
                if (!icp_pixel<T, true>(f, qn, t, first + i, J, r, seen)) continue;
                if (!icp_color_pair(f, cio, seen, J, r)) continue;
                int j = 0;
#pragma unroll
                for (int a = 0; a < 6; ++a)
#pragma unroll
                    for (int b = a; b < 6; ++b) { acc[j] = acc[j] + J[a] * J[b]; ++j; }
#pragma unroll
                for (int a = 0; a < 6; ++a) acc[21 + a] = acc[21 + a] + J[a] * r;
                acc[27] = acc[27] + r * r;
                acc[28] = acc[28] + 1.0;
            }
#pragma unroll
            for (int j = 0; j < NS; ++j)
                for (int off = 32; off > 0; off >>= 1) acc[j] = acc[j] + __shfl_xor(acc[j], off);
            if (lane == 0) {
#pragma unroll
                for (int j = 0; j < NS; ++j) chunks[chunk * ROW + NS + j] = acc[j];
            }
        }
    }
}

// One block.  totals_out != NULL: the 29 totals go there and nothing else happens (f3d_icp_sums).  Otherwise one round of f3d_icp: the
// solve, the update of `pose` and row `round` of stats.  COLOR: 58 totals, the photometric system weighted into the solve, a stats row of 5.
template <bool COLOR> struct icp_solve_color {};
template <> struct icp_solve_color<true> { double weight; };

template <bool COLOR>
__global__ __launch_bounds__(F3D_BLOCK) void k_icp_solve(const double* __restrict__ chunks, int64_t nchunks, double* __restrict__ totals_out,
                                                          double* __restrict__ pose, int* __restrict__ lost, double min_pairs,
                                                          double* __restrict__ stats, int round, icp_solve_color<COLOR> col) {
    constexpr int NS = COLOR ? NSC : F3D_ICP_NSUMS;
    constexpr int NSTAT = COLOR ? 5 : 3;
    __shared__ double tot[NS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool was_lost = totals_out ? false : *lost != 0;
    if (!was_lost) {
        for (int j = wave; j < NS; j += F3D_BLOCK / 64) {
            const double s = f3d_wave_sum(nchunks, lane, [&](int64_t c) { return chunks[c * NS + j]; });
            if (lane == 0) tot[j] = s;
        }
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    if (totals_out) {
        for (int j = 0; j < NS; ++j) totals_out[j] = tot[j];
        return;
    }
    double* row = stats + NSTAT * (int64_t)round;
    if (was_lost) {
        row[0] = 0.0; row[1] = 0.0; row[2] = (double)F3D_ICP_LOST;
        if constexpr (COLOR) { row[3] = 0.0; row[4] = 0.0; }
        return;
    }
    row[0] = tot[28]; row[1] = tot[27];
    if constexpr (COLOR) { row[3] = tot[29 + 28]; row[4] = tot[29 + 27]; }
    bool ok = !(tot[28] < min_pairs);
    double A[6][6], L[6][6], b[6], y[6], x[6];
    {
        int j = 0;
        for (int a = 0; a < 6; ++a)
            for (int c = a; c < 6; ++c) {
                double e = tot[j];
                if constexpr (COLOR) e = e + col.weight * tot[29 + j];
                A[a][c] = e; A[c][a] = e; ++j;
            }
        for (int a = 0; a < 6; ++a) {
            if constexpr (COLOR) b[a] = -(tot[21 + a] + col.weight * tot[29 + 21 + a]);
            else b[a] = -tot[21 + a];
        }
    }
    double maxd = A[0][0];
    for (int a = 1; a < 6; ++a) if (A[a][a] > maxd) maxd = A[a][a];
    const double floor_ = F3D_ICP_PIVOT_EPS * maxd;
    for (int j = 0; j < 6 && ok; ++j) {
        double s = A[j][j];
        for (int k = 0; k < j; ++k) s = s - L[j][k] * L[j][k];
        if (!(fabs(s) < INFINITY && s > floor_)) { ok = false; break; }
        L[j][j] = sqrt(s);
        for (int i = j + 1; i < 6; ++i) {
            double e = A[i][j];
            for (int k = 0; k < j; ++k) e = e - L[i][k] * L[j][k];
            L[i][j] = e / L[j][j];
        }
    }
    if (!ok) { row[2] = (double)F3D_ICP_LOST; *lost = 1; return; }
    for (int i = 0; i < 6; ++i) {
        double s = b[i];
        for (int k = 0; k < i; ++k) s = s - L[i][k] * y[k];
        y[i] = s / L[i][i];
    }
    for (int i = 5; i >= 0; --i) {
        double s = y[i];
        for (int k = i + 1; k < 6; ++k) s = s - L[k][i] * x[k];
        x[i] = s / L[i][i];
    }
    double qn[4], qp[4];
    normalised(pose, qn);
    const double a0 = 1.0, a1 = x[0] / 2.0, a2 = x[1] / 2.0, a3 = x[2] / 2.0;
    qp[0] = ((a0 * qn[0] - a1 * qn[1]) - a2 * qn[2]) - a3 * qn[3];
    qp[1] = ((a0 * qn[1] + a1 * qn[0]) + a2 * qn[3]) - a3 * qn[2];
    qp[2] = ((a0 * qn[2] - a1 * qn[3]) + a2 * qn[0]) + a3 * qn[1];
    qp[3] = ((a0 * qn[3] + a1 * qn[2]) - a2 * qn[1]) + a3 * qn[0];
    normalised(qp, qn);
    pose[0] = qn[0]; pose[1] = qn[1]; pose[2] = qn[2]; pose[3] = qn[3];
    pose[4] = pose[4] + x[3]; pose[5] = pose[5] + x[4]; pose[6] = pose[6] + x[5];
    row[2] = (double)F3D_ICP_OK;
}

// ---- cloud to cloud: the nearest target of every source point and its terms, one kernel ---------------------------------------------
// the nearest target of p within the radius under (d2, caller-order index): j = that index or -1, at = its place in the sorted copy
__device__ __forceinline__ void cloud_nearest(const f3d_gridview& gv, const f3d_gridsearch& gs, double px, double py, double pz, int& j, int& at) {
    double best = INFINITY;
    int jb = 0x7fffffff, kb = 0;
    if (f3d_in_box(gs.reach, px, py, pz))
        f3d_grid_walk_d2(gv, gs.g, px, py, pz, gs.r2, [&](int k, double d) {
            if (d <= best) {                                                       // (a candidate farther than the minimum needs no index)
                const int jn = (int)gv.perm[k];
                if (d < best || jn < jb) { best = d; jb = jn; kb = k; }
            }
            return false;
        });
    j = jb == 0x7fffffff ? -1 : jb;
    at = kb;
}

// One wave per chunk of F3D_ICP_CHUNK source points, the lane order, butterfly and chunk row of k_icp_terms.  pairs (NULL = not wanted)
// receives the nearest target of every source point, also where the pair is then rejected for its normal.
template <typename T, int MODE>
__global__ __launch_bounds__(F3D_BLOCK) void k_cloud_icp_terms(const T* __restrict__ source, int64_t n, int64_t nchunks, const double* __restrict__ sorted,
                                                                const uint32_t* __restrict__ perm, const int2* __restrict__ cells, f3d_gridsearch gs,
                                                                const double* __restrict__ normals, const double* __restrict__ pose,
                                                                const int* __restrict__ lost, double* __restrict__ chunks, int32_t* __restrict__ pairs) {
    if (*lost) return;
    const f3d_gridview gv = {sorted, perm, cells};
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double qn[4];
    normalised(pose, qn);
    const double t[3] = {pose[4], pose[5], pose[6]};
    for (int64_t chunk = (int64_t)blockIdx.x * ICP_WAVES + wave; chunk < nchunks; chunk += (int64_t)gridDim.x * ICP_WAVES) {
        const int64_t first = chunk * F3D_ICP_CHUNK;
        const int64_t count = n - first < F3D_ICP_CHUNK ? n - first : (int64_t)F3D_ICP_CHUNK;
        double acc[NS];
#pragma unroll
        for (int j = 0; j < NS; ++j) acc[j] = 0.0;
        for (int64_t i = lane; i < count; i += 64) {
            const f3d_p3 pr = f3d_rotate(qn, f3d_load_p3(source, first + i));
            const double px = pr.x + t[0], py = pr.y + t[1], pz = pr.z + t[2];
            int j, at;
            cloud_nearest(gv, gs, px, py, pz, j, at);
            if (pairs) pairs[first + i] = j;
            if (j < 0) continue;                                                  // + 0.0 leaves an accumulator as it is (none is ever -0.0)
            const double e0 = px - sorted[3 * (int64_t)at], e1 = py - sorted[3 * (int64_t)at + 1], e2 = pz - sorted[3 * (int64_t)at + 2];
            if constexpr (MODE == F3D_CLOUD_ICP_PLANE) {
                const double N0 = normals[3 * (int64_t)j], N1 = normals[3 * (int64_t)j + 1], N2 = normals[3 * (int64_t)j + 2];
                if (!(fabs(N0) < INFINITY && fabs(N1) < INFINITY && fabs(N2) < INFINITY)) continue;
                const double r = f3d_dot3(N0, N1, N2, e0, e1, e2);
                const double J[6] = {pr.y * N2 - pr.z * N1, pr.z * N0 - pr.x * N2, pr.x * N1 - pr.y * N0, N0, N1, N2};
                int s = 0;
#pragma unroll
                for (int a = 0; a < 6; ++a)
#pragma unroll
                    for (int b = a; b < 6; ++b) { acc[s] = acc[s] + J[a] * J[b]; ++s; }
#pragma unroll
                for (int a = 0; a < 6; ++a) acc[21 + a] = acc[21 + a] + J[a] * r;
                acc[27] = acc[27] + r * r;
            } else {
                // N = the unit axis a, a = 0, 1, 2 in turn: J = (cross(pr, e_a), e_a) has the entries written here and zeros, r = e[a].
                // The products with a zero entry are +-0.0 and leave their accumulator as it is, so they are not formed.
                const double nx = -pr.x, ny = -pr.y, nz = -pr.z;
                // a = 0: J = (0, pr.z, -pr.y, 1, 0, 0)
                acc[6] = acc[6] + pr.z * pr.z; acc[7] = acc[7] + pr.z * ny; acc[8] = acc[8] + pr.z;
                acc[11] = acc[11] + ny * ny; acc[12] = acc[12] + ny; acc[15] = acc[15] + 1.0;
                acc[22] = acc[22] + pr.z * e0; acc[23] = acc[23] + ny * e0; acc[24] = acc[24] + e0;
                acc[27] = acc[27] + e0 * e0;
                // a = 1: J = (-pr.z, 0, pr.x, 0, 1, 0)
                acc[0] = acc[0] + nz * nz; acc[2] = acc[2] + nz * pr.x; acc[4] = acc[4] + nz;
                acc[11] = acc[11] + pr.x * pr.x; acc[13] = acc[13] + pr.x; acc[18] = acc[18] + 1.0;
                acc[21] = acc[21] + nz * e1; acc[23] = acc[23] + pr.x * e1; acc[25] = acc[25] + e1;
                acc[27] = acc[27] + e1 * e1;
                // a = 2: J = (pr.y, -pr.x, 0, 0, 0, 1)
                acc[0] = acc[0] + pr.y * pr.y; acc[1] = acc[1] + pr.y * nx; acc[5] = acc[5] + pr.y;
                acc[6] = acc[6] + nx * nx; acc[10] = acc[10] + nx; acc[20] = acc[20] + 1.0;
                acc[21] = acc[21] + pr.y * e2; acc[22] = acc[22] + nx * e2; acc[26] = acc[26] + e2;
                acc[27] = acc[27] + e2 * e2;
            }
            acc[28] = acc[28] + 1.0;
        }
#pragma unroll
        for (int j = 0; j < NS; ++j)
            for (int off = 32; off > 0; off >>= 1) acc[j] = acc[j] + __shfl_xor(acc[j], off);
        if (lane == 0) {
#pragma unroll
            for (int j = 0; j < NS; ++j) chunks[chunk * NS + j] = acc[j];
        }
    }
}

// ---- coarse-to-fine: one pyramid step of a depth frame and of model maps ------------------------------------------------------
// Output pixel (u, v) reads the input pixels (2v, 2u), (2v, 2u+1), (2v+1, 2u), (2v+1, 2u+1), in that order; an odd last row or column
// of the input is never read.
template <typename T>
__global__ __launch_bounds__(F3D_BLOCK) void k_depth_half(const T* __restrict__ depth, int w, int w2, int64_t n2, double depth_scale, double max_depth,
                                                           double gate, double* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * F3D_BLOCK + threadIdx.x; i < n2; i += (int64_t)gridDim.x * F3D_BLOCK) {
        const int64_t v = i / w2, u = i - v * w2;
        const int64_t top = 2 * v * w + 2 * u;
        const int64_t at[4] = {top, top + 1, top + w, top + w + 1};
        double d[4], dmin = 0.0;
        bool ok[4], any = false;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            d[k] = raw_depth<T>::at(depth, at[k]) / depth_scale;
            ok[k] = d[k] > 0.0 && d[k] <= max_depth;
            if (ok[k] && (!any || d[k] < dmin)) dmin = d[k];
            any = any || ok[k];
        }
        double sum = 0.0;
        int count = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (ok[k] && d[k] - dmin <= gate) { sum = sum + d[k]; ++count; }
        out[i] = count ? sum / (double)count : 0.0;
    }
}

// the intensity arguments of k_maps_half<true>; the instantiation without carries none
template <bool INTENSITY> struct maps_half_io {};
template <> struct maps_half_io<true> { const double* intensity; double* out; };

// two neighbouring map rows: 6 doubles, 48 contiguous bytes at p (the compiler fetches them with three 16-byte loads)
__device__ __forceinline__ void load_row_pair(const double* __restrict__ p, double a[3], double b[3]) {
    a[0] = p[0]; a[1] = p[1]; a[2] = p[2]; b[0] = p[3]; b[1] = p[4]; b[2] = p[5];
}

template <bool INTENSITY>
__global__ __launch_bounds__(F3D_BLOCK) void k_maps_half(const double* __restrict__ vertex, const double* __restrict__ normal, int wm, int w2, int64_t n2,
                                                          const f3d_view* __restrict__ view, double gate,
                                                          double* __restrict__ vertex_out, double* __restrict__ normal_out, maps_half_io<INTENSITY> io) {
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    const f3d_view& mv = *view;
    for (int64_t i = (int64_t)blockIdx.x * F3D_BLOCK + threadIdx.x; i < n2; i += (int64_t)gridDim.x * F3D_BLOCK) {
        const int64_t v = i / w2, u = i - v * w2;
        const int64_t top = 2 * v * wm + 2 * u, bot = top + wm;
        const int64_t at[4] = {top, top + 1, bot, bot + 1};
        double V[4][3], N[4][3];
        load_row_pair(vertex + 3 * top, V[0], V[1]);
        load_row_pair(vertex + 3 * bot, V[2], V[3]);
        load_row_pair(normal + 3 * top, N[0], N[1]);
        load_row_pair(normal + 3 * bot, N[2], N[3]);
        double z[4], zmin = 0.0;
        bool ok[4], any = false;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool finite = fabs(V[k][0]) < INFINITY && fabs(V[k][1]) < INFINITY && fabs(V[k][2]) < INFINITY && fabs(N[k][0]) < INFINITY &&
                                fabs(N[k][1]) < INFINITY && fabs(N[k][2]) < INFINITY;
            f3d_p3 p;
            p.x = V[k][0]; p.y = V[k][1]; p.z = V[k][2];
            z[k] = f3d_project_h(mv.K, mv.qinv, mv.t, p).z;
            ok[k] = finite && z[k] > 0.0;
            if (ok[k] && (!any || z[k] < zmin)) zmin = z[k];
            any = any || ok[k];
        }
        double S[3] = {0.0, 0.0, 0.0}, G[3] = {0.0, 0.0, 0.0}, si = 0.0;
        int count = 0, ci = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (!(ok[k] && z[k] - zmin <= gate)) continue;
#pragma unroll
            for (int a = 0; a < 3; ++a) { S[a] = S[a] + V[k][a]; G[a] = G[a] + N[k][a]; }
            ++count;
            if constexpr (INTENSITY) {
                const double I = io.intensity[at[k]];
                if (fabs(I) < INFINITY) { si = si + I; ++ci; }
            }
        }
        double Vo[3] = {nan, nan, nan}, No[3] = {nan, nan, nan};
        if (count) {
            const double len = sqrt((G[0] * G[0] + G[1] * G[1]) + G[2] * G[2]);
            if (len > 0.0 && len < INFINITY) {
#pragma unroll
                for (int a = 0; a < 3; ++a) { Vo[a] = S[a] / (double)count; No[a] = G[a] / len; }
            }
        }
        vertex_out[3 * i] = Vo[0]; vertex_out[3 * i + 1] = Vo[1]; vertex_out[3 * i + 2] = Vo[2];
        normal_out[3 * i] = No[0]; normal_out[3 * i + 1] = No[1]; normal_out[3 * i + 2] = No[2];
        if constexpr (INTENSITY) io.out[i] = ci ? si / (double)ci : nan;
    }
}

struct icp_scratch { size_t chunks, pose, lost, bytes; };

icp_scratch icp_layout(int64_t npixels, int row = NS) {
    f3d_carve c;
    icp_scratch l;
    l.chunks = c.take((size_t)((npixels + F3D_ICP_CHUNK - 1) / F3D_ICP_CHUNK) * row * sizeof(double));
    l.pose = c.take(7 * sizeof(double));
    l.lost = c.take(sizeof(int));
    l.bytes = c.off;
    return l;
}

icp_frame frame_of(const f3d_icp_args& a) {
    icp_frame f;
    f.depth = a.depth; f.h = a.h; f.w = a.w;
    f.fx = a.K[0]; f.cx = a.K[2]; f.fy = a.K[4]; f.cy = a.K[5];
    f.depth_scale = a.depth_scale; f.max_depth = a.max_depth;
    f.model_vertex = a.model_vertex; f.model_normal = a.model_normal; f.hm = a.hm; f.wm = a.wm;
    f.model_view = a.model_view;
    f.max_dist2 = a.max_dist * a.max_dist;
    return f;
}

template <bool COLOR>
void launch_terms(const f3d_icp_args& a, const double* pose, const int* lost, double* chunks, icp_color_io<COLOR> cio, hipStream_t s) {
    const icp_frame f = frame_of(a);
    const int64_t npix = (int64_t)a.h * a.w, nchunks = (npix + F3D_ICP_CHUNK - 1) / F3D_ICP_CHUNK;
    const dim3 gr(f3d_grid_for(nchunks, ICP_WAVES, F3D_GRID_CAP)), b(F3D_BLOCK);
    if (a.depth_type == F3D_DEPTH_U16) hipLaunchKernelGGL((k_icp_terms<uint16_t, COLOR>), gr, b, 0, s, f, pose, lost, npix, nchunks, chunks, cio);
    else if (a.depth_type == F3D_DEPTH_F32) hipLaunchKernelGGL((k_icp_terms<float, COLOR>), gr, b, 0, s, f, pose, lost, npix, nchunks, chunks, cio);
    else hipLaunchKernelGGL((k_icp_terms<double, COLOR>), gr, b, 0, s, f, pose, lost, npix, nchunks, chunks, cio);
}

icp_color_io<true> color_of(const f3d_icp_color_args& c) {
    icp_color_io<true> cio;
    cio.model_intensity = c.model_intensity; cio.rgb = c.rgb; cio.hc = c.hc; cio.wc = c.wc_img;
    return cio;
}

ray_volume volume_of(const float* tsdf, const float* weight, int nx, int ny, int nz, const double lo[3], double vs, float min_weight) {
    ray_volume g;
    g.tsdf = tsdf; g.weight = weight; g.nx = nx; g.ny = ny; g.nz = nz; g.vs = vs; g.min_weight = min_weight;
    for (int c = 0; c < 3; ++c) g.lo[c] = lo[c];
    return g;
}

ray_camera camera_of(const double K[9], const double qn[4], const double t[3]) {
    ray_camera cam;
    cam.fx = K[0]; cam.cx = K[2]; cam.fy = K[4]; cam.cy = K[5];
    for (int c = 0; c < 3; ++c) cam.t[c] = t[c];
    for (int c = 0; c < 4; ++c) cam.qn[c] = qn[c];
    return cam;
}

// blocks of a raycast launch: the usual cap, or the smaller one a test set
int ray_blocks(int h, int w, int grid_cap) {
    const int64_t ntiles = (int64_t)((w + 7) / 8) * ((h + 7) / 8);
    const int usual = F3D_GRID_CAP * 16;
    return f3d_grid_for(ntiles, F3D_BLOCK / 64, grid_cap > 0 && grid_cap < usual ? grid_cap : usual);
}

}  // namespace

size_t f3d_icp_scratch_bytes(int64_t npixels) { return icp_layout(npixels).bytes; }
size_t f3d_icp_color_scratch_bytes(int64_t npixels) { return icp_layout(npixels, NSC).bytes; }

hipError_t f3d_launch_tsdf_raycast(const float* tsdf, const float* weight, int nx, int ny, int nz, const double lo[3], double vs, float min_weight,
                                   const double K[9], const double qn[4], const double t[3], int h, int w, double near, double step, int nsteps,
                                   double* vertex, double* normal, double* depth, int grid_cap, hipStream_t s) {
    const ray_volume g = volume_of(tsdf, weight, nx, ny, nz, lo, vs, min_weight);
    const ray_camera cam = camera_of(K, qn, t);
    const dim3 gr(ray_blocks(h, w, grid_cap)), b(F3D_BLOCK);
    hipLaunchKernelGGL(k_tsdf_raycast<false>, gr, b, 0, s, g, cam, h, w, near, step, nsteps, vertex, normal, depth, ray_color_io<false>{});
    return hipGetLastError();
}

hipError_t f3d_launch_tsdf_raycast_color(const float* tsdf, const float* weight, const float* color, int nx, int ny, int nz, const double lo[3],
                                         double vs, float min_weight, const double K[9], const double qn[4], const double t[3], int h, int w,
                                         double near, double step, int nsteps, double* vertex, double* normal, double* depth, double* rgb,
                                         double* intensity, int grid_cap, hipStream_t s) {
    const ray_volume g = volume_of(tsdf, weight, nx, ny, nz, lo, vs, min_weight);
    const ray_camera cam = camera_of(K, qn, t);
    ray_color_io<true> cio;
    cio.color = (const float4*)color; cio.rgb = rgb; cio.intensity = intensity;
    const dim3 gr(ray_blocks(h, w, grid_cap)), b(F3D_BLOCK);
    hipLaunchKernelGGL(k_tsdf_raycast<true>, gr, b, 0, s, g, cam, h, w, near, step, nsteps, vertex, normal, depth, cio);
    return hipGetLastError();
}

hipError_t f3d_launch_icp_sums(const f3d_icp_args& a, const double q[4], const double t[3], void* scratch, double* sums, hipStream_t s) {
    const int64_t npix = (int64_t)a.h * a.w;
    const icp_scratch l = icp_layout(npix);
    char* base = (char*)scratch;
    double *chunks = (double*)(base + l.chunks), *pose = (double*)(base + l.pose);
    int* lost = (int*)(base + l.lost);
    hipLaunchKernelGGL(k_icp_init, dim3(1), dim3(64), 0, s, pose, lost, q[0], q[1], q[2], q[3], t[0], t[1], t[2]);
    launch_terms(a, pose, lost, chunks, icp_color_io<false>{}, s);
    hipLaunchKernelGGL(k_icp_solve<false>, dim3(1), dim3(F3D_BLOCK), 0, s, chunks, (npix + F3D_ICP_CHUNK - 1) / F3D_ICP_CHUNK, sums, pose, lost, 0.0,
                       (double*)nullptr, 0, icp_solve_color<false>{});
    return hipGetLastError();
}

hipError_t f3d_launch_icp(const f3d_icp_args& a, const double q[4], const double t[3], int iterations, int min_pairs, void* scratch,
                          double* pose_out, double* stats, int32_t* status, hipStream_t s) {
    const int64_t npix = (int64_t)a.h * a.w;
    const icp_scratch l = icp_layout(npix);
    char* base = (char*)scratch;
    double *chunks = (double*)(base + l.chunks), *pose = (double*)(base + l.pose);
    int* lost = (int*)(base + l.lost);
    hipLaunchKernelGGL(k_icp_init, dim3(1), dim3(64), 0, s, pose, lost, q[0], q[1], q[2], q[3], t[0], t[1], t[2]);
    for (int round = 0; round < iterations; ++round) {
        launch_terms(a, pose, lost, chunks, icp_color_io<false>{}, s);
        hipLaunchKernelGGL(k_icp_solve<false>, dim3(1), dim3(F3D_BLOCK), 0, s, chunks, (npix + F3D_ICP_CHUNK - 1) / F3D_ICP_CHUNK, (double*)nullptr, pose,
                           lost, (double)min_pairs, stats, round, icp_solve_color<false>{});
    }
    F3D_TRY(hipGetLastError());
    F3D_TRY(hipMemcpyAsync(pose_out, pose, 7 * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (status) F3D_TRY(hipMemcpyAsync(status, lost, sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    return hipSuccess;
}

hipError_t f3d_launch_icp_color_sums(const f3d_icp_args& a, const f3d_icp_color_args& c, const double q[4], const double t[3], void* scratch,
                                     double* sums, hipStream_t s) {
    const int64_t npix = (int64_t)a.h * a.w;
    const icp_scratch l = icp_layout(npix, NSC);
    char* base = (char*)scratch;
    double *chunks = (double*)(base + l.chunks), *pose = (double*)(base + l.pose);
    int* lost = (int*)(base + l.lost);
    icp_solve_color<true> col;
    col.weight = c.color_weight;
    hipLaunchKernelGGL(k_icp_init, dim3(1), dim3(64), 0, s, pose, lost, q[0], q[1], q[2], q[3], t[0], t[1], t[2]);
    launch_terms(a, pose, lost, chunks, color_of(c), s);
    hipLaunchKernelGGL(k_icp_solve<true>, dim3(1), dim3(F3D_BLOCK), 0, s, chunks, (npix + F3D_ICP_CHUNK - 1) / F3D_ICP_CHUNK, sums, pose, lost, 0.0,
                       (double*)nullptr, 0, col);
    return hipGetLastError();
}

hipError_t f3d_launch_icp_color(const f3d_icp_args& a, const f3d_icp_color_args& c, const double q[4], const double t[3], int iterations,
                                int min_pairs, void* scratch, double* pose_out, double* stats, int32_t* status, hipStream_t s) {
    const int64_t npix = (int64_t)a.h * a.w;
    const icp_scratch l = icp_layout(npix, NSC);
    char* base = (char*)scratch;
    double *chunks = (double*)(base + l.chunks), *pose = (double*)(base + l.pose);
    int* lost = (int*)(base + l.lost);
    icp_solve_color<true> col;
    col.weight = c.color_weight;
    hipLaunchKernelGGL(k_icp_init, dim3(1), dim3(64), 0, s, pose, lost, q[0], q[1], q[2], q[3], t[0], t[1], t[2]);
    for (int round = 0; round < iterations; ++round) {
        launch_terms(a, pose, lost, chunks, color_of(c), s);
        hipLaunchKernelGGL(k_icp_solve<true>, dim3(1), dim3(F3D_BLOCK), 0, s, chunks, (npix + F3D_ICP_CHUNK - 1) / F3D_ICP_CHUNK, (double*)nullptr, pose,
                           lost, (double)min_pairs, stats, round, col);
    }
    F3D_TRY(hipGetLastError());
    F3D_TRY(hipMemcpyAsync(pose_out, pose, 7 * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (status) F3D_TRY(hipMemcpyAsync(status, lost, sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    return hipSuccess;
}

hipError_t f3d_launch_depth_half(const void* depth, int depth_type, int h, int w, double depth_scale, double max_depth, double gate, double* out,
                                 hipStream_t s) {
    const int w2 = w / 2;
    const int64_t n2 = (int64_t)(h / 2) * w2;
    const dim3 gr(f3d_grid_for(n2, F3D_BLOCK, F3D_GRID_CAP)), b(F3D_BLOCK);
    if (depth_type == F3D_DEPTH_U16)
        hipLaunchKernelGGL(k_depth_half<uint16_t>, gr, b, 0, s, (const uint16_t*)depth, w, w2, n2, depth_scale, max_depth, gate, out);
    else if (depth_type == F3D_DEPTH_F32)
        hipLaunchKernelGGL(k_depth_half<float>, gr, b, 0, s, (const float*)depth, w, w2, n2, depth_scale, max_depth, gate, out);
    else
        hipLaunchKernelGGL(k_depth_half<double>, gr, b, 0, s, (const double*)depth, w, w2, n2, depth_scale, max_depth, gate, out);
    return hipGetLastError();
}

hipError_t f3d_launch_maps_half(const double* vertex, const double* normal, const double* intensity, int hm, int wm, const f3d_view* view, double gate,
                                double* vertex_out, double* normal_out, double* intensity_out, hipStream_t s) {
    const int w2 = wm / 2;
    const int64_t n2 = (int64_t)(hm / 2) * w2;
    const dim3 gr(f3d_grid_for(n2, F3D_BLOCK, F3D_GRID_CAP)), b(F3D_BLOCK);
    if (intensity) {
        maps_half_io<true> io;
        io.intensity = intensity; io.out = intensity_out;
        hipLaunchKernelGGL(k_maps_half<true>, gr, b, 0, s, vertex, normal, wm, w2, n2, view, gate, vertex_out, normal_out, io);
    } else {
        hipLaunchKernelGGL(k_maps_half<false>, gr, b, 0, s, vertex, normal, wm, w2, n2, view, gate, vertex_out, normal_out,
                           maps_half_io<false>{});
    }
    return hipGetLastError();
}

namespace {

// the scratch of a levelled call is that of its level with the most source pixels
int64_t most_pixels(const f3d_icp_level* levels, int nlevels) {
    int64_t most = 0;
    for (int k = 0; k < nlevels; ++k) {
        const int64_t npix = (int64_t)levels[k].h * levels[k].w;
        if (npix > most) most = npix;
    }
    return most;
}

// The rounds of f3d_launch_icp / f3d_launch_icp_color, level after level: one k_icp_init, then per round of every level the same two
// launches, the running round index as the stats row.  The pose and the lost flag stay where they are between the levels.
template <bool COLOR>
hipError_t launch_levels(const f3d_icp_level* levels, int nlevels, double max_depth, const double q[4], const double t[3], const uint8_t* rgb, int hc,
                         int wc_img, double color_weight, void* scratch, double* pose_out, double* stats, int32_t* status, hipStream_t s) {
    const icp_scratch lay = icp_layout(most_pixels(levels, nlevels), COLOR ? NSC : NS);
    char* base = (char*)scratch;
    double *chunks = (double*)(base + lay.chunks), *pose = (double*)(base + lay.pose);
    int* lost = (int*)(base + lay.lost);
    icp_solve_color<COLOR> col;
    if constexpr (COLOR) col.weight = color_weight;
    hipLaunchKernelGGL(k_icp_init, dim3(1), dim3(64), 0, s, pose, lost, q[0], q[1], q[2], q[3], t[0], t[1], t[2]);
    int round = 0;
    for (int k = 0; k < nlevels; ++k) {
        const f3d_icp_level& lv = levels[k];
        f3d_icp_args a;
        a.depth = lv.depth; a.depth_type = lv.depth_type; a.h = lv.h; a.w = lv.w; a.K = lv.K; a.depth_scale = lv.depth_scale; a.max_depth = max_depth;
        a.model_vertex = lv.model_vertex; a.model_normal = lv.model_normal; a.hm = lv.hm; a.wm = lv.wm; a.model_view = lv.model_view;
        a.max_dist = lv.max_dist;
        icp_color_io<COLOR> cio;
        if constexpr (COLOR) { cio.model_intensity = lv.model_intensity; cio.rgb = rgb; cio.hc = hc; cio.wc = wc_img; }
        const int64_t npix = (int64_t)lv.h * lv.w;
        for (int it = 0; it < lv.iterations; ++it, ++round) {
            launch_terms(a, pose, lost, chunks, cio, s);
            hipLaunchKernelGGL(k_icp_solve<COLOR>, dim3(1), dim3(F3D_BLOCK), 0, s, chunks, (npix + F3D_ICP_CHUNK - 1) / F3D_ICP_CHUNK, (double*)nullptr,
                               pose, lost, (double)lv.min_pairs, stats, round, col);
        }
    }
    F3D_TRY(hipGetLastError());
    F3D_TRY(hipMemcpyAsync(pose_out, pose, 7 * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (status) F3D_TRY(hipMemcpyAsync(status, lost, sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    return hipSuccess;
}

}  // namespace

hipError_t f3d_launch_icp_levels(const f3d_icp_level* levels, int nlevels, double max_depth, const double q[4], const double t[3], const uint8_t* rgb,
                                 int hc, int wc_img, double color_weight, void* scratch, double* pose_out, double* stats, int32_t* status,
                                 hipStream_t s) {
    if (rgb) return launch_levels<true>(levels, nlevels, max_depth, q, t, rgb, hc, wc_img, color_weight, scratch, pose_out, stats, status, s);
    return launch_levels<false>(levels, nlevels, max_depth, q, t, nullptr, 0, 0, 0.0, scratch, pose_out, stats, status, s);
}

namespace {

template <typename T>
void launch_cloud_terms_of(const f3d_cloud_icp_args& a, const double* pose, const int* lost, double* chunks, int32_t* pairs, hipStream_t s) {
    const int64_t nchunks = (a.n + F3D_ICP_CHUNK - 1) / F3D_ICP_CHUNK;
    const dim3 gr(f3d_grid_for(nchunks, ICP_WAVES, F3D_GRID_CAP)), b(F3D_BLOCK);
    if (a.mode == F3D_CLOUD_ICP_PLANE)
        hipLaunchKernelGGL((k_cloud_icp_terms<T, F3D_CLOUD_ICP_PLANE>), gr, b, 0, s, (const T*)a.source, a.n, nchunks, a.gv.sorted, a.gv.perm, a.gv.cells,
                           a.gs, a.normals, pose, lost, chunks, pairs);
    else
        hipLaunchKernelGGL((k_cloud_icp_terms<T, F3D_CLOUD_ICP_POINT>), gr, b, 0, s, (const T*)a.source, a.n, nchunks, a.gv.sorted, a.gv.perm, a.gv.cells,
                           a.gs, a.normals, pose, lost, chunks, pairs);
}

void launch_cloud_terms(const f3d_cloud_icp_args& a, const double* pose, const int* lost, double* chunks, int32_t* pairs, hipStream_t s) {
    if (a.source_dtype == F3D_F64) launch_cloud_terms_of<double>(a, pose, lost, chunks, pairs, s);
    else launch_cloud_terms_of<float>(a, pose, lost, chunks, pairs, s);
}

}  // namespace

hipError_t f3d_launch_cloud_icp_sums(const f3d_cloud_icp_args& a, const double q[4], const double t[3], void* scratch, double* sums, int32_t* pairs,
                                     hipStream_t s) {
    const icp_scratch l = icp_layout(a.n);
    char* base = (char*)scratch;
    double *chunks = (double*)(base + l.chunks), *pose = (double*)(base + l.pose);
    int* lost = (int*)(base + l.lost);
    hipLaunchKernelGGL(k_icp_init, dim3(1), dim3(64), 0, s, pose, lost, q[0], q[1], q[2], q[3], t[0], t[1], t[2]);
    launch_cloud_terms(a, pose, lost, chunks, pairs, s);
    hipLaunchKernelGGL(k_icp_solve<false>, dim3(1), dim3(F3D_BLOCK), 0, s, chunks, (a.n + F3D_ICP_CHUNK - 1) / F3D_ICP_CHUNK, sums, pose, lost, 0.0,
                       (double*)nullptr, 0, icp_solve_color<false>{});
    return hipGetLastError();
}

hipError_t f3d_launch_cloud_icp(const f3d_cloud_icp_args& a, const double q[4], const double t[3], int iterations, int min_pairs, void* scratch,
                                double* pose_out, double* stats, int32_t* status, hipStream_t s) {
    const icp_scratch l = icp_layout(a.n);
    char* base = (char*)scratch;
    double *chunks = (double*)(base + l.chunks), *pose = (double*)(base + l.pose);
    int* lost = (int*)(base + l.lost);
    hipLaunchKernelGGL(k_icp_init, dim3(1), dim3(64), 0, s, pose, lost, q[0], q[1], q[2], q[3], t[0], t[1], t[2]);
    for (int round = 0; round < iterations; ++round) {
        launch_cloud_terms(a, pose, lost, chunks, nullptr, s);
        hipLaunchKernelGGL(k_icp_solve<false>, dim3(1), dim3(F3D_BLOCK), 0, s, chunks, (a.n + F3D_ICP_CHUNK - 1) / F3D_ICP_CHUNK, (double*)nullptr, pose,
                           lost, (double)min_pairs, stats, round, icp_solve_color<false>{});
    }
    F3D_TRY(hipGetLastError());
    F3D_TRY(hipMemcpyAsync(pose_out, pose, 7 * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (status) F3D_TRY(hipMemcpyAsync(status, lost, sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    return hipSuccess;
}
