// TSDF reconstruction (include/f3d.h "TSDF reconstruction"): posed depth frames -> truncated signed distance volume -> triangle mesh
// by surface nets.  The contract there is restated operation for operation in tests/tsdf_ref.py; everything that decides a result is
// float64 without contraction, in the order written.
//
//   k_tsdf_integrate  one thread per voxel, a wavefront = 64 consecutive x of one (y, z) row (coalesced state loads and stores).  The
//                     frame loop is inside: the state is read once and written once.  The record of the frame being applied is
//                     wave-uniform (scalar loads).  The cull takes 64 frames at a time, one per lane: the two end voxels of the
//                     wave's run are projected with the view's M (9 products each), a ballot lists the frames to apply, in ascending
//                     order.  The homogeneous pixel is affine along the run, so when both ends lie beyond one of the five frustum
//                     bounds by more than a margin that dwarfs every rounding, every voxel of the run fails the same per-voxel rule
//                     and the wave skips the frame.  The bounds are evaluated on the homogeneous pixel (h2 <= 0, h0 < 0,
//                     h0 >= w h2, h1 < 0, h1 >= h h2, h2 > max_depth + trunc), i.e. for the depth frames' own w, h and max_depth:
//                     the planes stored in the view were built for the view's image size and far distance, which the per-voxel
//                     rules do not read.  COLOR = true (f3d_tsdf_integrate_color) adds step 7 to the same kernel: the voxel's
//                     (r, g, b, wc) is read lazily, one 16-byte load at its first in-band sample, and stored only if it was read.
//   vertex colours    k_tsdf_vert_colors, shaped like k_tsdf_verts, on the codes, active cells and ranks the count pass left.
//   extract           k_tsdf_code (observed / inside per voxel) -> k_tsdf_cells (active cells) -> scan -> k_tsdf_quads (quad mask
//                     per voxel) -> scan; then k_tsdf_verts and k_tsdf_tris.  The scan is the project's block scan over tiles of
//                     F3D_TSDF_SCAN_TILE counts: tile sums, a one-block scan of the sums, and the tiles again.  Totals are integer
//                     atomics (one per wave).  No float atomics, nothing depends on the launch shape.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "f3d.h"
#include "f3d_math.h"
#include "f3d_kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int TSDF_ROWS = F3D_BLOCK / 64;                 // (y, z) rows a block of the integrate kernel takes: one per wave
constexpr int SCAN_PER_THREAD = F3D_TSDF_SCAN_TILE / F3D_BLOCK;
constexpr uint8_t CODE_OBSERVED = 1, CODE_INSIDE = 2;

struct tsdf_grid { int nx, ny, nz; double lo[3]; double vs; };

template <typename T> struct depth_of;
template <> struct depth_of<double> { static __device__ __forceinline__ double at(const double* d, int64_t i) { return d[i]; } };
template <> struct depth_of<float> { static __device__ __forceinline__ double at(const float* d, int64_t i) { return (double)d[i]; } };
template <> struct depth_of<uint16_t> { static __device__ __forceinline__ double at(const uint16_t* d, int64_t i) { return (double)d[i]; } };

// true when every voxel of the run between the end voxels a and b fails the per-voxel rules of this frame (image fw x fh, depths up to
// zmax = max_depth + trunc).  NaN anywhere -> false (the voxels decide for themselves).
__device__ __forceinline__ bool run_outside(const f3d_view& vw, f3d_p3 a, f3d_p3 b, double fw, double fh, double zmax) {
    const double ax = a.x - vw.t[0], ay = a.y - vw.t[1], az = a.z - vw.t[2];
    const double bx = b.x - vw.t[0], by = b.y - vw.t[1], bz = b.z - vw.t[2];
    const double mag = fmax(fabs(ax) + fabs(ay) + fabs(az), fabs(bx) + fabs(by) + fabs(bz));
    // 1e-9 of the operand magnitudes: seven decimal orders above the rounding of either evaluation order
    const double e0 = 1e-9 * (vw.mnorm[0] * mag), e1 = 1e-9 * (vw.mnorm[1] * mag), e2 = 1e-9 * (vw.mnorm[2] * mag);
    const double a0 = (vw.M[0] * ax + vw.M[1] * ay) + vw.M[2] * az, b0 = (vw.M[0] * bx + vw.M[1] * by) + vw.M[2] * bz;
    const double a1 = (vw.M[3] * ax + vw.M[4] * ay) + vw.M[5] * az, b1 = (vw.M[3] * bx + vw.M[4] * by) + vw.M[5] * bz;
    const double a2 = (vw.M[6] * ax + vw.M[7] * ay) + vw.M[8] * az, b2 = (vw.M[6] * bx + vw.M[7] * by) + vw.M[8] * bz;
    const bool behind = a2 < -e2 && b2 < -e2;                                   // h2 > 0 fails
    const bool far = a2 > zmax + e2 && b2 > zmax + e2;                          // d <= max_depth and sdf >= -trunc cannot both hold
    // the four side bounds hold for h2 > 0 only; a run with an end behind the camera is left to the voxels
    const bool front = a2 > e2 && b2 > e2;
    const bool left = a0 < -e0 && b0 < -e0;                                     // x >= 0 fails
    const bool up = a1 < -e1 && b1 < -e1;                                       // y >= 0 fails
    const double r0 = e0 + fw * e2, r1 = e1 + fh * e2;
    const bool right = a0 - fw * a2 > r0 && b0 - fw * b2 > r0;                  // x < w fails
    const bool down = a1 - fh * a2 > r1 && b1 - fh * b2 > r1;                   // y < h fails
    return behind || far || (front && (left || up || right || down));
}

// the colour arguments of k_tsdf_integrate<T, true>: the state (r, g, b, wc) per voxel and the colour images [F, hc, wc, 3]; the
// depth-only instantiations carry none
template <bool COLOR> struct tsdf_color_io {};
template <> struct tsdf_color_io<true> { float4* color; const uint8_t* rgb; int hc, wc; };

template <typename T, bool COLOR>
__global__ __launch_bounds__(F3D_BLOCK) void k_tsdf_integrate(float* __restrict__ tsdf, float* __restrict__ weight, tsdf_grid g, double trunc,
                                                               double max_weight, const T* __restrict__ depth, int nframes, int h, int w,
                                                               double depth_scale, double max_depth, const f3d_view* __restrict__ views,
                                                               int64_t nrows, int xtiles, tsdf_color_io<COLOR> cio) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double fw = (double)w, fh = (double)h, zmax = max_depth + trunc;
    const int64_t hw = (int64_t)h * w;
    const int64_t ntiles = ((nrows + TSDF_ROWS - 1) / TSDF_ROWS) * xtiles;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t row = (tile / xtiles) * TSDF_ROWS + wave;                 // row = k * ny + j: wave-uniform
        if (row >= nrows) continue;
        const int i0 = (int)(tile % xtiles) * 64;
        const int i1 = min(i0 + 63, g.nx - 1);
        const int i = i0 + lane;
        const int k = (int)(row / g.ny), j = (int)(row - (int64_t)k * g.ny);
        const bool live = i < g.nx;
        const int64_t lin = row * g.nx + (live ? i : i1);
        f3d_p3 c, ca, cb;
        c.x = g.lo[0] + ((double)(live ? i : i1) + 0.5) * g.vs;
        c.y = g.lo[1] + ((double)j + 0.5) * g.vs;
        c.z = g.lo[2] + ((double)k + 0.5) * g.vs;
        ca = c; cb = c;
        ca.x = g.lo[0] + ((double)i0 + 0.5) * g.vs;
        cb.x = g.lo[0] + ((double)i1 + 0.5) * g.vs;
        float T_old = 0.f, w_old = 0.f;
        if (live) { T_old = tsdf[lin]; w_old = weight[lin]; }
        bool touched = false;
        // colour (step 7): the voxel's 16 bytes are read at its first in-band sample and written back only if there was one
        [[maybe_unused]] float4 C_old = make_float4(0.f, 0.f, 0.f, 0.f);
        [[maybe_unused]] bool c_read = false;
        for (int f0 = 0; f0 < nframes; f0 += 64) {
          // the cull of 64 frames at once, one per lane (ca, cb are wave-uniform); the survivors in ascending order
          unsigned long long todo = __ballot(f0 + lane < nframes && !run_outside(views[min(f0 + lane, nframes - 1)], ca, cb, fw, fh, zmax));
          while (todo) {
            const int f = f0 + __ffsll((long long)todo) - 1;                    // wave-uniform: the record comes through scalar loads
            todo &= todo - 1;
            const f3d_view& vw = views[f];
            const f3d_p3 hp = f3d_project_h(vw.K, vw.qinv, vw.t, c);
            if (!(hp.z > 0.0)) continue;
            const double x = hp.x / hp.z, y = hp.y / hp.z;
            if (!(x >= 0.0 && x < fw && y >= 0.0 && y < fh)) continue;
            const int u = (int)floor(x), v = (int)floor(y);
            const double d = depth_of<T>::at(depth, (int64_t)f * hw + (int64_t)v * w + u) / depth_scale;
            if (!(d > 0.0 && d <= max_depth)) continue;
            const double sdf = d - hp.z;
            if (sdf < -trunc) continue;
            double val = sdf / trunc;
            if constexpr (COLOR) {
                if (!(val > 1.0)) {
                    if (!c_read) { C_old = cio.color[lin]; c_read = true; }
                    const int64_t uc = (int64_t)u * cio.wc / w, vc = (int64_t)v * cio.hc / h;
                    const uint8_t* pix = cio.rgb + (((int64_t)f * cio.hc + vc) * cio.wc + uc) * 3;
                    const double wc_old = (double)C_old.w;
                    C_old.x = (float)(((double)C_old.x * wc_old + (double)pix[0]) / (wc_old + 1.0));
                    C_old.y = (float)(((double)C_old.y * wc_old + (double)pix[1]) / (wc_old + 1.0));
                    C_old.z = (float)(((double)C_old.z * wc_old + (double)pix[2]) / (wc_old + 1.0));
                    C_old.w = (float)fmin(wc_old + 1.0, max_weight);
                }
            }
            if (val > 1.0) val = 1.0;
            const double wo = (double)w_old;
            T_old = (float)(((double)T_old * wo + val) / (wo + 1.0));
            w_old = (float)fmin(wo + 1.0, max_weight);
            touched = true;
          }
        }
        if (live && touched) { tsdf[lin] = T_old; weight[lin] = w_old; }
        if constexpr (COLOR) { if (live && c_read) cio.color[lin] = C_old; }
    }
}

// ---- extract ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(F3D_BLOCK) void k_tsdf_code(const float* __restrict__ tsdf, const float* __restrict__ weight, int64_t n, float min_weight,
                                                          uint8_t* __restrict__ code) {
    for (int64_t i = (int64_t)blockIdx.x * F3D_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * F3D_BLOCK) {
        const bool obs = weight[i] >= min_weight;
        code[i] = (uint8_t)((obs ? CODE_OBSERVED : 0) | (obs && tsdf[i] < 0.f ? CODE_INSIDE : 0));
    }
}

__device__ __forceinline__ void wave_count(unsigned long long* counter, unsigned v) {
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(counter, (unsigned long long)v);
}

// (i, j, k) of lin = (k * ny + j) * nx + i; lin < 2^31, so the divisions are 32-bit
__device__ __forceinline__ void voxel_of(int64_t lin, int nx, int ny, int& i, int& j, int& k) {
    const uint32_t l = (uint32_t)lin, row = l / (uint32_t)nx;
    i = (int)(l - row * (uint32_t)nx);
    k = (int)(row / (uint32_t)ny);
    j = (int)(row - (uint32_t)k * (uint32_t)ny);
}

// cell lin = (k * ny + j) * nx + i is active iff it is a cell (every index <= n - 2), its 8 corners are observed and not all on one side
__global__ __launch_bounds__(F3D_BLOCK) void k_tsdf_cells(const uint8_t* __restrict__ code, int nx, int ny, int nz, int64_t n, uint8_t* __restrict__ act,
                                                           uint32_t* __restrict__ rank, unsigned long long* __restrict__ counts) {
    const int64_t sy = nx, sz = (int64_t)nx * ny;
    unsigned mine = 0;
    for (int64_t base = (int64_t)blockIdx.x * F3D_BLOCK; base < n; base += (int64_t)gridDim.x * F3D_BLOCK) {
        const int64_t lin = base + threadIdx.x;
        if (lin >= n) continue;
        int i, j, k;
        voxel_of(lin, nx, ny, i, j, k);
        bool a = false;
        if (i <= nx - 2 && j <= ny - 2 && k <= nz - 2) {
            unsigned all = CODE_OBSERVED, in = 0, nin = 0;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const unsigned v = code[lin + (c & 1) + ((c >> 1) & 1) * sy + (c >> 2) * sz];
                all &= v; in += (v >> 1) & 1; nin += 1;
            }
            a = all && in > 0 && in < nin;
        }
        act[lin] = a; rank[lin] = a; mine += a;
    }
    wave_count(counts, mine);
}

__device__ __forceinline__ int axis_n(int a, int nx, int ny, int nz) { return a == 0 ? nx : a == 1 ? ny : nz; }

// bit a of qmask[lin]: the grid edge p -> p + e_a carries a quad
__global__ __launch_bounds__(F3D_BLOCK) void k_tsdf_quads(const uint8_t* __restrict__ code, const uint8_t* __restrict__ act, int nx, int ny, int nz, int64_t n,
                                                           uint8_t* __restrict__ qmask, uint32_t* __restrict__ qoff, unsigned long long* __restrict__ counts) {
    const int64_t st[3] = {1, nx, (int64_t)nx * ny};
    unsigned mine = 0;
    for (int64_t base = (int64_t)blockIdx.x * F3D_BLOCK; base < n; base += (int64_t)gridDim.x * F3D_BLOCK) {
        const int64_t lin = base + threadIdx.x;
        if (lin >= n) continue;
        int p[3];
        voxel_of(lin, nx, ny, p[0], p[1], p[2]);
        const unsigned c0 = code[lin];
        unsigned m = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const int b = (a + 1) % 3, c = (a + 2) % 3;
            if (p[a] > axis_n(a, nx, ny, nz) - 2 || p[b] < 1 || p[b] > axis_n(b, nx, ny, nz) - 2 || p[c] < 1 || p[c] > axis_n(c, nx, ny, nz) - 2) continue;
            const unsigned c1 = code[lin + st[a]];
            if (!(c0 & c1 & CODE_OBSERVED) || !((c0 ^ c1) & CODE_INSIDE)) continue;
            if (act[lin - st[b] - st[c]] && act[lin - st[c]] && act[lin] && act[lin - st[b]]) m |= 1u << a;
        }
        qmask[lin] = (uint8_t)m; qoff[lin] = __popc(m); mine += __popc(m);
    }
    wave_count(counts + 1, mine);
}

// exclusive scan of uint32 counts in place, tile by tile: PASS 0 writes the tile sums, PASS 1 (after k_tsdf_scan_sums) the scanned tile
__device__ __forceinline__ void scan_tile(uint32_t* __restrict__ v, int64_t n, uint32_t* __restrict__ sums, int pass, uint32_t* lds) {
    const int64_t first = (int64_t)blockIdx.x * F3D_TSDF_SCAN_TILE + (int64_t)threadIdx.x * SCAN_PER_THREAD;
    uint32_t x[SCAN_PER_THREAD], s = 0;
#pragma unroll
    for (int e = 0; e < SCAN_PER_THREAD; ++e) { x[e] = first + e < n ? v[first + e] : 0; s += x[e]; }
    uint32_t ex, tot;
    f3d_block_scan<F3D_BLOCK>(s, lds, ex, tot);
    if (pass == 0) { if (threadIdx.x == 0) sums[blockIdx.x] = tot; return; }
    uint32_t run = sums[blockIdx.x] + ex;
#pragma unroll
    for (int e = 0; e < SCAN_PER_THREAD; ++e) { if (first + e < n) v[first + e] = run; run += x[e]; }
}

__global__ __launch_bounds__(F3D_BLOCK) void k_tsdf_scan(uint32_t* __restrict__ v, int64_t n, uint32_t* __restrict__ sums, int pass) {
    __shared__ uint32_t lds[F3D_BLOCK];
    scan_tile(v, n, sums, pass, lds);
}

// one block: exclusive scan of the tile sums in place, F3D_BLOCK at a time with a carry
__global__ __launch_bounds__(F3D_BLOCK) void k_tsdf_scan_sums(uint32_t* __restrict__ sums, int64_t ntiles) {
    __shared__ uint32_t lds[F3D_BLOCK];
    uint32_t carry = 0;
    for (int64_t b = 0; b < ntiles; b += F3D_BLOCK) {
        const int64_t i = b + threadIdx.x;
        const uint32_t v = i < ntiles ? sums[i] : 0;
        uint32_t ex, tot;
        f3d_block_scan<F3D_BLOCK>(v, lds, ex, tot);
        if (i < ntiles) sums[i] = carry + ex;
        carry += tot;
    }
}

// vertex of every active cell: the mean of its edges' crossing points, edges in ascending e = 4 a + 2 oc + ob
__global__ __launch_bounds__(F3D_BLOCK) void k_tsdf_verts(const float* __restrict__ tsdf, const uint8_t* __restrict__ code, const uint8_t* __restrict__ act,
                                                           const uint32_t* __restrict__ rank, tsdf_grid g, int64_t n, double* __restrict__ verts) {
    const int64_t st[3] = {1, g.nx, (int64_t)g.nx * g.ny};
    for (int64_t lin = (int64_t)blockIdx.x * F3D_BLOCK + threadIdx.x; lin < n; lin += (int64_t)gridDim.x * F3D_BLOCK) {
        if (!act[lin]) continue;
        int cell[3];
        voxel_of(lin, g.nx, g.ny, cell[0], cell[1], cell[2]);
        double sum[3] = {0.0, 0.0, 0.0};
        int count = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const int b = (a + 1) % 3, c = (a + 2) % 3;
#pragma unroll
            for (int o = 0; o < 4; ++o) {
                const int ob = o & 1, oc = o >> 1;
                const int64_t at0 = lin + ob * st[b] + oc * st[c], at1 = at0 + st[a];
                if (!((code[at0] ^ code[at1]) & CODE_INSIDE)) continue;
                const double s0 = (double)tsdf[at0], s1 = (double)tsdf[at1];
                double L[3];
                L[a] = s0 / (s0 - s1); L[b] = (double)ob; L[c] = (double)oc;
                sum[0] = sum[0] + L[0]; sum[1] = sum[1] + L[1]; sum[2] = sum[2] + L[2];
                ++count;
            }
        }
        double* out = verts + 3 * (int64_t)rank[lin];
#pragma unroll
        for (int a = 0; a < 3; ++a) out[a] = g.lo[a] + (((double)cell[a] + 0.5) + sum[a] / (double)count) * g.vs;
    }
}

// colour of every active cell's vertex: the mean over its crossing edges (ascending e, L[a] as in k_tsdf_verts) of the colour at the
// crossing, taken from the ends that have one (wc > 0): both -> interpolated, one -> that end's, neither -> the edge adds nothing
__global__ __launch_bounds__(F3D_BLOCK) void k_tsdf_vert_colors(const float* __restrict__ tsdf, const float4* __restrict__ color,
                                                                 const uint8_t* __restrict__ code, const uint8_t* __restrict__ act,
                                                                 const uint32_t* __restrict__ rank, int nx, int ny, int64_t n,
                                                                 uint8_t* __restrict__ rgb, uint8_t* __restrict__ colored) {
    const int64_t st[3] = {1, nx, (int64_t)nx * ny};
    for (int64_t lin = (int64_t)blockIdx.x * F3D_BLOCK + threadIdx.x; lin < n; lin += (int64_t)gridDim.x * F3D_BLOCK) {
        if (!act[lin]) continue;
        double sum[3] = {0.0, 0.0, 0.0};
        int count = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const int b = (a + 1) % 3, c = (a + 2) % 3;
#pragma unroll
            for (int o = 0; o < 4; ++o) {
                const int ob = o & 1, oc = o >> 1;
                const int64_t at0 = lin + ob * st[b] + oc * st[c], at1 = at0 + st[a];
                if (!((code[at0] ^ code[at1]) & CODE_INSIDE)) continue;
                const float4 c0 = color[at0], c1 = color[at1];
                const bool has0 = c0.w > 0.f, has1 = c1.w > 0.f;
                if (!has0 && !has1) continue;
                double col[3];
                if (has0 && has1) {
                    const double s0 = (double)tsdf[at0], s1 = (double)tsdf[at1];
                    const double L = s0 / (s0 - s1);
                    col[0] = (double)c0.x + L * ((double)c1.x - (double)c0.x);
                    col[1] = (double)c0.y + L * ((double)c1.y - (double)c0.y);
                    col[2] = (double)c0.z + L * ((double)c1.z - (double)c0.z);
                } else {
                    const float4 e = has0 ? c0 : c1;
                    col[0] = (double)e.x; col[1] = (double)e.y; col[2] = (double)e.z;
                }
                sum[0] = sum[0] + col[0]; sum[1] = sum[1] + col[1]; sum[2] = sum[2] + col[2];
                ++count;
            }
        }
        const int64_t id = rank[lin];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            double m = count ? sum[ch] / (double)count : 0.0;
            m = m > 0.0 ? m : 0.0;                                              // NaN -> 0
            m = m < 255.0 ? m : 255.0;
            rgb[3 * id + ch] = (uint8_t)floor(m + 0.5);
        }
        if (colored) colored[id] = count > 0;
    }
}

__global__ __launch_bounds__(F3D_BLOCK) void k_tsdf_tris(const uint8_t* __restrict__ code, const uint8_t* __restrict__ qmask, const uint32_t* __restrict__ qoff,
                                                          const uint32_t* __restrict__ rank, int nx, int ny, int64_t n, int32_t* __restrict__ tris) {
    const int64_t st[3] = {1, nx, (int64_t)nx * ny};
    for (int64_t lin = (int64_t)blockIdx.x * F3D_BLOCK + threadIdx.x; lin < n; lin += (int64_t)gridDim.x * F3D_BLOCK) {
        const unsigned m = qmask[lin];
        if (!m) continue;
        const bool inside = code[lin] & CODE_INSIDE;
        int64_t q = qoff[lin];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (!(m >> a & 1)) continue;
            const int b = (a + 1) % 3, c = (a + 2) % 3;
            const int32_t A = (int32_t)rank[lin - st[b] - st[c]], B = (int32_t)rank[lin - st[c]], C = (int32_t)rank[lin], D = (int32_t)rank[lin - st[b]];
            const int32_t q1 = inside ? B : D, q3 = inside ? D : B;
            int32_t* t = tris + 6 * q;
            t[0] = A; t[1] = q1; t[2] = C;
            t[3] = A; t[4] = C; t[5] = q3;
            ++q;
        }
    }
}

struct tsdf_scratch { size_t counts, code, act, qmask, rank, qoff, sums, bytes; };

tsdf_scratch tsdf_layout(int64_t n) {
    f3d_carve c;
    tsdf_scratch l;
    l.counts = c.take(2 * sizeof(unsigned long long));
    l.code = c.take((size_t)n); l.act = c.take((size_t)n); l.qmask = c.take((size_t)n);
    l.rank = c.take((size_t)n * 4); l.qoff = c.take((size_t)n * 4);
    l.sums = c.take((size_t)((n + F3D_TSDF_SCAN_TILE - 1) / F3D_TSDF_SCAN_TILE) * 4);
    l.bytes = c.off;
    return l;
}

void scan_in_place(uint32_t* v, int64_t n, uint32_t* sums, hipStream_t s) {
    const int64_t ntiles = (n + F3D_TSDF_SCAN_TILE - 1) / F3D_TSDF_SCAN_TILE;
    hipLaunchKernelGGL(k_tsdf_scan, dim3((unsigned)ntiles), dim3(F3D_BLOCK), 0, s, v, n, sums, 0);
    hipLaunchKernelGGL(k_tsdf_scan_sums, dim3(1), dim3(F3D_BLOCK), 0, s, sums, ntiles);
    hipLaunchKernelGGL(k_tsdf_scan, dim3((unsigned)ntiles), dim3(F3D_BLOCK), 0, s, v, n, sums, 1);
}

// blocks of a launch: the usual cap, or the smaller one a test set (f3d_debug_tsdf_grid_cap; 0 = none); f3d_grid_for then applies the
// process-wide f3d_debug_grid_cap as well, so the smaller of the two holds
int capped(int64_t blocks, int64_t usual, int grid_cap) {
    const int64_t cap = grid_cap > 0 && grid_cap < usual ? grid_cap : usual;
    return f3d_grid_for(blocks, 1, (int)cap);
}

tsdf_grid grid_of(int nx, int ny, int nz, const double lo[3], double vs) {
    tsdf_grid g;
    g.nx = nx; g.ny = ny; g.nz = nz; g.vs = vs;
    for (int c = 0; c < 3; ++c) g.lo[c] = lo ? lo[c] : 0.0;
    return g;
}

template <bool COLOR>
hipError_t launch_integrate(float* tsdf, float* weight, int nx, int ny, int nz, const double lo[3], double vs, double trunc, double max_weight,
                            const void* depth, int depth_type, int nframes, int h, int w, double depth_scale, double max_depth,
                            const f3d_view* views_dev, tsdf_color_io<COLOR> cio, int grid_cap, hipStream_t s) {
    const tsdf_grid g = grid_of(nx, ny, nz, lo, vs);
    const int64_t nrows = (int64_t)ny * nz;
    const int xtiles = (nx + 63) / 64;
    const int64_t ntiles = ((nrows + TSDF_ROWS - 1) / TSDF_ROWS) * xtiles;
    const dim3 gr(capped(ntiles, (int64_t)F3D_GRID_CAP * 16, grid_cap)), b(F3D_BLOCK);
    if (depth_type == F3D_DEPTH_U16)
        hipLaunchKernelGGL((k_tsdf_integrate<uint16_t, COLOR>), gr, b, 0, s, tsdf, weight, g, trunc, max_weight, (const uint16_t*)depth, nframes, h, w,
                           depth_scale, max_depth, views_dev, nrows, xtiles, cio);
    else if (depth_type == F3D_DEPTH_F32)
        hipLaunchKernelGGL((k_tsdf_integrate<float, COLOR>), gr, b, 0, s, tsdf, weight, g, trunc, max_weight, (const float*)depth, nframes, h, w,
                           depth_scale, max_depth, views_dev, nrows, xtiles, cio);
    else
        hipLaunchKernelGGL((k_tsdf_integrate<double, COLOR>), gr, b, 0, s, tsdf, weight, g, trunc, max_weight, (const double*)depth, nframes, h, w,
                           depth_scale, max_depth, views_dev, nrows, xtiles, cio);
    return hipGetLastError();
}

}  // namespace

size_t f3d_tsdf_scratch_bytes(int64_t nvoxels) { return tsdf_layout(nvoxels).bytes; }

hipError_t f3d_launch_tsdf_integrate(float* tsdf, float* weight, int nx, int ny, int nz, const double lo[3], double vs, double trunc, double max_weight,
                                     const void* depth, int depth_type, int nframes, int h, int w, double depth_scale, double max_depth,
                                     const f3d_view* views_dev, int grid_cap, hipStream_t s) {
    return launch_integrate<false>(tsdf, weight, nx, ny, nz, lo, vs, trunc, max_weight, depth, depth_type, nframes, h, w, depth_scale, max_depth,
                                   views_dev, tsdf_color_io<false>{}, grid_cap, s);
}

hipError_t f3d_launch_tsdf_integrate_color(float* tsdf, float* weight, float* color, int nx, int ny, int nz, const double lo[3], double vs, double trunc,
                                           double max_weight, const void* depth, int depth_type, const uint8_t* rgb, int nframes, int h, int w,
                                           int hc, int wc, double depth_scale, double max_depth, const f3d_view* views_dev, int grid_cap,
                                           hipStream_t s) {
    const tsdf_color_io<true> cio = {(float4*)color, rgb, hc, wc};
    return launch_integrate<true>(tsdf, weight, nx, ny, nz, lo, vs, trunc, max_weight, depth, depth_type, nframes, h, w, depth_scale, max_depth,
                                  views_dev, cio, grid_cap, s);
}

hipError_t f3d_launch_tsdf_count(const float* tsdf, const float* weight, int nx, int ny, int nz, float min_weight, void* scratch,
                                 unsigned long long* counts_host, int grid_cap, hipStream_t s) {
    const int64_t n = (int64_t)nx * ny * nz;
    const tsdf_scratch l = tsdf_layout(n);
    char* base = (char*)scratch;
    unsigned long long* counts = (unsigned long long*)(base + l.counts);
    uint8_t *code = (uint8_t*)(base + l.code), *act = (uint8_t*)(base + l.act), *qmask = (uint8_t*)(base + l.qmask);
    uint32_t *rank = (uint32_t*)(base + l.rank), *qoff = (uint32_t*)(base + l.qoff), *sums = (uint32_t*)(base + l.sums);
    F3D_TRY(hipMemsetAsync(counts, 0, 2 * sizeof(unsigned long long), s));
    const dim3 gr(capped((n + F3D_BLOCK - 1) / F3D_BLOCK, F3D_GRID_CAP * 4, grid_cap)), b(F3D_BLOCK);
    hipLaunchKernelGGL(k_tsdf_code, gr, b, 0, s, tsdf, weight, n, min_weight, code);
    hipLaunchKernelGGL(k_tsdf_cells, gr, b, 0, s, code, nx, ny, nz, n, act, rank, counts);
    scan_in_place(rank, n, sums, s);
    hipLaunchKernelGGL(k_tsdf_quads, gr, b, 0, s, code, act, nx, ny, nz, n, qmask, qoff, counts);
    scan_in_place(qoff, n, sums, s);
    F3D_TRY(hipGetLastError());
    return hipMemcpyAsync(counts_host, counts, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s);   // the caller synchronises
}

hipError_t f3d_launch_tsdf_fill(const float* tsdf, int nx, int ny, int nz, const double lo[3], double vs, const void* scratch, double* verts,
                                int32_t* tris, int grid_cap, hipStream_t s) {
    const int64_t n = (int64_t)nx * ny * nz;
    const tsdf_scratch l = tsdf_layout(n);
    const char* base = (const char*)scratch;
    const uint8_t *code = (const uint8_t*)(base + l.code), *act = (const uint8_t*)(base + l.act), *qmask = (const uint8_t*)(base + l.qmask);
    const uint32_t *rank = (const uint32_t*)(base + l.rank), *qoff = (const uint32_t*)(base + l.qoff);
    const dim3 gr(capped((n + F3D_BLOCK - 1) / F3D_BLOCK, F3D_GRID_CAP * 4, grid_cap)), b(F3D_BLOCK);
    if (verts) hipLaunchKernelGGL(k_tsdf_verts, gr, b, 0, s, tsdf, code, act, rank, grid_of(nx, ny, nz, lo, vs), n, verts);
    if (tris) hipLaunchKernelGGL(k_tsdf_tris, gr, b, 0, s, code, qmask, qoff, rank, nx, ny, n, tris);
    return hipGetLastError();
}

hipError_t f3d_launch_tsdf_vert_colors(const float* tsdf, const float* color, int nx, int ny, int nz, const void* scratch, uint8_t* rgb,
                                       uint8_t* colored, int grid_cap, hipStream_t s) {
    const int64_t n = (int64_t)nx * ny * nz;
    const tsdf_scratch l = tsdf_layout(n);
    const char* base = (const char*)scratch;
    const uint8_t *code = (const uint8_t*)(base + l.code), *act = (const uint8_t*)(base + l.act);
    const uint32_t* rank = (const uint32_t*)(base + l.rank);
    const dim3 gr(capped((n + F3D_BLOCK - 1) / F3D_BLOCK, F3D_GRID_CAP * 4, grid_cap)), b(F3D_BLOCK);
    hipLaunchKernelGGL(k_tsdf_vert_colors, gr, b, 0, s, tsdf, (const float4*)color, code, act, rank, nx, ny, n, rgb, colored);
    return hipGetLastError();
}
