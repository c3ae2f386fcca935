// smooth_votes / smooth_segment: neighbour-summed vote rows over a CSR adjacency (include/f3d.h has the contract,
// tests/smooth_ref.py restates it).
//
// One wave per destination point.  Lane l owns columns l, l + 64, l + 128, l + 192 of the row (ncols <= 256), so a neighbour's row
// is read by contiguous 512-B wave-loads (128-B for uint16 input) and a column's sum lives in one lane: its order is the row order
// by construction, there is nothing to reduce across lanes and nothing atomic.
// The wave takes 64 row entries at a time: a coalesced index load, the gates evaluated lane-parallel on those 64 neighbours'
// normals / colours, a ballot of the contributing entries.  It then walks the set bits in row order, four at a time, with
// wave-uniform neighbour indices (v_readlane): the loads of four rows are issued before the adds that consume them, and the adds
// stay in row order.  A missing row of the last group is loaded again from the group's first neighbour (in bounds, cached) and
// its add is skipped, never replaced by "+ 0.0": -0.0 + 0.0 would change a bit.
// The kernel is a template on the number of 64-column chunks, so every accumulator index is a compile-time constant after
// unrolling: no private array is indexed at run time.
//
// k_sm_check runs first: offsets ascending from >= 0, every entry in [0, n).  It sets F3D_DEVERR_SMOOTH, and under that bit every
// k_smooth launch returns at once: nothing is written and no row outside the matrix is read.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "f3d.h"
#include "f3d_kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int SB = 256;                    // 4 waves = 4 destinations in flight per block
constexpr int SWAVES = SB / 64;
constexpr int SGRID = 256 * 8 * 4;

__global__ __launch_bounds__(SB) void k_sm_check(int64_t n, const int64_t* __restrict__ offs, const int32_t* __restrict__ nbrs,
                                                  int* __restrict__ err) {
    const int64_t tid = (int64_t)blockIdx.x * SB + threadIdx.x, step = (int64_t)gridDim.x * SB;
    const int64_t lo = offs[0], hi = offs[n];
    bool bad = lo < 0;
    for (int64_t i = tid; i < n; i += step) bad |= offs[i + 1] < offs[i];          // then every row lies inside [lo, hi)
    if (lo >= 0) {
        for (int64_t e = lo + tid; e < hi; e += step) {
            const int64_t j = nbrs[e];
            bad |= (j < 0) | (j >= n);
        }
    }
    if (bad) atomicOr(err, F3D_DEVERR_SMOOTH);
}

// a neighbour's (or the point's own) colour, widened; ONE wave-uniform branch around the three loads
__device__ __forceinline__ void sm_color(const void* __restrict__ colors, int cdtype, size_t i, double& c0, double& c1, double& c2) {
    if (cdtype == F3D_F64) { const double* c = reinterpret_cast<const double*>(colors) + 3 * i; c0 = c[0]; c1 = c[1]; c2 = c[2]; }
    else { const float* c = reinterpret_cast<const float*>(colors) + 3 * i; c0 = (double)c[0]; c1 = (double)c[1]; c2 = (double)c[2]; }
}

// the value of column `col` of the wave's row (acc[k] of lane l = column l + 64 k), in every lane
template <int NCH>
__device__ __forceinline__ double sm_column(const double (&acc)[NCH], int col) {
    const int src = col & 63, ch = col >> 6;
    double x = __shfl(acc[0], src);
#pragma unroll
    for (int k = 1; k < NCH; ++k) { const double y = __shfl(acc[k], src); x = ch == k ? y : x; }
    return x;
}

// NCH = ceil(ncols / 64) chunks of 64 columns.  Every load of a row is unconditional: a lane past the end of the last chunk reads
// column ncols - 1 again (in bounds) into an accumulator nobody looks at, so no load sits behind a branch and a wait of its own.
template <typename VT, int NCH, bool NRM, bool COL, bool SEG>
__global__ __launch_bounds__(SB) void k_smooth(const VT* __restrict__ v, int64_t n, int ncols, const int64_t* __restrict__ offs,
                                               const int32_t* __restrict__ nbrs, f3d_smooth_gates g, double self_weight,
                                               double* __restrict__ out, f3d_smooth_seg sg, int64_t* __restrict__ classes,
                                               const int* __restrict__ err) {
    if (*err & F3D_DEVERR_SMOOTH) return;
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * SWAVES + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * SWAVES;
    constexpr int LAST = NCH - 1;
    const bool tail = lane + 64 * LAST < ncols;                               // the lane owns a column of the last chunk
    const int tailcol = tail ? lane + 64 * LAST : ncols - 1;
#define SM_LOAD(x, r)                                                              \
    double x[NCH];                                                                 \
    _Pragma("unroll") for (int k = 0; k < LAST; ++k) x[k] = (double)(r)[lane + 64 * k]; \
    x[LAST] = (double)(r)[tailcol]
    for (int64_t i = wave; i < n; i += nwaves) {
        const int self = (int)i;
        const VT* own = v + (size_t)i * ncols;
        SM_LOAD(acc, own);
#pragma unroll
        for (int k = 0; k < NCH; ++k) acc[k] = self_weight * acc[k];
        double ni0 = 0.0, ni1 = 0.0, ni2 = 0.0, ci0 = 0.0, ci1 = 0.0, ci2 = 0.0;
        if (NRM) { const double* q = g.normals + 3 * (size_t)i; ni0 = q[0]; ni1 = q[1]; ni2 = q[2]; }
        if (COL) sm_color(g.colors, g.cdtype, (size_t)i, ci0, ci1, ci2);
        const int64_t beg = offs[i], end = offs[i + 1];
        for (int64_t base = beg; base < end; base += 64) {
            const int64_t e = base + lane;
            const int je = nbrs[e < end ? e : end - 1];
            const int j = e < end ? je : self;                                 // (the point itself is never one of its others)
            bool ok = j != self;
            if (NRM) {
                const double* q = g.normals + 3 * (size_t)j;
                const double q0 = q[0], q1 = q[1], q2 = q[2];
                const double d = (ni0 * q0 + ni1 * q1) + ni2 * q2;
                ok = ok & (fabs(d) >= g.cos_angle);
            }
            if (COL) {
                double cj0, cj1, cj2;
                sm_color(g.colors, g.cdtype, (size_t)j, cj0, cj1, cj2);
                const double dr = cj0 - ci0, dg = cj1 - ci1, db = cj2 - ci2;
                ok = ok & ((dr * dr + dg * dg) + db * db <= g.lim2);
            }
            unsigned long long m = __ballot(ok);
            while (m) {
                const int cnt = __popcll(m);
                const int b0 = __builtin_ctzll(m);
                m &= m - 1;
                int b1 = b0, b2 = b0, b3 = b0;                                 // a missing row: the first one again, its add skipped
                if (cnt > 1) { b1 = __builtin_ctzll(m); m &= m - 1; }
                if (cnt > 2) { b2 = __builtin_ctzll(m); m &= m - 1; }
                if (cnt > 3) { b3 = __builtin_ctzll(m); m &= m - 1; }
                const VT* r0 = v + (size_t)__builtin_amdgcn_readlane(j, b0) * ncols;
                const VT* r1 = v + (size_t)__builtin_amdgcn_readlane(j, b1) * ncols;
                const VT* r2 = v + (size_t)__builtin_amdgcn_readlane(j, b2) * ncols;
                const VT* r3 = v + (size_t)__builtin_amdgcn_readlane(j, b3) * ncols;
                SM_LOAD(x0, r0);
                SM_LOAD(x1, r1);
                SM_LOAD(x2, r2);
                SM_LOAD(x3, r3);
#pragma unroll
                for (int k = 0; k < NCH; ++k) acc[k] += x0[k];
                if (cnt > 1) {
#pragma unroll
                    for (int k = 0; k < NCH; ++k) acc[k] += x1[k];
                }
                if (cnt > 2) {
#pragma unroll
                    for (int k = 0; k < NCH; ++k) acc[k] += x2[k];
                }
                if (cnt > 3) {
#pragma unroll
                    for (int k = 0; k < NCH; ++k) acc[k] += x3[k];
                }
            }
        }
        if (!SEG) {
            double* o = out + (size_t)i * ncols;
#pragma unroll
            for (int k = 0; k < LAST; ++k) o[lane + 64 * k] = acc[k];
            if (tail) o[lane + 64 * LAST] = acc[LAST];
        } else {
            // the rules of k_segment_votes on the wave's row.  total: each lane adds its columns to 0.0 in ascending order, the
            // lanes meet in an xor butterfly 32, 16, .., 1 (exact, so equal to any other order, for integer votes below 2^53)
            double total = 0.0, best = -INFINITY;
            int besti = 0x7fffffff;
#pragma unroll
            for (int k = 0; k < LAST; ++k) total += acc[k];
            if (tail) total += acc[LAST];
            if (sg.flt.nfilter == 0) {
                const int last = sg.lastcol ? ncols - 1 : -1;                  // lastcol: the last column is no candidate
#pragma unroll
                for (int k = 0; k < NCH; ++k) {
                    const int c = lane + 64 * k;
                    if ((k < LAST || tail) && acc[k] > best && c != last) { best = acc[k]; besti = c; }
                }
            } else {                                                           // votes[:, filter_classes]: position in the list is the index
                for (int k0 = 0; k0 < sg.flt.nfilter; k0 += 64) {
                    const int k = k0 + lane;
                    const bool act = k < sg.flt.nfilter;
                    const double x = sm_column<NCH>(acc, sg.flt.cls_dev[act ? k : 0]);
                    if (act && x > best) { best = x; besti = k; }
                }
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                total += __shfl_xor(total, off);
                const double ob = __shfl_xor(best, off);
                const int oi = __shfl_xor(besti, off);
                if (ob > best || (ob == best && oi < besti)) { best = ob; besti = oi; }
            }
            if (sg.lastcol) total = sm_column<NCH>(acc, ncols - 1);
            if (lane == 0) {
                int64_t cls = besti;
                if (!(total > 0.0)) cls = sg.nclasses;
                else if (best / total < sg.threshold) cls = sg.nclasses;
                if (best == 0.0) cls = sg.nclasses;
                if (sg.flt.nfilter > 0) {
                    int64_t q = cls;
                    for (int k = 0; k < sg.flt.nfilter; ++k) {                 // sequential, aliasing: voting.py:133-135
                        if (q == k) {
                            q = sg.flt.cls_dev[k];
                            if (sg.lastcol && (sg.neg.w[k >> 5] >> (k & 31) & 1u)) q -= ncols;
                        }
                    }
                    cls = q;
                }
                classes[i] = cls;
            }
        }
    }
#undef SM_LOAD
}

template <typename VT, int NCH, bool SEG>
void sm_launch_gates(dim3 gr, hipStream_t s, const void* v, int64_t n, int ncols, const int64_t* offs, const int32_t* nbrs,
                     const f3d_smooth_gates& g, double self_weight, double* out, const f3d_smooth_seg& sg, int64_t* classes, const int* err) {
    const dim3 b(SB);
    const VT* vt = reinterpret_cast<const VT*>(v);
#define SM_GO(N, C) hipLaunchKernelGGL((k_smooth<VT, NCH, N, C, SEG>), gr, b, 0, s, vt, n, ncols, offs, nbrs, g, self_weight, out, sg, classes, err)
    if (g.normals && g.colors) SM_GO(true, true);
    else if (g.normals) SM_GO(true, false);
    else if (g.colors) SM_GO(false, true);
    else SM_GO(false, false);
#undef SM_GO
}

template <typename VT, bool SEG>
void sm_launch(dim3 gr, hipStream_t s, const void* v, int64_t n, int ncols, const int64_t* offs, const int32_t* nbrs,
               const f3d_smooth_gates& g, double self_weight, double* out, const f3d_smooth_seg& sg, int64_t* classes, const int* err) {
    switch ((ncols + 63) / 64) {
    case 1: sm_launch_gates<VT, 1, SEG>(gr, s, v, n, ncols, offs, nbrs, g, self_weight, out, sg, classes, err); break;
    case 2: sm_launch_gates<VT, 2, SEG>(gr, s, v, n, ncols, offs, nbrs, g, self_weight, out, sg, classes, err); break;
    case 3: sm_launch_gates<VT, 3, SEG>(gr, s, v, n, ncols, offs, nbrs, g, self_weight, out, sg, classes, err); break;
    default: sm_launch_gates<VT, 4, SEG>(gr, s, v, n, ncols, offs, nbrs, g, self_weight, out, sg, classes, err); break;
    }
}

}  // namespace

hipError_t f3d_launch_smooth_check(int64_t n, const int64_t* offs, const int32_t* nbrs, int* err, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_sm_check, dim3(f3d_grid_for(n * 16, SB, SGRID)), dim3(SB), 0, s, n, offs, nbrs, err);
    return hipGetLastError();
}

hipError_t f3d_launch_smooth(const void* votes, int vtype, int64_t n, int ncols, const int64_t* offs, const int32_t* nbrs,
                             const f3d_smooth_gates& g, double self_weight, double* out, const f3d_smooth_seg* seg, int64_t* classes,
                             const int* err, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    const dim3 gr(f3d_grid_for(n, SWAVES, SGRID));
    const f3d_smooth_seg none = {};
    if (vtype == F3D_VOTES_U16) {
        if (seg) sm_launch<uint16_t, true>(gr, s, votes, n, ncols, offs, nbrs, g, self_weight, out, *seg, classes, err);
        else sm_launch<uint16_t, false>(gr, s, votes, n, ncols, offs, nbrs, g, self_weight, out, none, classes, err);
    } else {
        if (seg) sm_launch<double, true>(gr, s, votes, n, ncols, offs, nbrs, g, self_weight, out, *seg, classes, err);
        else sm_launch<double, false>(gr, s, votes, n, ncols, offs, nbrs, g, self_weight, out, none, classes, err);
    }
    return hipGetLastError();
}
