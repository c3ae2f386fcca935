// Running-mean colour growing of CVSegmentation.color_segment (reference segUtils/cv.py:92-142, 367-399).
//
// The seeds depend on each other through `ids` and the neutral mask, and the running mean of a flood is a serial chain,
// so one workgroup runs the whole seed list (no host round trip per seed or per level).  Per seed and level:
//   * the threads stage the colours of the level's queue in LDS;
//   * lane 0 runs the acceptance recurrence in queue order, in the colours' dtype, operation for operation as NumPy
//     evaluates it: |sma - clr| > threshold (compared in float64) rejects, else npts += 1, sma = sma + (clr - sma) / npts;
//   * the threads write the accepted points' ids, clear their neutral flags, and expand them: every unvisited neutral
//     neighbour keeps the minimum of (accepted position << 32 | row position) (atomicMin), and a block scan places the
//     children in that order, which is the reference's FIFO order (a child is enqueued by its first accepted discoverer).
// `inq` holds the epoch (seed index + 1) that enqueued a point, so nothing is cleared per seed; `best` is reset by the
// placement that consumes it.  Clearing the neutral flag of an accepted point at once is the reference's post-seed
// `neutral_mask[ids == seed_id] = False` for that point (it is already in the queue); the full pass over `ids` is needed
// only the first time the seed id is itself a neutral id (a neutral point always still carries an original neutral id).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "f3d.h"
#include "f3d_kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int CT = 1024;                 // threads of the one workgroup
constexpr int CHUNK = CT;                // queue entries staged in LDS per step of the serial lane
constexpr int IB = 256;

__global__ __launch_bounds__(IB) void k_color_init(const int64_t* __restrict__ ids, int64_t n, f3d_color_args a, uint8_t* __restrict__ neutral,
                                                   int32_t* __restrict__ inq, unsigned long long* __restrict__ best) {
    for (int64_t i = (int64_t)blockIdx.x * IB + threadIdx.x; i < n; i += (int64_t)gridDim.x * IB) {
        const int64_t v = ids[i];
        uint8_t f = 0;
        for (int k = 0; k < a.nneutral; ++k) f |= (uint8_t)(v == a.neutral[k]);
        neutral[i] = f;
        inq[i] = 0;
        best[i] = ~0ull;
    }
}

template <typename T>
__global__ __launch_bounds__(CT) void k_color_grow(const T* __restrict__ colors, int64_t n, const int64_t* __restrict__ offs,
                                                   const int32_t* __restrict__ nbrs, int64_t* ids, const int64_t* __restrict__ seeds,
                                                   int64_t nseeds, f3d_color_args a, uint8_t* neutral, int32_t* inq, unsigned long long* best,
                                                   int32_t* qa, int32_t* qb, int32_t* acc, int64_t* stats, int* err) {
    __shared__ T clr[CHUNK * 3];
    __shared__ int lds[CT];
    __shared__ int s_nq, s_na;
    __shared__ int64_t s_seed_id;
    __shared__ uint8_t s_done[F3D_COLOR_MAX_NEUTRAL];
    const int t = threadIdx.x;
    if (t < F3D_COLOR_MAX_NEUTRAL) s_done[t] = 0;
    int64_t accepted = 0;                                    // lane 0's count
    __syncthreads();
    for (int64_t k = 0; k < nseeds; ++k) {
        const int32_t epoch = (int32_t)(k + 1);
        const int64_t seed = seeds[k];
        if (seed < 0 || seed >= n) { if (t == 0) atomicOr(err, F3D_DEVERR_COLOR); return; }
        // lane 0 only: the running mean and the point count of this seed
        T sma0 = 0, sma1 = 0, sma2 = 0;
        int64_t npts = 0;
        if (t == 0) {
            s_seed_id = ids[seed];
            inq[seed] = epoch;
            qa[0] = (int32_t)seed;
            s_nq = 1;
            sma0 = colors[seed * 3]; sma1 = colors[seed * 3 + 1]; sma2 = colors[seed * 3 + 2];
        }
        __syncthreads();
        const int64_t seed_id = s_seed_id;
        int32_t *q = qa, *qn = qb;
        for (int level = 1; s_nq > 0 && level != a.max_level; ++level) {
            const int nq = s_nq;
            if (t == 0) s_na = 0;
            // acceptance, in queue order
            for (int c0 = 0; c0 < nq; c0 += CHUNK) {
                const int m = min(CHUNK, nq - c0);
                if (t < m) {
                    const int64_t v = q[c0 + t];
                    clr[t * 3] = colors[v * 3]; clr[t * 3 + 1] = colors[v * 3 + 1]; clr[t * 3 + 2] = colors[v * 3 + 2];
                }
                __syncthreads();
                if (t == 0) {
                    int na = s_na;
                    for (int i = 0; i < m; ++i) {
                        const T c0v = clr[i * 3], c1v = clr[i * 3 + 1], c2v = clr[i * 3 + 2];
                        const T d0 = sma0 - c0v, d1 = sma1 - c1v, d2 = sma2 - c2v;
                        if ((double)(d0 < 0 ? -d0 : d0) > a.thr[0] || (double)(d1 < 0 ? -d1 : d1) > a.thr[1] ||
                            (double)(d2 < 0 ? -d2 : d2) > a.thr[2])
                            continue;
                        npts += 1;
                        const T den = (T)npts;
                        sma0 = sma0 + (c0v - sma0) / den;
                        sma1 = sma1 + (c1v - sma1) / den;
                        sma2 = sma2 + (c2v - sma2) / den;
                        acc[na++] = q[c0 + i];
                    }
                    s_na = na;
                }
                __syncthreads();
            }
            const int na = s_na;
            for (int i = t; i < na; i += CT) {
                const int32_t v = acc[i];
                ids[v] = seed_id;
                neutral[v] = 0;
            }
            if (t == 0) accepted += na;
            if (level + 1 == a.max_level) { __syncthreads(); break; }      // children would be skipped unseen
            // expand: minimum (accepted position, row position) per unvisited neutral neighbour
            f3d_flood_expand<CT>(acc, na, offs, nbrs, n, best, err, F3D_DEVERR_COLOR,
                                 [&](int64_t j) { return inq[j] != epoch && neutral[j]; });
            __syncthreads();
            // place the children in (accepted position, row position) order
            const int carry = f3d_flood_place<CT>(acc, na, offs, nbrs, n, best, qn, lds, [&](int64_t j) { inq[j] = epoch; });
            if (t == 0) s_nq = carry;
            int32_t* tmp = q; q = qn; qn = tmp;
            __syncthreads();
        }
        // neutral_mask[ids == seed_id] = False: needed over the whole cloud only the first time seed_id is a neutral id
        int which = -1;
        for (int z = 0; z < a.nneutral; ++z) if (a.neutral[z] == seed_id) { which = z; break; }
        if (which >= 0 && !s_done[which]) {
            for (int64_t v = t; v < n; v += CT) if (ids[v] == seed_id) neutral[v] = 0;
            __syncthreads();
            if (t == 0) s_done[which] = 1;
        }
        __syncthreads();
    }
    if (t == 0) *stats += accepted;
}

struct color_layout { size_t neutral, inq, best, qa, qb, acc, total; };

color_layout color_layout_for(int64_t n) {
    const size_t n4 = (size_t)(n < 1 ? 1 : n) * 4;
    f3d_carve c;                                                         // (a braced list is evaluated left to right)
    return {c.take(n4 / 4), c.take(n4), c.take(n4 * 2), c.take(n4), c.take(n4), c.take(n4), c.off};
}

}  // namespace

size_t f3d_color_scratch_bytes(int64_t n) { return color_layout_for(n).total; }

hipError_t f3d_launch_color_segment(const void* colors, int dtype, int64_t n, const int64_t* offs, const int32_t* nbrs, int64_t* ids,
                                    const int64_t* seeds, int64_t nseeds, const f3d_color_args& a, void* scratch, int64_t* stats_dev, int* err,
                                    hipStream_t s) {
    if (n <= 0 || nseeds <= 0) return hipSuccess;
    if (n > 0x7fffffffLL || nseeds > 0x7ffffffeLL) return hipErrorInvalidValue;
    const color_layout L = color_layout_for(n);
    char* base = (char*)scratch;
    uint8_t* neutral = (uint8_t*)(base + L.neutral);
    int32_t *inq = (int32_t*)(base + L.inq), *qa = (int32_t*)(base + L.qa), *qb = (int32_t*)(base + L.qb), *acc = (int32_t*)(base + L.acc);
    unsigned long long* best = (unsigned long long*)(base + L.best);
    hipLaunchKernelGGL(k_color_init, dim3(f3d_grid_for(n, IB, 16384)), dim3(IB), 0, s, ids, n, a, neutral, inq, best);
    if (dtype == F3D_F64)
        hipLaunchKernelGGL(k_color_grow<double>, dim3(1), dim3(CT), 0, s, (const double*)colors, n, offs, nbrs, ids, seeds, nseeds, a, neutral,
                           inq, best, qa, qb, acc, stats_dev, err);
    else
        hipLaunchKernelGGL(k_color_grow<float>, dim3(1), dim3(CT), 0, s, (const float*)colors, n, offs, nbrs, ids, seeds, nseeds, a, neutral,
                           inq, best, qa, qb, acc, stats_dev, err);
    return hipGetLastError();
}
