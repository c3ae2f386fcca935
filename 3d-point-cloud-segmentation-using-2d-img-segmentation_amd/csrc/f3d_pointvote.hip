// PointVotingSegmentation.vote (Fusion3DSeg/segUtils/voting.py:224-265): the radius search of every frame pixel in the cloud and the
// frame vote, fused -- no (pixel, point) pair is ever written to memory.
//
// Per frame the reference runs  nns = KDTree(cloud).query_radius(modPoints, r)  and then
//     votes[nns, repeat(mask, counts)] += 1 ;  votes[nns, -1] += 1
// with NumPy's buffered fancy-index rule: every DISTINCT cell gets +1 per frame however many pairs hit it.  So a frame adds 1 to
// (point, label) for every label that some pixel within r of the point carries, and 1 to (point, last column) if any pixel is
// within r.  A label equal to ncols - 1 lands on the last column as well, which then gets +2 from that frame.
//
//   k_pvote_prepass  : streams the masks and the queries once: is there a label >= ncols at all; first frame with a NaN / infinite
//                      coordinate (sklearn raises ValueError there)
//   k_pvote<.., true>: only when such a label exists: the first frame in which a pixel carrying one HAS a neighbour (NumPy raises
//                      IndexError there; np.repeat drops the labels of pixels that found nothing)
//   k_pvote<.., false>: the vote.  One thread per pixel searches the cloud's grid (f3d_launch_graph_grid, f3d_grid_walk) and feeds
//                      every hit into the frame's set of (point, label) keys.
// The set is a bitset per (frame of the group, point): bit 0 = "a pixel of the frame saw the point", bit 1 + l = label l.  A hit
// first reads its word (an L2 load; most hits are duplicates and end here), else one atomicOr sets the missing bits and its return
// value tells which of them this lane created: only the creator adds 1.0 to the vote cell.  The float64 atomic add is exact for
// these counts, so the result does not depend on the order of arrival.  `group` frames run per launch, each with a bitset of its
// own, cleared by one memset per launch; the bitsets depend on the cloud size and the column count only, never on the pair count.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "f3d.h"
#include "f3d_kernels.h"

namespace {

constexpr int PB = 256;

template <typename T>
__global__ __launch_bounds__(PB) void k_pvote_prepass(const T* __restrict__ q, const uint8_t* __restrict__ masks, int64_t total, int64_t hw,
                                                       int ncols, int* __restrict__ words) {
    bool label = false;
    int bad = F3D_PVOTE_NONE;
    for (int64_t i = (int64_t)blockIdx.x * PB + threadIdx.x; i < total; i += (int64_t)gridDim.x * PB) {
        label |= (int)masks[i] >= ncols;
        if (!f3d_finite((double)q[3 * i], (double)q[3 * i + 1], (double)q[3 * i + 2])) { const int f = (int)(i / hw); bad = f < bad ? f : bad; }
    }
    if (label) atomicOr(&words[0], 1);
    if (bad != F3D_PVOTE_NONE) atomicMin(&words[1], bad);
}

// frames [0, nframes) of the pointers given.  VALIDATE: words[2] = min(first frame with an out-of-range label on a pixel that has a
// neighbour).  Else: the vote of the frames before words[2]; frame f uses the bitset bits + (f % group) * m * wpp (the launcher
// passes one group at a time, so f < group).
template <typename T, bool VALIDATE>
__global__ __launch_bounds__(PB) void k_pvote(const T* __restrict__ q, const uint8_t* __restrict__ masks, int64_t total, int64_t hw, int frame0,
                                               int64_t m, int ncols, int wpp, const double* __restrict__ sorted,
                                               const uint32_t* __restrict__ perm, const int2* __restrict__ cells, f3d_gridsearch gs,
                                               double* __restrict__ votes, uint32_t* __restrict__ bits, int* __restrict__ words,
                                               const int* __restrict__ err) {
    // an earlier, untaken IndexError of this operation: nothing is written any more.  (The bit is set between launches only, by
    // k_pvote_flag: see the note in k_vote_uv2pt_batch.)
    if (!VALIDATE && (*err & F3D_DEVERR_PVOTE)) return;
    const int fb = VALIDATE ? F3D_PVOTE_NONE : words[2];
    const f3d_gridview gv = {sorted, perm, cells};
    for (int64_t i = (int64_t)blockIdx.x * PB + threadIdx.x; i < total; i += (int64_t)gridDim.x * PB) {
        const int f = (int)(i / hw);
        const int label = masks[i];
        if (VALIDATE) {
            if (label < ncols) continue;
            if (frame0 + f >= __hip_atomic_load(&words[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) continue;   // cannot lower it
        } else {
            if (frame0 + f >= fb) continue;                                    // the reference raised at frame fb: this one never ran
            if (label >= ncols) continue;                                      // (validated: such a pixel has no neighbour)
        }
        const double px = (double)q[3 * i], py = (double)q[3 * i + 1], pz = (double)q[3 * i + 2];
        if (!f3d_in_box(gs.reach, px, py, pz)) continue;
        uint32_t* fbits = VALIDATE ? nullptr : bits + (size_t)f * (size_t)m * wpp;
        const int lbit = label + 1;                                            // bit 0 of a point's first word: seen by this frame
        const uint32_t first = 1u | (lbit < 32 ? 1u << lbit : 0u);
        const bool found = f3d_grid_walk(gv, gs.g, px, py, pz, gs.r2, [&](int k) {
            if (VALIDATE) return true;
            const size_t j = perm[k];
            uint32_t* pw = fbits + j * wpp;
            double* row = votes + j * (size_t)ncols;
            const uint32_t have = __hip_atomic_load(pw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const uint32_t want = first & ~have;
            if (want) {
                const uint32_t made = want & ~atomicOr(pw, want);
                if (made & 1u) atomicAdd(row + (ncols - 1), 1.0);                  // votes[nns, -1] += 1
                if (made & ~1u) atomicAdd(row + label, 1.0);                       // votes[nns, label] += 1
            }
            if (lbit >= 32) {
                uint32_t* lw = pw + (lbit >> 5);
                const uint32_t b = 1u << (lbit & 31);
                if (!(__hip_atomic_load(lw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & b) && !(atomicOr(lw, b) & b))
                    atomicAdd(row + label, 1.0);
            }
            return false;
        });
        if (VALIDATE && found) atomicMin(&words[2], frame0 + f);
    }
}

__global__ void k_pvote_flag(const int* __restrict__ words, int limit, int* __restrict__ err) {
    if (words[2] < limit) atomicOr(err, F3D_DEVERR_PVOTE);
}

}  // namespace

// labels are bytes: bits 1 .. min(ncols, 256) + the "seen" bit
int f3d_pvote_words_per_point(int ncols) { return ((ncols < 256 ? ncols : 256) + 1 + 31) / 32; }

int f3d_pvote_group(int64_t m, int ncols) {
    const size_t per = (size_t)(m > 0 ? m : 1) * f3d_pvote_words_per_point(ncols) * 4;
    size_t gsz = F3D_PVOTE_BITS_BUDGET / per;
    if (gsz < 1) gsz = 1;
    if (gsz > F3D_PVOTE_MAX_GROUP) gsz = F3D_PVOTE_MAX_GROUP;
    return (int)gsz;
}

size_t f3d_pvote_bits_bytes(int64_t m, int ncols, int group) { return (size_t)group * (size_t)m * f3d_pvote_words_per_point(ncols) * 4; }

hipError_t f3d_launch_pvote_prepass(const void* queries, int qdtype, const uint8_t* masks, int64_t nframes, int64_t hw, int ncols, int* words,
                                    hipStream_t s) {
    hipError_t e = hipMemsetAsync(words, 0x7f, 16, s);                         // F3D_PVOTE_NONE everywhere ...
    if (e != hipSuccess) return e;
    if ((e = hipMemsetAsync(words, 0, 4, s)) != hipSuccess) return e;          // ... but the label flag
    const int64_t total = nframes * hw;
    const dim3 gr(f3d_grid_for(total, PB, F3D_GRID_CAP)), b(PB);
    if (qdtype == F3D_F64) hipLaunchKernelGGL(k_pvote_prepass<double>, gr, b, 0, s, (const double*)queries, masks, total, hw, ncols, words);
    else hipLaunchKernelGGL(k_pvote_prepass<float>, gr, b, 0, s, (const float*)queries, masks, total, hw, ncols, words);
    return hipGetLastError();
}

hipError_t f3d_launch_pvote_validate(const void* queries, int qdtype, const uint8_t* masks, int64_t nframes, int64_t hw, int ncols,
                                     const f3d_gridview& gv, const f3d_gridsearch& gs, int* words, hipStream_t s) {
    const int64_t total = nframes * hw;
    if (total <= 0) return hipSuccess;
    const dim3 gr(f3d_grid_for(total, PB, 1 << 20)), b(PB);
    if (qdtype == F3D_F64)
        hipLaunchKernelGGL((k_pvote<double, true>), gr, b, 0, s, (const double*)queries, masks, total, hw, 0, (int64_t)0, ncols, 0, gv.sorted, gv.perm,
                           gv.cells, gs, (double*)nullptr, (uint32_t*)nullptr, words, (const int*)nullptr);
    else
        hipLaunchKernelGGL((k_pvote<float, true>), gr, b, 0, s, (const float*)queries, masks, total, hw, 0, (int64_t)0, ncols, 0, gv.sorted, gv.perm,
                           gv.cells, gs, (double*)nullptr, (uint32_t*)nullptr, words, (const int*)nullptr);
    return hipGetLastError();
}

hipError_t f3d_launch_pvote_frames(const void* queries, int qdtype, const uint8_t* masks, int64_t nframes, int64_t hw, int64_t m, int ncols,
                                   const f3d_gridview& gv, const f3d_gridsearch& gs, double* votes, uint32_t* bits, int group,
                                   const int* words, const int* err, hipStream_t s) {
    const int wpp = f3d_pvote_words_per_point(ncols);
    const size_t qstride = (size_t)hw * 3 * (qdtype == F3D_F64 ? 8 : 4);
    for (int64_t f0 = 0; f0 < nframes; f0 += group) {
        const int64_t nf = nframes - f0 < group ? nframes - f0 : group;
        hipError_t e = hipMemsetAsync(bits, 0, f3d_pvote_bits_bytes(m, ncols, (int)nf), s);
        if (e != hipSuccess) return e;
        const int64_t total = nf * hw;
        const dim3 gr(f3d_grid_for(total, PB, 1 << 20)), b(PB);
        const char* qp = (const char*)queries + (size_t)f0 * qstride;
        const uint8_t* mp = masks + (size_t)f0 * hw;
        if (qdtype == F3D_F64)
            hipLaunchKernelGGL((k_pvote<double, false>), gr, b, 0, s, (const double*)qp, mp, total, hw, (int)f0, m, ncols, wpp, gv.sorted, gv.perm, gv.cells,
                               gs, votes, bits, const_cast<int*>(words), err);
        else
            hipLaunchKernelGGL((k_pvote<float, false>), gr, b, 0, s, (const float*)qp, mp, total, hw, (int)f0, m, ncols, wpp, gv.sorted, gv.perm, gv.cells,
                               gs, votes, bits, const_cast<int*>(words), err);
    }
    return hipGetLastError();
}

hipError_t f3d_launch_pvote_flag(const int* words, int limit, int* err, hipStream_t s) {
    hipLaunchKernelGGL(k_pvote_flag, dim3(1), dim3(1), 0, s, words, limit, err);
    return hipGetLastError();
}
