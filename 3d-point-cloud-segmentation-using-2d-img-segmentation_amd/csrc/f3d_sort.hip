// Cell sort of a point cloud: order the points by coarse grid cell (HBM-bound, key-index radix sort, all kernels our own).
//
// Why it exists: the fused kernel assigns 128 consecutive points to a wavefront.  When consecutive
// points are spatial neighbours, a wave is (almost always) entirely inside or entirely outside a
// view's frustum, so the expensive projection runs only for waves that have visible points.  A
// cloud in arbitrary order wastes ~60 % of the projection work on masked-off lanes.  Sorting changes
// nothing in the results: every point's label depends on its own xyz only, and the kernel writes it
// back to the caller's index through `perm`.
//
//   k_bbox_partial : finite bounding box of a strided sample of the cloud, <= 64 partial boxes (the cell grid -- 16 key bits dealt to
//                    the axes -- is derived from them by the first wave of every k_rs_keys block)
//   k_rs_keys      : ONE read of xyz: key[i] = 16-bit Morton code of point i's cell (2 B/point written) and, per 8192-point
//                    tile, the histogram of the keys' low bytes                                                  (streaming)
//   k_rs_scan      : per digit value, the exclusive scan of its counts over the tiles (one block per digit value)
//   k_rs_scatter<1>: LSD pass 1 (low byte): one record (high byte << 24 | index) per key in low-byte order, 4 B/point written
//                    (8 B beyond 2^24 points)
//   k_rs_hist2     : histogram of the high bytes per tile of that order
//   k_rs_scatter<2>: LSD pass 2 (high byte, stable): perm
//   k_gather_xyz   : sorted[j] = xyz[perm[j]]     (only for the "prepared layout" entry point; the
//                    in-step sort lets the fused kernel read xyz through perm instead)
//   k_rs_scatter_ride<1|2>, k_rs_scan_setup, k_rs_hist2 with `extra` : the same launches with RIDER blocks (f3d_sort_riders,
//                    f3d_fuse_blocks.h): streaming work of the one-shot fused call -- label presence, the label fill (beside pass 1 for a
//                    small cloud, beside k_rs_hist2 otherwise), k_fuse_setup with the code book, mask coding -- that depends on nothing
//                    the sort produces and uses the HBM bandwidth the ranking rounds leave idle
// A tile's ranks come from per-wave digit counts in LDS and, per round of 64 keys, one 64-bit lane mask per digit value in LDS (every lane
// ORs its bit into its digit's mask, reads the mask back and counts the lanes below it: k_rs_scatter): no global atomic, no look-back
// chain, the same perm in every run (equal keys keep their index order: both passes are stable).  (Until the lane masks a round matched
// the digit's bits with 8 ballots on a per-lane 64-bit mask and read its counts through a volatile generic pointer: 96 vector
// instructions and two flat round trips per round, 50 / 48 us per pass at 10M points against 42 / 38 now, profiles/sort_rank.md.)
// History: a first version used one returning global atomic per point (counting sort): ~0.5 ms per kernel at 10M points.  r1/r2
// used rocprim::radix_sort_pairs on (uint16 key, uint32 index): 0.27 ms for the whole sort at 10M points, of which 2 x 81 us in
// its onesweep passes (decoupled look-back); the passes here move fewer bytes (the index is implicit in pass 1, the key is
// 1 byte in pass 2) and need no look-back.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cstring>
#include "f3d.h"
#include "f3d_kernels.h"
#include "f3d_fuse_blocks.h"

namespace {

constexpr int SB = 256;
#define F3D_SORT_KEY_BITS 16                 // two 8-bit radix passes
typedef uint16_t sort_key_t;

struct bbox6 { double lo[3], hi[3]; };

template <typename T>
__global__ __launch_bounds__(SB) void k_bbox_partial(const T* __restrict__ xyz, int64_t n, int64_t stride, bbox6* __restrict__ partial) {
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
    // a strided sample is enough: points outside the sampled box are clamped into the border cells, which can only cost
    // a little coherence, never correctness
#pragma unroll 4
    for (int64_t i = ((int64_t)blockIdx.x * SB + threadIdx.x) * stride; i < n; i += (int64_t)gridDim.x * SB * stride) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double x = (double)xyz[3 * i + c];
            if (fabs(x) < 1e300) { lo[c] = fmin(lo[c], x); hi[c] = fmax(hi[c], x); }
        }
    }
    __shared__ double sl[3][SB / 64], sh[3][SB / 64];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double a = lo[c], b = hi[c];
        for (int off = 32; off >= 1; off >>= 1) { a = fmin(a, __shfl_xor(a, off, 64)); b = fmax(b, __shfl_xor(b, off, 64)); }
        if ((threadIdx.x & 63) == 0) { sl[c][threadIdx.x >> 6] = a; sh[c][threadIdx.x >> 6] = b; }
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        double a = sl[threadIdx.x][0], b = sh[threadIdx.x][0];
        for (int w = 1; w < SB / 64; ++w) { a = fmin(a, sl[threadIdx.x][w]); b = fmax(b, sh[threadIdx.x][w]); }
        partial[blockIdx.x].lo[threadIdx.x] = a; partial[blockIdx.x].hi[threadIdx.x] = b;
    }
}

// the cell grid from the partial boxes (at most 64 of them: one lane each).  Called by the first wave of every k_rs_keys block --
// 64 x 48 bytes out of L2 and ~100 scalar-ish instructions per block, instead of a one-block kernel of its own between two launches.
__device__ __forceinline__ void grid_from_partials(const bbox6* __restrict__ partial, int nparts, f3d_cellgrid* out /*LDS*/) {
    const int lane = threadIdx.x & 63;
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
    if (lane < nparts)
        for (int c = 0; c < 3; ++c) { lo[c] = partial[lane].lo[c]; hi[c] = partial[lane].hi[c]; }
#pragma unroll
    for (int c = 0; c < 3; ++c)
        for (int off = 32; off >= 1; off >>= 1) { lo[c] = fmin(lo[c], __shfl_xor(lo[c], off, 64)); hi[c] = fmax(hi[c], __shfl_xor(hi[c], off, 64)); }
    if (lane == 0) {
        f3d_cellgrid g;
        double ext[3];
        for (int c = 0; c < 3; ++c) {
            g.lo[c] = lo[c] <= hi[c] ? lo[c] : 0.0;
            ext[c] = lo[c] <= hi[c] ? (hi[c] - lo[c]) : 0.0;
            if (!(ext[c] > 1e-12)) ext[c] = 1e-12;
        }
        // F3D_SORT_KEY_BITS key bits are dealt to the axes one at a time, always to the axis whose cells are currently the
        // longest, so the cells come out as cubic as the box allows; the key interleaves the axes' bits from the most
        // significant level down (a Morton code with per-axis bit counts), so a contiguous run of sorted points is a
        // compact 3-D block (small footprint in every view's mask, good for gather coalescing and the per-XCD L2).
        int bits[3] = {0, 0, 0};
        for (int k = 0; k < F3D_SORT_KEY_BITS; ++k) {
            int best = 0;
            double bl = -1.0;
            for (int c = 0; c < 3; ++c) {
                const double len = ext[c] / (double)(1 << bits[c]);
                if (len > bl) { bl = len; best = c; }
            }
            ++bits[best];
        }
        for (int c = 0; c < 3; ++c) {
            g.dim[c] = 1 << bits[c];
            g.bits[c] = bits[c];
            g.inv_cell[c] = (double)g.dim[c] / (ext[c] * 1.0000001);
        }
        g.ncells = 1 << F3D_SORT_KEY_BITS;                     // key space; the last key also collects non-finite points
        *out = g;
    }
}

// the bits of axis c's cell index `i` at their places in the key (a Morton code with per-axis bit counts: from the most significant
// level down, every axis that still has a bit at that level contributes it)
__device__ __forceinline__ uint32_t spread_axis(uint32_t i, int c, const int bits[3]) {
    uint32_t key = 0;
    int pos = F3D_SORT_KEY_BITS;                                    // next output position, counted down
    for (int level = F3D_SORT_KEY_BITS - 1; level >= 0; --level)
        for (int a = 0; a < 3; ++a)
            if (bits[a] > level) { --pos; if (a == c) key |= ((i >> level) & 1u) << pos; }
    return key;
}

constexpr int RS_LUT = 1024;                 // per-axis spread tables in LDS when no axis has more cells than this (the usual case: 64 x 64 x 16)

// float32 is enough for the cell of a point: the ORDER of the points never changes a result, only how compact a wave's 128 points are
template <typename T>
__device__ __forceinline__ void cell_index(const T* __restrict__ p, const float lo[3], const float inv[3], const int dim[3], int idx[3], bool& ok) {
    ok = true;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float x = (float)p[c];
        ok = ok && (fabsf(x) < 1e30f);
        int k = (int)((x - lo[c]) * inv[c]);
        k = k < 0 ? 0 : (k >= dim[c] ? dim[c] - 1 : k);
        idx[c] = k;
    }
}

template <typename T>
__device__ __forceinline__ uint32_t cell_of(const T* __restrict__ p, const f3d_cellgrid& g) {
    int idx[3];
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double x = (double)p[c];
        ok = ok && (fabs(x) < 1e300);
        int k = (int)((x - g.lo[c]) * g.inv_cell[c]);
        k = k < 0 ? 0 : (k >= g.dim[c] ? g.dim[c] - 1 : k);
        idx[c] = k;
    }
    if (!ok) return (1u << F3D_SORT_KEY_BITS) - 1u;
    uint32_t key = 0;
    for (int level = F3D_SORT_KEY_BITS - 1; level >= 0; --level)     // at most 3 bits appended per level
#pragma unroll
        for (int c = 0; c < 3; ++c)
            if (g.bits[c] > level) key = (key << 1) | (((uint32_t)idx[c] >> level) & 1u);
    return key;
}

// ---- the radix passes --------------------------------------------------------------------------------------------
#ifndef F3D_RS_THREADS
#define F3D_RS_THREADS 512
#endif
#ifndef F3D_RS_ROUNDS
#define F3D_RS_ROUNDS 16
#endif
constexpr int RS_THREADS = F3D_RS_THREADS;   // 8 waves per block
constexpr int RS_WAVES = RS_THREADS / 64;
constexpr int RS_ROUNDS = F3D_RS_ROUNDS;     // a wave walks 16 x 64 consecutive keys
constexpr int RS_TILE = RS_THREADS * RS_ROUNDS;   // 8192 keys per block

// item (wave w, round r, lane l) of tile b: consecutive lanes = consecutive keys (coalesced), consecutive rounds and waves
// = ascending index (what makes the ranks below stable)
__device__ __forceinline__ int64_t rs_item(int64_t tile, int wave, int round, int lane) {
    return tile * RS_TILE + (int64_t)wave * (RS_ROUNDS * 64) + round * 64 + lane;
}

// keys of one tile + histogram of their low bytes.  blkhist is digit-major: [256][ntiles].  The block shape is this kernel's own
// (F3D_RK_THREADS threads walk the tile's 8192 points): measured 1024 / 512 / 256 / 128 / 64 threads = 76 / 64 / 57 / 74 / 114 us at 10M points --
// 1221 blocks of 512 threads are 1.2 "waves" of resident blocks at 4 per CU (the last fifth runs on an empty chip), 256 threads all fit at once.
#ifndef F3D_RK_THREADS
#define F3D_RK_THREADS 256
#endif
// A small cloud (fewer tiles than two per CU) takes 512 threads per tile: the chip is not full either way and the rounds of a thread halve
// (1.25M points: sort 71 -> 64 us).
constexpr int RK_SMALL_THREADS = 512;
template <typename T, int RK_THREADS>
__global__ __launch_bounds__(RK_THREADS) void k_rs_keys(const T* __restrict__ xyz, int64_t n, const bbox6* __restrict__ partial, int nparts,
                                                         sort_key_t* __restrict__ keys, uint32_t* __restrict__ blkhist, int ntiles) {
    __shared__ uint32_t hist[256];
    __shared__ f3d_cellgrid sg;
    __shared__ uint16_t lut[3][RS_LUT];
    constexpr int RK_ROUNDS = RS_TILE / RK_THREADS;
    static_assert(RK_THREADS >= 64 && RK_THREADS * RK_ROUNDS == RS_TILE, "the key kernel's block must cover a tile");
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (wave == 0) grid_from_partials(partial, nparts, &sg);
    for (int d = threadIdx.x; d < 256; d += RK_THREADS) hist[d] = 0u;
    __syncthreads();
    f3d_cellgrid g = sg;
#pragma unroll
    for (int c = 0; c < 3; ++c) {                                   // block-uniform: keep the integers in SGPRs (scalar branches in cell_of)
        g.dim[c] = __builtin_amdgcn_readfirstlane(g.dim[c]);
        g.bits[c] = __builtin_amdgcn_readfirstlane(g.bits[c]);
    }
    const bool tables = g.dim[0] <= RS_LUT && g.dim[1] <= RS_LUT && g.dim[2] <= RS_LUT;
    if (tables) {                                                   // key = lut[0][ix] | lut[1][iy] | lut[2][iz]: three LDS reads instead of a 48-step bit loop
        for (int c = 0; c < 3; ++c)
            for (int i = threadIdx.x; i < g.dim[c]; i += RK_THREADS) lut[c][i] = (uint16_t)spread_axis((uint32_t)i, c, g.bits);
        __syncthreads();
    }
    const float lo[3] = {(float)g.lo[0], (float)g.lo[1], (float)g.lo[2]};
    const float inv[3] = {(float)g.inv_cell[0], (float)g.inv_cell[1], (float)g.inv_cell[2]};
#pragma unroll 8
    for (int r = 0; r < RK_ROUNDS; ++r) {
        const int64_t i = (int64_t)blockIdx.x * RS_TILE + (int64_t)wave * (RK_ROUNDS * 64) + r * 64 + lane;
        if (i < n) {
            uint32_t key;
            if (tables) {
                int idx[3]; bool ok;
                cell_index(xyz + 3 * i, lo, inv, g.dim, idx, ok);
                key = ok ? ((uint32_t)lut[0][idx[0]] | lut[1][idx[1]] | lut[2][idx[2]]) : ((1u << F3D_SORT_KEY_BITS) - 1u);
            } else {
                key = cell_of(xyz + 3 * i, g);
            }
            keys[i] = (sort_key_t)key;
            atomicAdd(&hist[key & 0xFFu], 1u);
        }
    }
    __syncthreads();
    for (int d = threadIdx.x; d < 256; d += RK_THREADS) blkhist[(size_t)d * ntiles + blockIdx.x] = hist[d];
}

// Pass 1 hands pass 2 ONE record per key: (high byte << 24) | index in 32 bits while the indices fit 24 bits (n <= 2^24: 4 B/point),
// (high byte << 32) | index in 64 bits beyond.  (Separate 1-byte and 4-byte arrays cost two store instructions per key; the byte
// stores alone made pass 1 twice as slow as pass 2.)
template <typename R> struct rs_rec;
template <> struct rs_rec<uint32_t> { static constexpr int shift = 24; static constexpr uint32_t imask = 0xFFFFFFu; };
template <> struct rs_rec<uint64_t> { static constexpr int shift = 32; static constexpr uint64_t imask = 0xFFFFFFFFull; };

// histogram of the high bytes per tile of the pass-1 order.  F3D_RH_THREADS threads walk the tile's 8192 records with 16-byte loads, all
// of a thread's loads requested before the first is counted (with one 4-byte load per key and round the kernel took 15 us for 40 MB).
// The block shape is the kernel's own, as in k_rs_keys, but here 512 threads win: 256 (every block resident at once) measured 5 us
// slower per step at 10M points and 3 us at 1.25M (profiles/sort_occupancy.md).
// `extra` rider blocks (f3d_sort_riders::fill_blocks, f3d_rider_role) do the label fill instead of a tile: the kernel holds 1 KB of LDS and
// reads 4 B/point, so a rider takes no slot from it, and it runs in front of k_fuse, which is all the fill needs.
#ifndef F3D_RH_THREADS
#define F3D_RH_THREADS 512
#endif
constexpr int RH_THREADS = F3D_RH_THREADS;
template <typename R>
__global__ __launch_bounds__(RH_THREADS) void k_rs_hist2(const R* __restrict__ recs, int64_t n, uint32_t* __restrict__ blkhist, int ntiles,
                                                          int64_t* __restrict__ classes, int64_t nfill, int64_t fill_value, int extra) {
    const f3d_block_role role = f3d_rider_role(blockIdx.x, gridDim.x, (unsigned)extra);
    if (role.rider) { f3d_fill_labels_block(classes, nfill, fill_value, role.index, extra, RH_THREADS); return; }
    __shared__ uint32_t hist[256];
    constexpr int PER = 16 / sizeof(R);                              // records of a 16-byte load
    constexpr int LOADS = RS_TILE / (RH_THREADS * PER);
    static_assert(RH_THREADS >= 256 && LOADS * RH_THREADS * PER == RS_TILE, "the histogram kernel's block must cover a tile");
    typedef R vec_t __attribute__((ext_vector_type(PER)));
    if (threadIdx.x < 256) hist[threadIdx.x] = 0u;
    __syncthreads();
    const int64_t base = (int64_t)role.index * RS_TILE;
    if (base + RS_TILE <= n && !((uintptr_t)recs & 15)) {
        const vec_t* __restrict__ src = reinterpret_cast<const vec_t*>(recs + base);
        vec_t v[LOADS];
#pragma unroll
        for (int r = 0; r < LOADS; ++r) v[r] = src[r * RH_THREADS + threadIdx.x];
#pragma unroll
        for (int r = 0; r < LOADS; ++r)
#pragma unroll
            for (int c = 0; c < PER; ++c) atomicAdd(&hist[(uint32_t)(v[r][c] >> rs_rec<R>::shift) & 0xFFu], 1u);
    } else {                                                         // the last tile, or records that are not 16-byte aligned
        const int64_t end = base + RS_TILE < n ? base + RS_TILE : n;
        for (int64_t i = base + threadIdx.x; i < end; i += RH_THREADS) atomicAdd(&hist[(uint32_t)(recs[i] >> rs_rec<R>::shift) & 0xFFu], 1u);
    }
    __syncthreads();
    if (threadIdx.x < 256) blkhist[(size_t)threadIdx.x * ntiles + role.index] = hist[threadIdx.x];
}

// block d: exclusive scan of row d of blkhist (the tiles' counts of digit value d) in place; tot[d] = the row's sum
__device__ __forceinline__ void rs_scan_row(uint32_t* __restrict__ blkhist, int ntiles, uint32_t* __restrict__ tot, int d) {
    __shared__ uint32_t part[256];
    uint32_t* row = blkhist + (size_t)d * ntiles;
    const int per = (ntiles + 255) / 256;
    const int lo = threadIdx.x * per, hi = min(ntiles, lo + per);
    uint32_t sum = 0;
    for (int k = lo; k < hi; ++k) sum += row[k];
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {                        // Hillis-Steele inclusive scan over the 256 partial sums
        const uint32_t v = threadIdx.x >= off ? part[threadIdx.x - off] : 0u;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    uint32_t run = part[threadIdx.x] - sum;                          // exclusive prefix of this thread's piece
    for (int k = lo; k < hi; ++k) { const uint32_t c = row[k]; row[k] = run; run += c; }
    if (threadIdx.x == 255) tot[d] = part[255];
}
__global__ __launch_bounds__(256) void k_rs_scan(uint32_t* __restrict__ blkhist, int ntiles, uint32_t* __restrict__ tot) {
    rs_scan_row(blkhist, ntiles, tot, blockIdx.x);
}

// The same scan with the k_fuse_setup blocks (tables, threshold table, empty todo lists, the code book) riding in its launch: the
// book needs the label presence complete, which pass 1 (launched earlier on the stream) carried, and pass 2's coding rider needs the book.
__global__ __launch_bounds__(256) void k_rs_scan_setup(uint32_t* __restrict__ blkhist, int ntiles, uint32_t* __restrict__ tot, f3d_setup_args setup, int extra) {
    const f3d_block_role role = f3d_rider_role(blockIdx.x, gridDim.x, (unsigned)extra);
    if (role.rider) { f3d_fuse_setup_block(setup, role.index, extra, 256); return; }
    rs_scan_row(blkhist, ntiles, tot, role.index);
}

// exclusive prefix of `v` over threads 0..255 (threads >= 256 pass 0 and get garbage); every thread of the block must call it
__device__ __forceinline__ uint32_t rs_excl_scan256(uint32_t v, uint32_t* wsum /*[4]*/) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const uint32_t o = __shfl_up(inc, off, 64); if (lane >= off) inc += o; }
    __syncthreads();                                                  // (wsum may still be read by an earlier call)
    if (lane == 63 && wave < 4) wsum[wave] = inc;
    __syncthreads();
    uint32_t before = 0u;
    for (int w = 0; w < 4; ++w) before += (w < wave) ? wsum[w] : 0u;
    return before + inc - v;
}

// One point of order in a ranking round (see k_rs_scatter): an acquire-release fence over LDS at workgroup scope -- the compiler may
// move no LDS access across it, and it compiles to `s_waitcnt lgkmcnt(0)`, so every LDS instruction the wave issued above has
// completed -- and a wave barrier, which keeps the scheduler from moving anything else across.  (A wavefront-scope fence emits no wait.)
__device__ __forceinline__ void rs_round_order() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup", "local");
    __builtin_amdgcn_wave_barrier();
}

// One LSD pass over a tile.  PASS 1: digit = low byte of keys[i]; writes the record (high byte, i) to the key's place in low-byte
// order.  PASS 2: digit = the record's high byte (pass-1 order, stable); writes the record's index to perm.  offs = the scanned
// blkhist, tot = the digit totals.
// The tile is first ordered in LDS (per-wave digit counts -> positions; ranks inside a round from the wave's lane masks), then written
// out by consecutive threads: the keys of one digit value leave as one contiguous run (~128 B of records at 8192 keys / 256 values)
// instead of 64 scattered stores per instruction (measured at 10M keys: pass 1 144 -> 95 us with the run-wise output).
//
// Ranking a round (64 consecutive keys of a wave).  The wave owns wmask[wave][256], one 64-bit lane mask per digit value, all zero
// between rounds, and wcount[wave][256], the tile position of the wave's next key of each digit value, 16 bits each (a position is below
// RS_TILE = 8192; two digit values share a 32-bit word, and every access below is to one 16-bit half).
//   (1) every live lane ORs its lane bit into wmask[wave][digit]                     (ds_or_b64, no return; an OR has no order)
//   (2) every live lane reads wmask[wave][digit] and wcount[wave][digit]             (ds_read_b64, ds_read_u16)
//       rank = popc(mask & lanes below me): equal digits keep lane = index order; position = count + rank
//   (3) the lane of rank 0 stores count + popc(mask) and a zero mask                  (ds_write_b16, ds_write_b64)
// rs_round_order() stands between (1) and (2), between (2) and (3), and between (3) and the next round's (1): each time the wave
// waits until its own LDS instructions have completed (lgkmcnt(0)) before it issues the next group, and the compiler keeps the groups
// apart.  No other wave touches these words, so nothing else needs an order; the OR, the loads and the stores are relaxed atomics so that the
// compiler neither keeps a word in a register across a fence nor drops the store of the zero.  A lane without a key takes no part.
// (The 16-bit store of (3) writes its own half only: the leaders of digit values d and d + 1 may store into one 32-bit word in the same
// instruction, each its half.  Before the rounds the halves are COUNTS, at most 1024 per wave, added with one 32-bit LDS atomic on the
// pair -- 1 << 16 for the odd digit value; a half cannot carry into its neighbour.)
// The mask tables lie on the first RS_WAVES x 2 KB of `srec` (a table of their own would cost a CU a resident block), so the rounds
// only compute positions -- kept with the digit in dig[r], no further register -- and the records are placed after a block barrier.
//
// The output loop needs gdelta of the run position j lies in.  Pass 2 reads the digit out of the record.  Pass 1's record carries the
// HIGH byte while the run goes by the low one; a byte per position for it would be 8 KB of LDS (the fourth block of a CU) and one
// conflicted byte store per key.  Instead the 256 owners leave a bitmap of run starts with a running count per 64-bit word and gdelta
// compacted by the rank of the non-empty run (f3d_run_span_of, f3d_run_at: f3d_kernels.h); a wave of the output loop covers one word,
// so the word and its count are one broadcast read each.
//
// LDS of a block, uint32 records: records 32,768 + wcount 4,096 + gdelta 1,024 + wsum 16, pass 1 + 1,024 + 256 (bitmap, counts): with
// the riders' own tables 39,504 / 38,416 B for pass 1 / pass 2 -- four blocks in a CU's 160 KiB, which also takes 64 VGPRs or fewer.
constexpr int RS_WORDS = RS_TILE / 64;                               // 64-bit words of the run-start bitmap
template <int PASS, typename R> constexpr size_t rs_dyn_lds() { return (size_t)RS_TILE * sizeof(R) + (PASS == 1 ? RS_WORDS * (sizeof(unsigned long long) + sizeof(uint16_t)) : 0); }
// waves per SIMD the scatter kernels are compiled for: 8 (four 512-thread blocks per CU, 64 VGPRs) with 32-bit records; the 64-bit
// records take 64 KB and more of LDS per block, two blocks per CU at most
template <typename R> constexpr int rs_min_waves() { return sizeof(R) == 4 ? 8 : 2; }

template <int PASS, typename R>
__device__ __forceinline__ void rs_scatter_tile(const sort_key_t* __restrict__ keys, const R* __restrict__ recs_in, int64_t n,
                                                const uint32_t* __restrict__ offs, const uint32_t* __restrict__ tot, int ntiles,
                                                R* __restrict__ recs_out, uint32_t* __restrict__ perm_out, const int tile) {
    __shared__ uint16_t wcount[RS_WAVES][256];                       // per wave: count of each digit value, then its running position in the tile
    __shared__ uint32_t gdelta[256];                                 // global position of the tile's first key of a digit value - its position in the tile
    __shared__ uint32_t wsum[4];                                     //   (pass 1: of the r-th non-empty digit value)
    extern __shared__ unsigned long long rs_dyn[];                   // the tile in digit order: RS_TILE records (+ pass 1: the run-start bitmap and its counts)
    R* srec = reinterpret_cast<R*>(rs_dyn);
    unsigned long long* starts = reinterpret_cast<unsigned long long*>(srec + RS_TILE);      // pass 1 only
    uint16_t* before = reinterpret_cast<uint16_t*>(starts + RS_WORDS);
    static_assert((size_t)RS_WAVES * 256 * sizeof(unsigned long long) <= (size_t)RS_TILE * sizeof(uint32_t), "the lane masks must fit under the records");
    static_assert(RS_TILE <= (1 << 16) - 1 && RS_ROUNDS * 64 < (1 << 16), "a tile position and a wave's count fit 16 bits");
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    unsigned long long* const wmask = rs_dyn + wave * 256;           // this wave's lane masks (until the records are placed)
    // requested first: the two table entries of this thread's digit value (latency hidden behind the key loads and the counting)
    const int d_own = threadIdx.x & 255;
    const bool own = threadIdx.x < 256;
    const uint32_t t_d = own ? tot[d_own] : 0u;
    const uint32_t o_d = own ? offs[(size_t)d_own * ntiles + tile] : 0u;
    typedef uint32_t __attribute__((may_alias)) pair_t;
    pair_t* const wpair = reinterpret_cast<pair_t*>(&wcount[0][0]);  // the counts as pairs (digit values 2k, 2k + 1)
    for (int k = threadIdx.x; k < RS_WAVES * 256; k += RS_THREADS) { if (k < RS_WAVES * 128) wpair[k] = 0u; rs_dyn[k] = 0ull; }
    if (PASS == 1 && threadIdx.x < RS_WORDS) { starts[threadIdx.x] = 0ull; if (threadIdx.x == 0) before[0] = 0; }
    __syncthreads();
    uint32_t dig[RS_ROUNDS];                                         // the digit; after the ranking rounds (digit << 16) | tile position
    R val[RS_ROUNDS];                                                // the record that leaves (pass 1: built here; pass 2: the one that came in)
#pragma unroll
    for (int r = 0; r < RS_ROUNDS; ++r) {
        const int64_t i = rs_item(tile, wave, r, lane);
        dig[r] = 0xFFFFFFFFu; val[r] = 0;
        if (i < n) {
            if (PASS == 1) { const uint32_t k = keys[i]; dig[r] = k & 0xFFu; val[r] = ((R)(k >> 8) << rs_rec<R>::shift) | (R)i; }
            else { val[r] = recs_in[i]; dig[r] = (uint32_t)(val[r] >> rs_rec<R>::shift) & 0xFFu; }
            atomicAdd(&wpair[wave * 128 + (dig[r] >> 1)], 1u << (16 * (dig[r] & 1u)));
        }
    }
    __syncthreads();
    {
        uint32_t c_d = 0u;
        if (own) for (int w = 0; w < RS_WAVES; ++w) c_d += wcount[w][d_own];
        const uint32_t gstart = rs_excl_scan256(t_d, wsum);          // keys of smaller digit values in the whole array
        // ... in this tile (at most RS_TILE: 16 bits) and, pass 1, above them the NON-EMPTY smaller digit values: one scan for both
        const uint32_t both = rs_excl_scan256(PASS == 1 ? (c_d | (c_d ? 1u << 16 : 0u)) : c_d, wsum);
        const uint32_t lstart = both & 0xFFFFu;
        if (own) {
            const uint32_t gd = gstart + o_d - lstart;
            if (PASS == 1) {
                if (c_d) {
                    const uint32_t rank = both >> 16;
                    const f3d_run_span sp = f3d_run_span_of(lstart, c_d, RS_WORDS);
                    __hip_atomic_fetch_or(&starts[sp.word], 1ull << sp.bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    gdelta[rank] = gd;
                    for (uint32_t w = sp.first; w <= sp.last; ++w) before[w] = (uint16_t)(rank + 1u);
                }
            } else gdelta[d_own] = gd;
            uint32_t run = lstart;
            for (int w = 0; w < RS_WAVES; ++w) { const uint32_t c = wcount[w][d_own]; wcount[w][d_own] = (uint16_t)run; run += c; }
        }
    }
    __syncthreads();
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (int r = 0; r < RS_ROUNDS; ++r) {
        const uint32_t d = dig[r];
        const bool live = d != 0xFFFFFFFFu;
        if (live) __hip_atomic_fetch_or(&wmask[d], 1ull << lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        rs_round_order();                                            // (1) -> (2): the wave's ORs have landed
        unsigned long long m = 0ull;
        uint32_t base = 0u;
        if (live) {
            m = __hip_atomic_load(&wmask[d], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            base = __hip_atomic_load(&wcount[wave][d], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        rs_round_order();                                            // (2) -> (3): every lane has its mask and count
        const uint32_t rank = (uint32_t)__popcll(m & below);
        if (live && rank == 0u) {
            __hip_atomic_store(&wcount[wave][d], (uint16_t)(base + (uint32_t)__popcll(m)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __hip_atomic_store(&wmask[d], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        rs_round_order();                                            // (3) -> the next round's (1): count advanced, mask zero again
        if (live) dig[r] = (d << 16) | (base + rank);
    }
    __syncthreads();                                                 // every wave is done with its masks: the records may overwrite them
#pragma unroll
    for (int r = 0; r < RS_ROUNDS; ++r)
        if (dig[r] != 0xFFFFFFFFu) srec[dig[r] & 0xFFFFu] = val[r];
    __syncthreads();
    const int64_t left = n - (int64_t)tile * RS_TILE;
    const int count = (int)(left < RS_TILE ? left : RS_TILE);
#pragma unroll 4
    for (int j = threadIdx.x; j < count; j += RS_THREADS) {          // (a wave's 64 positions are one word of the bitmap)
        const R rec = srec[j];
        if (PASS == 1) recs_out[(uint32_t)j + gdelta[f3d_run_at(starts[j >> 6], before[j >> 6], (unsigned)j & 63u)]] = rec;
        else perm_out[(uint32_t)j + gdelta[(uint32_t)(rec >> rs_rec<R>::shift) & 0xFFu]] = (uint32_t)(rec & rs_rec<R>::imask);
    }
}

template <int PASS, typename R>
__global__ __launch_bounds__(RS_THREADS, rs_min_waves<R>()) void k_rs_scatter(const sort_key_t* __restrict__ keys, const R* __restrict__ recs_in, int64_t n,
                                                            const uint32_t* __restrict__ offs, const uint32_t* __restrict__ tot, int ntiles,
                                                            R* __restrict__ recs_out, uint32_t* __restrict__ perm_out) {
    rs_scatter_tile<PASS, R>(keys, recs_in, n, offs, tot, ntiles, recs_out, perm_out, blockIdx.x);
}

// The scatter passes with riders (f3d_sort_riders): `extra` blocks of the launch, spread evenly through the grid, do streaming work of the
// fused call instead of a tile -- the ranking rounds are chains of LDS round trips that leave HBM idle, the riders are pure HBM traffic.
// A rider block holds the kernel's LDS (one of the four resident slots of a CU) while it lives; it waits for nobody and nobody waits for it.
//   PASS 1: label presence over the mask bytes (masks == NULL: none), then the label fill (classes == NULL: none, or it rides beside
//   k_rs_hist2) -- pass 1 has bandwidth to spare, pass 2 + coding has not.   PASS 2: mask coding with the book the scan launch in front built.
template <int PASS, typename R>
__global__ __launch_bounds__(RS_THREADS, rs_min_waves<R>()) void k_rs_scatter_ride(const sort_key_t* __restrict__ keys, const R* __restrict__ recs_in, int64_t n,
                                                                 const uint32_t* __restrict__ offs, const uint32_t* __restrict__ tot, int ntiles,
                                                                 R* __restrict__ recs_out, uint32_t* __restrict__ perm_out,
                                                                 const uint8_t* __restrict__ masks, int64_t mask_bytes, f3d_codebook* __restrict__ cb,
                                                                 uint8_t* __restrict__ coded, int V, int H, int W,
                                                                 int64_t* __restrict__ classes, int64_t nfill, int64_t fill_value, int extra) {
    const f3d_block_role role = f3d_rider_role(blockIdx.x, gridDim.x, (unsigned)extra);
    if (role.rider) {
        if (PASS == 1) {
            if (masks) {
                if (!((uintptr_t)masks & 7)) f3d_presence_block_wide<F3D_RIDER_UNROLL_1>(masks, mask_bytes, cb, role.index, extra, RS_THREADS);
                else f3d_presence_block<false>(masks, mask_bytes, cb, role.index, extra, RS_THREADS);
            }
            if (classes) f3d_fill_labels_block(classes, nfill, fill_value, role.index, extra, RS_THREADS);
        } else {
            if (!(W & 7) && !((uintptr_t)masks & 7)) f3d_code_masks_block_rows<F3D_RIDER_UNROLL>(masks, coded, V, H, W, cb, role.index, extra, RS_THREADS);
            else f3d_code_masks_block<false>(masks, coded, V, H, W, cb, role.index, extra, RS_THREADS);
        }
        return;
    }
    rs_scatter_tile<PASS, R>(keys, recs_in, n, offs, tot, ntiles, recs_out, perm_out, role.index);
}

template <typename T>
__global__ __launch_bounds__(SB) void k_gather_xyz(const T* __restrict__ xyz, int64_t n, const int32_t* __restrict__ perm,
                                                    T* __restrict__ sorted) {
    for (int64_t i = (int64_t)blockIdx.x * SB + threadIdx.x; i < n; i += (int64_t)gridDim.x * SB) {
        const size_t src = (size_t)perm[i];
        sorted[3 * i] = xyz[3 * src]; sorted[3 * i + 1] = xyz[3 * src + 1]; sorted[3 * i + 2] = xyz[3 * src + 2];
    }
}

struct sort_layout {
    size_t partial, keys, recs, hist, tot, total;
    int ntiles;
    bool wide;                                                      // 64-bit records (more than 2^24 points)
};

sort_layout layout_for(int64_t n) {
    sort_layout L;
    f3d_carve c;
    L.ntiles = (int)((n + RS_TILE - 1) / RS_TILE);
    L.wide = n > (1 << 24);
    L.partial = c.take(64 * sizeof(bbox6));
    L.keys = c.take((size_t)n * sizeof(sort_key_t));
    L.recs = c.take((size_t)n * (L.wide ? 8 : 4));
    L.hist = c.take((size_t)256 * L.ntiles * 4);
    L.tot = c.take(256 * 4);
    L.total = c.off;
    return L;
}

template <typename R>
hipError_t run_passes(const sort_layout& L, char* base, int64_t n, int32_t* perm, hipStream_t s, const f3d_sort_riders* rd) {
    const sort_key_t* keys = reinterpret_cast<const sort_key_t*>(base + L.keys);
    R* recs = reinterpret_cast<R*>(base + L.recs);
    uint32_t* hist = reinterpret_cast<uint32_t*>(base + L.hist);
    uint32_t* tot = reinterpret_cast<uint32_t*>(base + L.tot);
    const dim3 gt(L.ntiles), bt(RS_THREADS);
    const size_t lds1 = rs_dyn_lds<1, R>(), lds2 = rs_dyn_lds<2, R>();
    if (lds1 > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void*)k_rs_scatter<1, R>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds1);
        if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k_rs_scatter<2, R>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds2);
        if (e != hipSuccess) return e;
    }
    if (rd) {
        if (lds1 > 48 * 1024) {
            hipError_t e = hipFuncSetAttribute((const void*)k_rs_scatter_ride<1, R>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds1);
            if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k_rs_scatter_ride<2, R>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds2);
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(k_rs_scan, dim3(256), dim3(256), 0, s, hist, L.ntiles, tot);
        const bool fill2 = rd->classes && rd->fill_blocks > 0;       // the fill rides beside the second histogram, not beside pass 1
        if (rd->pass1_blocks > 0)
            hipLaunchKernelGGL((k_rs_scatter_ride<1, R>), dim3(L.ntiles + rd->pass1_blocks), bt, lds1, s, keys, (const R*)nullptr, n, hist, tot, L.ntiles, recs,
                               (uint32_t*)nullptr, rd->presence ? rd->masks : (const uint8_t*)nullptr, rd->mask_bytes, rd->cb, (uint8_t*)nullptr, 0, 0, 0,
                               fill2 ? (int64_t*)nullptr : rd->classes, rd->n, rd->fill_value, rd->pass1_blocks);
        else hipLaunchKernelGGL((k_rs_scatter<1, R>), gt, bt, lds1, s, keys, (const R*)nullptr, n, hist, tot, L.ntiles, recs, (uint32_t*)nullptr);
        const int fb = fill2 ? rd->fill_blocks : 0;
        hipLaunchKernelGGL(k_rs_hist2<R>, dim3(L.ntiles + fb), dim3(RH_THREADS), 0, s, recs, n, hist, L.ntiles, fill2 ? rd->classes : (int64_t*)nullptr, rd->n, rd->fill_value, fb);
        hipLaunchKernelGGL(k_rs_scan_setup, dim3(256 + rd->setup_blocks), dim3(256), 0, s, hist, L.ntiles, tot, rd->setup, rd->setup_blocks);
        hipLaunchKernelGGL((k_rs_scatter_ride<2, R>), dim3(L.ntiles + rd->code_blocks), bt, lds2, s, (const sort_key_t*)nullptr, recs, n, hist, tot, L.ntiles,
                           (R*)nullptr, reinterpret_cast<uint32_t*>(perm), rd->masks, rd->mask_bytes, rd->cb, rd->coded, rd->V, rd->H, rd->W,
                           (int64_t*)nullptr, (int64_t)0, (int64_t)0, rd->code_blocks);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(k_rs_scan, dim3(256), dim3(256), 0, s, hist, L.ntiles, tot);
    hipLaunchKernelGGL((k_rs_scatter<1, R>), gt, bt, lds1, s, keys, (const R*)nullptr, n, hist, tot, L.ntiles, recs, (uint32_t*)nullptr);
    hipLaunchKernelGGL(k_rs_hist2<R>, gt, dim3(RH_THREADS), 0, s, recs, n, hist, L.ntiles, (int64_t*)nullptr, (int64_t)0, (int64_t)0, 0);
    hipLaunchKernelGGL(k_rs_scan, dim3(256), dim3(256), 0, s, hist, L.ntiles, tot);
    hipLaunchKernelGGL((k_rs_scatter<2, R>), gt, bt, lds2, s, (const sort_key_t*)nullptr, recs, n, hist, tot, L.ntiles, (R*)nullptr, reinterpret_cast<uint32_t*>(perm));
    return hipGetLastError();
}

}  // namespace

size_t f3d_sort_scratch_bytes(int64_t n) { return layout_for(n < 1 ? 1 : n).total; }

hipError_t f3d_launch_cell_sort(const void* xyz, int dtype, int64_t n, void* sorted_xyz, int32_t* perm, void* scratch, hipStream_t s,
                                const f3d_sort_riders* riders) {
    if (n <= 0) return hipSuccess;
    if (n > 0x7fffffffLL) return hipErrorInvalidValue;
    const sort_layout L = layout_for(n);
    char* base = reinterpret_cast<char*>(scratch);
    bbox6* partial = reinterpret_cast<bbox6*>(base + L.partial);
    sort_key_t* keys = reinterpret_cast<sort_key_t*>(base + L.keys);
    uint32_t* hist = reinterpret_cast<uint32_t*>(base + L.hist);
    const int64_t stride = n > (1 << 16) ? n >> 16 : 1;          // inspect <= ~65k points for the bounding box (4 strided loads per thread of 64 blocks)
    const int64_t sb = ((n + stride - 1) / stride + SB - 1) / SB;
    const int nparts = (int)(sb < 64 ? sb : 64);                 // (one lane of k_rs_keys' first wave per partial box)
    const int gstream = f3d_grid_for(n, SB, 8192);
    const dim3 gt(L.ntiles);
    const bool small = L.ntiles < 512;                          // fewer tiles than two per CU
    if (dtype == F3D_F64) {
        hipLaunchKernelGGL(k_bbox_partial<double>, dim3(nparts), dim3(SB), 0, s, (const double*)xyz, n, stride, partial);
        if (small) hipLaunchKernelGGL((k_rs_keys<double, RK_SMALL_THREADS>), gt, dim3(RK_SMALL_THREADS), 0, s, (const double*)xyz, n, partial, nparts, keys, hist, L.ntiles);
        else hipLaunchKernelGGL((k_rs_keys<double, F3D_RK_THREADS>), gt, dim3(F3D_RK_THREADS), 0, s, (const double*)xyz, n, partial, nparts, keys, hist, L.ntiles);
    } else {
        hipLaunchKernelGGL(k_bbox_partial<float>, dim3(nparts), dim3(SB), 0, s, (const float*)xyz, n, stride, partial);
        if (small) hipLaunchKernelGGL((k_rs_keys<float, RK_SMALL_THREADS>), gt, dim3(RK_SMALL_THREADS), 0, s, (const float*)xyz, n, partial, nparts, keys, hist, L.ntiles);
        else hipLaunchKernelGGL((k_rs_keys<float, F3D_RK_THREADS>), gt, dim3(F3D_RK_THREADS), 0, s, (const float*)xyz, n, partial, nparts, keys, hist, L.ntiles);
    }
    hipError_t e = L.wide ? run_passes<uint64_t>(L, base, n, perm, s, riders) : run_passes<uint32_t>(L, base, n, perm, s, riders);
    if (e != hipSuccess) return e;
    if (sorted_xyz) {
        if (dtype == F3D_F64) hipLaunchKernelGGL(k_gather_xyz<double>, dim3(gstream), dim3(SB), 0, s, (const double*)xyz, n, perm, (double*)sorted_xyz);
        else hipLaunchKernelGGL(k_gather_xyz<float>, dim3(gstream), dim3(SB), 0, s, (const float*)xyz, n, perm, (float*)sorted_xyz);
    }
    return hipGetLastError();
}
