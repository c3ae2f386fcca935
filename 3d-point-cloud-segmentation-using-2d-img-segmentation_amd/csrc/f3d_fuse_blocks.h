// The streaming helpers of the fused call as BLOCK FUNCTIONS: label presence, the code book, mask coding, the label fill and the
// per-call tables of k_fuse.  Each takes (block number, number of blocks, threads per block) and reads neither blockIdx, gridDim nor
// F3D_BLOCK, so the same body serves a kernel of its own (f3d_fuse.hip: the one-line __global__ callers) and a "rider" block inside a
// launch of the cell sort (f3d_sort.hip: the scatter passes run 512 threads, the scan 256).  A body walks its share of the work
// grid-strided: any number of blocks, one included, covers everything.  Presence and the vector form of coding have a second body for
// riders (f3d_presence_block_wide, f3d_code_masks_block_rows): a rider block occupies one of the sort's few resident slots, so it must
// keep several wide loads in flight per thread and spend few instructions per byte, inside the sort kernel's register budget.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "f3d.h"
#include "f3d_kernels.h"

// ------------------------------------------------------------------------------------------
// Vote-bin codes.  Code 0 = "no sample" (the coded planes end every view with 64 such bytes, and a lane without a pixel
// gathers from there instead of carrying a validity flag through the vote), code 1 = a label the reference would
// reject (> nclasses, IndexError at voting.py:98), then
//   presence book (no filter, or votes requested): one code per label that occurs in the masks, the SMALLEST label
//       getting the LARGEST code, so that the maximum of (count << 8 | code) is count desc, label asc = np.argmax's
//       first-maximum rule;
//   filter book: code 2 = any other valid label (it only counts towards the total, voting.py:120), codes 3.. = the
//       distinct entries of filter_classes.
// The book is built on the device (presence + code_lut), so no host round trip decides the histogram size:
// the launcher enqueues a SMALL-histogram and a FULL-histogram instance of k_fuse and each returns at once unless the
// book's size is in its range.
// ------------------------------------------------------------------------------------------
#define F3D_RIDER_THREADS 512                // threads of a rider block = those of the sort's scatter passes
#ifndef F3D_RIDER_UNROLL
#define F3D_RIDER_UNROLL 6                   // loads a rider thread keeps in flight (coding; 8 took 82 VGPRs: pass 2 must stay at 64 or below for its 4 blocks per CU)
#endif
#ifndef F3D_RIDER_UNROLL_1
#define F3D_RIDER_UNROLL_1 8                 // ... presence, 16-byte loads (pass 1 must stay at 64 VGPRs or below for its 4 blocks per CU)
#endif
#ifndef F3D_RIDER_BLOCKS_1
#define F3D_RIDER_BLOCKS_1 256               // rider blocks beside pass 1 (presence, fill), at most
#endif
#ifndef F3D_RIDER_BLOCKS_2
#define F3D_RIDER_BLOCKS_2 1024              // ... beside pass 2 (coding)
#endif
#ifndef F3D_RIDER_BLOCKS_FILL
#define F3D_RIDER_BLOCKS_FILL 512            // ... beside k_rs_hist2 (the label fill of a large cloud; 0: the fill always rides beside pass 1)
#endif
// A small cloud (fewer sort tiles than two per CU, as in f3d_launch_cell_sort) does not fill the chip: its riders run on idle CUs beside
// pass 1, where fewer of them disturb the tiles less, and k_rs_hist2 is too short to carry the fill (profiles/sort_occupancy.md).
#ifndef F3D_RIDER_SMALL_POINTS
#define F3D_RIDER_SMALL_POINTS (512 * 8192)
#endif
#ifndef F3D_RIDER_BLOCKS_1_SMALL
#define F3D_RIDER_BLOCKS_1_SMALL 128         // rider blocks beside pass 1 of a small cloud (presence and the fill)
#endif
#define F3D_CODE_NONE 0u
#define F3D_CODE_BAD 1u
#define F3D_CODE_OTHER 2u
#define F3D_VHEAD 15                         // the head of f3d_view in doubles: M[9], t[3], mnorm[3]

// One view of the coded masks: (ceil(H/8) + 2) x (ceil(W/8) + 2) tiles of 8x8 pixels (64 B each): the image plus a one-tile border of
// "no sample" all around, so that pixel (-1, -1) .. (W, H) are addressable -- tile (0, 0) of view 0, at offset 0, is such a border tile
// and serves as the address a lane without a pixel gathers from.
__host__ __device__ inline int f3d_coded_pitch(int W) { return ((W + 7) >> 3) + 2; }
__host__ __device__ inline size_t f3d_coded_plane(int H, int W) { return (size_t)(((H + 7) >> 3) + 2) * (size_t)f3d_coded_pitch(W) * 64; }

// a block's label set (8 dwords in LDS) into the code book's: one thread per dword adds only the bits the global set still lacks --
// thousands of waves hammering the same 8 dwords with atomics cost 0.38 ms; masks share their alphabet, so almost every block finds
// its bits set.  (After a barrier that made blkset complete.)
__device__ __forceinline__ void f3d_presence_publish(const unsigned* blkset, f3d_codebook* __restrict__ cb) {
    if (threadIdx.x < 8) {
        const unsigned want = blkset[threadIdx.x];
        const unsigned have = __hip_atomic_load(&cb->presence[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (want & ~have) atomicOr(&cb->presence[threadIdx.x], want);
    }
}

// which labels occur in the masks.  A thread keeps a 256-bit set in four 64-bit registers; masks are piecewise constant,
// so an 8-byte word whose bytes all equal the previous label costs two instructions.  VEC: src is 8-byte aligned.
template <bool VEC>
__device__ __forceinline__ void f3d_presence_block(const uint8_t* __restrict__ src, int64_t nbytes, f3d_codebook* __restrict__ cb,
                                                   int blk, int nblk, int nthr) {
    unsigned long long m0 = 0, m1 = 0, m2 = 0, m3 = 0;
    auto mark = [&](unsigned l) {
        const unsigned long long bit = 1ull << (l & 63u);
        const unsigned q = l >> 6;
        m0 |= q == 0u ? bit : 0ull; m1 |= q == 1u ? bit : 0ull; m2 |= q == 2u ? bit : 0ull; m3 |= q == 3u ? bit : 0ull;
    };
    const int64_t stride = (int64_t)nblk * nthr;
    if (VEC) {
        const int64_t nw = nbytes >> 3;
        const uint64_t* w = reinterpret_cast<const uint64_t*>(src);
        uint64_t last = ~0ull;                                     // the previous word when all of its bytes were equal
        for (int64_t k = (int64_t)blk * nthr + threadIdx.x; k < nw; k += stride) {
            const uint64_t x = w[k];
            if (x == last) continue;
            if (x == (x & 0xFFull) * 0x0101010101010101ull) { mark((unsigned)(x & 0xFFull)); last = x; continue; }
#pragma unroll
            for (int c = 0; c < 8; ++c) mark((unsigned)(x >> (8 * c)) & 0xFFu);
        }
        if (blk == 0 && (int64_t)threadIdx.x < (nbytes & 7)) mark(src[(nw << 3) + threadIdx.x]);
    } else {
        for (int64_t k = (int64_t)blk * nthr + threadIdx.x; k < nbytes; k += stride) mark(src[k]);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        m0 |= __shfl_xor(m0, off, 64); m1 |= __shfl_xor(m1, off, 64); m2 |= __shfl_xor(m2, off, 64); m3 |= __shfl_xor(m3, off, 64);
    }
    __shared__ unsigned blkset[8];                                 // block-level OR in LDS
    if (threadIdx.x < 8) blkset[threadIdx.x] = 0u;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
        const unsigned long long m[4] = {m0, m1, m2, m3};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if ((unsigned)m[q]) atomicOr(&blkset[2 * q], (unsigned)m[q]);
            if ((unsigned)(m[q] >> 32)) atomicOr(&blkset[2 * q + 1], (unsigned)(m[q] >> 32));
        }
    }
    __syncthreads();
    f3d_presence_publish(blkset, cb);
}

// The same for a rider block (src 8-byte aligned, at least 256 threads).  A rider holds one of the host kernel's few resident slots,
// so what it keeps in flight per thread decides what the riders cost the host: 16-byte loads, UNROLL of them requested before the first
// is looked at, and the set kept as 256 flag bytes in LDS (stores without a return value) instead of eight registers and twelve
// instructions per mark -- the register form of this loop does not fit the 64 VGPRs pass 1 of the sort may use.  A block takes
// nthr * UNROLL consecutive 16-byte pairs per step (one uniform base, 32-bit lane offsets); a word in front of the first 16-byte
// boundary, one behind the last pair and the last nbytes & 7 bytes are block 0's.
template <int UNROLL>
__device__ __forceinline__ void f3d_presence_block_wide(const uint8_t* __restrict__ src, int64_t nbytes, f3d_codebook* __restrict__ cb,
                                                        int blk, int nblk, int nthr) {
    __shared__ uint8_t seen[256];
    __shared__ unsigned blkset[8];
    if (threadIdx.x < 256) seen[threadIdx.x] = 0;
    __syncthreads();
    const int64_t nw = nbytes >> 3;
    const uint64_t* w = reinterpret_cast<const uint64_t*>(src);
    uint64_t last = ~0ull;                                         // the previous word when all of its bytes were equal
    auto word = [&](uint64_t x) {
        if (x == last) return;
        if (x == (x & 0xFFull) * 0x0101010101010101ull) { seen[x & 0xFFull] = 1; last = x; return; }
#pragma unroll
        for (int c = 0; c < 8; ++c) seen[(x >> (8 * c)) & 0xFFull] = 1;
    };
    const int64_t head = ((((uintptr_t)src >> 3) & 1) && nw > 0) ? 1 : 0;
    const int64_t np = (nw - head) >> 1;
    const ulonglong2* w2 = reinterpret_cast<const ulonglong2*>(w + head);
    const int64_t chunk = (int64_t)nthr * UNROLL;
    for (int64_t c0 = (int64_t)blk * chunk; c0 < np; c0 += (int64_t)nblk * chunk) {
        const ulonglong2* base = w2 + c0;
        const int64_t left = np - c0;
        ulonglong2 xs[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const int idx = u * nthr + (int)threadIdx.x;
            xs[u] = idx < left ? base[idx] : make_ulonglong2(0ull, 0ull);
        }
#pragma unroll
        for (int u = 0; u < UNROLL; ++u)
            if (u * nthr + (int)threadIdx.x < left) { word(xs[u].x); word(xs[u].y); }
    }
    if (blk == 0) {
        if (threadIdx.x == 0 && head) word(w[0]);
        if (threadIdx.x == 1 && ((nw - head) & 1)) word(w[nw - 1]);
        if ((int64_t)threadIdx.x < (nbytes & 7)) seen[src[(nw << 3) + threadIdx.x]] = 1;
    }
    __syncthreads();
    if (threadIdx.x < 256) {
        const unsigned long long m = __ballot(seen[threadIdx.x] != 0);
        if ((threadIdx.x & 63) == 0) { blkset[threadIdx.x >> 5] = (unsigned)m; blkset[(threadIdx.x >> 5) + 1] = (unsigned)(m >> 32); }
    }
    __syncthreads();
    f3d_presence_publish(blkset, cb);
}

// cb->cmin for this call's threshold (see segment_point): thread t < 256 finds, by bisection with the reference's own float64 division,
// how many c in 0..t give c / t < threshold.  One block of at least 256 threads.
__device__ __forceinline__ void f3d_threshold_table(f3d_codebook* __restrict__ cb, double threshold) {
    const int t = threadIdx.x;
    if (t >= 256) return;
    int lo = 0, hi = t + 1;                                   // c in [lo, hi): the first c that is NOT below the threshold
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((double)mid / (double)t < threshold) lo = mid + 1; else hi = mid;
    }
    cb->cmin[t] = (uint16_t)lo;                               // t = 0 is never looked up (no votes: voting.py:126)
}

// one block of at least 256 threads: thread l < 256 decides the code of label l (further threads only keep the barriers company).
// book: 0 = every label 0..nclasses has a bin (no presence pass ran), 1 = presence book, 2 = filter book.
__device__ __forceinline__ void f3d_code_lut_block(f3d_codebook* __restrict__ cb, int nclasses, int book, const f3d_filter_args& flt) {
    __shared__ unsigned pres[8];
    __shared__ int first_of[256];                                  // filter book: position of label l's first occurrence, -1 = not listed
    __shared__ unsigned long long wb[4], wr[4];
    const unsigned l = threadIdx.x;
    const bool act = l < 256u;
    if (l < 8) { pres[l] = book == 1 ? cb->presence[l] : 0xFFFFFFFFu; cb->presence[l] = 0u; }   // consumed (see f3d_launch_mask_presence)
    if (act) { first_of[l] = -1; cb->inv[l] = 0; }
    __syncthreads();
    if (book == 2) {
        if (l == 0)
            for (int k = flt.nfilter - 1; k >= 0; --k) { const int f = f3d_filter_at(flt, k); if (f >= 0 && f < 256) first_of[f] = k; }
        __syncthreads();
        if (!act) return;
        const bool listed = first_of[l] >= 0 && (int)l <= nclasses;
        int rank = 0;                                              // distinct listed labels below l
        for (unsigned j = 0; j < l; ++j) rank += (first_of[j] >= 0 && (int)j <= nclasses) ? 1 : 0;
        int distinct = 0;
        for (unsigned j = 0; j < 256; ++j) distinct += (first_of[j] >= 0 && (int)j <= nclasses) ? 1 : 0;
        const unsigned code = (int)l > nclasses ? F3D_CODE_BAD : (listed ? 3u + (unsigned)rank : F3D_CODE_OTHER);
        cb->lut[l] = (uint8_t)code;
        if (listed) cb->inv[code] = (uint8_t)l;
        if (l == 0) { cb->ncodes = 3 + distinct; cb->words = (3 + distinct + 3) >> 2; cb->book = 2; cb->pad = 0; }   // (pad: this book cannot tell)
        return;
    }
    const bool pv = act && (int)l <= nclasses && ((pres[(l >> 5) & 7u] >> (l & 31u)) & 1u);     // label l is valid and present
    const bool pr = act && (int)l > nclasses && ((pres[(l >> 5) & 7u] >> (l & 31u)) & 1u);      // label l is rejected and present
    const unsigned long long bal = __ballot(pv), balr = __ballot(pr);
    if (act && (l & 63u) == 0u) { wb[l >> 6] = bal; wr[l >> 6] = balr; }
    __syncthreads();
    if (!act) return;
    int K = 0, below = __popcll(bal & ((1ull << (l & 63u)) - 1ull));
    for (unsigned w = 0; w < 4; ++w) { const int c = __popcll(wb[w]); K += c; below += (w < (l >> 6)) ? c : 0; }
    unsigned code;
    if ((int)l > nclasses) code = F3D_CODE_BAD;                    // only meaningful when such a byte really occurs
    else if (pv) code = (unsigned)(K + 1 - below);                 // smallest present label -> K + 1, largest -> 2
    else code = F3D_CODE_NONE;                                     // never gathered; its vote row reads the always-zero bin 0
    cb->lut[l] = (uint8_t)code;
    if (code >= 2u) cb->inv[code] = (uint8_t)l;
    // pad = "no label above nclasses occurs in the masks": only the presence book knows.  k_fuse may then leave views out of a point's
    // vote without hiding the reference's IndexError (f3d_fuse_decide.h)
    if (l == 0) { cb->ncodes = K + 2; cb->words = (K + 2 + 3) >> 2; cb->book = book; cb->pad = (book == 1 && !(wr[0] | wr[1] | wr[2] | wr[3])) ? 1 : 0; }
}

// [V,H,W] row-major labels -> [V][ceil(H/8) + 2][ceil(W/8) + 2][8][8] bin codes (border tiles = "no sample"); one thread moves one
// tile row (8 bytes), a wave writes 512 contiguous bytes.  VEC: W % 8 == 0 and src 8-B aligned (one 8-B load per thread).
template <bool VEC>
__device__ __forceinline__ void f3d_code_masks_block(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int V, int H, int W,
                                                     const f3d_codebook* __restrict__ cb, int blk, int nblk, int nthr) {
    __shared__ uint32_t lut_w[64];
    if (threadIdx.x < 64) lut_w[threadIdx.x] = reinterpret_cast<const uint32_t*>(cb->lut)[threadIdx.x];
    __syncthreads();
    const uint8_t* lut = reinterpret_cast<const uint8_t*>(lut_w);
    const int tw = f3d_coded_pitch(W), th = ((H + 7) >> 3) + 2;    // border included
    const int64_t per_view = (int64_t)th * tw * 8;                 // 8-byte pieces per view
    const int64_t total = per_view * V;
    const size_t tplane = f3d_coded_plane(H, W);
    for (int64_t k = (int64_t)blk * nthr + threadIdx.x; k < total; k += (int64_t)nblk * nthr) {
        const int64_t v = k / per_view; const int64_t r = k - v * per_view;      // r indexes (tile, row-in-tile) of the destination
        uint64_t out = 0;                                                         // border and padding: F3D_CODE_NONE
        const int tile = (int)(r >> 3), ry = (int)(r & 7);
        const int ty = tile / tw, tx = tile - ty * tw;
        const int y = (ty - 1) * 8 + ry, x0 = (tx - 1) * 8;
        if (y >= 0 && y < H && x0 >= 0 && x0 < W) {
            const uint8_t* row = src + (size_t)v * H * W + (size_t)y * W + x0;
            if (VEC) {
                const uint64_t x = *reinterpret_cast<const uint64_t*>(row);
                if (x == (x & 0xFFull) * 0x0101010101010101ull) out = (uint64_t)lut[x & 0xFFull] * 0x0101010101010101ull;
                else {
#pragma unroll
                    for (int c = 0; c < 8; ++c) out |= (uint64_t)lut[(x >> (8 * c)) & 0xFFull] << (8 * c);
                }
            } else {
                for (int c = 0; c < 8; ++c) if (x0 + c < W) out |= (uint64_t)lut[row[c]] << (8 * c);
            }
        }
        *reinterpret_cast<uint64_t*>(dst + (size_t)v * tplane + (size_t)r * 8) = out;
    }
}

// The same for a rider block, vector form only (W % 8 == 0, src 8-byte aligned).  The loop above spends ~70 vector instructions per
// 8-byte piece, most of them on two divisions that turn the piece's index into (view, tile row, tile, row in tile): thousands of blocks
// on a whole chip hide that, a few hundred rider blocks sharing their SIMDs with the sort do not.  Here a WAVE takes one row of tiles of
// one view at a time (tw tiles x 8 rows = tw * 8 consecutive pieces of the destination): view and tile row come from one wave-uniform
// division per tile row, tile and row in tile from shifts, the source row from a uniform base and a 32-bit lane offset; UNROLL loads
// are requested before the first is coded.  "All bytes equal" is x == rotl(x, 8).
template <int UNROLL>
__device__ __forceinline__ void f3d_code_masks_block_rows(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int V, int H, int W,
                                                          const f3d_codebook* __restrict__ cb, int blk, int nblk, int nthr) {
    __shared__ uint32_t lut_w[64];
    if (threadIdx.x < 64) lut_w[threadIdx.x] = reinterpret_cast<const uint32_t*>(cb->lut)[threadIdx.x];
    __syncthreads();
    const uint8_t* lut = reinterpret_cast<const uint8_t*>(lut_w);
    const int tw = f3d_coded_pitch(W), th = ((H + 7) >> 3) + 2;    // border included
    const int per_row = tw * 8;                                    // 8-byte pieces per row of tiles
    const size_t tplane = f3d_coded_plane(H, W);
    const int lane = threadIdx.x & 63, wpb = nthr >> 6;
    const int64_t nunits = (int64_t)V * th;
    for (int64_t unit = (int64_t)blk * wpb + (threadIdx.x >> 6); unit < nunits; unit += (int64_t)nblk * wpb) {
        const int v = __builtin_amdgcn_readfirstlane((int)(unit / th));
        const int ty = __builtin_amdgcn_readfirstlane((int)(unit - (int64_t)v * th));
        uint64_t* out = reinterpret_cast<uint64_t*>(dst + (size_t)v * tplane + (size_t)ty * per_row * 8);
        const uint8_t* rows = src + (size_t)v * H * W + (int64_t)(ty - 1) * 8 * W - 8;      // pixel (x0 = -8, y = (ty - 1) * 8): tile 0's
        const int ylim = H - (ty - 1) * 8;                                                  // rows of this tile row inside the image (<= 0, > 8: none, all)
        const bool border = ty == 0 || ty == th - 1;
        for (int e0 = lane; e0 < per_row; e0 += 64 * UNROLL) {
            uint64_t xs[UNROLL];
            bool in[UNROLL];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                const int e = e0 + 64 * u, tx = e >> 3, ry = e & 7;
                in[u] = e < per_row && !border && tx >= 1 && tx <= (W >> 3) && ry < ylim;
                xs[u] = in[u] ? *reinterpret_cast<const uint64_t*>(rows + ry * W + tx * 8) : 0ull;
            }
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                const int e = e0 + 64 * u;
                if (e >= per_row) break;
                const uint64_t x = xs[u];
                uint64_t o = 0;                                                             // border and padding: F3D_CODE_NONE
                if (in[u]) {
                    if (x == ((x << 8) | (x >> 56))) { const uint32_t c = (uint32_t)lut[x & 0xFFull] * 0x01010101u; o = ((uint64_t)c << 32) | c; }
                    else {
#pragma unroll
                        for (int c = 0; c < 8; ++c) o |= (uint64_t)lut[(x >> (8 * c)) & 0xFFull] << (8 * c);
                    }
                }
                out[e] = o;
            }
        }
    }
}

// classes[0..n) = value by streaming (non-temporal) stores
__device__ __forceinline__ void f3d_fill_labels_block(int64_t* __restrict__ classes, int64_t n, int64_t value, int blk, int nblk, int nthr) {
    for (int64_t i = (int64_t)blk * nthr + threadIdx.x; i < n; i += (int64_t)nblk * nthr)
        __builtin_nontemporal_store(value, &classes[i]);
}

// What f3d_launch_fuse_setup prepares for a k_fuse launch: [group][field][view] copies of the per-view constants the lanes-over-views
// prologue reads (24 floats: cull planes, margins, image size; 15 doubles: M, t, mnorm), the call's threshold table, empty deferred
// lists and -- book >= 0 -- the code book.
struct f3d_setup_args {
    const f3d_view* views; int nviews;
    float* ctabT; double* vtabT;
    f3d_codebook* cb; double threshold;
    unsigned int* todo_count;                // NULL: the lists stay as they are (a later view chunk)
    int lut_nclasses, lut_book;              // lut_book < 0: no book; otherwise the LAST block builds it and takes no part in the tables
    f3d_filter_args flt;
};
__device__ __forceinline__ void f3d_fuse_setup_block(const f3d_setup_args& a, int blk, int nblk, int nthr) {
    if (a.lut_book >= 0 && blk == nblk - 1) { f3d_code_lut_block(a.cb, a.lut_nclasses, a.lut_book, a.flt); return; }
    if (blk == 0) {
        f3d_threshold_table(a.cb, a.threshold);                 // ... the call's threshold table (segment_point)
        if (a.todo_count && threadIdx.x < 4) a.todo_count[threadIdx.x] = 0u;   // ... and empty deferred lists
    }
    const int ngroups = (a.nviews + 63) >> 6;
    const int nsetup = a.lut_book >= 0 ? nblk - 1 : nblk;
    for (int k = blk * nthr + threadIdx.x; k < ngroups * 64 * 39; k += nsetup * nthr) {
        const int v = k / 39, f = k - v * 39, g = v >> 6, l = v & 63;
        const f3d_view& vw = a.views[v < a.nviews ? v : a.nviews - 1];
        if (f < 24) a.ctabT[(g * 24 + f) * 64 + l] = reinterpret_cast<const float*>(&vw.cull_n32[0][0])[f];
        else a.vtabT[(g * F3D_VHEAD + (f - 24)) * 64 + l] = reinterpret_cast<const double*>(&vw)[f - 24];
    }
}

// The riders of one cell sort (f3d_launch_cell_sort, f3d_kernels.h), as the launcher hands them to the sort
struct f3d_sort_riders {
    // beside k_rs_scatter<1> (pass1_blocks rider blocks): label presence over all mask bytes (presence == false: the filter book needs
    // none), then the label fill (classes == NULL: no fill; fill_blocks > 0: not here)
    const uint8_t* masks; int64_t mask_bytes; f3d_codebook* cb; bool presence;
    int64_t* classes; int64_t n; int64_t fill_value; int pass1_blocks;
    int fill_blocks;                         // > 0: the label fill rides beside k_rs_hist2 instead (that many rider blocks; large clouds)
    // inside the second k_rs_scan's launch: k_fuse_setup with the book (setup_blocks, the last of them the book's)
    f3d_setup_args setup; int setup_blocks;
    // beside k_rs_scatter<2>: mask coding
    uint8_t* coded; int V, H, W; int code_blocks;
};
