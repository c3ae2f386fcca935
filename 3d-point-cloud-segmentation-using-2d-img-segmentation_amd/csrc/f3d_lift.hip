// Mask lifting (include/f3d.h, f3d_lift_overlaps / f3d_lift_instances): per-frame 2D instance ids -> consistent 3D instance ids.
// Integer set arithmetic over the pixel-to-point lookups; the one floating-point operation is the merge test's double multiply.
//   k_lift_keys     : pixel -> key point << gbits | segment, or the sentinel npoints << gbits; flags an id > K or a lookup >= N.
//   (rocPRIM)       : radix sort of the keys, then unique: the incidence, ascending in (point, segment), the sentinel last.
//   k_lift_split    : incidence -> point column (padded with N: f3d_launch_key_starts gives the rows), segment column, size[].
//   k_lift_seen     : seen[] (when wanted) and Q = sum over the rows of len * (len - 1) / 2, the bound a grown pair table is sized by.
//   k_lift_pairs    : every pair of a row into an open-addressing table of 64-bit keys a << 32 | b with integer counts: a wave
//                     looks at 64 points, rows of up to 64 segments go one per lane, longer rows one at a time over the wave.
//                     A probe sequence that finds no slot raises the overflow flag: the caller reruns with a larger table.
//   k_lift_table    : the occupied slots: counted, compacted for the sort by key (overlaps), or tested and linked (instances).
//   k_lift_roots .. : roots of non-empty segments -> scan -> seg2inst; k_lift_vote: the row vote; k_lift_keep .. k_lift_final_*:
//                     wins per instance -> keep flags -> scan -> renumbered ids, seg2inst and inst_points.
// Cost grows with the sum of seen^2 (pairs and vote).  Every kernel after the first returns at once under the bad-input flag.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cstddef>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_select.hpp>
#include "f3d_groups.h"

namespace {

constexpr int LB = 256;
constexpr unsigned long long LIFT_EMPTY = ~0ull;
constexpr unsigned LIFT_MAX_PROBE = 4096;           // a longer probe sequence counts as a full table

struct lift_words {
    unsigned long long q;                           // pair occurrences: sum of len * (len - 1) / 2
    unsigned long long ucount;                      // distinct sorted keys, the sentinel included
    unsigned m;                                     // incidences
    int bad;                                        // an id > K or a lookup >= N was seen
    // from here on: cleared before every run of the pair table
    unsigned long long labelled;                    // points of the surviving instances
    unsigned p, ninst, nkept;                       // distinct pairs, instances before / after min_points
    int overflow;
};

__device__ __forceinline__ bool lift_bad(const lift_words* w) { return w->bad != 0; }

__global__ __launch_bounds__(LB) void k_lift_keys(const int32_t* __restrict__ luts, const uint16_t* __restrict__ inst, int64_t total, unsigned hw,
                                                  int64_t npoints, int max_ids, int gbits, unsigned long long* __restrict__ keys,
                                                  lift_words* w, int* err) {
    const unsigned long long sentinel = (unsigned long long)npoints << gbits;
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * LB + threadIdx.x; i < total; i += (int64_t)gridDim.x * LB) {
        const int32_t lut = luts[i];
        const int id = inst[i];
        unsigned long long key = sentinel;
        if (lut >= npoints || id > max_ids) bad = true;
        else if (lut >= 0 && id > 0) {
            const unsigned f = (unsigned)i / hw;
            key = (unsigned long long)lut << gbits | (unsigned long long)((int64_t)f * max_ids + (id - 1));
        }
        keys[i] = key;
    }
    if (bad) { atomicOr(err, F3D_DEVERR_LIFT); atomicOr(&w->bad, 1); }
}

__global__ __launch_bounds__(LB) void k_lift_split(const unsigned long long* __restrict__ ukeys, lift_words* w, int64_t total, int64_t npoints,
                                                   int gbits, uint32_t* __restrict__ pt, int32_t* __restrict__ seg, int32_t* __restrict__ size) {
    if (lift_bad(w)) return;
    const unsigned long long sentinel = (unsigned long long)npoints << gbits, gmask = ((unsigned long long)1 << gbits) - 1;
    int64_t m = (int64_t)w->ucount;
    if (m > 0 && ukeys[m - 1] == sentinel) --m;
    if (blockIdx.x == 0 && threadIdx.x == 0) w->m = (unsigned)m;
    for (int64_t j = (int64_t)blockIdx.x * LB + threadIdx.x; j < total; j += (int64_t)gridDim.x * LB) {
        if (j < m) {
            const unsigned long long k = ukeys[j];
            const int32_t g = (int32_t)(k & gmask);
            pt[j] = (uint32_t)(k >> gbits);
            seg[j] = g;
            atomicAdd(size + g, 1);
        } else {
            pt[j] = (uint32_t)npoints;
        }
    }
}

__global__ __launch_bounds__(LB) void k_lift_seen(const int64_t* __restrict__ rows, int64_t npoints, uint16_t* __restrict__ seen, lift_words* w) {
    if (lift_bad(w)) return;
    __shared__ unsigned long long part[LB];
    unsigned long long q = 0;
    for (int64_t p = (int64_t)blockIdx.x * LB + threadIdx.x; p < npoints; p += (int64_t)gridDim.x * LB) {
        const unsigned long long len = (unsigned long long)(rows[p + 1] - rows[p]);
        if (seen) seen[p] = (uint16_t)(len > 65535 ? 65535 : len);
        q += len * (len - (len > 0)) / 2;
    }
    part[threadIdx.x] = q;
    __syncthreads();
    for (int d = LB / 2; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) part[threadIdx.x] += part[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0 && part[0]) atomicAdd(&w->q, part[0]);
}

// A wave looks at 64 points: rows of up to 64 entries go to their lanes, one each (sh(p, first, len)); a longer row is taken by the
// whole wave, one row at a time (lg(p, first, len, lane), wave-uniform arguments).  Blocks of LB threads, grid-stride.
template <typename Short, typename Long>
__device__ __forceinline__ void lift_rows(const int64_t* __restrict__ rows, int64_t npoints, Short sh, Long lg) {
    const int lane = threadIdx.x & 63;
    for (int64_t w0 = (int64_t)blockIdx.x * LB + threadIdx.x - lane; w0 < npoints; w0 += (int64_t)gridDim.x * LB) {
        const int64_t p = w0 + lane;
        long long r = 0, len = 0;
        if (p < npoints) { r = rows[p]; len = rows[p + 1] - r; }
        if (p < npoints && len <= 64) sh(p, (int64_t)r, (int)len);
        unsigned long long todo = __ballot(len > 64);
        while (todo) {
            const int src = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            lg(w0 + src, (int64_t)__shfl(r, src), (int64_t)__shfl(len, src), lane);
        }
    }
}

__device__ __forceinline__ unsigned long long lift_mix(unsigned long long x) {        // splitmix64's finaliser
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27; x *= 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}

// counts the pair (a, b), a < b.  -> false: no slot within the probe limit (the table is too small)
__device__ __forceinline__ bool lift_insert(unsigned long long* tk, unsigned* tc, unsigned long long mask, unsigned limit, int32_t a, int32_t b) {
    const unsigned long long key = (unsigned long long)(uint32_t)a << 32 | (uint32_t)b;
    unsigned long long s = lift_mix(key) & mask;
    for (unsigned probe = 0; probe < limit; ++probe, s = (s + 1) & mask) {
        unsigned long long cur = __hip_atomic_load(tk + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // a slot never changes once taken
        if (cur == LIFT_EMPTY) {
            cur = atomicCAS(tk + s, LIFT_EMPTY, key);
            if (cur == LIFT_EMPTY) cur = key;
        }
        if (cur == key) { atomicAdd(tc + s, 1u); return true; }
    }
    return false;
}

__global__ __launch_bounds__(LB) void k_lift_pairs(const int64_t* __restrict__ rows, const int32_t* __restrict__ seg, int64_t npoints,
                                                   unsigned long long* tk, unsigned* tc, unsigned long long slots, lift_words* w) {
    if (lift_bad(w)) return;
    const unsigned long long mask = slots - 1;
    const unsigned limit = slots < LIFT_MAX_PROBE ? (unsigned)slots : LIFT_MAX_PROBE;
    lift_rows(rows, npoints,
        [&](int64_t, int64_t r, int len) {
            if (len < 2 || __hip_atomic_load(&w->overflow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
            bool ok = true;
            for (int i = 0; i + 1 < len && ok; ++i) {
                const int32_t a = seg[r + i];
                for (int j = i + 1; j < len && ok; ++j) ok = lift_insert(tk, tc, mask, limit, a, seg[r + j]);
            }
            if (!ok) atomicOr(&w->overflow, 1);
        },
        [&](int64_t, int64_t r, int64_t len, int lane) {
            if (__hip_atomic_load(&w->overflow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
            bool ok = true;
            for (int64_t i = 0; i + 1 < len && ok; ++i) {
                const int32_t a = seg[r + i];
                for (int64_t j = i + 1 + lane; j < len && ok; j += 64) ok = lift_insert(tk, tc, mask, limit, a, seg[r + j]);
            }
            if (!ok) atomicOr(&w->overflow, 1);
        });
}

__global__ __launch_bounds__(LB) void k_lift_init(int32_t* __restrict__ parent, int32_t* __restrict__ wins, int64_t nseg, const lift_words* w) {
    if (lift_bad(w)) return;
    for (int64_t g = (int64_t)blockIdx.x * LB + threadIdx.x; g <= nseg; g += (int64_t)gridDim.x * LB) {
        if (g < nseg) parent[g] = (int32_t)g;
        wins[g] = 0;
    }
}

// The occupied slots of the pair table, counted into w->p.  ck != NULL: slot number k of them (any order) goes to ck / cv when k < cap.
// parent != NULL: a pair that passes the merge test is linked.
__global__ __launch_bounds__(LB) void k_lift_table(const unsigned long long* __restrict__ tk, const unsigned* __restrict__ tc, unsigned long long slots,
                                                   lift_words* w, unsigned long long* __restrict__ ck, unsigned* __restrict__ cv, int64_t cap,
                                                   int32_t* parent, const int32_t* __restrict__ size, const int32_t* __restrict__ seg_classes,
                                                   double ratio, int64_t min_overlap) {
    if (lift_bad(w)) return;
    const int lane = threadIdx.x & 63;
    const unsigned long long lower = ((unsigned long long)1 << lane) - 1;
    const unsigned long long step = (unsigned long long)gridDim.x * LB;
    for (unsigned long long s0 = (unsigned long long)blockIdx.x * LB + threadIdx.x - lane; s0 < slots; s0 += step) {
        const unsigned long long s = s0 + lane;
        const unsigned long long key = s < slots ? tk[s] : LIFT_EMPTY;
        const bool used = key != LIFT_EMPTY;
        const unsigned long long ballot = __ballot(used);
        if (!ballot) continue;
        unsigned base = 0;
        if (lane == __ffsll((long long)ballot) - 1) base = atomicAdd(&w->p, (unsigned)__popcll(ballot));
        base = __shfl(base, __ffsll((long long)ballot) - 1);
        if (!used) continue;
        const unsigned cnt = tc[s];
        if (ck) {
            const int64_t k = (int64_t)base + __popcll(ballot & lower);
            if (k < cap) { ck[k] = key; cv[k] = cnt; }
        }
        if (parent) {
            const int32_t a = (int32_t)(key >> 32), b = (int32_t)(key & 0xffffffffu);
            const int32_t sa = size[a], sb = size[b];
            const bool link = (int64_t)cnt >= min_overlap && (double)cnt >= ratio * (double)(sa < sb ? sa : sb) &&
                              (!seg_classes || seg_classes[a] == seg_classes[b]);
            if (link) f3d_uf_link(parent, a, b);
        }
    }
}

__global__ __launch_bounds__(LB) void k_lift_emit(const unsigned long long* __restrict__ ck, const unsigned* __restrict__ cv, int64_t cap,
                                                  const lift_words* w, int32_t* __restrict__ pairs, int32_t* __restrict__ counts) {
    if (lift_bad(w) || w->overflow || (int64_t)w->p > cap) return;
    const int64_t np = (int64_t)w->p;
    for (int64_t j = (int64_t)blockIdx.x * LB + threadIdx.x; j < np; j += (int64_t)gridDim.x * LB) {
        const unsigned long long key = ck[j];
        pairs[2 * j] = (int32_t)(key >> 32);
        pairs[2 * j + 1] = (int32_t)(key & 0xffffffffu);
        counts[j] = (int32_t)cv[j];
    }
}

__global__ __launch_bounds__(LB) void k_lift_copy(const int32_t* __restrict__ src, int32_t* __restrict__ dst, int64_t n, const lift_words* w) {
    if (lift_bad(w)) return;
    for (int64_t i = (int64_t)blockIdx.x * LB + threadIdx.x; i < n; i += (int64_t)gridDim.x * LB) dst[i] = src[i];
}

// flags[g] = 1 for the root of a component of non-empty segments (an empty segment is never linked), flags[nseg] = 0
__global__ __launch_bounds__(LB) void k_lift_roots(const int32_t* __restrict__ parent, const int32_t* __restrict__ size, int64_t nseg,
                                                   uint32_t* __restrict__ flags, const lift_words* w) {
    if (lift_bad(w)) return;
    for (int64_t g = (int64_t)blockIdx.x * LB + threadIdx.x; g <= nseg; g += (int64_t)gridDim.x * LB)
        flags[g] = g < nseg && size[g] > 0 && f3d_uf_load(parent + g) == (int32_t)g;
}

// after the scan: rank[g] = roots before g, rank[nseg] = instances
__global__ __launch_bounds__(LB) void k_lift_seg2inst(const int32_t* __restrict__ parent, const int32_t* __restrict__ size, int64_t nseg,
                                                      const uint32_t* __restrict__ rank, int32_t* __restrict__ s2i, lift_words* w) {
    if (lift_bad(w)) return;
    if (blockIdx.x == 0 && threadIdx.x == 0) w->ninst = rank[nseg];
    for (int64_t g = (int64_t)blockIdx.x * LB + threadIdx.x; g < nseg; g += (int64_t)gridDim.x * LB)
        s2i[g] = size[g] > 0 ? (int32_t)rank[f3d_uf_root(parent, (int32_t)g)] + 1 : 0;
}

// incidence j -> its instance (the row vote reads a row many times over)
__global__ __launch_bounds__(LB) void k_lift_remap(const int32_t* __restrict__ seg, const int32_t* __restrict__ s2i, int32_t* __restrict__ iid,
                                                   const lift_words* w) {
    if (lift_bad(w)) return;
    const int64_t m = w->m;
    for (int64_t j = (int64_t)blockIdx.x * LB + threadIdx.x; j < m; j += (int64_t)gridDim.x * LB) iid[j] = s2i[seg[j]];
}

// (count, instance) ordered by the larger count, then the smaller instance
__device__ __forceinline__ unsigned long long lift_vote_key(unsigned c, int32_t i) { return (unsigned long long)c << 32 | (0xffffffffu - (uint32_t)i); }

// wins[i] += 1 for every calling lane with i > 0, as one atomic per distinct i among them: neighbouring points mostly win the same
// instance, and a million single adds to a few dozen addresses serialise (5.2 of 12.2 ms at the stress shape before this)
__device__ __forceinline__ void lift_count_wins(int32_t* wins, int32_t i) {
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(i > 0);                       // of the lanes that are here
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        const int32_t v = __shfl(i, src);
        const unsigned long long same = __ballot(i == v);
        if (lane == src) atomicAdd(wins + v, (int)__popcll(same));
        todo &= ~same;
    }
}

__global__ __launch_bounds__(LB) void k_lift_vote(const int64_t* __restrict__ rows, const int32_t* __restrict__ iid, int64_t npoints,
                                                  int32_t* __restrict__ ids, uint16_t* __restrict__ support, int32_t* wins, const lift_words* w) {
    if (lift_bad(w)) return;
    auto put = [&](int64_t p, unsigned long long best) {
        const unsigned c = (unsigned)(best >> 32);
        const int32_t i = c ? (int32_t)(0xffffffffu - (uint32_t)(best & 0xffffffffu)) : 0;
        ids[p] = i;
        support[p] = (uint16_t)(c > 65535 ? 65535 : c);
        lift_count_wins(wins, i);
    };
    lift_rows(rows, npoints,
        [&](int64_t p, int64_t r, int len) {
            unsigned long long best = 0;
            for (int e = 0; e < len; ++e) {
                const int32_t ie = iid[r + e];
                unsigned c = 0;
                for (int k = 0; k < len; ++k) c += iid[r + k] == ie;
                const unsigned long long key = lift_vote_key(c, ie);
                if (key > best) best = key;
            }
            put(p, best);
        },
        [&](int64_t p, int64_t r, int64_t len, int lane) {
            unsigned long long best = 0;
            for (int64_t e = lane; e < len; e += 64) {
                const int32_t ie = iid[r + e];
                unsigned c = 0;
                for (int64_t k = 0; k < len; ++k) c += iid[r + k] == ie;
                const unsigned long long key = lift_vote_key(c, ie);
                if (key > best) best = key;
            }
            for (int off = 32; off > 0; off >>= 1) {
                const unsigned long long o = __shfl_xor(best, off);
                if (o > best) best = o;
            }
            if (lane == 0) put(p, best);
        });
}

// keep[x] = instance x + 1 survives, for x in [0, nseg] (0 from the instance count on)
__global__ __launch_bounds__(LB) void k_lift_keep(const int32_t* __restrict__ wins, int64_t nseg, int64_t min_points, uint32_t* __restrict__ keep,
                                                  const lift_words* w) {
    if (lift_bad(w)) return;
    const int64_t ninst = w->ninst;
    for (int64_t x = (int64_t)blockIdx.x * LB + threadIdx.x; x <= nseg; x += (int64_t)gridDim.x * LB)
        keep[x] = x < ninst && (int64_t)wins[x + 1] >= min_points;
}

// after the scan: rank[x] = survivors before instance x + 1; it survives iff rank[x + 1] > rank[x]
__device__ __forceinline__ int32_t lift_renumber(const uint32_t* rank, int32_t i) {
    return i > 0 && rank[i] > rank[i - 1] ? (int32_t)rank[i - 1] + 1 : 0;
}

__global__ __launch_bounds__(LB) void k_lift_final_points(int32_t* __restrict__ ids, uint16_t* __restrict__ support, int64_t npoints,
                                                          const uint32_t* __restrict__ rank, const lift_words* w) {
    if (lift_bad(w)) return;
    for (int64_t p = (int64_t)blockIdx.x * LB + threadIdx.x; p < npoints; p += (int64_t)gridDim.x * LB) {
        const int32_t i = ids[p];
        if (i == 0) continue;
        const int32_t n = lift_renumber(rank, i);
        ids[p] = n;
        if (n == 0) support[p] = 0;
    }
}

__global__ __launch_bounds__(LB) void k_lift_final_segs(const int32_t* __restrict__ s2i, int32_t* __restrict__ seg2inst, int64_t nseg,
                                                        const uint32_t* __restrict__ rank, const int32_t* __restrict__ wins,
                                                        int64_t* __restrict__ inst_points, lift_words* w) {
    if (lift_bad(w)) return;
    const int64_t ninst = w->ninst;
    if (blockIdx.x == 0 && threadIdx.x == 0) w->nkept = rank[ninst];
    unsigned long long labelled = 0;
    for (int64_t g = (int64_t)blockIdx.x * LB + threadIdx.x; g < nseg; g += (int64_t)gridDim.x * LB) {
        seg2inst[g] = lift_renumber(rank, s2i[g]);
        if (g < ninst) {                                                   // thread g also files instance g + 1
            const int32_t n = lift_renumber(rank, (int32_t)g + 1);
            if (n > 0) { inst_points[n] = wins[g + 1]; labelled += (unsigned long long)wins[g + 1]; }
        }
    }
    if (labelled) atomicAdd(&w->labelled, labelled);
}

__global__ void k_lift_unlabelled(int64_t npoints, int64_t* __restrict__ inst_points, const lift_words* w) {
    if (lift_bad(w)) return;
    inst_points[0] = npoints - (int64_t)w->labelled;
}

struct lift_layout { size_t keys_a, keys_b, pt, seg, rows, size, parent, rank, wins, s2i, words, temp, total; size_t temp_bytes; };

lift_layout lift_layout_for(int64_t pixels, int64_t npoints, int64_t nseg) {
    lift_layout L;
    size_t a = 0, b = 0, c = 0;
    (void)rocprim::radix_sort_keys(nullptr, a, (unsigned long long*)nullptr, (unsigned long long*)nullptr, (size_t)pixels, 0u, 64u);
    (void)rocprim::unique(nullptr, b, (unsigned long long*)nullptr, (unsigned long long*)nullptr, (unsigned long long*)nullptr, (size_t)pixels);
    (void)rocprim::exclusive_scan(nullptr, c, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t)0, (size_t)nseg + 1, rocprim::plus<uint32_t>());
    L.temp_bytes = (a > b ? (a > c ? a : c) : (b > c ? b : c)) + 256;
    f3d_carve cv;
    const size_t t4 = (size_t)pixels * 4, t8 = (size_t)pixels * 8, s4 = (size_t)(nseg + 2) * 4;
    L.keys_a = cv.take(t8); L.keys_b = cv.take(t8); L.pt = cv.take(t4); L.seg = cv.take(t4); L.rows = cv.take((size_t)(npoints + 2) * 8);
    L.size = cv.take(s4); L.parent = cv.take(s4); L.rank = cv.take(s4); L.wins = cv.take(s4); L.s2i = cv.take(s4);
    L.words = cv.take(sizeof(lift_words)); L.temp = cv.take(L.temp_bytes);
    L.total = cv.off;
    return L;
}

struct lift_table { size_t keys, counts, ck_a, ck_b, cv_a, cv_b, temp, total; size_t temp_bytes; };

lift_table lift_table_for(uint64_t slots, int64_t cap) {
    lift_table L;
    L.temp_bytes = 0;
    if (cap > 0) {
        (void)rocprim::radix_sort_pairs(nullptr, L.temp_bytes, (unsigned long long*)nullptr, (unsigned long long*)nullptr, (unsigned*)nullptr,
                                        (unsigned*)nullptr, (size_t)cap, 0u, 64u);
        L.temp_bytes += 256;
    }
    f3d_carve c;
    L.keys = c.take((size_t)slots * 8); L.counts = c.take((size_t)slots * 4);
    L.ck_a = c.take((size_t)cap * 8); L.ck_b = c.take((size_t)cap * 8); L.cv_a = c.take((size_t)cap * 4); L.cv_b = c.take((size_t)cap * 4);
    L.temp = c.take(L.temp_bytes);
    L.total = c.off;
    return L;
}

int lift_gbits(const f3d_lift_job& j) { return f3d_bits_for((int64_t)j.nframes * j.max_ids, 1); }
dim3 lift_grid(int64_t n) { return dim3((unsigned)f3d_grid_for(n, LB, F3D_GRID_CAP)); }

}  // namespace

size_t f3d_lift_scratch_bytes(int64_t pixels, int64_t npoints, int64_t nseg) { return lift_layout_for(pixels, npoints, nseg).total; }
size_t f3d_lift_table_bytes(uint64_t slots, int64_t cap) { return lift_table_for(slots, cap).total; }

hipError_t f3d_launch_lift_incidence(const f3d_lift_job& j) {
    const int64_t pixels = (int64_t)j.nframes * j.hw, nseg = (int64_t)j.nframes * j.max_ids;
    const lift_layout L = lift_layout_for(pixels, j.npoints, nseg);
    char* base = (char*)j.scratch;
    unsigned long long *ka = (unsigned long long*)(base + L.keys_a), *kb = (unsigned long long*)(base + L.keys_b);
    uint32_t* pt = (uint32_t*)(base + L.pt);
    int32_t *seg = (int32_t*)(base + L.seg), *size = (int32_t*)(base + L.size);
    int64_t* rows = (int64_t*)(base + L.rows);
    lift_words* w = (lift_words*)(base + L.words);
    const int gbits = lift_gbits(j);
    const dim3 b(LB), gt = lift_grid(pixels);
    hipStream_t s = j.stream;

    F3D_TRY(hipMemsetAsync(w, 0, sizeof(lift_words), s));
    F3D_TRY(hipMemsetAsync(size, 0, (size_t)nseg * 4, s));
    hipLaunchKernelGGL(k_lift_keys, gt, b, 0, s, j.luts, j.inst, pixels, (unsigned)j.hw, j.npoints, j.max_ids, gbits, ka, w, j.err);
    size_t tb = L.temp_bytes;
    F3D_TRY(rocprim::radix_sort_keys(base + L.temp, tb, ka, kb, (size_t)pixels, 0u, (unsigned)(gbits + f3d_bits_for(j.npoints + 1, 1)), s));
    tb = L.temp_bytes;
    F3D_TRY(rocprim::unique(base + L.temp, tb, kb, ka, &w->ucount, (size_t)pixels, rocprim::equal_to<unsigned long long>(), s));
    hipLaunchKernelGGL(k_lift_split, gt, b, 0, s, ka, w, pixels, j.npoints, gbits, pt, seg, size);
    F3D_TRY(f3d_launch_key_starts(pt, pixels, j.npoints, nullptr, &w->bad, rows, s));
    hipLaunchKernelGGL(k_lift_seen, lift_grid(j.npoints), b, 0, s, rows, j.npoints, j.seen, w);
    if (j.sizes) hipLaunchKernelGGL(k_lift_copy, lift_grid(nseg), b, 0, s, size, j.sizes, nseg, w);
    return hipGetLastError();
}

hipError_t f3d_launch_lift_merge(const f3d_lift_job& j, int64_t stats[F3D_LIFT_NSTATS]) {
    const int64_t pixels = (int64_t)j.nframes * j.hw, nseg = (int64_t)j.nframes * j.max_ids;
    const lift_layout L = lift_layout_for(pixels, j.npoints, nseg);
    const lift_table T = lift_table_for(j.slots, j.instances ? 0 : j.cap);
    char *base = (char*)j.scratch, *tbase = (char*)j.table;
    int32_t *iid = (int32_t*)(base + L.pt), *seg = (int32_t*)(base + L.seg), *size = (int32_t*)(base + L.size);
    int32_t *parent = (int32_t*)(base + L.parent), *wins = (int32_t*)(base + L.wins), *s2i = (int32_t*)(base + L.s2i);
    uint32_t* rank = (uint32_t*)(base + L.rank);
    int64_t* rows = (int64_t*)(base + L.rows);
    lift_words* w = (lift_words*)(base + L.words);
    unsigned long long *tk = (unsigned long long*)(tbase + T.keys), *ck_a = (unsigned long long*)(tbase + T.ck_a), *ck_b = (unsigned long long*)(tbase + T.ck_b);
    unsigned *tc = (unsigned*)(tbase + T.counts), *cv_a = (unsigned*)(tbase + T.cv_a), *cv_b = (unsigned*)(tbase + T.cv_b);
    const dim3 b(LB), gp = lift_grid(j.npoints), gs = lift_grid(nseg + 1), gtab = lift_grid((int64_t)j.slots);
    hipStream_t s = j.stream;

    // (a rerun after an overflow: everything from the table on is computed again)
    F3D_TRY(hipMemsetAsync(&w->labelled, 0, sizeof(lift_words) - offsetof(lift_words, labelled), s));
    F3D_TRY(hipMemsetAsync(tk, 0xff, (size_t)j.slots * 8, s));
    F3D_TRY(hipMemsetAsync(tc, 0, (size_t)j.slots * 4, s));
    hipLaunchKernelGGL(k_lift_pairs, gp, b, 0, s, rows, seg, j.npoints, tk, tc, (unsigned long long)j.slots, w);
    if (!j.instances) {
        const bool emit = j.cap > 0;
        if (emit) F3D_TRY(hipMemsetAsync(ck_a, 0xff, (size_t)j.cap * 8, s));
        hipLaunchKernelGGL(k_lift_table, gtab, b, 0, s, tk, tc, (unsigned long long)j.slots, w, emit ? ck_a : nullptr, cv_a, j.cap,
                           (int32_t*)nullptr, size, (const int32_t*)nullptr, 0.0, (int64_t)0);
        if (emit) {
            size_t tb = T.temp_bytes;
            F3D_TRY(rocprim::radix_sort_pairs(tbase + T.temp, tb, ck_a, ck_b, cv_a, cv_b, (size_t)j.cap, 0u, (unsigned)(32 + f3d_bits_for(nseg, 1)), s));
            hipLaunchKernelGGL(k_lift_emit, lift_grid(j.cap), b, 0, s, ck_b, cv_b, j.cap, w, j.pairs, j.counts);
        }
    } else {
        hipLaunchKernelGGL(k_lift_init, gs, b, 0, s, parent, wins, nseg, w);
        hipLaunchKernelGGL(k_lift_table, gtab, b, 0, s, tk, tc, (unsigned long long)j.slots, w, (unsigned long long*)nullptr, (unsigned*)nullptr,
                           (int64_t)0, parent, size, j.seg_classes, j.ratio, j.min_overlap);
        hipLaunchKernelGGL(k_lift_roots, gs, b, 0, s, parent, size, nseg, rank, w);
        size_t tb = L.temp_bytes;
        F3D_TRY(rocprim::exclusive_scan(base + L.temp, tb, rank, rank, (uint32_t)0, (size_t)nseg + 1, rocprim::plus<uint32_t>(), s));
        hipLaunchKernelGGL(k_lift_seg2inst, gs, b, 0, s, parent, size, nseg, rank, s2i, w);
        hipLaunchKernelGGL(k_lift_remap, lift_grid(pixels), b, 0, s, seg, s2i, iid, w);
        hipLaunchKernelGGL(k_lift_vote, gp, b, 0, s, rows, iid, j.npoints, j.ids, j.support, wins, w);
        hipLaunchKernelGGL(k_lift_keep, gs, b, 0, s, wins, nseg, j.min_points, rank, w);
        tb = L.temp_bytes;
        F3D_TRY(rocprim::exclusive_scan(base + L.temp, tb, rank, rank, (uint32_t)0, (size_t)nseg + 1, rocprim::plus<uint32_t>(), s));
        hipLaunchKernelGGL(k_lift_final_points, gp, b, 0, s, j.ids, j.support, j.npoints, rank, w);
        hipLaunchKernelGGL(k_lift_final_segs, gs, b, 0, s, s2i, j.seg2inst, nseg, rank, wins, j.inst_points, w);
        hipLaunchKernelGGL(k_lift_unlabelled, dim3(1), dim3(1), 0, s, j.npoints, j.inst_points, w);
    }
    F3D_TRY(hipGetLastError());
    lift_words hw;
    F3D_TRY(hipMemcpyAsync(&hw, w, sizeof(hw), hipMemcpyDeviceToHost, s));
    F3D_TRY(hipStreamSynchronize(s));
    stats[0] = hw.p; stats[1] = hw.nkept; stats[2] = hw.ninst; stats[3] = hw.m; stats[4] = (int64_t)hw.q; stats[5] = hw.overflow; stats[6] = hw.bad;
    return hipSuccess;
}
