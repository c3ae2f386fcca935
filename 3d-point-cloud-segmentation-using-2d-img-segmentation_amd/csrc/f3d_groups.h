// components -> groups -> shaped sums: what f3d_mesh.hip, f3d_planes.hip and f3d_obb.hip share behind the union-find of f3d_kernels.h
// ("components -> groups -> shaped sums").  Items carry a 32-bit group key; f3d_group_pairs lists every group's members in
// ascending item index; a group's sum is cut into chunks of CHUNK members, each summed by one wave, and the chunk sums are summed the
// same way, so the bits of a sum depend on the member count alone.
#pragma once
#include "f3d_kernels.h"

// lane l adds the items l, l + 64, l + 128, ... of [0, count) left to right, then the 64 lane sums meet in an xor butterfly
template <typename At>
__device__ __forceinline__ double f3d_wave_sum(int64_t count, int lane, At at) {
    double acc = 0.0;
    for (int64_t i = lane; i < count; i += 64) acc = acc + at(i);
    for (int off = 32; off > 0; off >>= 1) acc = acc + __shfl_xor(acc, off);
    return acc;
}

// The chunk heads of the n grouped positions: position p of group c = skeys[p] < ngroups heads a chunk when p - starts[c] is a multiple
// of CHUNK.  A wave looks at 64 positions, finds the heads among them and calls body(q, len, c) for each with all of its lanes: the
// chunk is the grouped positions [q, q + len) of group c.  Blocks of NT threads, grid-stride.
template <int CHUNK, int NT, typename Body>
__device__ __forceinline__ void f3d_chunk_heads(const uint32_t* __restrict__ skeys, const int64_t* __restrict__ starts, int64_t n,
                                                int64_t ngroups, Body body) {
    const int lane = threadIdx.x & 63;
    for (int64_t w0 = (int64_t)blockIdx.x * NT + threadIdx.x - lane; w0 < n; w0 += (int64_t)gridDim.x * NT) {
        const int64_t p = w0 + lane;
        bool head = false;
        long long e = 0, c = 0;
        if (p < n) {
            c = (long long)skeys[p];
            if (c < ngroups) { e = starts[c + 1]; head = ((p - starts[c]) % CHUNK) == 0; }
        }
        unsigned long long todo = __ballot(head);
        while (todo) {
            const int src = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const int64_t q = w0 + src, ce = (int64_t)__shfl(e, src);
            body(q, ce - q < CHUNK ? ce - q : (int64_t)CHUNK, (int64_t)__shfl(c, src));
        }
    }
}

// one wave per group: body(c, b, e) with all lanes, [b, e) = the grouped positions of group c.  Blocks of NT threads, grid-stride.
template <int NT, typename Body>
__device__ __forceinline__ void f3d_group_waves(const int64_t* __restrict__ starts, int64_t ngroups, Body body) {
    for (int64_t c = ((int64_t)blockIdx.x * NT + threadIdx.x) >> 6; c < ngroups; c += ((int64_t)gridDim.x * NT) >> 6)
        body(c, starts[c], starts[c + 1]);
}

// the sum of group [b, e): f3d_wave_sum of its chunk sums, part(q) = the sum of the chunk whose head is grouped position q
template <int CHUNK, typename Part>
__device__ __forceinline__ double f3d_chunks_sum(int64_t b, int64_t e, int lane, Part part) {
    return f3d_wave_sum((e - b + CHUNK - 1) / CHUNK, lane, [&](int64_t j) { return part(b + j * CHUNK); });
}

// starts[k] = first position of key k in the ascending keys[0 .. n) (lower bound), k = 0 .. nkeys.  nkeys_dev (device, may be NULL):
// the count is min(*nkeys_dev, nkeys).  skip (device, may be NULL): nothing is written when *skip != 0 -- a caller's early-out flag;
// of an int64 flag that only holds 0 or 1, pass the low word.
hipError_t f3d_launch_key_starts(const uint32_t* keys, int64_t n, int64_t nkeys, const uint32_t* nkeys_dev, const int32_t* skip,
                                 int64_t* starts, hipStream_t s);
// bytes of `temp` for f3d_group_pairs of n pairs that sorts at most `bits` key bits (ascending in bits)
size_t f3d_group_temp_bytes(int64_t n, unsigned bits = 32);
// The n pairs (keys_a, vals_a) in a stable order of the low `bits` key bits -> (keys_b, vals_b), then f3d_launch_key_starts of keys_b:
// with vals_a = 0, 1, 2, .. the values of a key are its items in ascending index.
hipError_t f3d_group_pairs(uint32_t* keys_a, uint32_t* keys_b, uint32_t* vals_a, uint32_t* vals_b, int64_t n, int bits, void* temp,
                           size_t temp_bytes, int64_t nkeys, const uint32_t* nkeys_dev, const int32_t* skip, int64_t* starts,
                           hipStream_t s);
