// Grouping of 32-bit keyed items (f3d_groups.h): the one 32-bit rocPRIM pair sort of the library and the lower bound of every key.
//   k_key_starts : starts[k] = lower bound of k in the sorted keys, grid-stride over the keys.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <rocprim/device/device_radix_sort.hpp>
#include "f3d_groups.h"

namespace {

constexpr int GB = 256;

__global__ __launch_bounds__(GB) void k_key_starts(const uint32_t* __restrict__ keys, int64_t n, int64_t nkeys,
                                                   const uint32_t* __restrict__ nkeys_dev, const int32_t* __restrict__ skip,
                                                   int64_t* __restrict__ starts) {
    if (skip && *skip) return;
    if (nkeys_dev && (int64_t)*nkeys_dev < nkeys) nkeys = (int64_t)*nkeys_dev;
    for (int64_t k = (int64_t)blockIdx.x * GB + threadIdx.x; k <= nkeys; k += (int64_t)gridDim.x * GB) {
        int64_t lo = 0, hi = n;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if ((int64_t)keys[mid] < k) lo = mid + 1; else hi = mid;
        }
        starts[k] = lo;
    }
}

}  // namespace

hipError_t f3d_launch_key_starts(const uint32_t* keys, int64_t n, int64_t nkeys, const uint32_t* nkeys_dev, const int32_t* skip,
                                 int64_t* starts, hipStream_t s) {
    const int64_t most = nkeys_dev && n < nkeys ? n : nkeys;             // a count on the device is a number of distinct keys: <= n
    hipLaunchKernelGGL(k_key_starts, dim3(f3d_grid_for(most + 1, GB, 8192)), dim3(GB), 0, s, keys, n, nkeys, nkeys_dev, skip, starts);
    return hipGetLastError();
}

size_t f3d_group_temp_bytes(int64_t n, unsigned bits) {
    size_t tb = 0;
    (void)rocprim::radix_sort_pairs(nullptr, tb, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, (size_t)n, 0u, bits);
    return tb;
}

hipError_t f3d_group_pairs(uint32_t* keys_a, uint32_t* keys_b, uint32_t* vals_a, uint32_t* vals_b, int64_t n, int bits, void* temp,
                           size_t temp_bytes, int64_t nkeys, const uint32_t* nkeys_dev, const int32_t* skip, int64_t* starts,
                           hipStream_t s) {
    F3D_TRY(rocprim::radix_sort_pairs(temp, temp_bytes, keys_a, keys_b, vals_a, vals_b, (size_t)n, 0u, (unsigned)bits, s));
    return f3d_launch_key_starts(keys_b, n, nkeys, nkeys_dev, skip, starts, s);
}
