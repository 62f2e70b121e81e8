// What sparse_kernels.hip and sparse_mixed.hip share on the device.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace arctopk {

// first position in a[lo, hi) with a[p] >= target (a ascending), one wave
__device__ __forceinline__ int64_t wave_lower_bound(const int32_t* __restrict__ a, int64_t lo, int64_t hi,
                                                    int32_t target) {
    const int lane = threadIdx.x & 63;
    while (hi - lo > 64) {
        const int64_t step = (hi - lo + 63) / 64;
        const int64_t p = lo + (int64_t)lane * step;
        const bool pred = p < hi && a[p] < target;
        const int c = __popcll(__ballot(pred));
        if (c == 0) return lo;
        const int64_t nlo = lo + (int64_t)(c - 1) * step + 1;
        const int64_t phi = lo + (int64_t)c * step;
        hi = phi < hi ? phi : hi;
        lo = nlo;
    }
    const int64_t p = lo + lane;
    return lo + __popcll(__ballot(p < hi && a[p] < target));
}

}  // namespace arctopk
