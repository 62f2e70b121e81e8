// Plain-stream ceilings for the byte patterns of arctopk_pack_wire16 and arctopk_decode_wire16 on
// one MI355X, per 4 elements, nontemporal, flat grid-stride -- scripts/stream_bench.hip's "cold"
// method (every launch on the next of `sets` disjoint sets of arrays, so no launch finds its data
// in the Infinity Cache):
//   rw8w2  : 16 B of an fp32 array read and written back, 8 B of bf16 written (the EF14 pack: 10 B
//            per element)
//   r4rw8w2: 16 B of a second fp32 array read as well (the EF21 pack: 14 B per element)
//   w4r2   : 16 B of fp32 written for every unit, 8 B of bf16 read for one unit in five (the noef /
//            EF14 decode at ratio 0.2: 4 N + 2 K bytes)
//   r2w4   : 8 B of bf16 read and 16 B of fp32 written for the first fifth of the units, contiguous
//            (the zero-ahead scatter at ratio 0.2, arctopk_decode_wire16_scatter: 6 K bytes)
//   hipcc --offload-arch=gfx950 -O3 scripts/stream_wire16.hip -o scripts/stream_wire16
//   ./scripts/stream_wire16 [Mi elements per array] [sets]
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CK(x)                                                                              \
    do {                                                                                   \
        hipError_t e_ = (x);                                                               \
        if (e_ != hipSuccess) {                                                            \
            std::printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); \
            std::exit(1);                                                                  \
        }                                                                                  \
    } while (0)

typedef float v4f __attribute__((ext_vector_type(4)));
typedef unsigned int v2u __attribute__((ext_vector_type(2)));

__device__ __forceinline__ v2u to_bf4(v4f a) {  // (truncation: the stream's bytes, not the codec's rounding)
    return v2u{(__float_as_uint(a.x) >> 16) | (__float_as_uint(a.y) & 0xFFFF0000u),
               (__float_as_uint(a.z) >> 16) | (__float_as_uint(a.w) & 0xFFFF0000u)};
}

template <bool G>
__global__ void __launch_bounds__(256) k_pack(const v4f* __restrict__ g, v4f* __restrict__ e, v2u* __restrict__ p,
                                              size_t n4) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        v4f a = __builtin_nontemporal_load(e + i);
        if constexpr (G) {
            const v4f b = __builtin_nontemporal_load(g + i);
            a = v4f{b.x - a.x, b.y - a.y, b.z - a.z, b.w - a.w};
        }
        const v2u w = to_bf4(a);
        __builtin_nontemporal_store(w, p + i);
        __builtin_nontemporal_store(v4f{a.x - __uint_as_float(w.x << 16), a.y - __uint_as_float(w.x & 0xFFFF0000u),
                                        a.z - __uint_as_float(w.y << 16), a.w - __uint_as_float(w.y & 0xFFFF0000u)},
                                    e + i);
    }
}

__global__ void __launch_bounds__(256) k_decode(const v2u* __restrict__ p, v4f* __restrict__ out, size_t n4) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        v4f o = v4f{0.0f, 0.0f, 0.0f, 0.0f};
        if ((i / 512) % 5 == 0) {  // one run of 512 units (a 2048-element row) in five is "selected"
            const v2u w = __builtin_nontemporal_load(p + (i / 2560) * 512 + i % 512);
            o = v4f{__uint_as_float(w.x << 16), __uint_as_float(w.x & 0xFFFF0000u), __uint_as_float(w.y << 16),
                    __uint_as_float(w.y & 0xFFFF0000u)};
        }
        __builtin_nontemporal_store(o, out + i);
    }
}

__global__ void __launch_bounds__(256) k_scatter(const v2u* __restrict__ p, v4f* __restrict__ out, size_t k4) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < k4; i += (size_t)gridDim.x * 256) {
        const v2u w = __builtin_nontemporal_load(p + i);
        __builtin_nontemporal_store(v4f{__uint_as_float(w.x << 16), __uint_as_float(w.x & 0xFFFF0000u),
                                        __uint_as_float(w.y << 16), __uint_as_float(w.y & 0xFFFF0000u)},
                                    out + i);
    }
}

int main(int argc, char** argv) {
    const size_t mi = argc > 1 ? (size_t)std::atoll(argv[1]) : 64;
    const int sets = argc > 2 ? std::atoi(argv[2]) : 4;
    const size_t n = mi << 20, n4 = n / 4;
    std::vector<void*> G(sets), E(sets), P(sets);
    for (int s = 0; s < sets; ++s) {
        CK(hipMalloc(&G[s], n * 4));
        CK(hipMalloc(&E[s], n * 4));
        CK(hipMalloc(&P[s], n * 2));
        CK(hipMemset(G[s], 0, n * 4));
        CK(hipMemset(E[s], 0, n * 4));
        CK(hipMemset(P[s], 0, n * 2));
    }
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    std::printf("%zu Mi elements per array, %d sets, cold\n", mi, sets);
    const char* names[4] = {"rw8w2", "r4rw8w2", "w4r2", "r2w4"};
    const double bytes[4] = {n * 10.0, n * 14.0, n * 4.0 + (n / 5) * 2.0, (n / 5) * 6.0};
    for (int pat = 0; pat < 4; ++pat) {
        for (unsigned grid : {2048u, 4096u, 8192u, 16384u}) {
            std::vector<float> us;
            for (int it = 0; it < 24; ++it) {
                const int s = it % sets;
                CK(hipEventRecord(e0, nullptr));
                if (pat == 0)
                    hipLaunchKernelGGL(k_pack<false>, dim3(grid), dim3(256), 0, nullptr, (const v4f*)G[s], (v4f*)E[s],
                                       (v2u*)P[s], n4);
                else if (pat == 1)
                    hipLaunchKernelGGL(k_pack<true>, dim3(grid), dim3(256), 0, nullptr, (const v4f*)G[s], (v4f*)E[s],
                                       (v2u*)P[s], n4);
                else if (pat == 2)
                    hipLaunchKernelGGL(k_decode, dim3(grid), dim3(256), 0, nullptr, (const v2u*)P[s], (v4f*)E[s], n4);
                else
                    hipLaunchKernelGGL(k_scatter, dim3(grid), dim3(256), 0, nullptr, (const v2u*)P[s], (v4f*)E[s],
                                       n4 / 5);
                CK(hipEventRecord(e1, nullptr));
                CK(hipEventSynchronize(e1));
                float ms = 0;
                CK(hipEventElapsedTime(&ms, e0, e1));
                if (it >= 4) us.push_back(ms * 1e3f);
            }
            std::sort(us.begin(), us.end());
            const float med = us[us.size() / 2];
            std::printf("%-8s cold grid %6u: %5.0f GB/s  %6.1f us (min %.1f, max %.1f)\n", names[pat], grid,
                        bytes[pat] / med / 1e3, med, us.front(), us.back());
        }
    }
    for (int s = 0; s < sets; ++s) {
        CK(hipFree(G[s]));
        CK(hipFree(E[s]));
        CK(hipFree(P[s]));
    }
    return 0;
}
