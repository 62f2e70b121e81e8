// Plain-stream ceiling for the byte pattern of arctopk_encode_mixed on one MI355X: per 8 elements
// read 16 B of a bf16 array and 2 x 16 B of an fp32 array, write the 2 x 16 B back in place
// (E := f(G) + E; 10 B per element), nontemporal, flat grid-stride -- scripts/stream_bench.hip's
// "cold" method (every launch on the next of `sets` disjoint sets of arrays, so no launch finds its
// data in the Infinity Cache) for a mix that program does not have.
//   hipcc --offload-arch=gfx950 -O3 scripts/stream_mixed.hip -o scripts/stream_mixed
//   ./scripts/stream_mixed [Mi elements per array] [sets]
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
typedef unsigned int v4u __attribute__((ext_vector_type(4)));

template <int U>
__global__ void __launch_bounds__(256) k_mixed(const v4u* __restrict__ g, v4f* __restrict__ e, size_t n8) {
    for (size_t i = (size_t)blockIdx.x * 256 * U + threadIdx.x; i < n8; i += (size_t)gridDim.x * 256 * U) {
        v4u w[U];
        v4f a[U], b[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const size_t j = i + u * 256 < n8 ? i + u * 256 : n8 - 1;
            w[u] = __builtin_nontemporal_load(g + j);
            a[u] = __builtin_nontemporal_load(e + 2 * j);
            b[u] = __builtin_nontemporal_load(e + 2 * j + 1);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (i + u * 256 >= n8) continue;
            const size_t j = i + u * 256;
            a[u].x += __uint_as_float(w[u].x << 16), a[u].y += __uint_as_float(w[u].x & 0xFFFF0000u);
            a[u].z += __uint_as_float(w[u].y << 16), a[u].w += __uint_as_float(w[u].y & 0xFFFF0000u);
            b[u].x += __uint_as_float(w[u].z << 16), b[u].y += __uint_as_float(w[u].z & 0xFFFF0000u);
            b[u].z += __uint_as_float(w[u].w << 16), b[u].w += __uint_as_float(w[u].w & 0xFFFF0000u);
            __builtin_nontemporal_store(a[u], e + 2 * j);
            __builtin_nontemporal_store(b[u], e + 2 * j + 1);
        }
    }
}

int main(int argc, char** argv) {
    const size_t mi = argc > 1 ? (size_t)std::atoll(argv[1]) : 64;
    const int sets = argc > 2 ? std::atoi(argv[2]) : 4;
    const size_t n = mi << 20, n8 = n / 8;
    std::vector<void*> G(sets), E(sets);
    for (int s = 0; s < sets; ++s) {
        CK(hipMalloc(&G[s], n * 2));
        CK(hipMalloc(&E[s], n * 4));
        CK(hipMemset(G[s], 0, n * 2));
        CK(hipMemset(E[s], 0, n * 4));
    }
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    std::printf("%zu Mi elements per array (bf16 read + fp32 read + fp32 write, 10 B each), %d sets, cold\n", mi, sets);
    for (unsigned grid : {1024u, 2048u, 4096u, 8192u, 16384u}) {
        std::vector<float> us;
        for (int it = 0; it < 24; ++it) {
            const int s = it % sets;
            CK(hipEventRecord(e0, nullptr));
            hipLaunchKernelGGL(k_mixed<4>, dim3(grid), dim3(256), 0, nullptr, (const v4u*)G[s], (v4f*)E[s], n8);
            CK(hipEventRecord(e1, nullptr));
            CK(hipEventSynchronize(e1));
            float ms = 0;
            CK(hipEventElapsedTime(&ms, e0, e1));
            if (it >= 4) us.push_back(ms * 1e3f);
        }
        std::sort(us.begin(), us.end());
        const float med = us[us.size() / 2];
        std::printf("cold grid %6u: %5.0f GB/s  %6.1f us (min %.1f, max %.1f)\n", grid, n * 10.0 / med / 1e3, med,
                    us.front(), us.back());
    }
    for (int s = 0; s < sets; ++s) {
        CK(hipFree(G[s]));
        CK(hipFree(E[s]));
    }
    return 0;
}
