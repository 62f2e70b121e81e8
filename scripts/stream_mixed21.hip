// Plain-stream ceilings for the byte patterns of the EF21 fp32-residual kernels (DESIGN.md section
// 4e) on one MI355X, per 8 elements, nontemporal, flat grid-stride, scripts/stream_bench.hip's
// "cold" method (every launch on the next of `sets` disjoint sets of arrays):
//   r6   : read 16 B of a bf16 array and 2 x 16 B of an fp32 array, write nothing (the encode: 6 B
//          per element; the sum is kept alive by a store no thread reaches)
//   rw12 : read both, write both back (the pack, and the decode on selected rows: 12 B per element)
//   r4w2 : read the fp32 array, write the bf16 one (the decode on unselected rows: 6 B per element)
//   hipcc --offload-arch=gfx950 -O3 scripts/stream_mixed21.hip -o scripts/stream_mixed21
//   ./scripts/stream_mixed21 [Mi elements per array] [sets]
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
typedef __bf16 bf2 __attribute__((ext_vector_type(2)));
typedef float f2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ unsigned pk(float a, float b) {
    return __builtin_bit_cast(unsigned, __builtin_convertvector(f2{a, b}, bf2));
}

enum { R6 = 0, RW12 = 1, R4W2 = 2 };

template <int MODE, int U>
__global__ void __launch_bounds__(256) k_stream(v4u* __restrict__ g, v4f* __restrict__ e, size_t n8, float never) {
    float sink = 0.f;
    for (size_t i = (size_t)blockIdx.x * 256 * U + threadIdx.x; i < n8; i += (size_t)gridDim.x * 256 * U) {
        v4u w[U];
        v4f a[U], b[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const size_t j = i + u * 256 < n8 ? i + u * 256 : n8 - 1;
            if (MODE != R4W2) w[u] = __builtin_nontemporal_load(g + j);
            a[u] = __builtin_nontemporal_load(e + 2 * j);
            b[u] = __builtin_nontemporal_load(e + 2 * j + 1);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (i + u * 256 >= n8) continue;
            const size_t j = i + u * 256;
            if (MODE != R4W2) {
                a[u].x -= __uint_as_float(w[u].x << 16), a[u].y -= __uint_as_float(w[u].x & 0xFFFF0000u);
                a[u].z -= __uint_as_float(w[u].y << 16), a[u].w -= __uint_as_float(w[u].y & 0xFFFF0000u);
                b[u].x -= __uint_as_float(w[u].z << 16), b[u].y -= __uint_as_float(w[u].z & 0xFFFF0000u);
                b[u].z -= __uint_as_float(w[u].w << 16), b[u].w -= __uint_as_float(w[u].w & 0xFFFF0000u);
            }
            if (MODE == R6) {
                sink += a[u].x + a[u].y + a[u].z + a[u].w + b[u].x + b[u].y + b[u].z + b[u].w;
                continue;
            }
            if (MODE == RW12) {
                __builtin_nontemporal_store(a[u], e + 2 * j);
                __builtin_nontemporal_store(b[u], e + 2 * j + 1);
            }
            __builtin_nontemporal_store(v4u{pk(a[u].x, a[u].y), pk(a[u].z, a[u].w), pk(b[u].x, b[u].y), pk(b[u].z, b[u].w)},
                                        g + j);
        }
    }
    if (MODE == R6 && sink == never) e[0].x = sink;  // (never: the arrays hold zeros, `never` is not 0)
}

template <int MODE>
void run(const char* name, double bytes_per_el, std::vector<void*>& G, std::vector<void*>& E, size_t n, int sets,
         hipEvent_t e0, hipEvent_t e1) {
    const size_t n8 = n / 8;
    for (unsigned grid : {2048u, 4096u, 8192u, 16384u}) {
        std::vector<float> us;
        for (int it = 0; it < 24; ++it) {
            const int s = it % sets;
            CK(hipEventRecord(e0, nullptr));
            hipLaunchKernelGGL((k_stream<MODE, 4>), dim3(grid), dim3(256), 0, nullptr, (v4u*)G[s], (v4f*)E[s], n8, 1.5f);
            CK(hipEventRecord(e1, nullptr));
            CK(hipEventSynchronize(e1));
            float ms = 0;
            CK(hipEventElapsedTime(&ms, e0, e1));
            if (it >= 4) us.push_back(ms * 1e3f);
        }
        std::sort(us.begin(), us.end());
        const float med = us[us.size() / 2];
        std::printf("%-5s cold grid %6u: %5.0f GB/s  %6.1f us (min %.1f, max %.1f)\n", name, grid,
                    n * bytes_per_el / med / 1e3, med, us.front(), us.back());
    }
}

int main(int argc, char** argv) {
    const size_t mi = argc > 1 ? (size_t)std::atoll(argv[1]) : 64;
    const int sets = argc > 2 ? std::atoi(argv[2]) : 4;
    const size_t n = mi << 20;
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
    std::printf("%zu Mi elements per array (bf16 and fp32), %d sets, cold\n", mi, sets);
    run<R6>("r6", 6.0, G, E, n, sets, e0, e1);
    run<RW12>("rw12", 12.0, G, E, n, sets, e0, e1);
    run<R4W2>("r4w2", 6.0, G, E, n, sets, e0, e1);
    for (int s = 0; s < sets; ++s) {
        CK(hipFree(G[s]));
        CK(hipFree(E[s]));
    }
    return 0;
}
