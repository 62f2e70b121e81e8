// fp32 residuals under a bf16 bucket for the TopK / RandK baselines (SparseState.error_dtype,
// DESIGN.md section 4g) on MI355X (gfx950): three plain HBM streams around the existing fp32
// selects (arctopk_topk_select / arctopk_seg_select / arctopk_randk_select on the fp32 buffer).
//
//   fold     EF14: E := f(g) (+ E)        EF21: D := f(g) - E          whole bucket, 16-B units
//   pack     vals = b(src[idx]);  EF14: E[idx] := src - f(vals)  EF21: E[idx] := fma(d, f(vals), E)
//   decode   EF21: scratch = rank-ordered fp32 sums; gE := fma(d, scratch / ws, gE); out = b(gE)
//
// f = bf16 -> fp32 (exact), b = fp32 -> bf16 as everywhere in the library (cvt_pk_bf16).  The wire,
// the index exchange and EF14's decode are the bf16 path's (sparse_kernels.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "common.h"
#include "mixed_common.h"

namespace {

using arctopk::bf_bits_f;
using arctopk::f_to_bf;
using arctopk::ld_f4_nt;
using arctopk::MeanScale;
using arctopk::st_f4_nt;
using arctopk::u4_t;
using arctopk::vf4_t;

constexpr int kB = ARCTOPK_SPARSE_MAX_BATCH;
constexpr int kUnits = 4;        // 16-B bf16 units (8 elements) per lane per step, loads before stores
constexpr int kStreamGrid = 4096;  // blocks of a whole-bucket stream at most

struct MixedBatch {
    int64_t off[kB];
    int64_t n[kB];
    int64_t k[kB];
    int64_t koff[kB];
};

// the 8 bf16 of a 16-B unit as two fp32 quads
__device__ __forceinline__ void unpack8(u4_t w, vf4_t& a, vf4_t& b) {
    a = vf4_t{__uint_as_float(w.x << 16), __uint_as_float(w.x & 0xFFFF0000u), __uint_as_float(w.y << 16),
              __uint_as_float(w.y & 0xFFFF0000u)};
    b = vf4_t{__uint_as_float(w.z << 16), __uint_as_float(w.z & 0xFFFF0000u), __uint_as_float(w.w << 16),
              __uint_as_float(w.w & 0xFFFF0000u)};
}

// fold modes: E := f(g) | E := f(g) + E | D := f(g) - E
enum : int { FOLD_COPY = 0, FOLD_ADD = 1, FOLD_SUB = 2 };

template <int MODE>
__device__ __forceinline__ float fold1(float g, float e) {
    if constexpr (MODE == FOLD_COPY) return g;
    else if constexpr (MODE == FOLD_ADD) return g + e;
    else return g - e;
}

// 16 B of g and 2 x 16 B of `in` per unit, 2 x 16 B of `out` written (EF14: out == in, element-wise in
// place), nontemporal; kUnits units' loads are issued before the first store.  Block 0 also does
// the numel % 8 elements behind the last unit.
template <int MODE>
__global__ void __launch_bounds__(256) k_fold_units(const u4_t* __restrict__ g, const float* in, float* out,
                                                    int64_t n8, int64_t numel) {
    for (int64_t i = (int64_t)blockIdx.x * 256 * kUnits + threadIdx.x; i < n8;
         i += (int64_t)gridDim.x * 256 * kUnits) {
        u4_t w[kUnits];
        vf4_t a[kUnits], b[kUnits];
#pragma unroll
        for (int u = 0; u < kUnits; ++u) {
            const int64_t j = i + u * 256 < n8 ? i + u * 256 : n8 - 1;
            w[u] = __builtin_nontemporal_load(g + j);
            if constexpr (MODE != FOLD_COPY) {
                a[u] = ld_f4_nt(in + 8 * j);
                b[u] = ld_f4_nt(in + 8 * j + 4);
            }
        }
#pragma unroll
        for (int u = 0; u < kUnits; ++u) {
            const int64_t j = i + u * 256;
            if (j >= n8) continue;
            vf4_t ga, gb;
            unpack8(w[u], ga, gb);
            if constexpr (MODE == FOLD_ADD) ga = ga + a[u], gb = gb + b[u];
            if constexpr (MODE == FOLD_SUB) ga = ga - a[u], gb = gb - b[u];
            st_f4_nt(out + 8 * j, ga);
            st_f4_nt(out + 8 * j + 4, gb);
        }
    }
    const int64_t t = n8 * 8 + threadIdx.x;
    if (blockIdx.x == 0 && t < numel) {
        const uint16_t* gs = reinterpret_cast<const uint16_t*>(g);
        out[t] = fold1<MODE>(bf_bits_f(gs[t]), MODE == FOLD_COPY ? 0.0f : in[t]);
    }
}

// element by element, for pointers that are not 16-B aligned
template <int MODE>
__global__ void __launch_bounds__(256) k_fold_scalar(const uint16_t* __restrict__ g, const float* in, float* out,
                                                     int64_t numel) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < numel; i += (int64_t)gridDim.x * 256)
        out[i] = fold1<MODE>(bf_bits_f(g[i]), MODE == FOLD_COPY ? 0.0f : in[i]);
}

// vals = b(src[idx]) and the residual at the selected elements; an index outside its tensor is
// skipped (vals = 0, E untouched)
template <int EF>
__global__ void __launch_bounds__(256) k_pack(MixedBatch b, const float* src, float* E,
                                              const int32_t* __restrict__ idx, uint16_t* __restrict__ vals,
                                              float decay) {
    const int t = blockIdx.y;
    const int64_t k = b.k[t];
    const int64_t n = b.n[t];
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < k; j += (int64_t)gridDim.x * 256) {
        const int64_t i = idx[b.koff[t] + j];
        if (i < 0 || i >= n) {
            vals[b.koff[t] + j] = 0;
            continue;
        }
        const float x = src[b.off[t] + i];
        const uint16_t v = f_to_bf(x);
        const float fv = bf_bits_f(v);
        vals[b.koff[t] + j] = v;
        if constexpr (EF == ARCTOPK_EF14) E[b.off[t] + i] = x - fv;  // exact: the rounding remainder
        else E[b.off[t] + i] = __fmaf_rn(decay, fv, E[b.off[t] + i]);
    }
}

// one rank's payload into the fp32 sums; indices within a payload are distinct, the ranks' launches
// are ordered by the stream.  FIRST: the sums are zero (0 + v, so a -0 value becomes +0)
template <bool FIRST>
__global__ void __launch_bounds__(256) k_scatter21(MixedBatch b, float* __restrict__ sums,
                                                   const int32_t* __restrict__ idx,
                                                   const uint16_t* __restrict__ vals) {
    const int t = blockIdx.y;
    const int64_t k = b.k[t];
    const int64_t n = b.n[t];
    float* s = sums + b.off[t];
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < k; j += (int64_t)gridDim.x * 256) {
        const int64_t i = idx[b.koff[t] + j];
        if (i < 0 || i >= n) continue;
        const float v = bf_bits_f(vals[b.koff[t] + j]);
        s[i] = (FIRST ? 0.0f : s[i]) + v;
    }
}

__device__ __forceinline__ float final1(float s, float ge, const MeanScale& sc, float decay) {
    return __fmaf_rn(decay, sc(s), ge);
}

// gE := fma(d, sums / ws, gE); out = b(gE): 2 x 16 B of sums and of gE in, 2 x 16 B of gE and 16 B
// of out written per unit
__global__ void __launch_bounds__(256) k_final21_units(u4_t* __restrict__ out, float* __restrict__ gE,
                                                       const float* __restrict__ sums, int64_t n8, int64_t numel,
                                                       MeanScale sc, float decay) {
    for (int64_t i = (int64_t)blockIdx.x * 256 * kUnits + threadIdx.x; i < n8;
         i += (int64_t)gridDim.x * 256 * kUnits) {
        vf4_t s0[kUnits], s1[kUnits], g0[kUnits], g1[kUnits];
#pragma unroll
        for (int u = 0; u < kUnits; ++u) {
            const int64_t j = i + u * 256 < n8 ? i + u * 256 : n8 - 1;
            s0[u] = ld_f4_nt(sums + 8 * j);
            s1[u] = ld_f4_nt(sums + 8 * j + 4);
            g0[u] = ld_f4_nt(gE + 8 * j);
            g1[u] = ld_f4_nt(gE + 8 * j + 4);
        }
#pragma unroll
        for (int u = 0; u < kUnits; ++u) {
            const int64_t j = i + u * 256;
            if (j >= n8) continue;
            vf4_t a, b;
            a.x = final1(s0[u].x, g0[u].x, sc, decay), a.y = final1(s0[u].y, g0[u].y, sc, decay);
            a.z = final1(s0[u].z, g0[u].z, sc, decay), a.w = final1(s0[u].w, g0[u].w, sc, decay);
            b.x = final1(s1[u].x, g1[u].x, sc, decay), b.y = final1(s1[u].y, g1[u].y, sc, decay);
            b.z = final1(s1[u].z, g1[u].z, sc, decay), b.w = final1(s1[u].w, g1[u].w, sc, decay);
            st_f4_nt(gE + 8 * j, a);
            st_f4_nt(gE + 8 * j + 4, b);
            __builtin_nontemporal_store(u4_t{arctopk::cvt_pk_bf16(a.x, a.y), arctopk::cvt_pk_bf16(a.z, a.w),
                                             arctopk::cvt_pk_bf16(b.x, b.y), arctopk::cvt_pk_bf16(b.z, b.w)},
                                        out + j);
        }
    }
    const int64_t t = n8 * 8 + threadIdx.x;
    if (blockIdx.x == 0 && t < numel) {
        const float v = final1(sums[t], gE[t], sc, decay);
        gE[t] = v;
        reinterpret_cast<uint16_t*>(out)[t] = f_to_bf(v);
    }
}

__global__ void __launch_bounds__(256) k_final21_scalar(uint16_t* __restrict__ out, float* __restrict__ gE,
                                                        const float* __restrict__ sums, int64_t numel,
                                                        MeanScale sc, float decay) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < numel; i += (int64_t)gridDim.x * 256) {
        const float v = final1(sums[i], gE[i], sc, decay);
        gE[i] = v;
        out[i] = f_to_bf(v);
    }
}

inline int stream_grid(int64_t work_items, int per_block) {
    return (int)std::max<int64_t>(1, std::min<int64_t>(kStreamGrid, (work_items + per_block - 1) / per_block));
}

// Tensor `first + i`'s extent is offsets[next] - offsets[this] (the last one's ends at numel): the
// tensors tile [offsets[0], numel) in order.  EINVAL for anything else, or a k outside [1, extent].
int fill_batch(MixedBatch& b, int32_t first, int32_t count, int32_t nt, int64_t numel, const int64_t* offsets,
               const int64_t* ks, const int64_t* k_off, int64_t& maxk) {
    maxk = 0;
    for (int i = 0; i < count; ++i) {
        const int32_t t = first + i;
        const int64_t end = t + 1 < nt ? offsets[t + 1] : numel;
        b.off[i] = offsets[t];
        b.n[i] = end - offsets[t];
        b.k[i] = ks[t];
        b.koff[i] = k_off[t];
        if (offsets[t] < 0 || end > numel || b.n[i] < 1 || b.n[i] >= (1ll << 31)) return ARCTOPK_EINVAL;
        if (b.k[i] < 1 || b.k[i] > b.n[i] || b.koff[i] < 0) return ARCTOPK_EINVAL;
        maxk = std::max(maxk, b.k[i]);
    }
    return 0;
}

inline int gather_grid(int64_t maxk) { return (int)std::max<int64_t>(1, std::min<int64_t>(2048, (maxk + 255) / 256)); }

}  // namespace

extern "C" int arctopk_sparse_fold_mixed(const void* g, void* E, void* D, int64_t numel, int32_t ef, int32_t err_in,
                                         void* stream) {
    if (!g || !E || numel < 0 || (ef != ARCTOPK_EF14 && ef != ARCTOPK_EF21)) return ARCTOPK_EINVAL;
    if (ef == ARCTOPK_EF21 && !D) return ARCTOPK_EINVAL;
    if (arctopk::low_bits(g, 1) || arctopk::low_bits(E, 3) || arctopk::low_bits(D, 3)) return ARCTOPK_EINVAL;
    if (numel == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const float* in = static_cast<const float*>(E);
    float* out = ef == ARCTOPK_EF14 ? static_cast<float*>(E) : static_cast<float*>(D);
    const int mode = ef == ARCTOPK_EF21 ? FOLD_SUB : err_in ? FOLD_ADD : FOLD_COPY;
    const bool units = !arctopk::low_bits(g, 15) && !arctopk::low_bits(in, 15) && !arctopk::low_bits(out, 15) &&
                       numel >= 8;
    if (units) {
        const int64_t n8 = numel / 8;
        const u4_t* g4 = static_cast<const u4_t*>(g);
        const dim3 grid(stream_grid(n8, 256 * kUnits));
        if (mode == FOLD_COPY) hipLaunchKernelGGL(k_fold_units<FOLD_COPY>, grid, dim3(256), 0, st, g4, in, out, n8, numel);
        else if (mode == FOLD_ADD) hipLaunchKernelGGL(k_fold_units<FOLD_ADD>, grid, dim3(256), 0, st, g4, in, out, n8, numel);
        else hipLaunchKernelGGL(k_fold_units<FOLD_SUB>, grid, dim3(256), 0, st, g4, in, out, n8, numel);
    } else {
        const uint16_t* g1 = static_cast<const uint16_t*>(g);
        const dim3 grid(stream_grid(numel, 256));
        if (mode == FOLD_COPY) hipLaunchKernelGGL(k_fold_scalar<FOLD_COPY>, grid, dim3(256), 0, st, g1, in, out, numel);
        else if (mode == FOLD_ADD) hipLaunchKernelGGL(k_fold_scalar<FOLD_ADD>, grid, dim3(256), 0, st, g1, in, out, numel);
        else hipLaunchKernelGGL(k_fold_scalar<FOLD_SUB>, grid, dim3(256), 0, st, g1, in, out, numel);
    }
    return (int)hipGetLastError();
}

extern "C" int arctopk_sparse_pack_mixed(const void* src, void* E, int64_t numel, int32_t nt, const int64_t* offsets,
                                         const int64_t* ks, const int64_t* k_off, const int32_t* idx, void* vals,
                                         int32_t ef, float decay, void* stream) {
    if (!src || !E || !offsets || !ks || !k_off || !idx || !vals || nt < 1 || numel < 1) return ARCTOPK_EINVAL;
    if (ef != ARCTOPK_EF14 && ef != ARCTOPK_EF21) return ARCTOPK_EINVAL;
    if (ef == ARCTOPK_EF14 && src != E) return ARCTOPK_EINVAL;
    if (arctopk::low_bits(src, 3) || arctopk::low_bits(E, 3) || arctopk::low_bits(vals, 1)) return ARCTOPK_EINVAL;
    // every batch is checked before the first launch: nothing is enqueued for a bad layout
    std::vector<MixedBatch> batches((nt + kB - 1) / kB);
    std::vector<int64_t> maxk(batches.size());
    for (int32_t first = 0, q = 0; first < nt; first += kB, ++q) {
        const int e = fill_batch(batches[q], first, std::min<int32_t>(kB, nt - first), nt, numel, offsets, ks, k_off,
                                 maxk[q]);
        if (e) return e;
    }
    hipStream_t st = (hipStream_t)stream;
    const float* s = static_cast<const float*>(src);
    float* Ef = static_cast<float*>(E);
    uint16_t* v = static_cast<uint16_t*>(vals);
    for (int32_t first = 0, q = 0; first < nt; first += kB, ++q) {
        const dim3 grid(gather_grid(maxk[q]), std::min<int32_t>(kB, nt - first));
        if (ef == ARCTOPK_EF14)
            hipLaunchKernelGGL(k_pack<ARCTOPK_EF14>, grid, dim3(256), 0, st, batches[q], s, Ef, idx, v, decay);
        else
            hipLaunchKernelGGL(k_pack<ARCTOPK_EF21>, grid, dim3(256), 0, st, batches[q], s, Ef, idx, v, decay);
        const int e = (int)hipGetLastError();
        if (e) return e;
    }
    return 0;
}

extern "C" int arctopk_sparse_decode_mixed21(void* out, void* gE, void* scratch, int64_t numel, int32_t nt,
                                             const int64_t* offsets, const int64_t* ks, const int64_t* k_off,
                                             int64_t packed_len, const int32_t* idx, const void* vals, int32_t nranks,
                                             int32_t world_size, float decay, void* stream) {
    if (!out || !gE || !scratch || !offsets || !ks || !k_off || !idx || !vals || nt < 1 || nranks < 1 ||
        world_size < 1 || numel < 1 || packed_len < 0)
        return ARCTOPK_EINVAL;
    if (arctopk::low_bits(out, 1) || arctopk::low_bits(gE, 3) || arctopk::low_bits(scratch, 3) ||
        arctopk::low_bits(vals, 1))
        return ARCTOPK_EINVAL;
    std::vector<MixedBatch> batches((nt + kB - 1) / kB);
    std::vector<int64_t> maxk(batches.size());
    for (int32_t first = 0, q = 0; first < nt; first += kB, ++q) {
        const int e = fill_batch(batches[q], first, std::min<int32_t>(kB, nt - first), nt, numel, offsets, ks, k_off,
                                 maxk[q]);
        if (e) return e;
        for (int i = 0; i < std::min<int32_t>(kB, nt - first); ++i)
            if (batches[q].koff[i] + batches[q].k[i] > packed_len) return ARCTOPK_EINVAL;
    }
    hipStream_t st = (hipStream_t)stream;
    float* sums = static_cast<float*>(scratch);
    float* ge = static_cast<float*>(gE);
    hipError_t he = hipMemsetAsync(sums, 0, (size_t)numel * sizeof(float), st);
    if (he != hipSuccess) return (int)he;
    for (int32_t r = 0; r < nranks; ++r) {
        const int32_t* ir = idx + (int64_t)r * packed_len;
        const uint16_t* vr = static_cast<const uint16_t*>(vals) + (int64_t)r * packed_len;
        for (int32_t first = 0, q = 0; first < nt; first += kB, ++q) {
            const dim3 grid(gather_grid(maxk[q]), std::min<int32_t>(kB, nt - first));
            if (r == 0) hipLaunchKernelGGL(k_scatter21<true>, grid, dim3(256), 0, st, batches[q], sums, ir, vr);
            else hipLaunchKernelGGL(k_scatter21<false>, grid, dim3(256), 0, st, batches[q], sums, ir, vr);
            const int e = (int)hipGetLastError();
            if (e) return e;
        }
    }
    const MeanScale sc = arctopk::make_mean_scale(world_size);
    if (!arctopk::low_bits(out, 15) && !arctopk::low_bits(gE, 15) && !arctopk::low_bits(scratch, 15) && numel >= 8) {
        const int64_t n8 = numel / 8;
        hipLaunchKernelGGL(k_final21_units, dim3(stream_grid(n8, 256 * kUnits)), dim3(256), 0, st,
                           static_cast<u4_t*>(out), ge, sums, n8, numel, sc, decay);
    } else {
        hipLaunchKernelGGL(k_final21_scalar, dim3(stream_grid(numel, 256)), dim3(256), 0, st,
                           static_cast<uint16_t*>(out), ge, sums, numel, sc, decay);
    }
    return (int)hipGetLastError();
}
