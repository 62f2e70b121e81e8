// The two mixed-precision options of the TopK / RandK baselines on MI355X (gfx950), around the
// existing fp32 selects (arctopk_topk_select / arctopk_seg_select / arctopk_randk_select):
//
// fp32 residuals under a bf16 bucket (SparseState.error_dtype)
//   fold     EF14: E := f(g) (+ E)        EF21: D := f(g) - E          whole bucket, 16-B units
//   pack     vals = b(src[idx]) and the residual at the selected elements (below)
//   decode   EF21: scratch = rank-ordered fp32 sums; gE := fma(d, scratch / ws, gE); out = b(gE)
//            (the wire, the index exchange and EF14's decode are the bf16 path's, sparse_kernels.hip)
//
// bf16 values on the wire for an fp32 bucket (SparseState.wire_dtype); fold and
// selection are the fp32 path's
//   pack     vals16 = b(v) from the selects' contiguous fp32 values, and the residual
//   decode   s = rank-ordered fp32 sum of f(vals16) from 0; m = s / ws; out = m, or under EF21
//            gE := fma(d, m, gE), out = gE
//            merged    every tensor's indices ascend: a block composes a 4096-element chunk from all
//                      ranks' slices in LDS, applies mean and gE and writes it once
//            scattered any index order: memset, one scatter per rank, one finalize pass
//
// The pack rule of both (pack1): bits = b(x); EF14: E[i] := x - f(bits), the remainder of the
// rounding; EF21: E[i] := fma(d, f(bits), E[i]).  f = bf16 -> fp32 (exact), b = fp32 -> bf16 as
// everywhere in the library (cvt_pk_bf16).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "common.h"
#include "mixed_common.h"
#include "sparse_common.h"

namespace {

using arctopk::bf_bits_f;
using arctopk::f_to_bf;
using arctopk::ld_f4_nt;
using arctopk::MeanScale;
using arctopk::st_f4_nt;
using arctopk::u4_t;
using arctopk::vf4_t;
using arctopk::wave_lower_bound;

constexpr int kB = ARCTOPK_SPARSE_MAX_BATCH;
constexpr int kChunk = 4096;       // elements of a tensor a merged-decode block composes in LDS
constexpr int kUnits = 4;          // 16-B units per lane per step, loads before stores
constexpr int kStreamGrid = 4096;  // blocks of a whole-bucket stream at most

typedef int32_t vi4_t __attribute__((ext_vector_type(4)));
typedef uint32_t vu2_t __attribute__((ext_vector_type(2)));

struct MixedBatch {
    int64_t off[kB];
    int64_t n[kB];
    int64_t k[kB];
    int64_t koff[kB];
};

// ---- fold (error_dtype) --------------------------------------------------------------------
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

// ---- pack ----------------------------------------------------------------------------------
// one selected element: the bf16 bits of v and its residual (e: EF21's E[i], read by the caller); an
// index outside the tensor writes a zero value and nothing else
template <int EF>
__device__ __forceinline__ uint32_t pack1(float v, int64_t i, int64_t n, float e, float* Et, float decay) {
    if (i < 0 || i >= n) return 0u;
    const uint32_t bits = f_to_bf(v);
    const float fv = bf_bits_f(bits);
    if constexpr (EF == ARCTOPK_EF14) Et[i] = v - fv;  // exact: the rounding remainder
    if constexpr (EF == ARCTOPK_EF21) Et[i] = __fmaf_rn(decay, fv, e);
    return bits;
}

// error_dtype: the values are gathered from src (EF14: src == E) at indices inside the tensor
template <int EF>
__global__ void __launch_bounds__(256) k_pack(MixedBatch b, const float* src, float* E,
                                              const int32_t* __restrict__ idx, uint16_t* __restrict__ vals,
                                              float decay) {
    const int t = blockIdx.y;
    const int64_t k = b.k[t];
    const int64_t n = b.n[t];
    float* Et = E + b.off[t];
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < k; j += (int64_t)gridDim.x * 256) {
        const int64_t i = idx[b.koff[t] + j];
        float x = 0.f, e = 0.f;
        if (i >= 0 && i < n) {
            x = src[b.off[t] + i];
            if constexpr (EF == ARCTOPK_EF21) e = Et[i];
        }
        vals[b.koff[t] + j] = (uint16_t)pack1<EF>(x, i, n, e, Et, decay);
    }
}

// wire_dtype: tensor blockIdx.y's k values: 16 B of indices and of values in, 8 B of vals16 out per
// unit of 4 where the tensor's slice of the payload is 16-B aligned (aligned16: the three payload
// pointers are, so koff % 4 == 0 decides), nontemporal, the unit's loads (EF21: its four E reads too)
// before its stores; the k % 4 elements behind the last unit, or every element otherwise, one by one.
template <int EF>
__global__ void __launch_bounds__(256) k_pack16(MixedBatch b, const float* __restrict__ v, float* E,
                                                const int32_t* __restrict__ idx, uint16_t* __restrict__ vals16,
                                                float decay, int aligned16) {
    const int t = blockIdx.y;
    const int64_t k = b.k[t];
    const int64_t n = b.n[t];
    const int64_t ko = b.koff[t];
    float* Et = EF == ARCTOPK_EF_NONE ? nullptr : E + b.off[t];
    const int64_t k4 = aligned16 && (ko & 3) == 0 ? k / 4 : 0;
    for (int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x; u < k4; u += (int64_t)gridDim.x * 256) {
        const vi4_t i4 = __builtin_nontemporal_load(reinterpret_cast<const vi4_t*>(idx + ko) + u);
        const vf4_t x4 = ld_f4_nt(v + ko + 4 * u);
        float e[4] = {0.f, 0.f, 0.f, 0.f};
        if constexpr (EF == ARCTOPK_EF21) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (i4[q] >= 0 && i4[q] < n) e[q] = Et[i4[q]];
        }
        uint32_t w[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) w[q] = pack1<EF>(x4[q], i4[q], n, e[q], Et, decay);
        __builtin_nontemporal_store(vu2_t{w[0] | (w[1] << 16), w[2] | (w[3] << 16)},
                                    reinterpret_cast<vu2_t*>(vals16 + ko) + u);
    }
    for (int64_t j = k4 * 4 + (int64_t)blockIdx.x * 256 + threadIdx.x; j < k; j += (int64_t)gridDim.x * 256) {
        const int64_t i = idx[ko + j];
        float e = 0.f;
        if constexpr (EF == ARCTOPK_EF21)
            if (i >= 0 && i < n) e = Et[i];
        vals16[ko + j] = (uint16_t)pack1<EF>(v[ko + j], i, n, e, Et, decay);
    }
}

// ---- decode --------------------------------------------------------------------------------
// the mean of the sums, and under GE the new gE
template <bool GE>
__device__ __forceinline__ float final1(float s, float ge, const MeanScale& sc, float decay) {
    const float m = sc(s);
    return GE ? __fmaf_rn(decay, m, ge) : m;
}

// wire_dtype, merged: block (x, y) composes elements [4096 x, 4096 (x + 1)) of tensor y: the chunk
// starts as zeros in LDS; for each rank in order, waves 0 and 1 find the rank's slice of (ascending)
// indices that fall in the chunk and the block adds the slice's values at their places.  Indices
// within a payload are distinct, so the barrier between two ranks (which also publishes the next
// slice's bounds, kept in alternating slots) is the only ordering the sums need.  Then mean and gE,
// and the chunk is written once: 16-B nontemporal units between a scalar head up to the first 16-B
// boundary of `out` and a scalar tail, a step's gE loads before its stores.  An index outside the
// chunk -- a payload that does not ascend, or one outside the tensor -- is skipped.
template <bool GE>
__global__ void __launch_bounds__(256) k_decode_merged(MixedBatch b, float* __restrict__ out, float* __restrict__ gE,
                                                       const int32_t* __restrict__ idx,
                                                       const uint16_t* __restrict__ vals16, int nranks,
                                                       int64_t packed_len, MeanScale sc, float decay) {
    __shared__ __attribute__((aligned(16))) float lds[kChunk + 4];
    __shared__ int64_t s_lb[2][2];
    const int t = blockIdx.y;
    const int64_t n = b.n[t];
    const int64_t c0 = (int64_t)blockIdx.x * kChunk;
    if (c0 >= n) return;
    const int64_t c1 = min<int64_t>(n, c0 + kChunk);
    const int len = (int)(c1 - c0);
    const int wave = threadIdx.x >> 6;
    float* o = out + b.off[t] + c0;
    float* g = GE ? gE + b.off[t] + c0 : nullptr;
    // the chunk sits in LDS at o's offset within 16 B, so its 16-B units are the bucket's
    float* chunk = lds + (((uintptr_t)o & 15) >> 2);
#pragma unroll
    for (int u = 0; u < kChunk / 4 / 256; ++u)
        reinterpret_cast<vf4_t*>(lds)[threadIdx.x + u * 256] = vf4_t{0.f, 0.f, 0.f, 0.f};
    if (threadIdx.x < 4) lds[kChunk + threadIdx.x] = 0.f;
    for (int r = 0; r < nranks; ++r) {
        const int32_t* it = idx + (int64_t)r * packed_len + b.koff[t];
        const uint16_t* vt = vals16 + (int64_t)r * packed_len + b.koff[t];
        if (wave < 2) {
            const int64_t lb = wave_lower_bound(it, 0, b.k[t], (int32_t)(wave == 0 ? c0 : c1));
            if ((threadIdx.x & 63) == 0) s_lb[r & 1][wave] = lb;
        }
        __syncthreads();
        const int64_t j1 = s_lb[r & 1][1];
        for (int64_t j = s_lb[r & 1][0] + threadIdx.x; j < j1; j += 256) {
            const int64_t e = (int64_t)it[j] - c0;
            if (e >= 0 && e < len) chunk[e] += bf_bits_f(vt[j]);
        }
    }
    __syncthreads();
    // elements before the first 16-B boundary of o; everything when gE's boundary is elsewhere
    int head = (int)(((16 - ((uintptr_t)o & 15)) & 15) >> 2);
    if (GE && (((uintptr_t)o ^ (uintptr_t)g) & 15)) head = len;
    head = min(head, len);
    const int nu = (len - head) / 4;
    for (int e = threadIdx.x; e < head; e += 256) {
        const float r = final1<GE>(chunk[e], GE ? g[e] : 0.f, sc, decay);
        if (GE) g[e] = r;
        o[e] = r;
    }
    for (int u0 = threadIdx.x; u0 < nu; u0 += 256 * kUnits) {
        vf4_t ge[kUnits];
        if constexpr (GE) {
#pragma unroll
            for (int q = 0; q < kUnits; ++q) {
                const int u = u0 + q * 256 < nu ? u0 + q * 256 : nu - 1;
                ge[q] = ld_f4_nt(g + head + 4 * u);
            }
        }
#pragma unroll
        for (int q = 0; q < kUnits; ++q) {
            const int u = u0 + q * 256;
            if (u >= nu) continue;
            const vf4_t c = *reinterpret_cast<const vf4_t*>(chunk + head + 4 * u);  // 16-B aligned in LDS too
            vf4_t r;
            r.x = final1<GE>(c.x, GE ? ge[q].x : 0.f, sc, decay);
            r.y = final1<GE>(c.y, GE ? ge[q].y : 0.f, sc, decay);
            r.z = final1<GE>(c.z, GE ? ge[q].z : 0.f, sc, decay);
            r.w = final1<GE>(c.w, GE ? ge[q].w : 0.f, sc, decay);
            if (GE) st_f4_nt(g + head + 4 * u, r);
            st_f4_nt(o + head + 4 * u, r);
        }
    }
    for (int e = head + 4 * nu + threadIdx.x; e < len; e += 256) {
        const float r = final1<GE>(chunk[e], GE ? g[e] : 0.f, sc, decay);
        if (GE) g[e] = r;
        o[e] = r;
    }
}

// one rank's payload into the fp32 sums (error_dtype: the scratch; wire_dtype: the bucket itself);
// indices within a payload are distinct, the ranks' launches are ordered by the stream; an index
// outside its tensor is skipped.  FIRST: the sums are zero (0 + v, so a -0 value becomes +0)
template <bool FIRST>
__global__ void __launch_bounds__(256) k_scatter(MixedBatch b, float* __restrict__ sums,
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

// error_dtype: gE := fma(d, sums / ws, gE); out = b(gE): 2 x 16 B of sums and of gE in, 2 x 16 B of
// gE and 16 B of out written per unit
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
            a.x = final1<true>(s0[u].x, g0[u].x, sc, decay), a.y = final1<true>(s0[u].y, g0[u].y, sc, decay);
            a.z = final1<true>(s0[u].z, g0[u].z, sc, decay), a.w = final1<true>(s0[u].w, g0[u].w, sc, decay);
            b.x = final1<true>(s1[u].x, g1[u].x, sc, decay), b.y = final1<true>(s1[u].y, g1[u].y, sc, decay);
            b.z = final1<true>(s1[u].z, g1[u].z, sc, decay), b.w = final1<true>(s1[u].w, g1[u].w, sc, decay);
            st_f4_nt(gE + 8 * j, a);
            st_f4_nt(gE + 8 * j + 4, b);
            __builtin_nontemporal_store(u4_t{arctopk::cvt_pk_bf16(a.x, a.y), arctopk::cvt_pk_bf16(a.z, a.w),
                                             arctopk::cvt_pk_bf16(b.x, b.y), arctopk::cvt_pk_bf16(b.z, b.w)},
                                        out + j);
        }
    }
    const int64_t t = n8 * 8 + threadIdx.x;
    if (blockIdx.x == 0 && t < numel) {
        const float v = final1<true>(sums[t], gE[t], sc, decay);
        gE[t] = v;
        reinterpret_cast<uint16_t*>(out)[t] = f_to_bf(v);
    }
}

__global__ void __launch_bounds__(256) k_final21_scalar(uint16_t* __restrict__ out, float* __restrict__ gE,
                                                        const float* __restrict__ sums, int64_t numel,
                                                        MeanScale sc, float decay) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < numel; i += (int64_t)gridDim.x * 256) {
        const float v = final1<true>(sums[i], gE[i], sc, decay);
        gE[i] = v;
        out[i] = f_to_bf(v);
    }
}

// wire_dtype: out := sums / ws in place, or gE := fma(d, sums / ws, gE), out = gE: 16-B units,
// nontemporal, kUnits units' loads before the first store; block 0 also does the numel % 4 elements
// behind them
template <bool GE>
__global__ void __launch_bounds__(256) k_final16_units(float* __restrict__ out, float* __restrict__ gE, int64_t n4,
                                                       int64_t numel, MeanScale sc, float decay) {
    for (int64_t i = (int64_t)blockIdx.x * 256 * kUnits + threadIdx.x; i < n4;
         i += (int64_t)gridDim.x * 256 * kUnits) {
        vf4_t s[kUnits], ge[kUnits];
#pragma unroll
        for (int u = 0; u < kUnits; ++u) {
            const int64_t j = i + u * 256 < n4 ? i + u * 256 : n4 - 1;
            s[u] = ld_f4_nt(out + 4 * j);
            if constexpr (GE) ge[u] = ld_f4_nt(gE + 4 * j);
        }
#pragma unroll
        for (int u = 0; u < kUnits; ++u) {
            const int64_t j = i + u * 256;
            if (j >= n4) continue;
            vf4_t r;
            r.x = final1<GE>(s[u].x, GE ? ge[u].x : 0.f, sc, decay);
            r.y = final1<GE>(s[u].y, GE ? ge[u].y : 0.f, sc, decay);
            r.z = final1<GE>(s[u].z, GE ? ge[u].z : 0.f, sc, decay);
            r.w = final1<GE>(s[u].w, GE ? ge[u].w : 0.f, sc, decay);
            if (GE) st_f4_nt(gE + 4 * j, r);
            st_f4_nt(out + 4 * j, r);
        }
    }
    const int64_t t = n4 * 4 + threadIdx.x;
    if (blockIdx.x == 0 && t < numel) {
        const float r = final1<GE>(out[t], GE ? gE[t] : 0.f, sc, decay);
        if (GE) gE[t] = r;
        out[t] = r;
    }
}

// element by element, for pointers that are not 16-B aligned
template <bool GE>
__global__ void __launch_bounds__(256) k_final16_scalar(float* __restrict__ out, float* __restrict__ gE,
                                                        int64_t numel, MeanScale sc, float decay) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < numel; i += (int64_t)gridDim.x * 256) {
        const float r = final1<GE>(out[i], GE ? gE[i] : 0.f, sc, decay);
        if (GE) gE[i] = r;
        out[i] = r;
    }
}

// ---- host ----------------------------------------------------------------------------------
inline int stream_grid(int64_t work_items, int per_block) {
    return (int)std::max<int64_t>(1, std::min<int64_t>(kStreamGrid, (work_items + per_block - 1) / per_block));
}

inline int gather_grid(int64_t work) { return (int)std::max<int64_t>(1, std::min<int64_t>(2048, (work + 255) / 256)); }

// Every batch of the layout, checked, before anything is launched: tensor i's extent is
// offsets[i + 1] - offsets[i] (the last one's ends at numel), the tensors tile [offsets[0], numel) in
// order, 1 <= k <= extent and the payload slices lie in [0, packed_len) (packed_len < 0: not
// checked).  ARCTOPK_EINVAL otherwise.
struct Batches {
    std::vector<MixedBatch> b;
    std::vector<int64_t> maxk, maxn;
    int32_t nt;
    int count(size_t q) const { return std::min<int32_t>(kB, nt - (int32_t)q * kB); }  // tensors of batch q
};

int fill_batches(Batches& bs, int32_t nt, int64_t numel, const int64_t* offsets, const int64_t* ks,
                 const int64_t* k_off, int64_t packed_len) {
    bs.nt = nt;
    bs.b.resize((nt + kB - 1) / kB);
    bs.maxk.assign(bs.b.size(), 0);
    bs.maxn.assign(bs.b.size(), 0);
    for (int32_t t = 0; t < nt; ++t) {
        MixedBatch& b = bs.b[t / kB];
        const int i = t % kB;
        const int64_t end = t + 1 < nt ? offsets[t + 1] : numel;
        b.off[i] = offsets[t];
        b.n[i] = end - offsets[t];
        b.k[i] = ks[t];
        b.koff[i] = k_off[t];
        if (offsets[t] < 0 || end > numel || b.n[i] < 1 || b.n[i] >= (1ll << 31)) return ARCTOPK_EINVAL;
        if (b.k[i] < 1 || b.k[i] > b.n[i] || b.koff[i] < 0) return ARCTOPK_EINVAL;
        if (packed_len >= 0 && b.koff[i] + b.k[i] > packed_len) return ARCTOPK_EINVAL;
        bs.maxk[t / kB] = std::max(bs.maxk[t / kB], b.k[i]);
        bs.maxn[t / kB] = std::max(bs.maxn[t / kB], b.n[i]);
    }
    return 0;
}

// every rank's payload into the (zeroed) sums, in rank order, batch by batch
int scatter_ranks(const Batches& bs, float* sums, const int32_t* idx, const uint16_t* vals, int32_t nranks,
                  int64_t packed_len, hipStream_t st) {
    for (int32_t r = 0; r < nranks; ++r) {
        const int32_t* ir = idx + (int64_t)r * packed_len;
        const uint16_t* vr = vals + (int64_t)r * packed_len;
        for (size_t q = 0; q < bs.b.size(); ++q) {
            const dim3 grid(gather_grid(bs.maxk[q]), bs.count(q));
            if (r == 0) hipLaunchKernelGGL(k_scatter<true>, grid, dim3(256), 0, st, bs.b[q], sums, ir, vr);
            else hipLaunchKernelGGL(k_scatter<false>, grid, dim3(256), 0, st, bs.b[q], sums, ir, vr);
            const int e = (int)hipGetLastError();
            if (e) return e;
        }
    }
    return 0;
}

}  // namespace

// ---- error_dtype ---------------------------------------------------------------------------
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
    Batches bs;
    const int e0 = fill_batches(bs, nt, numel, offsets, ks, k_off, -1);
    if (e0) return e0;
    hipStream_t st = (hipStream_t)stream;
    const float* s = static_cast<const float*>(src);
    float* Ef = static_cast<float*>(E);
    uint16_t* v = static_cast<uint16_t*>(vals);
    for (size_t q = 0; q < bs.b.size(); ++q) {
        const dim3 grid(gather_grid(bs.maxk[q]), bs.count(q));
        if (ef == ARCTOPK_EF14)
            hipLaunchKernelGGL(k_pack<ARCTOPK_EF14>, grid, dim3(256), 0, st, bs.b[q], s, Ef, idx, v, decay);
        else
            hipLaunchKernelGGL(k_pack<ARCTOPK_EF21>, grid, dim3(256), 0, st, bs.b[q], s, Ef, idx, v, decay);
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
    Batches bs;
    const int e0 = fill_batches(bs, nt, numel, offsets, ks, k_off, packed_len);
    if (e0) return e0;
    hipStream_t st = (hipStream_t)stream;
    float* sums = static_cast<float*>(scratch);
    float* ge = static_cast<float*>(gE);
    hipError_t he = hipMemsetAsync(sums, 0, (size_t)numel * sizeof(float), st);
    if (he != hipSuccess) return (int)he;
    const int e1 = scatter_ranks(bs, sums, idx, static_cast<const uint16_t*>(vals), nranks, packed_len, st);
    if (e1) return e1;
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

// ---- wire_dtype ----------------------------------------------------------------------------
extern "C" int arctopk_sparse_pack_wire16(const void* values, void* E, int64_t numel, int32_t nt,
                                          const int64_t* offsets, const int64_t* ks, const int64_t* k_off,
                                          const int32_t* idx, void* vals16, int32_t ef, float decay, void* stream) {
    if (!values || !offsets || !ks || !k_off || !idx || !vals16 || nt < 1 || numel < 1) return ARCTOPK_EINVAL;
    if (!arctopk::ef_known(ef) || (ef != ARCTOPK_EF_NONE && !E)) return ARCTOPK_EINVAL;
    if (arctopk::low_bits(values, 3) || arctopk::low_bits(E, 3) || arctopk::low_bits(idx, 3) ||
        arctopk::low_bits(vals16, 1))
        return ARCTOPK_EINVAL;
    Batches bs;
    const int e0 = fill_batches(bs, nt, numel, offsets, ks, k_off, -1);
    if (e0) return e0;
    hipStream_t st = (hipStream_t)stream;
    const float* v = static_cast<const float*>(values);
    float* Ef = static_cast<float*>(E);
    uint16_t* o = static_cast<uint16_t*>(vals16);
    const int aligned16 = !arctopk::low_bits(values, 15) && !arctopk::low_bits(idx, 15) && !arctopk::low_bits(vals16, 7);
    for (size_t q = 0; q < bs.b.size(); ++q) {
        const dim3 grid(gather_grid((bs.maxk[q] + 3) / 4), bs.count(q));
        if (ef == ARCTOPK_EF14)
            hipLaunchKernelGGL(k_pack16<ARCTOPK_EF14>, grid, dim3(256), 0, st, bs.b[q], v, Ef, idx, o, decay, aligned16);
        else if (ef == ARCTOPK_EF21)
            hipLaunchKernelGGL(k_pack16<ARCTOPK_EF21>, grid, dim3(256), 0, st, bs.b[q], v, Ef, idx, o, decay, aligned16);
        else
            hipLaunchKernelGGL(k_pack16<ARCTOPK_EF_NONE>, grid, dim3(256), 0, st, bs.b[q], v, Ef, idx, o, decay,
                               aligned16);
        const int e = (int)hipGetLastError();
        if (e) return e;
    }
    return 0;
}

extern "C" int arctopk_sparse_decode_wire16(void* out, int64_t numel, int32_t nt, const int64_t* offsets,
                                            const int64_t* ks, const int64_t* k_off, int64_t packed_len,
                                            const int32_t* idx, const void* vals16, int32_t nranks, int32_t world_size,
                                            int32_t accumulate, void* gE, float decay, void* stream) {
    if (!out || !offsets || !ks || !k_off || !idx || !vals16 || nt < 1 || nranks < 1 || world_size < 1 || numel < 1 ||
        packed_len < 0 || accumulate < 0 || accumulate > 3)
        return ARCTOPK_EINVAL;
    if (arctopk::low_bits(out, 3) || arctopk::low_bits(gE, 3) || arctopk::low_bits(idx, 3) ||
        arctopk::low_bits(vals16, 1))
        return ARCTOPK_EINVAL;
    Batches bs;
    const int e0 = fill_batches(bs, nt, numel, offsets, ks, k_off, packed_len);
    if (e0) return e0;
    hipStream_t st = (hipStream_t)stream;
    float* o = static_cast<float*>(out);
    float* ge = static_cast<float*>(gE);
    const uint16_t* v = static_cast<const uint16_t*>(vals16);
    const MeanScale sc = arctopk::make_mean_scale(world_size);
    const bool ranked = accumulate == 1 || accumulate == 3;
    const int nr = ranked ? nranks : 1;  // RandK: the one all-reduced payload
    // the tensors tile [offsets[0], numel) in order (fill_batches); from 0, the chunks cover the bucket
    if ((accumulate == 1 || accumulate == 2) && offsets[0] == 0) {
        for (size_t q = 0; q < bs.b.size(); ++q) {
            const dim3 grid((unsigned)((bs.maxn[q] + kChunk - 1) / kChunk), bs.count(q));
            if (ge)
                hipLaunchKernelGGL(k_decode_merged<true>, grid, dim3(256), 0, st, bs.b[q], o, ge, idx, v, nr,
                                   packed_len, sc, decay);
            else
                hipLaunchKernelGGL(k_decode_merged<false>, grid, dim3(256), 0, st, bs.b[q], o, ge, idx, v, nr,
                                   packed_len, sc, decay);
            const int e = (int)hipGetLastError();
            if (e) return e;
        }
        return 0;
    }
    hipError_t he = hipMemsetAsync(o, 0, (size_t)numel * sizeof(float), st);
    if (he != hipSuccess) return (int)he;
    const int e1 = scatter_ranks(bs, o, idx, v, nr, packed_len, st);
    if (e1) return e1;
    if (world_size == 1 && !ge) return 0;  // s / 1 == s for every s
    if (!arctopk::low_bits(out, 15) && !arctopk::low_bits(gE, 15) && numel >= 4) {
        const int64_t n4 = numel / 4;
        const dim3 grid(stream_grid(n4, 256 * kUnits));
        if (ge) hipLaunchKernelGGL(k_final16_units<true>, grid, dim3(256), 0, st, o, ge, n4, numel, sc, decay);
        else hipLaunchKernelGGL(k_final16_units<false>, grid, dim3(256), 0, st, o, ge, n4, numel, sc, decay);
    } else {
        const dim3 grid(stream_grid(numel, 256));
        if (ge) hipLaunchKernelGGL(k_final16_scalar<true>, grid, dim3(256), 0, st, o, ge, numel, sc, decay);
        else hipLaunchKernelGGL(k_final16_scalar<false>, grid, dim3(256), 0, st, o, ge, numel, sc, decay);
    }
    return (int)hipGetLastError();
}
