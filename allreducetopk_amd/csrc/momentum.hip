// Momentum fold of a whole bucket for MI355X (gfx950): the reference's momentum compression
// (comm_hooks/utils.py:54-65), grad.mul_(1 - beta1).add_(exp_avg, alpha=beta1) per parameter,
// as one launch per bucket (per ARCTOPK_SPARSE_MAX_BATCH tensors).
//
//   bucket[off_i + j] = rnd( fma(b, m_i[j], rnd(bucket[off_i + j] * a)) ),  j < numel_i
//
// rnd rounds to the bucket's element type (identity for fp32), a = float(1 - beta1) and
// b = float(beta1): torch's GPU functors take the Python scalars as fp32 and form `self + alpha *
// other` as one fused multiply-add, for fp32 and bf16 tensors alike; a bf16 bucket with fp32
// moments promotes to fp32 and rounds once per op (tests/test_gpu_momentum.py pins the rule per
// dtype pair against the torch ops on the GPU).
//
// In place, 12 B per fp32 element: read G, read M, write G.  The moments are the optimizer's own
// exp_avg tensors, separate allocations, so the launch carries a table of pointers by value.  The
// batch's elements are cut into chunks of kMomUnits 16-B units of the bucket, one block per
// chunk; a block finds its tensor by binary search over the per-tensor first-chunk indices.  Chunk
// boundaries sit on 16-B boundaries of the bucket: scalar head and tail elements are peeled, the
// body loads and stores G 16 B per lane and loads M with the widest access its address allows
// (a view at an odd element offset is not co-aligned with its moment).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "common.h"

#ifndef ARCTOPK_MOM_NT_LOAD
#define ARCTOPK_MOM_NT_LOAD 1    // nontemporal loads of G and M
#endif
#ifndef ARCTOPK_MOM_NT_STORE
#define ARCTOPK_MOM_NT_STORE 0   // plain stores of G: the encode that follows reads the same lines
#endif

namespace {

using arctopk::bf16_t;
using arctopk::u2_t;
using arctopk::u4_t;

constexpr int kB = ARCTOPK_SPARSE_MAX_BATCH;
constexpr int kMomUnits = 2048;  // 16-B units of the bucket per chunk (32 KiB; 8 per lane)
constexpr int kMomInFlight = 4;  // units a lane loads before it computes
constexpr bool kNtLoad = ARCTOPK_MOM_NT_LOAD != 0;
constexpr bool kNtStore = ARCTOPK_MOM_NT_STORE != 0;

struct MomBatch {
    const void* m[kB];       // moment of each tensor
    int64_t off[kB];         // its element offset in the bucket
    int64_t n[kB];           // its elements (> 0)
    int32_t first[kB + 1];   // first chunk of each tensor; first[nt] = blocks
    int32_t nt;
};

// elements in front of the first 16-B boundary of p, at most n
template <typename T>
__host__ __device__ inline int64_t mom_head(const void* p, int64_t n) {
    const int64_t h = (int64_t)((16 - ((uintptr_t)p & 15)) & 15) / (int64_t)sizeof(T);
    return h < n ? h : n;
}

template <typename TG>
__device__ __forceinline__ float fold1(float g, float m, float a, float b) {
    return arctopk::rnd<TG>(__fmaf_rn(b, m, arctopk::rnd<TG>(__fmul_rn(g, a))));
}

template <typename V, bool NT>
__device__ __forceinline__ V ldv(const V* p) {
    if constexpr (NT) return __builtin_nontemporal_load(p);
    else return *p;
}

// VG moments at p (aligned to W bytes, W >= sizeof(TM)) as floats, by W-byte loads
template <typename TM, int W, int VG, bool NT>
__device__ __forceinline__ void ld_mom(const TM* p, float (&mv)[VG]) {
    if constexpr (W == 2) {
#pragma unroll
        for (int i = 0; i < VG; ++i) mv[i] = arctopk::ld1<TM, NT>(p + i);
    } else {
        constexpr int kWords = VG * (int)sizeof(TM) / 4;
        uint32_t w[kWords];
        if constexpr (W == 16) {
#pragma unroll
            for (int i = 0; i < kWords / 4; ++i) {
                const u4_t v = ldv<u4_t, NT>(reinterpret_cast<const u4_t*>(p) + i);
                w[4 * i] = v.x, w[4 * i + 1] = v.y, w[4 * i + 2] = v.z, w[4 * i + 3] = v.w;
            }
        } else if constexpr (W == 8) {
#pragma unroll
            for (int i = 0; i < kWords / 2; ++i) {
                const u2_t v = ldv<u2_t, NT>(reinterpret_cast<const u2_t*>(p) + i);
                w[2 * i] = v.x, w[2 * i + 1] = v.y;
            }
        } else {
#pragma unroll
            for (int i = 0; i < kWords; ++i) w[i] = ldv<uint32_t, NT>(reinterpret_cast<const uint32_t*>(p) + i);
        }
        if constexpr (sizeof(TM) == 4) {
#pragma unroll
            for (int i = 0; i < VG; ++i) mv[i] = __uint_as_float(w[i]);
        } else {
#pragma unroll
            for (int i = 0; i < kWords; ++i) {
                mv[2 * i] = __uint_as_float(w[i] << 16);
                mv[2 * i + 1] = __uint_as_float(w[i] & 0xFFFF0000u);
            }
        }
    }
}

// the 16-B units [0, nunits) of g (16-B aligned) against the moments at m (W-byte aligned)
template <typename TG, typename TM, int W>
__device__ __forceinline__ void fold_units(TG* __restrict__ g, const TM* __restrict__ m, int nunits, float a,
                                           float b) {
    constexpr int VG = 16 / (int)sizeof(TG);
    constexpr int Q = arctopk::kQuadsPer16<TG>;
    for (int u0 = threadIdx.x; u0 < nunits; u0 += 256 * kMomInFlight) {
        u4_t graw[kMomInFlight];
        float mv[kMomInFlight][VG];
#pragma unroll
        for (int k = 0; k < kMomInFlight; ++k) {
            const int u = u0 + k * 256;
            if (u < nunits) {
                graw[k] = arctopk::ld16raw<TG, kNtLoad>(g, u);
                ld_mom<TM, W, VG, kNtLoad>(m + (int64_t)u * VG, mv[k]);
            }
        }
#pragma unroll
        for (int k = 0; k < kMomInFlight; ++k) {
            const int u = u0 + k * 256;
            if (u < nunits) {
                float4 q[Q];
                arctopk::unpack16<TG>(graw[k], q);
#pragma unroll
                for (int j = 0; j < Q; ++j) {
                    float4 t = make_float4(__fmul_rn(q[j].x, a), __fmul_rn(q[j].y, a), __fmul_rn(q[j].z, a),
                                           __fmul_rn(q[j].w, a));
                    t = arctopk::rnd4<TG>(t);
                    // st16 rounds the sums to TG
                    q[j] = make_float4(__fmaf_rn(b, mv[k][4 * j], t.x), __fmaf_rn(b, mv[k][4 * j + 1], t.y),
                                       __fmaf_rn(b, mv[k][4 * j + 2], t.z), __fmaf_rn(b, mv[k][4 * j + 3], t.w));
                }
                arctopk::st16<TG, kNtStore>(g, u, q);
            }
        }
    }
}

template <typename TG, typename TM>
__global__ void __launch_bounds__(256) k_momentum_fold(const MomBatch bt, TG* __restrict__ bucket, float a, float b) {
    constexpr int VG = 16 / (int)sizeof(TG);
    const int x = (int)blockIdx.x;
    int lo_t = 0, hi_t = bt.nt - 1;  // last tensor with first <= x (binary search over kernel arguments)
    while (lo_t < hi_t) {
        const int mid = (lo_t + hi_t + 1) >> 1;
        if (bt.first[mid] <= x) lo_t = mid;
        else hi_t = mid - 1;
    }
    const int t = lo_t;
    const int64_t c = x - bt.first[t];
    const int64_t n = bt.n[t];
    TG* g = bucket + bt.off[t];
    const TM* m = static_cast<const TM*>(bt.m[t]);
    // chunk c of the tensor: elements [lo, hi); its 16-B units start at element al
    const int64_t h = mom_head<TG>(g, n);
    const int64_t lo = c == 0 ? 0 : h + c * (int64_t)(kMomUnits * VG);
    const int64_t hi = min(n, h + (c + 1) * (int64_t)(kMomUnits * VG));
    const int64_t al = c == 0 ? h : lo;
    const int nunits = (int)((hi - al) / VG);
    const int64_t tail = al + (int64_t)nunits * VG;
    const int tid = threadIdx.x;
    if (lo + tid < al)  // scalar head (first chunk only): fewer than VG elements
        arctopk::st1<TG>(g + lo + tid, fold1<TG>(arctopk::ld1<TG>(g + lo + tid), arctopk::ld1<TM>(m + lo + tid), a, b));
    if (tail + tid < hi)  // scalar tail (last chunk only): fewer than VG elements
        arctopk::st1<TG>(g + tail + tid,
                         fold1<TG>(arctopk::ld1<TG>(g + tail + tid), arctopk::ld1<TM>(m + tail + tid), a, b));
    if (nunits == 0) return;
    const TM* ma = m + al;
    const uintptr_t mbits = (uintptr_t)ma;  // every unit advances M by 16 or 32 B: one width per chunk
    if ((mbits & 15) == 0) fold_units<TG, TM, 16>(g + al, ma, nunits, a, b);
    else if ((mbits & 7) == 0) fold_units<TG, TM, 8>(g + al, ma, nunits, a, b);
    else if ((mbits & 3) == 0) fold_units<TG, TM, 4>(g + al, ma, nunits, a, b);
    else if constexpr (sizeof(TM) == 2) fold_units<TG, TM, 2>(g + al, ma, nunits, a, b);
}

template <typename TG>
int64_t mom_chunks(const void* g, int64_t n) {
    constexpr int64_t che = (int64_t)kMomUnits * (16 / (int64_t)sizeof(TG));
    const int64_t h = mom_head<TG>(g, n);
    return n > h ? (n - h + che - 1) / che : 1;
}

template <typename TG, typename TM>
int fold_all(TG* bucket, int32_t nt, const int64_t* offsets, const int64_t* numels, const void* const* moments,
             float a, float b, hipStream_t st) {
    int32_t j = 0;
    while (j < nt) {
        MomBatch bt;
        bt.nt = 0;
        bt.first[0] = 0;
        for (; j < nt && bt.nt < kB; ++j) {
            if (numels[j] == 0) continue;
            const int64_t nch = mom_chunks<TG>(bucket + offsets[j], numels[j]);
            if (bt.first[bt.nt] + nch > INT32_MAX) break;  // the grid is full: this tensor opens the next launch
            bt.m[bt.nt] = moments[j];
            bt.off[bt.nt] = offsets[j];
            bt.n[bt.nt] = numels[j];
            bt.first[bt.nt + 1] = bt.first[bt.nt] + (int32_t)nch;
            ++bt.nt;
        }
        if (bt.nt == 0) continue;
        hipLaunchKernelGGL((k_momentum_fold<TG, TM>), dim3((unsigned)bt.first[bt.nt]), dim3(256), 0, st, bt, bucket,
                           a, b);
        const int e = (int)hipGetLastError();
        if (e) return e;
    }
    return 0;
}

}  // namespace

extern "C" int arctopk_momentum_fold(void* bucket, int32_t ntensors, const int64_t* offsets, const int64_t* numels,
                                     const void* const* moments, double one_minus_beta, double beta, int32_t dtype,
                                     int32_t mom_dtype, void* stream) {
    // every argument check comes before the first device call
    if (!bucket || !offsets || !numels || !moments || ntensors < 0) return ARCTOPK_EINVAL;
    const bool g32 = dtype == ARCTOPK_F32, g16 = dtype == ARCTOPK_BF16;
    const bool m32 = mom_dtype == ARCTOPK_F32, m16 = mom_dtype == ARCTOPK_BF16;
    if (!((g32 && m32) || (g16 && m16) || (g16 && m32))) return ARCTOPK_EDTYPE;
    const uintptr_t gs = g32 ? 4 : 2, ms = m32 ? 4 : 2;
    if ((uintptr_t)bucket & (gs - 1)) return ARCTOPK_EINVAL;
    for (int32_t j = 0; j < ntensors; ++j) {
        if (offsets[j] < 0 || numels[j] < 0) return ARCTOPK_EINVAL;
        if (numels[j] == 0) continue;
        if (!moments[j] || ((uintptr_t)moments[j] & (ms - 1))) return ARCTOPK_EINVAL;
        const void* g = static_cast<const char*>(bucket) + offsets[j] * (int64_t)gs;
        if ((g32 ? mom_chunks<float>(g, numels[j]) : mom_chunks<bf16_t>(g, numels[j])) > INT32_MAX)
            return ARCTOPK_EINVAL;
    }
    // the Python scalars as torch's GPU functors take them: cast to fp32 (the opmath type of
    // fp32 and bf16 tensors)
    const float a = (float)one_minus_beta, b = (float)beta;
    hipStream_t st = (hipStream_t)stream;
    if (g32) return fold_all<float, float>(static_cast<float*>(bucket), ntensors, offsets, numels, moments, a, b, st);
    if (m16)
        return fold_all<bf16_t, bf16_t>(static_cast<bf16_t*>(bucket), ntensors, offsets, numels, moments, a, b, st);
    return fold_all<bf16_t, float>(static_cast<bf16_t*>(bucket), ntensors, offsets, numels, moments, a, b, st);
}
