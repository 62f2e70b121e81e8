// What sparse_kernels.hip, sparse_mixed.hip, sparse_idx16.hip and sparse_bitmap.hip share (the last two
// through sparse_index_wire.h as well).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "arctopk.h"

namespace arctopk {

// first position in a[lo, hi) with a[p] >= target (a ascending: int32 indices, or their 16-bit halves), one wave
template <typename T>
__device__ __forceinline__ int64_t wave_lower_bound(const T* __restrict__ a, int64_t lo, int64_t hi, int32_t target) {
    const int lane = threadIdx.x & 63;
    while (hi - lo > 64) {
        const int64_t step = (hi - lo + 63) / 64;
        const int64_t p = lo + (int64_t)lane * step;
        const bool pred = p < hi && (int32_t)a[p] < target;
        const int c = __popcll(__ballot(pred));
        if (c == 0) return lo;
        const int64_t nlo = lo + (int64_t)(c - 1) * step + 1;
        const int64_t phi = lo + (int64_t)c * step;
        hi = phi < hi ? phi : hi;
        lo = nlo;
    }
    const int64_t p = lo + lane;
    return lo + __popcll(__ballot(p < hi && (int32_t)a[p] < target));
}

}  // namespace arctopk

// ---- the layout of a bucket's payload, batch by batch (sparse_mixed.hip, sparse_idx16.hip) ------
// Each file has its own copy (the kernels take MixedBatch by value under the file's own name).
namespace {

typedef int32_t vi4_t __attribute__((ext_vector_type(4)));  // 16 B of indices

struct MixedBatch {
    int64_t off[ARCTOPK_SPARSE_MAX_BATCH];
    int64_t n[ARCTOPK_SPARSE_MAX_BATCH];
    int64_t k[ARCTOPK_SPARSE_MAX_BATCH];
    int64_t koff[ARCTOPK_SPARSE_MAX_BATCH];
};

// Every batch of the layout, checked, before anything is launched: tensor i's extent is
// offsets[i + 1] - offsets[i] (the last one's ends at numel), the tensors tile [offsets[0], numel) in
// order, 1 <= k <= extent and the payload slices lie in [0, packed_len) (packed_len < 0: not
// checked).  ARCTOPK_EINVAL otherwise.
struct Batches {
    std::vector<MixedBatch> b;
    std::vector<int64_t> maxk, maxn;
    int32_t nt;
    int count(size_t q) const {  // tensors of batch q
        return std::min<int32_t>(ARCTOPK_SPARSE_MAX_BATCH, nt - (int32_t)q * ARCTOPK_SPARSE_MAX_BATCH);
    }
};

int fill_batches(Batches& bs, int32_t nt, int64_t numel, const int64_t* offsets, const int64_t* ks,
                 const int64_t* k_off, int64_t packed_len) {
    constexpr int kB = ARCTOPK_SPARSE_MAX_BATCH;
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

// launch(q) for every batch q in order; the first launch that leaves an error ends the loop, and that
// error is returned
template <typename Launch>
int launch_batches(const Batches& bs, Launch launch) {
    for (size_t q = 0; q < bs.b.size(); ++q) {
        launch(q);
        const int e = (int)hipGetLastError();
        if (e) return e;
    }
    return 0;
}

}  // namespace
