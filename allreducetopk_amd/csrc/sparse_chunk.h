// What the two chunk decodes, k_decode_merged (sparse_mixed.hip) and k_decode_idx16 (sparse_idx16.hip),
// state once: the chunk's geometry and the finalize rule.  (Their bodies stay apart: DESIGN.md section 9.)
#pragma once

#include "mixed_common.h"
#include "sparse_common.h"

namespace {

constexpr int kChunk = 4096;  // elements of a tensor a decode block composes in LDS
constexpr int kUnits = 4;     // 16-B units per lane per step, loads before stores

// the mean of the sums, and under GE the new gE
template <bool GE>
__device__ __forceinline__ float final1(float s, float ge, const arctopk::MeanScale& sc, float decay) {
    const float m = sc(s);
    return GE ? __fmaf_rn(decay, m, ge) : m;
}

}  // namespace
