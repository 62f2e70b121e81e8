// The matrix-instruction encode of sketch ranks 16 and 32 (encode_mfma.hip).
#pragma once
#include "common.h"

namespace arctopk {

constexpr int kMaxRank = 32;  // largest sketch rank a plan accepts (kMaxR: largest VALU-encode rank)
// ranks a plan accepts: the VALU encode's 1..kMaxR, the matrix encode's 16 and 32
inline bool rank_ok(int r) { return (r >= 1 && r <= kMaxR) || r == 16 || r == 32; }
inline bool rank_mfma(int r) { return r > kMaxR; }

// Tile geometry shared by the plan and the kernel.  A block walks its rows' columns in K-slabs of
// kMfSlabBytes per row (256 fp32 / 512 bf16 columns); the V^T slab [r][slab] and one X tile
// [r rows][slab] live in LDS, rows padded by one 16-B unit: 2 r (kMfSlabBytes + 16) bytes, of which
// V^T takes r (kMfSlabBytes + 16) <= 33,280 (within kVLdsMaxBytes).
constexpr int kMfSlabBytes = 1024;
constexpr int kMfRowBytes = kMfSlabBytes + 16;
constexpr int kMfTileRows = 64;     // most rows of a block's tile: 64 / r row tiles of r rows each
constexpr int kMfFillBlocks = 512;  // fewer row tiles than this in a bucket: wide rows split into column parts
static_assert(kMaxRank * kMfRowBytes <= kVLdsMaxBytes, "the V^T slab stays within the LDS budget for V");

// the ENC_MFMA tiles [tile0, tile0 + ntiles) of the plan's table; done (may be null): completed by the kernel
int encode_mfma(const arctopk_plan* p, int tile0, int ntiles, const void* grad, void* err, int ef, int err_in,
                const void* V, void* sketch, uint32_t* keys, hipStream_t st, hipEvent_t done);

}  // namespace arctopk
