// What mixed_ef.hip (fp32 residuals under a bf16 bucket) and wire16.hip (bf16 packed values of an
// fp32 bucket) share: the layout of their work tables and the host loops that fill them, the mean
// scale of their decodes, the entry points' small argument checks, and the bf16 / 16-B fp32 device
// helpers.  No kernel lives here: each file keeps its own, tuned for its unit width (8 bf16 or 4
// fp32 per 16 B).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "common.h"

namespace arctopk {

// ---- work tables ---------------------------------------------------------------------------
struct PackChunk {
    int32_t seg;
    int32_t mode;    // the file's pack chunk mode (rows, rows in 16-B units, DENSE)
    int64_t j0;      // first selected row (DENSE: first element)
    int32_t nj;      // selected rows (DENSE: elements)
    int32_t pad;
};

struct RowTile {
    int32_t seg;
    int32_t flags;   // the file's tile flags
    int64_t row0;    // first row (RAW, DENSE: first element)
    int32_t nrows;   // rows (RAW, DENSE: elements)
    int32_t lanes;   // lanes per row
    int32_t rstride; // the tile's rows are row0 + q * rstride, q < nrows: the tiles of a tensor
    int32_t pad;     //   interleave, so the blocks in flight stream one advancing window of it
};

// a device copy of v (one element allocated for an empty one)
template <class T>
hipError_t upload(const std::vector<T>& v, T** d) {
    hipError_t e = hipMalloc((void**)d, std::max<size_t>(1, v.size()) * sizeof(T));
    if (e == hipSuccess && !v.empty()) e = hipMemcpy(*d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
    return e;
}

inline int pow2_at_least(int64_t x) {
    int p = 1;
    while (p < x && p < 64) p <<= 1;
    return p;
}

// `count` selected rows of m columns (a DENSE segment: its elements, m = 1) in chunks of about
// `elems` elements
inline void push_pack_chunks(std::vector<PackChunk>& out, int seg, int32_t mode, int64_t count, int64_t m,
                             int64_t elems) {
    const int64_t per = std::max<int64_t>(1, elems / m);
    for (int64_t j = 0; j < count; j += per)
        out.push_back(PackChunk{seg, mode, j, (int32_t)std::min<int64_t>(per, count - j), 0});
}

// `count` consecutive rows (or elements) in tiles of `per`, a lane each
inline void push_range_tiles(std::vector<RowTile>& out, int seg, int32_t flags, int64_t count, int64_t per) {
    for (int64_t e = 0; e < count; e += per)
        out.push_back(RowTile{seg, flags, e, (int32_t)std::min<int64_t>(per, count - e), 1, 1, 0});
}

// The n rows of m columns of a segment in interleaved tiles of about `elems` elements for blocks of
// `block` threads: a power of two of lanes shares a row, one per 16-B unit of `unit` elements when
// `vec`, else one per element.  Returns the number of tiles appended.
inline int64_t push_row_tiles(std::vector<RowTile>& out, int seg, int32_t flags, int64_t n, int64_t m, bool vec,
                              int unit, int block, int64_t elems) {
    const int lanes = pow2_at_least(vec ? m / unit : m);
    const int groups = block / lanes;
    // whole rounds of the block's groups, at least one
    int64_t per = std::max<int64_t>(1, elems / m);
    per = std::max<int64_t>(groups, per / groups * groups);
    // tile ti holds rows ti, ti + ntiles, ...: consecutive blocks touch adjacent rows
    const int64_t ntiles = (n + per - 1) / per;
    for (int64_t ti = 0; ti < ntiles; ++ti)
        out.push_back(RowTile{seg, flags, ti, (int32_t)((n - ti + ntiles - 1) / ntiles), lanes, (int32_t)ntiles, 0});
    return ntiles;
}

// ---- entry point checks --------------------------------------------------------------------
inline uintptr_t low_bits(const void* a, uintptr_t mask) { return (uintptr_t)a & mask; }
inline bool ef_known(int32_t ef) { return ef == ARCTOPK_EF_NONE || ef == ARCTOPK_EF14 || ef == ARCTOPK_EF21; }

// ---- decode --------------------------------------------------------------------------------
// mean of the all-reduced values: x / ws correctly rounded (Scale of arctopk_kernels.hip)
struct MeanScale {
    float ws, inv;
    int pow2;
    __device__ __forceinline__ float operator()(float x) const { return pow2 ? x * inv : __fdiv_rn(x, ws); }
};
inline MeanScale make_mean_scale(int32_t world_size) {
    MeanScale sc;
    sc.ws = (float)world_size;
    sc.pow2 = (world_size & (world_size - 1)) == 0;
    sc.inv = 1.0f / (float)world_size;
    return sc;
}

// ---- device helpers ------------------------------------------------------------------------
__device__ __forceinline__ float bf_bits_f(uint32_t u16) { return __uint_as_float(u16 << 16); }
__device__ __forceinline__ uint16_t f_to_bf(float f) { return (uint16_t)(cvt_pk_bf16(f, 0.0f) & 0xFFFFu); }

typedef float vf4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ vf4_t ld_f4_nt(const float* p) {
    return __builtin_nontemporal_load(reinterpret_cast<const vf4_t*>(p));
}
__device__ __forceinline__ void st_f4_nt(float* p, vf4_t v) {
    __builtin_nontemporal_store(v, reinterpret_cast<vf4_t*>(p));
}

}  // namespace arctopk
