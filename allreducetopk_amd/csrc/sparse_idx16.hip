// TopK's indices as 16-bit block offsets on the wire (SparseState.index_wire = "idx16", DESIGN.md
// section 4i) on MI355X (gfx950).  Every tensor's indices are tensor-relative and ascending
// (arctopk_topk_select, arctopk_seg_select by row), so one rank's index payload is
//
//   lo16[p] = idx[p] & 0xFFFF                       packed_len x uint16, zero padding to 16 B
//   T[tb_i + b] = #{indices of tensor i below b * 65536}   one int32 per 65,536-element block of
//                                                   every tensor, zero padding to 16 B
//
// (include/arctopk.h).  Block b's entries of tensor i are [T[tb_i + b], T[tb_i + b + 1]) -- the last
// block's end at ks[i] -- and entry j of them is b << 16 | lo16[k_off[i] + j].
//
//   pack     streams the int32 indices once: 2 x 16 B in, 16 B of halves out per unit of 8; the thread
//            holding entry j also holds entry j - 1's block number and writes the table entries of
//            the blocks between the two, so empty blocks need no second pass and no atomic
//   decode   k_decode_merged's work split (sparse_mixed.hip): a block composes a 4096-element chunk of
//            a tensor in LDS from all ranks in rank order.  A chunk lies inside one 65,536-element
//            block, so per rank the block reads two table entries and searches only that slice of
//            lo16 for the chunk's two 16-bit bounds; values fp32 or bf16
//   unpack   block (b, tensor, rank) expands its slice back to int32, for the decodes that read
//            int32 indices
//
// What comes from other ranks is never trusted with an address: table entries are clamped to
// [0, ks] and ordered, a reconstructed index outside the chunk is skipped.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "common.h"
#include "mixed_common.h"
#include "sparse_chunk.h"
#include "sparse_common.h"
#include "sparse_index_wire.h"

namespace {

using arctopk::bf_bits_f;
using arctopk::ld_f4_nt;
using arctopk::MeanScale;
using arctopk::st_f4_nt;
using arctopk::u4_t;
using arctopk::vf4_t;
using arctopk::wave_lower_bound;

constexpr int kB = ARCTOPK_SPARSE_MAX_BATCH;
constexpr int kBlockBits = 16;  // a block of the format: 65,536 elements of a tensor
static_assert((1 << kBlockBits) % kChunk == 0, "a chunk must lie inside one block");

// next to a MixedBatch: where each tensor's table entries start, and (first batch only) the padding
// the pack zeroes: lo16 entries [pad_lo, pad_lo + n_pad_lo), table entries [pad_t, pad_t + n_pad_t)
struct Idx16Batch {
    int64_t tb[kB];
    int64_t pad_lo, pad_t;
    int32_t n_pad_lo, n_pad_t;
};

__device__ __forceinline__ int32_t blocks_of(int64_t n) { return (int32_t)((n + (1 << kBlockBits) - 1) >> kBlockBits); }
// the block number of an index; whatever the bits, in [0, 65535]
__device__ __forceinline__ int32_t block_of(uint32_t idx) { return (int32_t)(idx >> kBlockBits); }

// ---- pack ----------------------------------------------------------------------------------
// Entry j (of k) with block number h, its predecessor's hp (-1 before entry 0): the blocks in
// (hp, h] start at entry j; behind the last entry every later block starts (and ends) at k.
// Every store is clamped to the tensor's nb blocks, so a payload that does not ascend gives
// some table, never a store outside it.
__device__ __forceinline__ void table_entry(int32_t* __restrict__ Tt, int32_t nb, int64_t j, int64_t k, int32_t hp,
                                            int32_t h) {
    if (h > hp) {
        const int32_t top = min(h, nb - 1);
        for (int32_t bb = hp + 1; bb <= top; ++bb) Tt[bb] = (int32_t)j;
    }
    if (j == k - 1)
        for (int32_t bb = h + 1; bb < nb; ++bb) Tt[bb] = (int32_t)k;
}

// tensor blockIdx.y's k indices.  Where the tensor's slices of idx and of lo16 are both 16-B
// aligned: units of 8 (2 x 16 B in, 16 B out, nontemporal), kUnits units' loads -- and each unit's
// predecessor entry -- before the first store; the k % 8 entries behind the last unit, or every
// entry otherwise, one by one.
__global__ void __launch_bounds__(256) k_idx16_pack(MixedBatch b, Idx16Batch x, const int32_t* __restrict__ idx,
                                                    uint16_t* __restrict__ lo16, int32_t* __restrict__ T) {
    const int t = blockIdx.y;
    const int64_t k = b.k[t];
    const int32_t nb = blocks_of(b.n[t]);
    const int32_t* it = idx + b.koff[t];
    uint16_t* lt = lo16 + b.koff[t];
    int32_t* Tt = T + x.tb[t];
    if (blockIdx.x == 0 && t == 0) {
        if ((int)threadIdx.x < x.n_pad_lo) lo16[x.pad_lo + threadIdx.x] = 0;
        if ((int)threadIdx.x < x.n_pad_t) T[x.pad_t + threadIdx.x] = 0;
    }
    const int64_t k8 = (((uintptr_t)it | (uintptr_t)lt) & 15) == 0 ? k / 8 : 0;
    const vi4_t* it4 = reinterpret_cast<const vi4_t*>(it);
    for (int64_t i = (int64_t)blockIdx.x * 256 * kUnits + threadIdx.x; i < k8;
         i += (int64_t)gridDim.x * 256 * kUnits) {
        vi4_t a[kUnits], c[kUnits];
        int32_t hp[kUnits];
#pragma unroll
        for (int u = 0; u < kUnits; ++u) {
            const int64_t j = i + u * 256 < k8 ? i + u * 256 : k8 - 1;
            a[u] = __builtin_nontemporal_load(it4 + 2 * j);
            c[u] = __builtin_nontemporal_load(it4 + 2 * j + 1);
            hp[u] = j > 0 ? block_of((uint32_t)it[8 * j - 1]) : -1;
        }
#pragma unroll
        for (int u = 0; u < kUnits; ++u) {
            const int64_t j = i + u * 256;
            if (j >= k8) continue;
            const uint32_t w[8] = {(uint32_t)a[u].x, (uint32_t)a[u].y, (uint32_t)a[u].z, (uint32_t)a[u].w,
                                   (uint32_t)c[u].x, (uint32_t)c[u].y, (uint32_t)c[u].z, (uint32_t)c[u].w};
            __builtin_nontemporal_store(u4_t{(w[0] & 0xFFFFu) | (w[1] << 16), (w[2] & 0xFFFFu) | (w[3] << 16),
                                             (w[4] & 0xFFFFu) | (w[5] << 16), (w[6] & 0xFFFFu) | (w[7] << 16)},
                                        reinterpret_cast<u4_t*>(lt) + j);
            int32_t h = hp[u];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int32_t hq = block_of(w[q]);
                table_entry(Tt, nb, 8 * j + q, k, h, hq);
                h = hq;
            }
        }
    }
    for (int64_t j = k8 * 8 + (int64_t)blockIdx.x * 256 + threadIdx.x; j < k; j += (int64_t)gridDim.x * 256) {
        const uint32_t w = (uint32_t)it[j];
        const int32_t hp = j > 0 ? block_of((uint32_t)it[j - 1]) : -1;
        lt[j] = (uint16_t)w;
        table_entry(Tt, nb, j, k, hp, block_of(w));
    }
}

// ---- what a reader takes from one rank's payload -----------------------------------------
// block blk's slice [j0, j1) of a tensor's k entries, from a table that may hold anything
__device__ __forceinline__ void block_slice(const int32_t* __restrict__ Tt, int32_t blk, int32_t nb, int64_t k,
                                            int64_t& j0, int64_t& j1) {
    j0 = min<int64_t>(max<int64_t>(Tt[blk], 0), k);
    j1 = blk + 1 < nb ? min<int64_t>(max<int64_t>(Tt[blk + 1], 0), k) : k;
    j1 = max(j0, j1);
}

// ---- unpack --------------------------------------------------------------------------------
// block (blk, tensor, rank): idx_out[j] = blk << 16 | lo16[j] over the block's slice
__global__ void __launch_bounds__(256) k_idx16_unpack(MixedBatch b, Idx16Batch x, const uint8_t* __restrict__ wire,
                                                      int64_t stride, int64_t table_off, int64_t packed_len,
                                                      int32_t* __restrict__ idx_out) {
    const int t = blockIdx.y;
    const int32_t blk = blockIdx.x;
    const int32_t nb = blocks_of(b.n[t]);
    if (blk >= nb) return;
    const uint8_t* wr = wire + (int64_t)blockIdx.z * stride;
    const uint16_t* lt = reinterpret_cast<const uint16_t*>(wr) + b.koff[t];
    int32_t* ot = idx_out + (int64_t)blockIdx.z * packed_len + b.koff[t];
    int64_t j0, j1;
    block_slice(reinterpret_cast<const int32_t*>(wr + table_off) + x.tb[t], blk, nb, b.k[t], j0, j1);
    for (int64_t j = j0 + threadIdx.x; j < j1; j += 256) ot[j] = (blk << kBlockBits) | (int32_t)lt[j];
}

// ---- decode --------------------------------------------------------------------------------
__device__ __forceinline__ float val_f(const float* p) { return *p; }
__device__ __forceinline__ float val_f(const uint16_t* p) { return bf_bits_f(*p); }

// (final1<GE>, the mean of the sums and under GE the new gE: sparse_chunk.h)

// block (x, y) composes elements [4096 x, 4096 (x + 1)) of tensor y: the chunk starts as zeros in
// LDS; for each rank in order, waves 0 and 1 read the two table entries of the chunk's 65,536-element
// block and search that slice of lo16 for the chunk's lower and upper bound, and the block adds the
// slice's values at their places.  Indices within a payload are distinct, so the barrier between
// two ranks (which also publishes the next slice's bounds, kept in alternating slots) is the only
// ordering the sums need.  Then mean and gE, and the chunk is written once: 16-B nontemporal units
// between a scalar head up to the first 16-B boundary of `out` and a scalar tail, a step's gE loads
// before its stores.  V: the values' type on the wire (float, or uint16_t for bf16).
template <bool GE, typename V>
__global__ void __launch_bounds__(256) k_decode_idx16(MixedBatch b, Idx16Batch x, float* __restrict__ out,
                                                      float* __restrict__ gE, const uint8_t* __restrict__ wire,
                                                      int64_t stride, int64_t table_off, const V* __restrict__ vals,
                                                      int nranks, int64_t packed_len, MeanScale sc, float decay) {
    __shared__ __attribute__((aligned(16))) float lds[kChunk + 4];
    __shared__ int64_t s_lb[2][2];
    const int t = blockIdx.y;
    const int64_t n = b.n[t];
    const int64_t c0 = (int64_t)blockIdx.x * kChunk;
    if (c0 >= n) return;
    const int64_t c1 = min<int64_t>(n, c0 + kChunk);
    const int len = (int)(c1 - c0);
    const int wave = threadIdx.x >> 6;
    const int32_t blk = (int32_t)(c0 >> kBlockBits);
    const int32_t nb = blocks_of(n);
    const int32_t base = (int32_t)(c0 & ((1 << kBlockBits) - 1));  // the chunk's start within its block
    float* o = out + b.off[t] + c0;
    float* g = GE ? gE + b.off[t] + c0 : nullptr;
    // the chunk sits in LDS at o's offset within 16 B, so its 16-B units are the bucket's
    float* chunk = lds + (((uintptr_t)o & 15) >> 2);
#pragma unroll
    for (int u = 0; u < kChunk / 4 / 256; ++u)
        reinterpret_cast<vf4_t*>(lds)[threadIdx.x + u * 256] = vf4_t{0.f, 0.f, 0.f, 0.f};
    if (threadIdx.x < 4) lds[kChunk + threadIdx.x] = 0.f;
    for (int r = 0; r < nranks; ++r) {
        const uint8_t* wr = wire + (int64_t)r * stride;
        const uint16_t* lt = reinterpret_cast<const uint16_t*>(wr) + b.koff[t];
        const V* vt = vals + (int64_t)r * packed_len + b.koff[t];
        if (wave < 2) {
            int64_t j0, j1;
            block_slice(reinterpret_cast<const int32_t*>(wr + table_off) + x.tb[t], blk, nb, b.k[t], j0, j1);
            const int64_t lb = wave_lower_bound(lt, j0, j1, wave == 0 ? base : base + len);
            if ((threadIdx.x & 63) == 0) s_lb[r & 1][wave] = lb;
        }
        __syncthreads();
        const int64_t j1 = s_lb[r & 1][1];
        for (int64_t j = s_lb[r & 1][0] + threadIdx.x; j < j1; j += 256) {
            const int e = (int)lt[j] - base;  // both inside the chunk's block
            if (e >= 0 && e < len) chunk[e] += val_f(vt + j);
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

// ---- host ----------------------------------------------------------------------------------
// The format for the shared driver (sparse_index_wire.h): the body is lo16, packed_len halves; the table
// is T, a tensor's blocks at tb.
struct Idx16Wire {
    using Batch = Idx16Batch;
    using Body = uint16_t;
    static void place(WireLayout<Batch>& L, int64_t& body, int64_t& table) {
        for (int32_t t = 0; t < L.bs.nt; ++t) {
            L.xb[t / kB].tb[t % kB] = table;
            table += (L.bs.b[t / kB].n[t % kB] + (1 << kBlockBits) - 1) >> kBlockBits;
        }
        body = L.packed_len;
    }
    static void pads(Batch& x0, int64_t body, int32_t n_body, int64_t table, int32_t n_table) {
        x0.pad_lo = body, x0.n_pad_lo = n_body;
        x0.pad_t = table, x0.n_pad_t = n_table;
    }
    static unsigned pack_grid_x(const Batches& bs, size_t q) {
        const int64_t steps = (bs.maxk[q] + 8 * 256 * kUnits - 1) / (8 * 256 * kUnits);
        return (unsigned)std::max<int64_t>(1, std::min<int64_t>(2048, steps));
    }
    static unsigned unpack_grid_x(const Batches& bs, size_t q) {
        return (unsigned)((bs.maxn[q] + (1 << kBlockBits) - 1) >> kBlockBits);
    }
    static constexpr auto pack_kernel = k_idx16_pack;
    static constexpr auto unpack_kernel = k_idx16_unpack;
    template <bool GE, typename V>
    static constexpr auto decode_kernel = k_decode_idx16<GE, V>;
};

}  // namespace

extern "C" int64_t arctopk_sparse_idx16_bytes(int64_t numel, int32_t nt, const int64_t* offsets, const int64_t* ks,
                                              const int64_t* k_off) {
    return wire_bytes<Idx16Wire>(numel, nt, offsets, ks, k_off);
}

extern "C" int arctopk_sparse_idx16_pack(int64_t numel, int32_t nt, const int64_t* offsets, const int64_t* ks,
                                         const int64_t* k_off, const int32_t* idx, void* wire, void* stream) {
    return wire_pack<Idx16Wire>(numel, nt, offsets, ks, k_off, idx, wire, stream);
}

extern "C" int arctopk_sparse_idx16_unpack(int64_t numel, int32_t nt, const int64_t* offsets, const int64_t* ks,
                                           const int64_t* k_off, int64_t packed_len, const void* wire,
                                           int64_t wire_stride_bytes, int32_t nranks, int32_t* idx_out,
                                           void* stream) {
    return wire_unpack<Idx16Wire>(numel, nt, offsets, ks, k_off, packed_len, wire, wire_stride_bytes, nranks, idx_out,
                                  stream);
}

extern "C" int arctopk_sparse_decode_idx16(void* out, int64_t numel, int32_t nt, const int64_t* offsets,
                                           const int64_t* ks, const int64_t* k_off, int64_t packed_len,
                                           const void* wire, int64_t wire_stride_bytes, const void* vals,
                                           int32_t val_dtype, int32_t nranks, int32_t world_size, void* gE,
                                           float decay, void* stream) {
    return wire_decode<Idx16Wire>(out, numel, nt, offsets, ks, k_off, packed_len, wire, wire_stride_bytes, vals,
                                  val_dtype, nranks, world_size, gE, decay, stream);
}
