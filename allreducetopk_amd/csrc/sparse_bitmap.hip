// TopK's indices as a per-tensor bitmap on the wire (SparseState.index_wire = "bitmap", DESIGN.md
// section 4j) on MI355X (gfx950).  Every tensor's indices are tensor-relative and ascending
// (arctopk_topk_select, arctopk_seg_select by row), so one rank's index payload is
//
//   W[wb_i + e / 32] bit e % 32   set iff element e of tensor i is selected; ceil(n_i / 32) uint32 per
//                                 tensor, bits at or above n_i zero, zero padding to 16 B
//   C[cb_i + c] = #{indices of tensor i below c * 4096}   one int32 per 4096-element chunk of every
//                                 tensor, zero padding to 16 B
//
// (include/arctopk.h).  Selected element e of tensor i has its value at
// k_off[i] + C[cb_i + e / 4096] + popcount(the chunk's bits below e).
//
//   pack     a block takes kSpan consecutive chunks of a tensor: one wave per chunk finds the lower
//            bound of the chunk's first element in the tensor's index slice (the chunk's table entry),
//            the block sets the slice's bits in LDS with ds_or and streams the span's words out once
//   decode   k_decode_idx16's work split (a block composes a 4096-element chunk of a tensor from all
//            ranks in rank order), but no search and no LDS chunk: per rank 128 lanes load the chunk's
//            128 words and scan their popcounts, and every thread keeps the 16 sums of the four 16-B
//            output units it owns in registers, finding a set bit's value by popcount
//   unpack   block (chunk, tensor, rank), the same word / prefix / base step; a set bit's owner writes
//            its int32 index at the bit's position, for the decodes that read int32 indices
//
// What comes from other ranks is never trusted with an address: a table entry is clamped to
// [0, ks], a position at or beyond ks is skipped, bits at or above n_i are masked.
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
constexpr int kGroup = 4096;           // elements per table entry of the format (include/arctopk.h)
constexpr int kWords = kGroup / 32;    // bitmap words of a group
static_assert(kGroup == kChunk, "the format's table has one entry per decode chunk (sparse_chunk.h)");
static_assert(kWords == 128 && kChunk / 4 == 256 * kUnits, "two waves load a chunk's words; a thread owns kUnits units");
#ifndef ARCTOPK_BITMAP_SPAN
#define ARCTOPK_BITMAP_SPAN 4
#endif
constexpr int kSpan = ARCTOPK_BITMAP_SPAN;  // chunks a pack block takes (measured: DESIGN.md section 4j)

// next to a MixedBatch: where each tensor's words and table entries start, and (first batch only)
// the padding the pack zeroes: words [pad_w, pad_w + n_pad_w), table entries [pad_c, pad_c + n_pad_c)
struct BitmapBatch {
    int64_t wb[kB];
    int64_t cb[kB];
    int64_t pad_w, pad_c;
    int32_t n_pad_w, n_pad_c;
};

__device__ __forceinline__ int64_t chunks_of(int64_t n) { return (n + kChunk - 1) / kChunk; }

// ---- pack ----------------------------------------------------------------------------------
// block (x, y): chunks [kSpan x, kSpan (x + 1)) of tensor y.  Wave w finds the bound of chunk
// kSpan x + w (its table entry), wave 0 also the span's end (the next chunk's bound; k behind the
// tensor's last chunk).  The words of the span start as zeros in LDS; the block walks the index
// slice between the first and the last bound, 256 consecutive entries a step, and sets each
// entry's bit unless it lies outside the span; then the words go out once, in 16-B nontemporal
// units where the span's place in W is 16-B aligned.  Indices that do not ascend give some
// bounds in [0, k] and so some payload: every store is to the span's own words and entries.
__global__ void __launch_bounds__(256) k_bitmap_pack(MixedBatch b, BitmapBatch x, const int32_t* __restrict__ idx,
                                                     uint32_t* __restrict__ W, int32_t* __restrict__ C) {
    __shared__ __attribute__((aligned(16))) uint32_t s_w[kSpan * kWords];
    __shared__ int64_t s_lb[kSpan + 1];
    const int t = blockIdx.y;
    if (blockIdx.x == 0 && t == 0) {
        if ((int)threadIdx.x < x.n_pad_w) W[x.pad_w + threadIdx.x] = 0;
        if ((int)threadIdx.x < x.n_pad_c) C[x.pad_c + threadIdx.x] = 0;
    }
    const int64_t n = b.n[t];
    const int64_t k = b.k[t];
    const int64_t nc = chunks_of(n);
    const int64_t ch0 = (int64_t)blockIdx.x * kSpan;
    if (ch0 >= nc) return;
    const int32_t* it = idx + b.koff[t];
    const int wave = threadIdx.x >> 6;
    for (int q = wave; q <= kSpan; q += 4) {
        const int64_t ch = ch0 + q;
        const int64_t lb = ch < nc ? wave_lower_bound(it, 0, k, (int32_t)(ch * kChunk)) : k;
        if ((threadIdx.x & 63) == 0) {
            s_lb[q] = lb;
            if (q < kSpan && ch < nc) C[x.cb[t] + ch] = (int32_t)lb;
        }
    }
    for (int u = threadIdx.x; u < kSpan * kWords / 4; u += 256) reinterpret_cast<u4_t*>(s_w)[u] = u4_t{0u, 0u, 0u, 0u};
    __syncthreads();
    const int64_t e0 = ch0 * kChunk;
    const int64_t len = min<int64_t>(n - e0, (int64_t)kSpan * kChunk);
    const int64_t j1 = s_lb[kSpan];
    for (int64_t j = s_lb[0] + threadIdx.x; j < j1; j += 256) {
        const int64_t e = (int64_t)it[j] - e0;
        if (e >= 0 && e < len) atomicOr(&s_w[e >> 5], 1u << (e & 31));
    }
    __syncthreads();
    uint32_t* Wt = W + x.wb[t] + ch0 * kWords;
    const int nsw = (int)((len + 31) >> 5);  // the span's words: the tensor's last one included
    const int nu = ((uintptr_t)Wt & 15) == 0 ? nsw / 4 : 0;
    for (int u = threadIdx.x; u < nu; u += 256)
        __builtin_nontemporal_store(reinterpret_cast<const u4_t*>(s_w)[u], reinterpret_cast<u4_t*>(Wt) + u);
    for (int i = 4 * nu + threadIdx.x; i < nsw; i += 256) Wt[i] = s_w[i];
}

// ---- what a reader takes from one rank's payload -----------------------------------------
// One rank's view of a chunk, in one of two alternating slots: the chunk's 128 words (a word past the
// tensor's last reads as zero, the last is masked to n), each word's exclusive popcount prefix within
// its wave of 64 words, the first 64 words' total (which the readers of words 64.. add), and the
// chunk's base: its table entry clamped to [0, ks].
struct ChunkBits {
    uint32_t word[2][kWords];
    uint32_t pre[2][kWords];
    uint32_t tot[2];
    uint32_t base[2];
};

// threads 0..127 (waves 0 and 1): which bits of the thread's word of the chunk lie inside the tensor
__device__ __forceinline__ uint32_t word_mask(int64_t chunk, int64_t n) {
    const int64_t rem = n - (chunk * kWords + threadIdx.x) * 32;
    return rem >= 32 ? ~0u : rem > 0 ? (1u << rem) - 1u : 0u;
}

// ... the raw loads of one rank's payload `wr`: the thread's word (where any of it lies inside the tensor)
// and the chunk's table entry.  Nothing is computed from them here, so a caller may issue them early.
__device__ __forceinline__ void load_bits(const uint8_t* __restrict__ wr, int64_t table_off, int64_t wb, int64_t cb,
                                          int64_t chunk, uint32_t mask, uint32_t& w, int32_t& c) {
    w = 0u;
    if (mask) w = reinterpret_cast<const uint32_t*>(wr)[wb + chunk * kWords + threadIdx.x];
    c = reinterpret_cast<const int32_t*>(wr + table_off)[cb + chunk];
}

// ... and publish them, masked and clamped, in slot `slot`; the caller's barrier follows
__device__ __forceinline__ void publish_bits(ChunkBits& s, int slot, uint32_t w, uint32_t mask, int32_t c, int64_t ks) {
    w &= mask;
    const int l = threadIdx.x;  // < 128
    const uint32_t pc = __popc(w);
    uint32_t inc = pc;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(inc, d);
        if ((l & 63) >= d) inc += o;
    }
    s.word[slot][l] = w;
    s.pre[slot][l] = inc - pc;
    if (l == 63) s.tot[slot] = inc;
    if (l == 0) s.base[slot] = (uint32_t)min<int64_t>(max<int64_t>(c, 0), ks);
}

// The 16-B unit `u` (of 1024) of the chunk as slot `slot` holds it: its four membership bits, and the
// position (in the tensor's ks values) of the first of them that is set.  At most 2^31 + 4095.
__device__ __forceinline__ uint32_t unit_bits(const ChunkBits& s, int slot, int u, uint32_t& pos) {
    const int wi = u >> 3;
    const int sh = (u & 7) * 4;
    const uint32_t w = s.word[slot][wi];
    pos = s.base[slot] + s.pre[slot][wi] + (wi >= 64 ? s.tot[slot] : 0u) + __popc(w & ((1u << sh) - 1u));
    return (w >> sh) & 15u;
}

// ---- unpack --------------------------------------------------------------------------------
// block (chunk, tensor, rank): the owner of a set bit writes chunk start + bit at the bit's position
__global__ void __launch_bounds__(256) k_bitmap_unpack(MixedBatch b, BitmapBatch x, const uint8_t* __restrict__ wire,
                                                       int64_t stride, int64_t table_off, int64_t packed_len,
                                                       int32_t* __restrict__ idx_out) {
    __shared__ ChunkBits s;
    const int t = blockIdx.y;
    const int64_t n = b.n[t];
    const int64_t c0 = (int64_t)blockIdx.x * kChunk;
    if (c0 >= n) return;
    const uint8_t* wr = wire + (int64_t)blockIdx.z * stride;
    const uint32_t ks = (uint32_t)b.k[t];
    if (threadIdx.x < kWords) {
        const uint32_t mask = word_mask(blockIdx.x, n);
        uint32_t w;
        int32_t c;
        load_bits(wr, table_off, x.wb[t], x.cb[t], blockIdx.x, mask, w, c);
        publish_bits(s, 0, w, mask, c, b.k[t]);
    }
    __syncthreads();
    int32_t* ot = idx_out + (int64_t)blockIdx.z * packed_len + b.koff[t];
#pragma unroll
    for (int q = 0; q < kUnits; ++q) {
        const int u = threadIdx.x + q * 256;
        uint32_t pos;
        const uint32_t nib = unit_bits(s, 0, u, pos);
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if ((nib >> e) & 1u) {
                if (pos < ks) ot[pos] = (int32_t)(c0 + 4 * u + e);
                ++pos;
            }
    }
}

// ---- decode --------------------------------------------------------------------------------
// a value as its load leaves it in a register (bf16: zero-extended), and as the fp32 it stands for
template <typename V> struct RawOf { using type = float; };
template <> struct RawOf<uint16_t> { using type = uint32_t; };
__device__ __forceinline__ float val_f(float v) { return v; }
__device__ __forceinline__ float val_f(uint32_t v) { return bf_bits_f(v); }

// block (x, y) composes elements [4096 x, 4096 (x + 1)) of tensor y.  Thread t owns the 16-B units
// t + 256 q (q < kUnits) of the chunk for every rank, their 16 sums in registers from 0.0f.  For each
// rank in order, waves 0 and 1 publish the rank's view of the chunk in slot r & 1 (the one barrier of
// the rank: a slot is rewritten two ranks later, behind the barrier in between) and load the next rank's
// words, so that load runs beside this rank's value loads; every thread adds the values of its units'
// set bits.  Then mean and gE, and the units are written once: where the
// chunk's place in `out` (and in gE) is 16-B aligned, straight from registers as 16-B nontemporal
// stores, the gE loads before the first store; otherwise element by element.  (A misaligned chunk
// means a tensor at an element offset that is no multiple of 4: staging 16 KiB in LDS for those, as
// k_decode_idx16 does, would cost every block its occupancy for what real buckets rarely hold.)
// V: the values' type on the wire (float, or uint16_t for bf16).
template <bool GE, typename V>
__global__ void __launch_bounds__(256) k_decode_bitmap(MixedBatch b, BitmapBatch x, float* __restrict__ out,
                                                       float* __restrict__ gE, const uint8_t* __restrict__ wire,
                                                       int64_t stride, int64_t table_off, const V* __restrict__ vals,
                                                       int nranks, int64_t packed_len, MeanScale sc, float decay) {
    __shared__ ChunkBits s;
    const int t = blockIdx.y;
    const int64_t n = b.n[t];
    const int64_t c0 = (int64_t)blockIdx.x * kChunk;
    if (c0 >= n) return;
    const int len = (int)min<int64_t>(n - c0, kChunk);
    const uint32_t ks = (uint32_t)b.k[t];
    float sum[kUnits][4];
#pragma unroll
    for (int q = 0; q < kUnits; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) sum[q][e] = 0.f;
    // waves 0 and 1: the next rank's word and table entry, loaded a rank ahead
    const uint32_t mask = threadIdx.x < kWords ? word_mask(blockIdx.x, n) : 0u;
    uint32_t w = 0;
    int32_t c = 0;
    if (threadIdx.x < kWords) load_bits(wire, table_off, x.wb[t], x.cb[t], blockIdx.x, mask, w, c);
    for (int r = 0; r < nranks; ++r) {
        const V* vt = vals + (int64_t)r * packed_len + b.koff[t];
        if (threadIdx.x < kWords) publish_bits(s, r & 1, w, mask, c, b.k[t]);
        __syncthreads();
        if (threadIdx.x < kWords && r + 1 < nranks)
            load_bits(wire + (int64_t)(r + 1) * stride, table_off, x.wb[t], x.cb[t], blockIdx.x, mask, w, c);
        // every value load of the rank is issued, raw, before the first conversion and add, so nothing
        // serialises them (the empty asm keeps the compiler from moving bf16's shift up behind each load,
        // where it would wait for that load alone)
        typename RawOf<V>::type v[kUnits][4];
        uint32_t on = 0;
#pragma unroll
        for (int q = 0; q < kUnits; ++q) {
            uint32_t pos;
            const uint32_t nib = unit_bits(s, r & 1, threadIdx.x + q * 256, pos);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const uint32_t bit = (nib >> e) & 1u;
                const bool sel = bit && pos < ks;
                v[q][e] = 0;
                if (sel) v[q][e] = vt[pos];
                on |= (uint32_t)sel << (4 * q + e);
                pos += bit;
            }
        }
#pragma unroll
        for (int q = 0; q < kUnits; ++q)
#pragma unroll
            for (int e = 0; e < 4; ++e) asm volatile("" : "+v"(v[q][e]));
#pragma unroll
        for (int q = 0; q < kUnits; ++q)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if ((on >> (4 * q + e)) & 1u) sum[q][e] += val_f(v[q][e]);
    }
    float* o = out + b.off[t] + c0;
    float* g = GE ? gE + b.off[t] + c0 : nullptr;
    const bool vec = (((uintptr_t)o | (GE ? (uintptr_t)g : 0)) & 15) == 0;
    vf4_t ge[kUnits];
    if (vec && len == kChunk) {  // a whole aligned chunk: kUnits gE loads in flight, then the stores
#pragma unroll
        for (int q = 0; q < kUnits; ++q)
            if (GE) ge[q] = ld_f4_nt(g + 4 * (threadIdx.x + q * 256));
#pragma unroll
        for (int q = 0; q < kUnits; ++q) {
            const int e0 = 4 * (threadIdx.x + q * 256);
            vf4_t r;
            r.x = final1<GE>(sum[q][0], GE ? ge[q].x : 0.f, sc, decay);
            r.y = final1<GE>(sum[q][1], GE ? ge[q].y : 0.f, sc, decay);
            r.z = final1<GE>(sum[q][2], GE ? ge[q].z : 0.f, sc, decay);
            r.w = final1<GE>(sum[q][3], GE ? ge[q].w : 0.f, sc, decay);
            if (GE) st_f4_nt(g + e0, r);
            st_f4_nt(o + e0, r);
        }
        return;
    }
    // a chunk's aligned units before the tensor's end, and everything else element by element
    if constexpr (GE) {
#pragma unroll
        for (int q = 0; q < kUnits; ++q) {
            const int e0 = 4 * (threadIdx.x + q * 256);
            if (vec && e0 + 4 <= len) {
                ge[q] = ld_f4_nt(g + e0);
            } else {
                ge[q].x = e0 < len ? g[e0] : 0.f;
                ge[q].y = e0 + 1 < len ? g[e0 + 1] : 0.f;
                ge[q].z = e0 + 2 < len ? g[e0 + 2] : 0.f;
                ge[q].w = e0 + 3 < len ? g[e0 + 3] : 0.f;
            }
        }
    }
#pragma unroll
    for (int q = 0; q < kUnits; ++q) {
        const int e0 = 4 * (threadIdx.x + q * 256);
        vf4_t r;
        r.x = final1<GE>(sum[q][0], GE ? ge[q].x : 0.f, sc, decay);
        r.y = final1<GE>(sum[q][1], GE ? ge[q].y : 0.f, sc, decay);
        r.z = final1<GE>(sum[q][2], GE ? ge[q].z : 0.f, sc, decay);
        r.w = final1<GE>(sum[q][3], GE ? ge[q].w : 0.f, sc, decay);
        if (vec && e0 + 4 <= len) {
            if (GE) st_f4_nt(g + e0, r);
            st_f4_nt(o + e0, r);
        } else {
            const float rr[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (e0 + e < len) {
                    if (GE) g[e0 + e] = rr[e];
                    o[e0 + e] = rr[e];
                }
        }
    }
}

// ---- host ----------------------------------------------------------------------------------
// The format for the shared driver (sparse_index_wire.h): the body is W, a tensor's words at wb; the
// table is C, a tensor's chunks at cb.
struct BitmapWire {
    using Batch = BitmapBatch;
    using Body = uint32_t;
    static void place(WireLayout<Batch>& L, int64_t& body, int64_t& table) {
        for (int32_t t = 0; t < L.bs.nt; ++t) {
            const int64_t n = L.bs.b[t / kB].n[t % kB];
            L.xb[t / kB].wb[t % kB] = body;
            L.xb[t / kB].cb[t % kB] = table;
            body += (n + 31) >> 5;
            table += (n + kChunk - 1) / kChunk;
        }
    }
    static void pads(Batch& x0, int64_t body, int32_t n_body, int64_t table, int32_t n_table) {
        x0.pad_w = body, x0.n_pad_w = n_body;
        x0.pad_c = table, x0.n_pad_c = n_table;
    }
    static unsigned pack_grid_x(const Batches& bs, size_t q) {
        const int64_t span = (int64_t)kSpan * kChunk;
        return (unsigned)((bs.maxn[q] + span - 1) / span);
    }
    static unsigned unpack_grid_x(const Batches& bs, size_t q) { return (unsigned)((bs.maxn[q] + kChunk - 1) / kChunk); }
    static constexpr auto pack_kernel = k_bitmap_pack;
    static constexpr auto unpack_kernel = k_bitmap_unpack;
    template <bool GE, typename V>
    static constexpr auto decode_kernel = k_decode_bitmap<GE, V>;
};

}  // namespace

extern "C" int64_t arctopk_sparse_bitmap_bytes(int64_t numel, int32_t nt, const int64_t* offsets, const int64_t* ks,
                                               const int64_t* k_off) {
    return wire_bytes<BitmapWire>(numel, nt, offsets, ks, k_off);
}

extern "C" int arctopk_sparse_bitmap_pack(int64_t numel, int32_t nt, const int64_t* offsets, const int64_t* ks,
                                          const int64_t* k_off, const int32_t* idx, void* wire, void* stream) {
    return wire_pack<BitmapWire>(numel, nt, offsets, ks, k_off, idx, wire, stream);
}

extern "C" int arctopk_sparse_bitmap_unpack(int64_t numel, int32_t nt, const int64_t* offsets, const int64_t* ks,
                                            const int64_t* k_off, int64_t packed_len, const void* wire,
                                            int64_t wire_stride_bytes, int32_t nranks, int32_t* idx_out,
                                            void* stream) {
    return wire_unpack<BitmapWire>(numel, nt, offsets, ks, k_off, packed_len, wire, wire_stride_bytes, nranks, idx_out,
                                   stream);
}

extern "C" int arctopk_sparse_decode_bitmap(void* out, int64_t numel, int32_t nt, const int64_t* offsets,
                                            const int64_t* ks, const int64_t* k_off, int64_t packed_len,
                                            const void* wire, int64_t wire_stride_bytes, const void* vals,
                                            int32_t val_dtype, int32_t nranks, int32_t world_size, void* gE,
                                            float decay, void* stream) {
    return wire_decode<BitmapWire>(out, numel, nt, offsets, ks, k_off, packed_len, wire, wire_stride_bytes, vals,
                                   val_dtype, nranks, world_size, gE, decay, stream);
}
