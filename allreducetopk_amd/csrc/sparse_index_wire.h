// The host side the index-wire formats share (sparse_idx16.hip, sparse_bitmap.hip; include/arctopk.h):
// one rank's payload is a body (the format's own entries), zero padding to 16 B, a table of int32
// entries, zero padding to 16 B.  Here, once: the checked layout, what a reader checks of the gathered
// payloads, and the bodies of the four entries (bytes, pack, unpack, decode) over the format's traits F:
//
//   F::Batch         the per-batch struct its kernels take next to a MixedBatch
//   F::Body          the type of a body entry (its size is the body's unit)
//   F::place(L, body, table)    fills every tensor's bases in L.xb; the body's and the table's entries
//   F::pads(x0, body, n_body, table, n_table)   batch 0's pad fields: n_body zero entries behind the
//                    body's `body`, n_table behind the table's `table`
//   F::pack_grid_x(bs, q), F::unpack_grid_x(bs, q)   the x-dimension of batch q's grids
//   F::pack_kernel, F::unpack_kernel, F::decode_kernel<GE, V>   the kernels
#pragma once

#include <hip/hip_runtime.h>

#include <vector>

#include "common.h"
#include "mixed_common.h"
#include "sparse_chunk.h"
#include "sparse_common.h"

namespace {

inline int64_t up16(int64_t bytes) { return (bytes + 15) & ~(int64_t)15; }

// The checked layout and the format's geometry: table_off, the byte offset of the table; bytes, one
// rank's whole payload.
template <typename X>
struct WireLayout {
    Batches bs;
    std::vector<X> xb;
    int64_t packed_len, table_off, bytes;
};

// ARCTOPK_EINVAL as fill_batches
template <typename F>
int wire_layout(WireLayout<typename F::Batch>& L, int64_t numel, int32_t nt, const int64_t* offsets, const int64_t* ks,
                const int64_t* k_off) {
    if (!offsets || !ks || !k_off || nt < 1 || numel < 1) return ARCTOPK_EINVAL;
    L.packed_len = k_off[nt - 1] + ks[nt - 1];
    const int e = fill_batches(L.bs, nt, numel, offsets, ks, k_off, L.packed_len);
    if (e) return e;
    L.xb.assign(L.bs.b.size(), typename F::Batch{});
    int64_t body = 0, table = 0;
    F::place(L, body, table);
    constexpr int64_t unit = sizeof(typename F::Body);
    L.table_off = up16(unit * body);
    L.bytes = L.table_off + up16(4 * table);
    F::pads(L.xb[0], body, (int32_t)(L.table_off / unit - body), table, (int32_t)((L.bytes - L.table_off) / 4 - table));
    return 0;
}

// what the two readers check of the gathered payloads
template <typename X>
int wire_ok(const WireLayout<X>& L, int64_t packed_len, const void* wire, int64_t stride, int32_t nranks) {
    if (!wire || arctopk::low_bits(wire, 3) || nranks < 1 || nranks > 65535) return ARCTOPK_EINVAL;
    if (packed_len != L.packed_len || stride < L.bytes || (stride & 3)) return ARCTOPK_EINVAL;
    return 0;
}

template <typename F>
int64_t wire_bytes(int64_t numel, int32_t nt, const int64_t* offsets, const int64_t* ks, const int64_t* k_off) {
    WireLayout<typename F::Batch> L;
    const int e = wire_layout<F>(L, numel, nt, offsets, ks, k_off);
    return e ? -(int64_t)e : L.bytes;
}

template <typename F>
int wire_pack(int64_t numel, int32_t nt, const int64_t* offsets, const int64_t* ks, const int64_t* k_off,
              const int32_t* idx, void* wire, void* stream) {
    if (!idx || !wire || arctopk::low_bits(idx, 3) || arctopk::low_bits(wire, 3)) return ARCTOPK_EINVAL;
    WireLayout<typename F::Batch> L;
    const int e0 = wire_layout<F>(L, numel, nt, offsets, ks, k_off);
    if (e0) return e0;
    typename F::Body* body = static_cast<typename F::Body*>(wire);
    int32_t* table = reinterpret_cast<int32_t*>(static_cast<uint8_t*>(wire) + L.table_off);
    return launch_batches(L.bs, [&](size_t q) {
        hipLaunchKernelGGL(F::pack_kernel, dim3(F::pack_grid_x(L.bs, q), L.bs.count(q)), dim3(256), 0,
                           (hipStream_t)stream, L.bs.b[q], L.xb[q], idx, body, table);
    });
}

template <typename F>
int wire_unpack(int64_t numel, int32_t nt, const int64_t* offsets, const int64_t* ks, const int64_t* k_off,
                int64_t packed_len, const void* wire, int64_t wire_stride_bytes, int32_t nranks, int32_t* idx_out,
                void* stream) {
    if (!idx_out || arctopk::low_bits(idx_out, 3)) return ARCTOPK_EINVAL;
    WireLayout<typename F::Batch> L;
    const int e0 = wire_layout<F>(L, numel, nt, offsets, ks, k_off);
    if (e0) return e0;
    const int e1 = wire_ok(L, packed_len, wire, wire_stride_bytes, nranks);
    if (e1) return e1;
    return launch_batches(L.bs, [&](size_t q) {
        hipLaunchKernelGGL(F::unpack_kernel, dim3(F::unpack_grid_x(L.bs, q), L.bs.count(q), nranks), dim3(256), 0,
                           (hipStream_t)stream, L.bs.b[q], L.xb[q], static_cast<const uint8_t*>(wire),
                           wire_stride_bytes, L.table_off, packed_len, idx_out);
    });
}

template <typename F>
int wire_decode(void* out, int64_t numel, int32_t nt, const int64_t* offsets, const int64_t* ks, const int64_t* k_off,
                int64_t packed_len, const void* wire, int64_t wire_stride_bytes, const void* vals, int32_t val_dtype,
                int32_t nranks, int32_t world_size, void* gE, float decay, void* stream) {
    if (!out || !vals || world_size < 1 || (val_dtype != ARCTOPK_F32 && val_dtype != ARCTOPK_BF16))
        return ARCTOPK_EINVAL;
    if (arctopk::low_bits(out, 3) || arctopk::low_bits(gE, 3) ||
        arctopk::low_bits(vals, val_dtype == ARCTOPK_F32 ? 3 : 1))
        return ARCTOPK_EINVAL;
    WireLayout<typename F::Batch> L;
    const int e0 = wire_layout<F>(L, numel, nt, offsets, ks, k_off);
    if (e0) return e0;
    const int e1 = wire_ok(L, packed_len, wire, wire_stride_bytes, nranks);
    if (e1) return e1;
    // the tensors tile [offsets[0], numel) in order (fill_batches); only from 0 do the chunks cover
    // the bucket, and every element has to be written
    if (offsets[0] != 0) return ARCTOPK_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    float* o = static_cast<float*>(out);
    float* ge = static_cast<float*>(gE);
    const uint8_t* w = static_cast<const uint8_t*>(wire);
    const arctopk::MeanScale sc = arctopk::make_mean_scale(world_size);
    return launch_batches(L.bs, [&](size_t q) {
        const dim3 grid((unsigned)((L.bs.maxn[q] + kChunk - 1) / kChunk), L.bs.count(q));
#define ARCTOPK_WIRE_DECODE(GE, V)                                                                               \
    hipLaunchKernelGGL((F::template decode_kernel<GE, V>), grid, dim3(256), 0, st, L.bs.b[q], L.xb[q], o, ge, w,  \
                       wire_stride_bytes, L.table_off, static_cast<const V*>(vals), nranks, packed_len, sc, decay)
        if (val_dtype == ARCTOPK_F32) {
            if (ge) ARCTOPK_WIRE_DECODE(true, float);
            else ARCTOPK_WIRE_DECODE(false, float);
        } else {
            if (ge) ARCTOPK_WIRE_DECODE(true, uint16_t);
            else ARCTOPK_WIRE_DECODE(false, uint16_t);
        }
#undef ARCTOPK_WIRE_DECODE
    });
}

}  // namespace
