// The packed values of an fp32 bucket sent as bf16, for MI355X (gfx950): the pack and decode phases
// of an fp32 plan whose packed all-reduce carries bf16 (GroupTopKState.wire_dtype, DESIGN.md section
// 4f).  Bucket, sketch, projections and residuals stay fp32; only the packed values are 2 bytes.
// With f = bf16 -> fp32 (exact) and b = fp32 -> bf16 (round to nearest even, NaN -> 0x7FC0:
// cvt_pk_bf16 of common.h):
//
//   pack   : selected row, selected element of a RAW segment, every element of a DENSE segment:
//            noef: packed = b(G)
//            EF14: X is the E the encode stored (DENSE: X = G + E or G, formed here);
//                  packed = b(X); E := X - f(packed), one fp32 subtract; other rows keep E = X
//            EF21: D = G - E, one fp32 subtract; packed = b(D); E := E + f(packed), one fp32 add
//   decode : P the all-reduced value, mean = f(P) / ws in fp32 (not rounded to bf16)
//            noef, EF14: out = mean on selected elements, 0 elsewhere
//            EF21: gE := gE + mean on selected elements; out = gE on every element
//
// Encode and select are the plan's own (arctopk_encode, arctopk_select).  `packed` has the plan's
// packed layout in elements, so a segment's bf16 values start 8-B aligned (packed_off % 4 == 0) and
// 16-B aligned only where packed_off % 8 == 0.  The kernels share nothing with the library's other
// kernels but the plan's segment table; the table layouts, their host loops and the small bf16 /
// fp32 16-B helpers are mixed_common.h's, shared with mixed_ef.hip.  The plan's zero-rows record is
// not set (a selected row of E holds its remainder, not zero).
//
// Work mapping.  A plan gets one table of pack chunks and one of decode tiles at its first call
// here (w16_table; freed with the plan), so a phase is one launch and no copy.
//   pack: chunks of about 8192 elements of selected rows; where the segment's `vec` holds (m,
//     offset and packed_off multiples of 4) a thread takes two 16-B units of fp32 per step and
//     stores their 2 x 8 B of bf16 as one 16-B store where the packed address allows (8 elements
//     of one row when m % 8 == 0 and the chunk's packed values start 16-B aligned; else pairs of
//     units with a lone 8-B unit at either end of the chunk), else element by element.  RAW
//     segments: element chunks of selected elements.  DENSE segments:
//     chunks of 8192 elements, in units when the bucket and packed offsets are multiples of 4.
//   decode: tiles of about 8192 elements.  Rows of m >= 4: `lanes` lanes (a power of two, 1 .. 64)
//     share a row, read its slot once (a row ahead) and stream 16-B units of out (and 8 B of
//     packed, 2 x 16 B of gE under EF21); rows of fewer than 512 columns that are no 16-B units
//     (m % 4 != 0, an odd offset): the tile's contiguous element range in 16-B units across rows;
//     rows of fewer than four columns and RAW tensors: a thread per row; DENSE segments: element
//     tiles.
//   scatter (the zero-ahead drain: out is already zero, NONE / EF14): the pack's chunks again, the
//     other way round -- a thread reads 16 B of packed values (8 B at either end of a chunk whose
//     packed values start 8 B off the 16-B grid) and stores their two 16-B units of out; element by
//     element where the segment's `vec` does not hold.  2 B read and 4 B written per selected
//     element, nothing else touched; no LDS.
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <vector>

#include "common.h"
#include "mixed_common.h"

namespace {

using namespace arctopk;

constexpr int kW16Block = 256;
constexpr int64_t kW16PackElems = 8192;   // elements per pack chunk (as mixed_ef.hip's)
constexpr int64_t kW16ShortElems = 4096;  // rows per thread-per-row decode tile
constexpr int kW16Units = 4;              // 16-B units of out a decode lane takes per step
constexpr int64_t kW16DecElems = 8192;    // elements per decode row tile (common.h: ARCTOPK_DEC_CHUNK)
constexpr int64_t kW16FlatMaxM = 512;     // rows below this that are no 16-B units decode as flat element ranges

enum : int32_t { W16P_ROWS = 0, W16P_ROWS_VEC = 1, W16P_DENSE = 2 };  // pack chunk modes
enum : int32_t { W16_VEC = 1, W16_SHORT = 2, W16_DENSE = 4, W16_FLAT = 8 };  // decode tile flags
// the residual rule of a kernel (the ARCTOPK_EF_* codes)
enum W16Ef : int { W16_NONE = ARCTOPK_EF_NONE, W16_EF14 = ARCTOPK_EF14, W16_EF21 = ARCTOPK_EF21 };

using W16Chunk = PackChunk;  // (mixed_common.h)
using W16Tile = RowTile;
using W16Scale = MeanScale;
using wf4_t = vf4_t;

struct W16Tab {      // the plan's work tables (device) and their sizes
    W16Chunk* d_chunks;
    W16Tile* d_tiles;
    int n_chunks, n_tiles;
};

// the 4 bf16 of an 8-B unit as floats
__device__ __forceinline__ wf4_t unpack4(u2_t w) {
    return wf4_t{__uint_as_float(w.x << 16), __uint_as_float(w.x & 0xFFFF0000u),
                 __uint_as_float(w.y << 16), __uint_as_float(w.y & 0xFFFF0000u)};
}

// ---- pack ----------------------------------------------------------------------------------
// What one 16-B unit (4 elements) loads: G where the mode reads it, E where it does.  X of an
// EF14 row is the E the encode stored, so G is not read there (grad may be null:
// arctopk_pack_wire16 allows it for EF14 on a plan without DENSE segments).
template <int EF, bool DENSE>
struct W16Load {
    static constexpr bool kG = EF != W16_EF14 || DENSE;   // G is read
    static constexpr bool kE = EF != W16_NONE;            // E is read (EF14 DENSE: only when err_in)
    wf4_t g, e;
    __device__ __forceinline__ void load(const float* __restrict__ grad, const float* __restrict__ err, int64_t el,
                                         bool err_in) {
        g = wf4_t{0.0f, 0.0f, 0.0f, 0.0f};
        e = wf4_t{0.0f, 0.0f, 0.0f, 0.0f};
        if constexpr (kG) g = ld_f4_nt(grad + el);
        if constexpr (kE) {
            if (!(EF == W16_EF14 && DENSE) || err_in) e = ld_f4_nt(err + el);
        }
    }
};
// ... X, packed = b(X) and the new E of one element (e: 0 when it was not loaded)
template <int EF, bool DENSE>
__device__ __forceinline__ float w16_x(float g, float e, bool err_in) {
    if constexpr (EF == W16_NONE) return g;
    else if constexpr (EF == W16_EF21) return g - e;
    else if constexpr (DENSE) return err_in ? g + e : g;
    else return e;
}
template <int EF>
__device__ __forceinline__ float w16_e(float x, float e, float y) {
    return EF == W16_EF21 ? e + y : x - y;
}
// the unit's packed 8 B; stores its new E (el: its first bucket element)
template <int EF, bool DENSE>
__device__ __forceinline__ u2_t w16_unit(const W16Load<EF, DENSE>& L, float* __restrict__ err, int64_t el, bool err_in) {
    const float x0 = w16_x<EF, DENSE>(L.g.x, L.e.x, err_in), x1 = w16_x<EF, DENSE>(L.g.y, L.e.y, err_in);
    const float x2 = w16_x<EF, DENSE>(L.g.z, L.e.z, err_in), x3 = w16_x<EF, DENSE>(L.g.w, L.e.w, err_in);
    const u2_t w = u2_t{cvt_pk_bf16(x0, x1), cvt_pk_bf16(x2, x3)};
    if constexpr (EF != W16_NONE) {
        const wf4_t y = unpack4(w);
        st_f4_nt(err + el, wf4_t{w16_e<EF>(x0, L.e.x, y.x), w16_e<EF>(x1, L.e.y, y.y),
                                 w16_e<EF>(x2, L.e.z, y.z), w16_e<EF>(x3, L.e.w, y.w)});
    }
    return w;
}
// ... and one element
template <int EF, bool DENSE>
__device__ __forceinline__ void w16_elem(const float* __restrict__ grad, float* __restrict__ err, int64_t el,
                                         bool err_in, bf16_t* __restrict__ p) {
    float g = 0.0f, e = 0.0f;
    if constexpr (W16Load<EF, DENSE>::kG) g = __builtin_nontemporal_load(grad + el);
    if constexpr (W16Load<EF, DENSE>::kE) {
        if (!(EF == W16_EF14 && DENSE) || err_in) e = err[el];
    }
    const float x = w16_x<EF, DENSE>(g, e, err_in);
    const uint16_t w = f_to_bf(x);
    __builtin_nontemporal_store(w, &p->u);
    if constexpr (EF != W16_NONE) err[el] = w16_e<EF>(x, e, bf_bits_f(w));
}

// The nu units of a chunk whose packed values are contiguous from p (8-B aligned): unit u's 4
// elements start at bucket element src(u), or src(u) < 0: the unit is skipped.  A thread takes a
// pair of units whose packed 16 B are aligned (one 16-B store), a lone unit at either end of the
// chunk (one 8-B store); all loads of the step are issued before its stores.
template <int EF, bool DENSE, class Src>
__device__ __forceinline__ void w16_pairs(const float* __restrict__ grad, float* __restrict__ err, bool err_in,
                                          bf16_t* __restrict__ p, int nu, Src src) {
    const int head = ((uintptr_t)p & 15) ? 1 : 0;  // a lone first unit brings the pairs to 16 B
    const int nitems = (nu + head + 1) / 2;
    for (int it = threadIdx.x; it < nitems; it += kW16Block) {
        const int ua = 2 * it - head, ub = ua + 1;
        const int64_t ea = ua >= 0 ? src(ua) : -1, eb = ub < nu ? src(ub) : -1;
        W16Load<EF, DENSE> la, lb;
        if (ea >= 0) la.load(grad, err, ea, err_in);
        if (eb >= 0) lb.load(grad, err, eb, err_in);
        u2_t wa = u2_t{0u, 0u}, wb = u2_t{0u, 0u};
        if (ea >= 0) wa = w16_unit<EF, DENSE>(la, err, ea, err_in);
        if (eb >= 0) wb = w16_unit<EF, DENSE>(lb, err, eb, err_in);
        if (ea >= 0 && eb >= 0) {
            __builtin_nontemporal_store(u4_t{wa.x, wa.y, wb.x, wb.y}, reinterpret_cast<u4_t*>(p + 4 * (int64_t)ua));
        } else if (ea >= 0) {
            __builtin_nontemporal_store(wa, reinterpret_cast<u2_t*>(p + 4 * (int64_t)ua));
        } else if (eb >= 0) {
            __builtin_nontemporal_store(wb, reinterpret_cast<u2_t*>(p + 4 * (int64_t)ub));
        }
    }
}

template <int EF>
__global__ void __launch_bounds__(kW16Block) k_w16_pack(const SegDev* __restrict__ segs,
                                                       const W16Chunk* __restrict__ chunks,
                                                       const float* __restrict__ grad, float* __restrict__ err,
                                                       int err_in, const int32_t* __restrict__ rowlist,
                                                       bf16_t* __restrict__ packed) {
    const W16Chunk ch = chunks[blockIdx.x];
    const SegDev& s = segs[ch.seg];
    const int m = (int)s.m;
    const bool ein = err_in != 0;
    if (ch.mode == W16P_DENSE) {  // every element is selected (and has no encode work: X is formed here)
        const int64_t e0 = s.offset + ch.j0;
        bf16_t* p = packed + s.packed_off + ch.j0;
        int done = 0;
        if (s.offset % 4 == 0 && s.packed_off % 4 == 0) {  // (chunks start at multiples of 8 elements)
            const int nu = ch.nj / 4;
            w16_pairs<EF, true>(grad, err, ein, p, nu, [&](int u) { return e0 + 4 * (int64_t)u; });
            done = nu * 4;
        }
        for (int i = done + (int)threadIdx.x; i < ch.nj; i += kW16Block) w16_elem<EF, true>(grad, err, e0 + i, ein, p + i);
        return;
    }
    const int32_t* rl = rowlist + s.sel_off + ch.j0;
    bf16_t* p = packed + s.packed_off + ch.j0 * (int64_t)m;
    if (ch.mode == W16P_ROWS_VEC) {
        if (m % 8 == 0 && ((uintptr_t)p & 15) == 0) {  // 8 elements of one row per thread: one 16-B packed store
            const int U8 = m / 8, n8 = ch.nj * U8;
            for (int u = threadIdx.x; u < n8; u += kW16Block) {
                const int jj = u / U8, c8 = u - jj * U8;
                const int64_t row = rl[jj];
                if ((uint64_t)row >= (uint64_t)s.n) continue;  // (never, for a select's row list)
                const int64_t el = s.offset + row * (int64_t)m + 8 * c8;
                W16Load<EF, false> la, lb;
                la.load(grad, err, el, ein);
                lb.load(grad, err, el + 4, ein);
                const u2_t wa = w16_unit<EF, false>(la, err, el, ein), wb = w16_unit<EF, false>(lb, err, el + 4, ein);
                __builtin_nontemporal_store(u4_t{wa.x, wa.y, wb.x, wb.y}, reinterpret_cast<u4_t*>(p + 8 * (int64_t)u));
            }
            return;
        }
        const int U = m / 4;
        w16_pairs<EF, false>(grad, err, ein, p, ch.nj * U, [&](int u) -> int64_t {
            const int jj = u / U, c4 = u - jj * U;
            const int64_t row = rl[jj];
            if ((uint64_t)row >= (uint64_t)s.n) return -1;  // (never, for a select's row list)
            return s.offset + row * (int64_t)m + 4 * c4;
        });
        return;
    }
    const int ne = ch.nj * m;
    for (int i = threadIdx.x; i < ne; i += kW16Block) {
        const int jj = i / m, c = i - jj * m;
        const int64_t row = rl[jj];
        if ((uint64_t)row >= (uint64_t)s.n) continue;
        w16_elem<EF, false>(grad, err, s.offset + row * (int64_t)m + c, ein, p + i);
    }
}

// ---- decode --------------------------------------------------------------------------------
__device__ __forceinline__ wf4_t w16_mean4(u2_t w, const W16Scale sc) {
    const wf4_t y = unpack4(w);
    return wf4_t{sc(y.x), sc(y.y), sc(y.z), sc(y.w)};
}
// one element: out, and gE on a selected element under EF21
template <int EF>
__device__ __forceinline__ void w16_dec_elem(const bf16_t* __restrict__ pk, bool sel, const W16Scale sc,
                                             float* __restrict__ gerr, float* __restrict__ out, int64_t el) {
    float x = 0.0f;
    if constexpr (EF == W16_EF21) x = gerr[el];
    if (sel) {
        const float mean = sc(to_f(*pk));
        if constexpr (EF == W16_EF21) {
            x += mean;
            gerr[el] = x;
        } else {
            x = mean;
        }
    }
    out[el] = x;
}

// One decode tile of rows of m >= 4 columns: `lanes` lanes per row, the row's slot read once.
template <int EF, bool VEC>
__device__ __forceinline__ void w16_dec_rows(const SegDev& s, const W16Tile& t, const bf16_t* __restrict__ packed,
                                             const int32_t* __restrict__ slotmap, const W16Scale sc,
                                             float* __restrict__ gerr, float* __restrict__ out) {
    const int m = (int)s.m;
    const int lanes = t.lanes, groups = kW16Block / lanes;
    const int g = (int)threadIdx.x / lanes, l = (int)threadIdx.x % lanes;
    // (the next row's slot is loaded a row ahead: the lookup is off the row's critical path)
    int32_t next = g < t.nrows ? slotmap[s.row_off + t.row0 + (int64_t)g * t.rstride] : -1;
    for (int q = g; q < t.nrows; q += groups) {
        const int64_t row = t.row0 + (int64_t)q * t.rstride;
        const int64_t base = s.offset + row * (int64_t)m;
        const int32_t slot = next;
        if (q + groups < t.nrows) next = slotmap[s.row_off + row + (int64_t)groups * t.rstride];
        const bool sel = (uint32_t)slot < (uint32_t)s.k_rows;  // (-1: not selected)
        const bf16_t* pk = packed + s.packed_off + (sel ? (int64_t)slot * m : 0);
        if constexpr (VEC) {
            for (int u0 = l; u0 < m / 4; u0 += lanes * kW16Units) {
                wf4_t x[kW16Units];
                u2_t pw[kW16Units];
#pragma unroll
                for (int k = 0; k < kW16Units; ++k) {
                    const int u = u0 + k * lanes;
                    x[k] = wf4_t{0.0f, 0.0f, 0.0f, 0.0f};
                    pw[k] = u2_t{0u, 0u};
                    if (u < m / 4) {
                        if constexpr (EF == W16_EF21) x[k] = ld_f4_nt(gerr + base + 4 * (int64_t)u);
                        if (sel) pw[k] = __builtin_nontemporal_load(reinterpret_cast<const u2_t*>(pk + 4 * u));
                    }
                }
#pragma unroll
                for (int k = 0; k < kW16Units; ++k) {
                    const int u = u0 + k * lanes;
                    if (u >= m / 4) break;
                    wf4_t o = x[k];
                    if (sel) {
                        const wf4_t mean = w16_mean4(pw[k], sc);
                        if constexpr (EF == W16_EF21) {
                            o = wf4_t{o.x + mean.x, o.y + mean.y, o.z + mean.z, o.w + mean.w};
                            st_f4_nt(gerr + base + 4 * (int64_t)u, o);
                        } else {
                            o = mean;
                        }
                    }
                    st_f4_nt(out + base + 4 * (int64_t)u, o);
                }
            }
        } else {
            for (int c = l; c < m; c += lanes) w16_dec_elem<EF>(pk + c, sel, sc, gerr, out, base + c);
        }
    }
}

// One decode tile of whole short rows that are not 16-B units themselves (m % 4 != 0, or an odd
// offset): the tile's contiguous element range in 16-B units of out, whatever rows a unit spans
// (its first elements up to the alignment, and its last, one by one).  EF21 stores a unit of gE
// when it holds a selected element; its other elements get back the bits they had.
template <int EF>
__device__ __forceinline__ void w16_dec_flat(const SegDev& s, const W16Tile& t, const bf16_t* __restrict__ packed,
                                             const int32_t* __restrict__ slotmap, const W16Scale sc,
                                             float* __restrict__ gerr, float* __restrict__ out) {
    const int m = (int)s.m;
    const int64_t a = s.offset + t.row0 * (int64_t)m, b = a + (int64_t)t.nrows * m;
    const int64_t qa = std::min<int64_t>(b, (a + 3) & ~int64_t(3)), qb = std::max<int64_t>(qa, b & ~int64_t(3));
    const auto one = [&](int64_t el) {
        const uint32_t rel = (uint32_t)(el - a), r = div32(rel, s.magic32);
        const int32_t slot = slotmap[s.row_off + t.row0 + r];
        const bool sel = (uint32_t)slot < (uint32_t)s.k_rows;
        w16_dec_elem<EF>(packed + s.packed_off + (sel ? (int64_t)slot * m : 0) + (rel - r * m), sel, sc, gerr, out, el);
    };
    const int nedge = (int)((qa - a) + (b - qb));
    for (int i = threadIdx.x; i < nedge; i += kW16Block) one(i < qa - a ? a + i : qb + (i - (qa - a)));
    const int nq = (int)((qb - qa) / 4);
    for (int i = threadIdx.x; i < nq; i += kW16Block) {
        const int64_t el = qa + 4 * (int64_t)i;
        const uint32_t rel = (uint32_t)(el - a);
        uint32_t r = div32(rel, s.magic32);
        int c = (int)(rel - r * m);
        wf4_t x = wf4_t{0.0f, 0.0f, 0.0f, 0.0f};
        if constexpr (EF == W16_EF21) x = ld_f4_nt(gerr + el);
        int32_t slot = slotmap[s.row_off + t.row0 + r];
        bool any = false;
        float v[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (c == m) {  // (the next row: within the tile, since el + j < qb <= b)
                c = 0;
                slot = slotmap[s.row_off + t.row0 + ++r];
            }
            if ((uint32_t)slot < (uint32_t)s.k_rows) {
                const float mean = sc(to_f(packed[s.packed_off + (int64_t)slot * m + c]));
                v[j] = EF == W16_EF21 ? v[j] + mean : mean;
                any = true;
            }
            ++c;
        }
        const wf4_t o = wf4_t{v[0], v[1], v[2], v[3]};
        if constexpr (EF == W16_EF21) {
            if (any) st_f4_nt(gerr + el, o);
        }
        st_f4_nt(out + el, o);
    }
}

template <int EF>
__global__ void __launch_bounds__(kW16Block) k_w16_decode(const SegDev* __restrict__ segs,
                                                         const W16Tile* __restrict__ tiles,
                                                         const bf16_t* __restrict__ packed,
                                                         const int32_t* __restrict__ slotmap, const W16Scale sc,
                                                         float* __restrict__ gerr, float* __restrict__ out) {
    const W16Tile t = tiles[blockIdx.x];
    const SegDev& s = segs[t.seg];
    if (t.flags & W16_DENSE) {  // elements row0 .. row0 + nrows of a DENSE segment, all selected
        const int64_t e0 = s.offset + t.row0;
        const bf16_t* p = packed + s.packed_off + t.row0;
        int done = 0;
        if (t.flags & W16_VEC) {  // (bucket and packed offsets multiples of 4, as the tile's first element)
            const int nu = t.nrows / 4;
            for (int u = threadIdx.x; u < nu; u += kW16Block) {
                const u2_t w = __builtin_nontemporal_load(reinterpret_cast<const u2_t*>(p + 4 * u));
                wf4_t o = w16_mean4(w, sc);
                if constexpr (EF == W16_EF21) {
                    const wf4_t a = ld_f4_nt(gerr + e0 + 4 * u);
                    o = wf4_t{a.x + o.x, a.y + o.y, a.z + o.z, a.w + o.w};
                    st_f4_nt(gerr + e0 + 4 * u, o);
                }
                st_f4_nt(out + e0 + 4 * u, o);
            }
            done = nu * 4;
        }
        for (int i = done + (int)threadIdx.x; i < t.nrows; i += kW16Block)
            w16_dec_elem<EF>(p + i, true, sc, gerr, out, e0 + i);
        return;
    }
    if (t.flags & W16_SHORT) {  // rows of fewer than four columns (RAW: one): a thread per row
        const int m = (int)s.m;
        for (int i = threadIdx.x; i < t.nrows; i += kW16Block) {
            const int64_t row = t.row0 + i;
            const int32_t slot = slotmap[s.row_off + row];
            const bool sel = (uint32_t)slot < (uint32_t)s.k_rows;
            const bf16_t* pk = packed + s.packed_off + (sel ? (int64_t)slot * m : 0);
            for (int c = 0; c < m; ++c) w16_dec_elem<EF>(pk + c, sel, sc, gerr, out, s.offset + row * m + c);
        }
        return;
    }
    if (t.flags & W16_FLAT) {
        w16_dec_flat<EF>(s, t, packed, slotmap, sc, gerr, out);
        return;
    }
    if (t.flags & W16_VEC) w16_dec_rows<EF, true>(s, t, packed, slotmap, sc, gerr, out);
    else w16_dec_rows<EF, false>(s, t, packed, slotmap, sc, gerr, out);
}

// ---- zero-ahead scatter --------------------------------------------------------------------
// out = mean on the selected elements only, into a bucket a memset zeroed while the packed values
// were on the wire (exchange.cpp, x_fin 3): the pack's chunk table, read the other way round.
__device__ __forceinline__ void w16_sc_elem(const bf16_t* __restrict__ p, const W16Scale sc, float* __restrict__ out,
                                            int64_t el) {
    const uint16_t w = __builtin_nontemporal_load(&p->u);
    __builtin_nontemporal_store(sc(bf_bits_f(w)), out + el);
}

// The nu units of a chunk whose packed values are contiguous from p (8-B aligned): unit u's 4
// elements go to bucket element dst(u), or dst(u) < 0: the unit is skipped.  A thread takes a pair of
// units whose packed 16 B are aligned (one 16-B load), a lone unit at either end of the chunk (one
// 8-B load); the step's loads are issued before its two 16-B stores.
template <class Dst>
__device__ __forceinline__ void w16_sc_pairs(const bf16_t* __restrict__ p, int nu, const W16Scale sc,
                                             float* __restrict__ out, Dst dst) {
    const int head = ((uintptr_t)p & 15) ? 1 : 0;
    const int nitems = (nu + head + 1) / 2;
    for (int it = threadIdx.x; it < nitems; it += kW16Block) {
        const int ua = 2 * it - head, ub = ua + 1;
        const int64_t ea = ua >= 0 ? dst(ua) : -1, eb = ub < nu ? dst(ub) : -1;
        u2_t wa = u2_t{0u, 0u}, wb = u2_t{0u, 0u};
        if (ea >= 0 && eb >= 0) {
            const u4_t w = __builtin_nontemporal_load(reinterpret_cast<const u4_t*>(p + 4 * (int64_t)ua));
            wa = u2_t{w.x, w.y};
            wb = u2_t{w.z, w.w};
        } else if (ea >= 0) {
            wa = __builtin_nontemporal_load(reinterpret_cast<const u2_t*>(p + 4 * (int64_t)ua));
        } else if (eb >= 0) {
            wb = __builtin_nontemporal_load(reinterpret_cast<const u2_t*>(p + 4 * (int64_t)ub));
        }
        if (ea >= 0) st_f4_nt(out + ea, w16_mean4(wa, sc));
        if (eb >= 0) st_f4_nt(out + eb, w16_mean4(wb, sc));
    }
}

__global__ void __launch_bounds__(kW16Block) k_w16_scatter(const SegDev* __restrict__ segs,
                                                          const W16Chunk* __restrict__ chunks,
                                                          const bf16_t* __restrict__ packed,
                                                          const int32_t* __restrict__ rowlist, const W16Scale sc,
                                                          float* __restrict__ out) {
    const W16Chunk ch = chunks[blockIdx.x];
    const SegDev& s = segs[ch.seg];
    const int m = (int)s.m;
    if (ch.mode == W16P_DENSE) {  // every element is selected
        const int64_t e0 = s.offset + ch.j0;
        const bf16_t* p = packed + s.packed_off + ch.j0;
        int done = 0;
        if (s.offset % 4 == 0 && s.packed_off % 4 == 0) {  // (chunks start at multiples of 8 elements)
            const int nu = ch.nj / 4;
            w16_sc_pairs(p, nu, sc, out, [&](int u) { return e0 + 4 * (int64_t)u; });
            done = nu * 4;
        }
        for (int i = done + (int)threadIdx.x; i < ch.nj; i += kW16Block) w16_sc_elem(p + i, sc, out, e0 + i);
        return;
    }
    const int32_t* rl = rowlist + s.sel_off + ch.j0;
    const bf16_t* p = packed + s.packed_off + ch.j0 * (int64_t)m;
    if (ch.mode == W16P_ROWS_VEC) {
        if (m % 8 == 0 && ((uintptr_t)p & 15) == 0) {  // 8 elements of one row per thread: one 16-B packed load
            const int U8 = m / 8, n8 = ch.nj * U8;
            for (int u = threadIdx.x; u < n8; u += kW16Block) {
                const int jj = u / U8, c8 = u - jj * U8;
                const int64_t row = rl[jj];
                if ((uint64_t)row >= (uint64_t)s.n) continue;  // (never, for a select's row list)
                const int64_t el = s.offset + row * (int64_t)m + 8 * c8;
                const u4_t w = __builtin_nontemporal_load(reinterpret_cast<const u4_t*>(p + 8 * (int64_t)u));
                st_f4_nt(out + el, w16_mean4(u2_t{w.x, w.y}, sc));
                st_f4_nt(out + el + 4, w16_mean4(u2_t{w.z, w.w}, sc));
            }
            return;
        }
        const int U = m / 4;
        w16_sc_pairs(p, ch.nj * U, sc, out, [&](int u) -> int64_t {
            const int jj = u / U, c4 = u - jj * U;
            const int64_t row = rl[jj];
            if ((uint64_t)row >= (uint64_t)s.n) return -1;  // (never, for a select's row list)
            return s.offset + row * (int64_t)m + 4 * c4;
        });
        return;
    }
    const int ne = ch.nj * m;
    for (int i = threadIdx.x; i < ne; i += kW16Block) {
        const int jj = i / m, c = i - jj * m;
        const int64_t row = rl[jj];
        if ((uint64_t)row >= (uint64_t)s.n) continue;
        w16_sc_elem(p + i, sc, out, s.offset + row * (int64_t)m + c);
    }
}

// ---- the plan's tables ---------------------------------------------------------------------
void w16_free(W16Tab* t) {
    if (t->d_chunks) (void)hipFree(t->d_chunks);
    if (t->d_tiles) (void)hipFree(t->d_tiles);
    delete t;
}

int w16_table(const arctopk_plan* p, W16Tab** out) {
    if (p->w16) {
        *out = static_cast<W16Tab*>(p->w16);
        return 0;
    }
    std::vector<W16Chunk> chunks;
    std::vector<W16Tile> tiles;
    for (int i = 0; i < p->nseg; ++i) {
        const arctopk_segment& s = p->h_segs[i];
        const bool quad = s.offset % 4 == 0 && s.packed_off % 4 == 0;
        if (s.kind == ARCTOPK_SEG_DENSE) {
            push_pack_chunks(chunks, i, W16P_DENSE, s.n, 1, kW16PackElems);
            push_range_tiles(tiles, i, W16_DENSE | (quad ? W16_VEC : 0), s.n, kW16PackElems);
            continue;
        }
        const bool vec = quad && s.m % 4 == 0;  // (SegDev::vec)
        if (s.m < 4) {  // RAW tensors and rows of up to three columns: a decode thread per row
            push_range_tiles(tiles, i, W16_SHORT, s.n, kW16ShortElems);
        } else if (!vec && s.m < kW16FlatMaxM) {  // short rows off the 16-B grid: contiguous row ranges
            push_range_tiles(tiles, i, W16_FLAT, s.n, std::max<int64_t>(1, kW16DecElems / s.m));
        } else {
            push_row_tiles(tiles, i, vec ? W16_VEC : 0, s.n, s.m, vec, 4, kW16Block, kW16DecElems);
        }
        push_pack_chunks(chunks, i, vec ? W16P_ROWS_VEC : W16P_ROWS, s.k_rows, s.m, kW16PackElems);
    }
    W16Tab* t = new (std::nothrow) W16Tab;
    if (!t) return ARCTOPK_EINVAL;
    t->d_chunks = nullptr;
    t->d_tiles = nullptr;
    t->n_chunks = (int)chunks.size();
    t->n_tiles = (int)tiles.size();
    hipError_t e = hipSetDevice(p->device);
    if (e == hipSuccess) e = upload(chunks, &t->d_chunks);
    if (e == hipSuccess) e = upload(tiles, &t->d_tiles);
    if (e != hipSuccess) {
        w16_free(t);
        return (int)e;
    }
    const_cast<arctopk_plan*>(p)->w16 = t;
    *out = t;
    return 0;
}

// a launch that completes `done` itself when given one (hipExtLaunchKernelGGL's stop event: no
// marker packet on the stream)
template <typename... KArgs, typename... Args>
void w16_launch(void (*k)(KArgs...), int n, void* stream, void* done, Args... args) {
    if (done)
        hipExtLaunchKernelGGL(k, dim3((unsigned)n), dim3(kW16Block), 0, (hipStream_t)stream, nullptr,
                              (hipEvent_t)done, 0, args...);
    else
        hipLaunchKernelGGL(k, dim3((unsigned)n), dim3(kW16Block), 0, (hipStream_t)stream, args...);
}

template <int EF>
void launch_pack(const arctopk_plan* p, const W16Tab* t, const void* grad, void* err, int32_t err_in,
                 const int32_t* rowlist, void* packed, void* stream, void* done) {
    w16_launch(&k_w16_pack<EF>, t->n_chunks, stream, done, (const SegDev*)p->d_segs, (const W16Chunk*)t->d_chunks,
               static_cast<const float*>(grad), static_cast<float*>(err), (int)err_in, rowlist,
               static_cast<bf16_t*>(packed));
}

// what an empty work table leaves to do: `done` recorded, if given
int w16_nothing(int st, void* stream, void* done) {
    if (st != 0 || !done) return st;
    return (int)hipEventRecord((hipEvent_t)done, (hipStream_t)stream);
}

}  // namespace

namespace arctopk {
void wire16_forget(arctopk_plan* p) {
    if (!p->w16) return;
    w16_free(static_cast<W16Tab*>(p->w16));
    p->w16 = nullptr;
}
}  // namespace arctopk

namespace arctopk {
int pack_wire16_signal(const arctopk_plan* p, const void* grad, void* err, int32_t ef, int32_t err_in,
                       const int32_t* rowlist, const int32_t* slotmap, void* packed, void* stream, void* done) {
    if (!p || p->dtype != ARCTOPK_F32 || !ef_known(ef) || (err_in != 0 && err_in != 1)) return ARCTOPK_EINVAL;
    if (!rowlist || !slotmap || !packed) return ARCTOPK_EINVAL;
    if (ef != ARCTOPK_EF_NONE && !err) return ARCTOPK_EINVAL;
    // EF14 reads G for a DENSE segment only, whose X = G + E is formed here; noef and EF21 for every selected row
    if (!grad && (ef != ARCTOPK_EF14 || p->n_dense > 0)) return ARCTOPK_EINVAL;
    if (low_bits(grad, 15) | low_bits(err, 15) | low_bits(packed, 7)) return ARCTOPK_EINVAL;
    W16Tab* t = nullptr;
    const int st = w16_table(p, &t);
    if (st != 0 || t->n_chunks == 0) return w16_nothing(st, stream, done);
    if (ef == ARCTOPK_EF14) launch_pack<W16_EF14>(p, t, grad, err, err_in, rowlist, packed, stream, done);
    else if (ef == ARCTOPK_EF21) launch_pack<W16_EF21>(p, t, grad, err, err_in, rowlist, packed, stream, done);
    else launch_pack<W16_NONE>(p, t, grad, err, err_in, rowlist, packed, stream, done);
    return (int)hipGetLastError();
}

int decode_wire16_signal(const arctopk_plan* p, const void* packed, const int32_t* rowlist, const int32_t* slotmap,
                         int32_t world_size, int32_t ef, void* gerr, void* out, bool scatter, void* stream,
                         void* done) {
    if (!p || p->dtype != ARCTOPK_F32 || !ef_known(ef) || world_size < 1) return ARCTOPK_EINVAL;
    if (!packed || !slotmap || !out || (ef == ARCTOPK_EF21 && !gerr)) return ARCTOPK_EINVAL;
    if (scatter && (!rowlist || ef == ARCTOPK_EF21)) return ARCTOPK_EINVAL;  // (EF21 writes gE everywhere)
    if (low_bits(gerr, 15) | low_bits(out, 15) | low_bits(packed, 7)) return ARCTOPK_EINVAL;
    W16Tab* t = nullptr;
    const int st = w16_table(p, &t);
    if (st != 0 || (scatter ? t->n_chunks : t->n_tiles) == 0) return w16_nothing(st, stream, done);
    const W16Scale sc = make_mean_scale(world_size);
    const SegDev* segs = p->d_segs;
    const W16Tile* tiles = t->d_tiles;
    const bf16_t* pk = static_cast<const bf16_t*>(packed);
    float *ge = static_cast<float*>(gerr), *o = static_cast<float*>(out);
    if (scatter)
        w16_launch(&k_w16_scatter, t->n_chunks, stream, done, segs, (const W16Chunk*)t->d_chunks, pk, rowlist, sc, o);
    else if (ef == ARCTOPK_EF21)
        w16_launch(&k_w16_decode<W16_EF21>, t->n_tiles, stream, done, segs, tiles, pk, slotmap, sc, ge, o);
    else
        w16_launch(&k_w16_decode<W16_NONE>, t->n_tiles, stream, done, segs, tiles, pk, slotmap, sc, ge, o);
    return (int)hipGetLastError();
}
}  // namespace arctopk

extern "C" int arctopk_pack_wire16(const arctopk_plan* p, const void* grad, void* err, int32_t ef, int32_t err_in,
                                   const int32_t* rowlist, const int32_t* slotmap, void* packed, void* stream) {
    return pack_wire16_signal(p, grad, err, ef, err_in, rowlist, slotmap, packed, stream, nullptr);
}

extern "C" int arctopk_decode_wire16(const arctopk_plan* p, const void* packed, const int32_t* slotmap,
                                     int32_t world_size, int32_t ef, void* gerr, void* out, void* stream) {
    return decode_wire16_signal(p, packed, nullptr, slotmap, world_size, ef, gerr, out, false, stream, nullptr);
}

extern "C" int arctopk_decode_wire16_scatter(const arctopk_plan* p, const void* packed, const int32_t* rowlist,
                                             const int32_t* slotmap, int32_t world_size, void* out, void* stream) {
    return decode_wire16_signal(p, packed, rowlist, slotmap, world_size, ARCTOPK_EF_NONE, nullptr, out, true, stream,
                                nullptr);
}

extern "C" int arctopk_plan_bind_wire16(arctopk_plan* p, void* packed) {
    if (!p || p->dtype != ARCTOPK_F32 || low_bits(packed, 7)) return ARCTOPK_EINVAL;
    if (p->x_deferred || p->x_trail) return ARCTOPK_EINVAL;  // the caller finishes the plan's step first
    p->b_packed16 = packed;
    return 0;
}

// Diagnostics: exchange steps of `p` whose decode was the zero-ahead scatter so far
extern "C" int arctopk_diag_wire16_scatters(const arctopk_plan* p, int64_t* count) {
    if (!p || !count) return ARCTOPK_EINVAL;
    *count = p->w16_scatters;
    return 0;
}
