// Error feedback with fp32 residuals under a bf16 bucket, for MI355X (gfx950): the phases of a plan
// whose bucket, sketch, projections and packed values are bf16 while the residuals are kept in
// fp32 (DESIGN.md sections 4d and 4e).  One encode kernel and one pack kernel serve two residual
// rules, fixed at compile time by a residual mode (MX_EF14_NEW / MX_EF14_ADD / MX_EF21).  With
// f = bf16 -> fp32 (exact) and b = fp32 -> bf16 (round to nearest even, NaN -> 0x7FC0: cvt_pk_bf16
// of common.h):
//
//   encode : X = f(G) (EF14, err_in = 0), f(G) + E (EF14, err_in = 1) or f(G) - E (EF21): one fp32
//            operation.  EF14 stores E := X; EF21 only reads E.
//            sketch[SKETCH seg][row][j] = b( sum_c X[row][c] * f(V[c][j]) ), fp32 sum, one rounding
//            sketch[RAW seg][e] = b(X[e]);  DENSE segments: nothing
//   pack   : selected row (every element of a DENSE segment), packed = b(X), where
//            EF14: X is the E the encode stored (DENSE: formed here as above);  E := X - f(packed),
//                  one fp32 subtract; other rows keep E = X.  G is read for DENSE segments only.
//            EF21: X = f(G) - E again;  E := E + f(packed)
//   decode : EF14 uses the plan's own (arctopk_decode).  EF21 (k_mx_decode21), selected element:
//            gE := gE + f(P) / ws (the mean is not rounded to bf16); out = b(gE) on every element of
//            the bucket; gE of the other rows is left as stored.
//
// Select is the plan's own (arctopk_select): every phase here reads or writes the plan's sketch and
// packed layouts.  Nothing is shared with the bf16-residual kernels of arctopk_kernels.hip but the
// plan's segment table; the table layouts, their host loops and the small bf16 / fp32 16-B helpers
// are mixed_common.h's, shared with wire16.hip.
//
// Work mapping.  A plan gets one table of encode tiles, one of pack chunks and one of EF21 decode
// tiles, built at its first call here (mixed_table; freed with the plan), so a phase is one launch
// and no copy.
//   encode rows: `lanes` (a power of two, 1 .. 64) lanes of a wave share a row, the block's
//     256 / lanes groups take the tile's rows in turn; a lane strides over the row in 16-B units of
//     G (8 elements: 16 B of G, 2 x 16 B of E in and out, nontemporal) where the tensor's offset and
//     m are multiples of 8 (four units' loads in flight per step), else element by element; partial
//     sums meet in a butterfly of `lanes`.  The tiles of a tensor interleave their rows.
//     So m >= 512 runs a wave per row, m = 64 eight rows per wave, m = 18 two rows per wave, m <= 2
//     a lane per element.  The block's V is staged transposed in LDS as bf16 ([r][m]: a lane's 8
//     columns of one j are one 16-B read) when m * r * 4 <= 64 KiB, the bound of the existing
//     encode's column split; past it V is read from global memory (L2) and the sketch is still
//     written directly: no partial sums, no second launch.
//   encode RAW: an element per thread.
//   pack: chunks of about 8192 elements of selected rows (16-B units under the same alignment
//     rule, else elements), DENSE segments in chunks of 8192 elements (units when the segment's
//     bucket and packed offsets are multiples of 8).
//   EF21 decode: the encode's row tiles again for rows of more than two columns, element tiles
//     with a thread per row for RAW tensors and rows of one or two columns, and element tiles for
//     DENSE segments.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <vector>

#include "common.h"
#include "mixed_common.h"

namespace {

using namespace arctopk;

constexpr int kMxBlock = 256;
constexpr int64_t kMxPackElems = 8192;   // elements per pack chunk
constexpr int64_t kMxRawElems = 4096;    // elements per RAW encode tile
constexpr int kMxUnits = 4;             // 16-B units of G (and 32 B of E) a lane loads per step
                                        // (a pack thread takes one unit per step: the EF14 headline pack
                                        // measured 35.4 us with 1, 37.9 with 2, 38.7 with 4: its blocks are short)
constexpr int64_t kMxTargetBlocks = 2048;  // row tiles a bucket aims at (common.h: kEncTargetBlocks)

enum : int32_t { MX_RAW = 1, MX_VEC = 2, MX_VLDS = 4,          // encode tile flags
                 MX_SHORT = 8, MX_DENSE = 16 };                // ... and those of the EF21 decode's tiles
enum : int32_t { MXP_ROWS = 0, MXP_ROWS_VEC = 1, MXP_DENSE = 2 };  // pack chunk modes

// The residual mode of an encode or pack kernel: how X is formed from f(G) and E, and what becomes
// of E.                  X            encode        pack (packed = b(X), y = f(packed))
enum MxMode : int {
    MX_EF14_NEW = 0,  //  f(G)         E := X        E := X - y   (err_in = 0: E is not read before)
    MX_EF14_ADD = 1,  //  f(G) + E     E := X        E := X - y
    MX_EF21 = 2,      //  f(G) - E     E only read   E := E + y
};
// What the encode's E points at.  (A named trait: the type is part of the kernels' mangled names,
// which the host and device passes must spell alike; an unnamed enum inside them is numbered per pass.)
template <int MODE> struct MxErr { using type = float; };
template <> struct MxErr<MX_EF21> { using type = const float; };
template <int MODE>
using mx_err_t = typename MxErr<MODE>::type;
// X of one element; e is not evaluated into the result under MX_EF14_NEW
template <int MODE>
__device__ __forceinline__ float mx_x(float g, float e) {
    if constexpr (MODE == MX_EF14_ADD) return g + e;
    else if constexpr (MODE == MX_EF21) return g - e;
    else return g;
}

using MxTile = RowTile;      // (mixed_common.h)
using MxChunk = PackChunk;
using MxScale = MeanScale;

struct MxTab {       // the plan's mixed work tables (device) and their sizes
    MxTile* d_tiles;
    MxChunk* d_chunks;
    MxTile* d_dtiles;  // EF21's decode tiles (k_mx_decode21)
    int n_tiles, n_chunks, n_dtiles;
    int lds_bytes;   // dynamic LDS of the encode launch
    int n_vlds, n_vglobal;  // row tiles of d_tiles with / without MX_VLDS (diagnostics)
};

// the 8 bf16 of a 16-B unit as floats
__device__ __forceinline__ void unpack8(u4_t w, float (&x)[8]) {
    x[0] = __uint_as_float(w.x << 16), x[1] = __uint_as_float(w.x & 0xFFFF0000u);
    x[2] = __uint_as_float(w.y << 16), x[3] = __uint_as_float(w.y & 0xFFFF0000u);
    x[4] = __uint_as_float(w.z << 16), x[5] = __uint_as_float(w.z & 0xFFFF0000u);
    x[6] = __uint_as_float(w.w << 16), x[7] = __uint_as_float(w.w & 0xFFFF0000u);
}
__device__ __forceinline__ u4_t pack8(const float (&x)[8]) {
    return u4_t{cvt_pk_bf16(x[0], x[1]), cvt_pk_bf16(x[2], x[3]), cvt_pk_bf16(x[4], x[5]), cvt_pk_bf16(x[6], x[7])};
}

// the 8 bf16 at p (8-B aligned; 16-B aligned when a16)
__device__ __forceinline__ u4_t ld8bf(const bf16_t* p, bool a16) {
    if (a16) return *reinterpret_cast<const u4_t*>(p);
    const u2_t a = reinterpret_cast<const u2_t*>(p)[0], b = reinterpret_cast<const u2_t*>(p)[1];
    return u4_t{a.x, a.y, b.x, b.y};
}
__device__ __forceinline__ void st8bf(bf16_t* p, bool a16, u4_t w) {
    if (a16) {
        __builtin_nontemporal_store(w, reinterpret_cast<u4_t*>(p));
    } else {
        reinterpret_cast<u2_t*>(p)[0] = u2_t{w.x, w.y};
        reinterpret_cast<u2_t*>(p)[1] = u2_t{w.z, w.w};
    }
}

// ---- encode --------------------------------------------------------------------------------
// One tile of rows.  RR: the rank when it is 4, else 0 (rank r at run time, up to kMaxR).  MODE: the
// residual mode; it fixes whether E is loaded, how it enters X and whether X is stored back.
template <int RR, int MODE, bool VEC, bool VLDS>
__device__ __forceinline__ void enc_rows(const SegDev& s, const MxTile& t, int r, const bf16_t* __restrict__ grad,
                                         mx_err_t<MODE>* __restrict__ err, const bf16_t* __restrict__ V,
                                         bf16_t* __restrict__ sketch, const uint16_t* __restrict__ vt) {
    constexpr int NR = RR ? RR : kMaxR;
    constexpr bool LOAD_E = MODE != MX_EF14_NEW, STORE_E = MODE != MX_EF21;
    const int m = (int)s.m;
    const int mp = (m + 7) & ~7;  // LDS row of V^T, in elements
    const int lanes = t.lanes, groups = kMxBlock / lanes;
    const int g = (int)threadIdx.x / lanes, l = (int)threadIdx.x % lanes;
    const bf16_t* Vs = V + (VLDS ? 0 : s.v_off);
    for (int rb = 0; rb < t.nrows; rb += groups) {  // (uniform trip count: every lane joins the butterfly)
        const int q = rb + g;
        const bool on = q < t.nrows;
        const int64_t row = t.row0 + (int64_t)q * t.rstride;
        float acc[NR];
#pragma unroll
        for (int j = 0; j < NR; ++j) acc[j] = 0.0f;
        if (on) {
            const int64_t base = s.offset + row * (int64_t)m;
            if constexpr (VEC) {
                // kMxUnits units per lane per step, every load of the step issued before its first use
                for (int u0 = l; u0 < m / 8; u0 += lanes * kMxUnits) {
                    u4_t graw[kMxUnits];
                    vf4_t ea[kMxUnits], eb[kMxUnits];
#pragma unroll
                    for (int k = 0; k < kMxUnits; ++k) {
                        const int u = u0 + k * lanes;
                        if (u < m / 8) {
                            graw[k] = ld16raw<bf16_t, kEncNtLoad>(grad + base + 8 * (int64_t)u, 0);
                            if constexpr (LOAD_E) {
                                ea[k] = ld_f4_nt(err + base + 8 * (int64_t)u);
                                eb[k] = ld_f4_nt(err + base + 8 * (int64_t)u + 4);
                            }
                        }
                    }
#pragma unroll
                    for (int k = 0; k < kMxUnits; ++k) {
                        const int u = u0 + k * lanes;
                        if (u >= m / 8) break;
                        float x[8];
                        unpack8(graw[k], x);
                        if constexpr (LOAD_E) {
                            x[0] = mx_x<MODE>(x[0], ea[k].x), x[1] = mx_x<MODE>(x[1], ea[k].y);
                            x[2] = mx_x<MODE>(x[2], ea[k].z), x[3] = mx_x<MODE>(x[3], ea[k].w);
                            x[4] = mx_x<MODE>(x[4], eb[k].x), x[5] = mx_x<MODE>(x[5], eb[k].y);
                            x[6] = mx_x<MODE>(x[6], eb[k].z), x[7] = mx_x<MODE>(x[7], eb[k].w);
                        }
                        if constexpr (STORE_E) {
                            float* e8 = err + base + 8 * (int64_t)u;
                            st_f4_nt(e8, vf4_t{x[0], x[1], x[2], x[3]});
                            st_f4_nt(e8 + 4, vf4_t{x[4], x[5], x[6], x[7]});
                        }
#pragma unroll
                        for (int j = 0; j < NR; ++j) {
                            if (RR == 0 && j >= r) break;
                            float v[8];
                            if constexpr (VLDS) {
                                unpack8(*reinterpret_cast<const u4_t*>(vt + j * mp + 8 * u), v);
                            } else {
#pragma unroll
                                for (int i = 0; i < 8; ++i) v[i] = to_f(Vs[(int64_t)(8 * u + i) * r + j]);
                            }
#pragma unroll
                            for (int i = 0; i < 8; ++i) acc[j] += x[i] * v[i];
                        }
                    }
                }
            } else {
                for (int c = l; c < m; c += lanes) {
                    float x = ld1<bf16_t, kEncNtLoad>(grad + base + c);
                    if constexpr (LOAD_E) x = mx_x<MODE>(x, err[base + c]);
                    if constexpr (STORE_E) err[base + c] = x;
#pragma unroll
                    for (int j = 0; j < NR; ++j) {
                        if (RR == 0 && j >= r) break;
                        const float v = VLDS ? bf_bits_f(vt[j * mp + c]) : to_f(Vs[(int64_t)c * r + j]);
                        acc[j] += x * v;
                    }
                }
            }
        }
        for (int o = lanes >> 1; o > 0; o >>= 1) {
#pragma unroll
            for (int j = 0; j < NR; ++j) acc[j] += __shfl_xor(acc[j], o);
        }
        if (on && l == 0) {
            bf16_t* out = sketch + s.sketch_off + row * (int64_t)r;
#pragma unroll
            for (int j = 0; j < NR; ++j) {
                if (RR == 0 && j >= r) break;
                out[j].u = f_to_bf(acc[j]);
            }
        }
    }
}

template <int RR, int MODE>
__global__ void __launch_bounds__(kMxBlock) k_mx_encode(const SegDev* __restrict__ segs,
                                                       const MxTile* __restrict__ tiles, int r,
                                                       const bf16_t* __restrict__ grad,
                                                       mx_err_t<MODE>* __restrict__ err,
                                                       const bf16_t* __restrict__ V, bf16_t* __restrict__ sketch) {
    extern __shared__ __attribute__((aligned(16))) uint16_t mx_vt[];
    const MxTile t = tiles[blockIdx.x];
    const SegDev& s = segs[t.seg];
    if (t.flags & MX_RAW) {
        for (int i = threadIdx.x; i < t.nrows; i += kMxBlock) {
            const int64_t e = t.row0 + i;
            float x = ld1<bf16_t, kEncNtLoad>(grad + s.offset + e);
            if constexpr (MODE != MX_EF14_NEW) x = mx_x<MODE>(x, err[s.offset + e]);
            if constexpr (MODE != MX_EF21) err[s.offset + e] = x;
            sketch[s.sketch_off + e].u = f_to_bf(x);
        }
        return;
    }
    if (t.flags & MX_VLDS) {  // V^T of this tensor, bf16, rows of mp elements
        const int m = (int)s.m, mp = (m + 7) & ~7;
        const bf16_t* Vs = V + s.v_off;
        for (int i = threadIdx.x; i < m * r; i += kMxBlock) {
            const int c = i / r, j = i - c * r;
            mx_vt[j * mp + c] = Vs[i].u;
        }
        __syncthreads();
        if (t.flags & MX_VEC) enc_rows<RR, MODE, true, true>(s, t, r, grad, err, V, sketch, mx_vt);
        else enc_rows<RR, MODE, false, true>(s, t, r, grad, err, V, sketch, mx_vt);
    } else {
        if (t.flags & MX_VEC) enc_rows<RR, MODE, true, false>(s, t, r, grad, err, V, sketch, mx_vt);
        else enc_rows<RR, MODE, false, false>(s, t, r, grad, err, V, sketch, mx_vt);
    }
}

// ---- pack ----------------------------------------------------------------------------------
// One 16-B unit (8 elements) of a selected row, or of a DENSE segment: packed = b(X) to p8 (16-B
// aligned when p16, else 8-B) and E by the mode's rule.  X of an EF14 row is the E the encode
// stored, so g8 is not read there (it may be null: arctopk_pack_mixed allows grad = NULL for a plan
// without DENSE segments); everywhere else X is formed from f(G) and E as in the encode.
template <int MODE, bool DENSE>
__device__ __forceinline__ void pack_unit(const bf16_t* __restrict__ g8, float* __restrict__ e8,
                                          bf16_t* __restrict__ p8, bool p16) {
    constexpr bool X_IS_E = MODE != MX_EF21 && !DENSE;
    float x[8], e[8] = {}, y[8];
    if constexpr (!X_IS_E) unpack8(ld16raw<bf16_t, kEncNtLoad>(g8, 0), x);
    if constexpr (X_IS_E || MODE != MX_EF14_NEW) {
        const vf4_t a = ld_f4_nt(e8), b = ld_f4_nt(e8 + 4);
        e[0] = a.x, e[1] = a.y, e[2] = a.z, e[3] = a.w, e[4] = b.x, e[5] = b.y, e[6] = b.z, e[7] = b.w;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = X_IS_E ? e[i] : mx_x<MODE>(x[i], e[i]);
    const u4_t w = pack8(x);
    unpack8(w, y);
    st8bf(p8, p16, w);
    const auto en = [&](int i) { return MODE == MX_EF21 ? e[i] + y[i] : x[i] - y[i]; };  // the new E
    st_f4_nt(e8, vf4_t{en(0), en(1), en(2), en(3)});
    st_f4_nt(e8 + 4, vf4_t{en(4), en(5), en(6), en(7)});
}
// ... and one element
template <int MODE, bool DENSE>
__device__ __forceinline__ void pack_elem(const bf16_t* __restrict__ g, float* __restrict__ e,
                                          bf16_t* __restrict__ p) {
    constexpr bool X_IS_E = MODE != MX_EF21 && !DENSE;
    float ev = 0.0f, x;
    if constexpr (X_IS_E || MODE != MX_EF14_NEW) ev = *e;
    if constexpr (X_IS_E) x = ev;
    else x = mx_x<MODE>(to_f(*g), ev);
    const uint16_t w = f_to_bf(x);
    p->u = w;
    *e = MODE == MX_EF21 ? ev + bf_bits_f(w) : x - bf_bits_f(w);
}

template <int MODE>
__global__ void __launch_bounds__(kMxBlock) k_mx_pack(const SegDev* __restrict__ segs,
                                                     const MxChunk* __restrict__ chunks,
                                                     const bf16_t* __restrict__ grad, float* __restrict__ err,
                                                     const int32_t* __restrict__ rowlist,
                                                     bf16_t* __restrict__ packed) {
    const MxChunk ch = chunks[blockIdx.x];
    const SegDev& s = segs[ch.seg];
    const int m = (int)s.m;
    if (ch.mode == MXP_DENSE) {  // every element is selected (and has no encode work: X is formed here)
        const bf16_t* g = grad + s.offset + ch.j0;
        float* e = err + s.offset + ch.j0;
        bf16_t* p = packed + s.packed_off + ch.j0;
        int done = 0;
        if (s.offset % 8 == 0 && s.packed_off % 8 == 0) {  // (chunks start at multiples of 8 elements)
            const int nu = ch.nj / 8;
            for (int u = threadIdx.x; u < nu; u += kMxBlock) pack_unit<MODE, true>(g + 8 * u, e + 8 * u, p + 8 * u, true);
            done = nu * 8;
        }
        for (int i = done + (int)threadIdx.x; i < ch.nj; i += kMxBlock) pack_elem<MODE, true>(g + i, e + i, p + i);
        return;
    }
    // rows: EF14 forms no address from grad
    const int32_t* rl = rowlist + s.sel_off + ch.j0;
    bf16_t* p = packed + s.packed_off + ch.j0 * (int64_t)m;
    if (ch.mode == MXP_ROWS_VEC) {
        const int U = m / 8, nu = ch.nj * U;
        const bool p16 = s.packed_off % 8 == 0;  // (m % 8 == 0: every row of the segment alike)
        for (int u = threadIdx.x; u < nu; u += kMxBlock) {
            const int jj = u / U, c8 = u - jj * U;
            const int64_t row = rl[jj];
            if ((uint64_t)row >= (uint64_t)s.n) continue;  // (never, for a select's row list)
            const int64_t el = s.offset + row * (int64_t)m + 8 * c8;
            pack_unit<MODE, false>(MODE == MX_EF21 ? grad + el : nullptr, err + el, p + 8 * (int64_t)u, p16);
        }
        return;
    }
    const int ne = ch.nj * m;
    for (int i = threadIdx.x; i < ne; i += kMxBlock) {
        const int jj = i / m, c = i - jj * m;
        const int64_t row = rl[jj];
        if ((uint64_t)row >= (uint64_t)s.n) continue;
        const int64_t el = s.offset + row * (int64_t)m + c;
        pack_elem<MODE, false>(MODE == MX_EF21 ? grad + el : nullptr, err + el, p + i);
    }
}

// ---- EF21 decode ---------------------------------------------------------------------------
// One decode tile of rows: `lanes` lanes per row as in the encode, the row's slot read once.
template <bool VEC>
__device__ __forceinline__ void dec21_rows(const SegDev& s, const MxTile& t, const bf16_t* __restrict__ packed,
                                           const int32_t* __restrict__ slotmap, const MxScale sc,
                                           float* __restrict__ gerr, bf16_t* __restrict__ out) {
    const int m = (int)s.m;
    const int lanes = t.lanes, groups = kMxBlock / lanes;
    const int g = (int)threadIdx.x / lanes, l = (int)threadIdx.x % lanes;
    const bool p16 = s.packed_off % 8 == 0;
    for (int q = g; q < t.nrows; q += groups) {
        const int64_t row = t.row0 + (int64_t)q * t.rstride;
        const int64_t base = s.offset + row * (int64_t)m;
        const int32_t slot = slotmap[s.row_off + row];
        const bool sel = (uint32_t)slot < (uint32_t)s.k_rows;  // (-1: not selected)
        const bf16_t* pk = packed + s.packed_off + (sel ? (int64_t)slot * m : 0);
        if constexpr (VEC) {
            for (int u0 = l; u0 < m / 8; u0 += lanes * kMxUnits) {
                vf4_t ea[kMxUnits], eb[kMxUnits];
                u4_t pw[kMxUnits];
#pragma unroll
                for (int k = 0; k < kMxUnits; ++k) {
                    const int u = u0 + k * lanes;
                    if (u < m / 8) {
                        ea[k] = ld_f4_nt(gerr + base + 8 * (int64_t)u);
                        eb[k] = ld_f4_nt(gerr + base + 8 * (int64_t)u + 4);
                        if (sel) pw[k] = ld8bf(pk + 8 * u, p16);
                    }
                }
#pragma unroll
                for (int k = 0; k < kMxUnits; ++k) {
                    const int u = u0 + k * lanes;
                    if (u >= m / 8) break;
                    float x[8] = {ea[k].x, ea[k].y, ea[k].z, ea[k].w, eb[k].x, eb[k].y, eb[k].z, eb[k].w};
                    if (sel) {
                        float y[8];
                        unpack8(pw[k], y);
#pragma unroll
                        for (int i = 0; i < 8; ++i) x[i] += sc(y[i]);
                        float* e8 = gerr + base + 8 * (int64_t)u;
                        st_f4_nt(e8, vf4_t{x[0], x[1], x[2], x[3]});
                        st_f4_nt(e8 + 4, vf4_t{x[4], x[5], x[6], x[7]});
                    }
                    __builtin_nontemporal_store(pack8(x), reinterpret_cast<u4_t*>(out + base + 8 * (int64_t)u));
                }
            }
        } else {
            for (int c = l; c < m; c += lanes) {
                float x = gerr[base + c];
                if (sel) {
                    x += sc(to_f(pk[c]));
                    gerr[base + c] = x;
                }
                out[base + c].u = f_to_bf(x);
            }
        }
    }
}

__global__ void __launch_bounds__(kMxBlock) k_mx_decode21(const SegDev* __restrict__ segs,
                                                         const MxTile* __restrict__ tiles,
                                                         const bf16_t* __restrict__ packed,
                                                         const int32_t* __restrict__ slotmap, const MxScale sc,
                                                         float* __restrict__ gerr, bf16_t* __restrict__ out) {
    const MxTile t = tiles[blockIdx.x];
    const SegDev& s = segs[t.seg];
    if (t.flags & MX_DENSE) {  // elements row0 .. row0 + nrows of a DENSE segment, all selected
        float* e = gerr + s.offset + t.row0;
        bf16_t* o = out + s.offset + t.row0;
        const bf16_t* p = packed + s.packed_off + t.row0;
        int done = 0;
        if (t.flags & MX_VEC) {  // (bucket and packed offsets multiples of 8, as the tile's first element)
            const int nu = t.nrows / 8;
            for (int u = threadIdx.x; u < nu; u += kMxBlock) {
                float y[8];
                unpack8(*reinterpret_cast<const u4_t*>(p + 8 * u), y);
                const vf4_t a = ld_f4_nt(e + 8 * u), b = ld_f4_nt(e + 8 * u + 4);
                const float x[8] = {a.x + sc(y[0]), a.y + sc(y[1]), a.z + sc(y[2]), a.w + sc(y[3]),
                                    b.x + sc(y[4]), b.y + sc(y[5]), b.z + sc(y[6]), b.w + sc(y[7])};
                st_f4_nt(e + 8 * u, vf4_t{x[0], x[1], x[2], x[3]});
                st_f4_nt(e + 8 * u + 4, vf4_t{x[4], x[5], x[6], x[7]});
                __builtin_nontemporal_store(pack8(x), reinterpret_cast<u4_t*>(o + 8 * u));
            }
            done = nu * 8;
        }
        for (int i = done + (int)threadIdx.x; i < t.nrows; i += kMxBlock) {
            const float x = e[i] + sc(to_f(p[i]));
            e[i] = x;
            o[i].u = f_to_bf(x);
        }
        return;
    }
    if (t.flags & MX_SHORT) {  // rows of one or two columns (RAW: one): a thread per row
        const int m = (int)s.m;
        for (int i = threadIdx.x; i < t.nrows; i += kMxBlock) {
            const int64_t row = t.row0 + i;
            const int32_t slot = slotmap[s.row_off + row];
            const bool sel = (uint32_t)slot < (uint32_t)s.k_rows;
            for (int c = 0; c < m; ++c) {
                const int64_t el = s.offset + row * m + c;
                float x = gerr[el];
                if (sel) {
                    x += sc(to_f(packed[s.packed_off + (int64_t)slot * m + c]));
                    gerr[el] = x;
                }
                out[el].u = f_to_bf(x);
            }
        }
        return;
    }
    if (t.flags & MX_VEC) dec21_rows<true>(s, t, packed, slotmap, sc, gerr, out);
    else dec21_rows<false>(s, t, packed, slotmap, sc, gerr, out);
}

// ---- the plan's tables ---------------------------------------------------------------------
void mixed_free(MxTab* t) {
    if (t->d_tiles) (void)hipFree(t->d_tiles);
    if (t->d_chunks) (void)hipFree(t->d_chunks);
    if (t->d_dtiles) (void)hipFree(t->d_dtiles);
    delete t;
}

int mixed_table(const arctopk_plan* p, MxTab** out) {
    if (p->mx) {
        *out = static_cast<MxTab*>(p->mx);
        return 0;
    }
    const int r = p->r;
    std::vector<MxTile> tiles, dtiles;
    std::vector<MxChunk> chunks;
    int lds = 0;
    int64_t row_work = 0;
    for (int i = 0; i < p->nseg; ++i)
        if (p->h_segs[i].kind == ARCTOPK_SEG_SKETCH) row_work += p->h_segs[i].n * p->h_segs[i].m;
    // elements per row tile: the bucket's rows cut into about kMxTargetBlocks blocks, 8 Ki .. 64 Ki each
    const int64_t tile_elems = std::min<int64_t>(65536, std::max<int64_t>(8192, row_work / kMxTargetBlocks));
    for (int i = 0; i < p->nseg; ++i) {
        const arctopk_segment& s = p->h_segs[i];
        const bool vec = s.m % 8 == 0 && s.offset % 8 == 0;
        if (s.kind == ARCTOPK_SEG_DENSE) {
            push_pack_chunks(chunks, i, MXP_DENSE, s.n, 1, kMxPackElems);
            const int dflags = MX_DENSE | ((s.offset % 8 == 0 && s.packed_off % 8 == 0) ? MX_VEC : 0);
            push_range_tiles(dtiles, i, dflags, s.n, kMxPackElems);
            continue;
        }
        if (s.kind == ARCTOPK_SEG_RAW) {
            push_range_tiles(tiles, i, MX_RAW, s.n, kMxRawElems);
        } else {
            const bool vlds = s.m * r * 4 <= (int64_t)kVLdsMaxBytes;
            const int flags = (vec ? MX_VEC : 0) | (vlds ? MX_VLDS : 0);
            const int64_t ntiles = push_row_tiles(tiles, i, flags, s.n, s.m, vec, 8, kMxBlock, tile_elems);
            if (s.m > 2) dtiles.insert(dtiles.end(), tiles.end() - ntiles, tiles.end());  // the decode walks the same rows
            if (vlds) lds = std::max<int>(lds, (int)(((s.m + 7) & ~int64_t(7)) * r * 2));
        }
        if (s.m <= 2)  // RAW tensors and rows of one or two columns: a decode thread per row
            push_range_tiles(dtiles, i, MX_SHORT, s.n, kMxRawElems);
        push_pack_chunks(chunks, i, vec ? MXP_ROWS_VEC : MXP_ROWS, s.k_rows, s.m, kMxPackElems);
    }
    MxTab* t = new (std::nothrow) MxTab;
    if (!t) return ARCTOPK_EINVAL;
    t->d_tiles = nullptr;
    t->d_chunks = nullptr;
    t->d_dtiles = nullptr;
    t->n_dtiles = (int)dtiles.size();
    t->n_tiles = (int)tiles.size();
    t->n_chunks = (int)chunks.size();
    t->lds_bytes = lds;
    t->n_vlds = t->n_vglobal = 0;
    for (const MxTile& mt : tiles)
        if (!(mt.flags & MX_RAW)) ++((mt.flags & MX_VLDS) ? t->n_vlds : t->n_vglobal);
    hipError_t e = hipSetDevice(p->device);
    if (e == hipSuccess) e = upload(tiles, &t->d_tiles);
    if (e == hipSuccess) e = upload(chunks, &t->d_chunks);
    if (e == hipSuccess) e = upload(dtiles, &t->d_dtiles);
    if (e != hipSuccess) {
        mixed_free(t);
        return (int)e;
    }
    const_cast<arctopk_plan*>(p)->mx = t;
    *out = t;
    return 0;
}

// What every entry point does after its own null checks: a bf16 plan, no misaligned pointer
// (`misaligned`: the pointers' low bits under their masks, or-ed), the plan's tables.  *out stays
// null, with status 0, when the table the phase walks (`count`) is empty: nothing to launch.
int mixed_begin(const arctopk_plan* p, uintptr_t misaligned, int MxTab::*count, MxTab** out) {
    *out = nullptr;
    if (p->dtype != ARCTOPK_BF16 || misaligned) return ARCTOPK_EINVAL;
    MxTab* t = nullptr;
    const int st = mixed_table(p, &t);
    if (st == 0 && t->*count > 0) *out = t;
    return st;
}

template <int MODE>
int mixed_encode(const arctopk_plan* p, const void* grad, mx_err_t<MODE>* err, const void* V, void* sketch,
                 void* stream) {
    if (!p || !grad || !err) return ARCTOPK_EINVAL;
    if ((p->info.v_len > 0 && !V) || (p->info.sketch_len > 0 && !sketch)) return ARCTOPK_EINVAL;
    MxTab* t = nullptr;
    const int st = mixed_begin(p, low_bits(grad, 15) | low_bits(err, 15) | low_bits(V, 1) | low_bits(sketch, 1),
                               &MxTab::n_tiles, &t);
    if (!t) return st;  // (no tiles: DENSE segments only, whose X is formed by the pack)
    const bf16_t* g = static_cast<const bf16_t*>(grad);
    const bf16_t* v = static_cast<const bf16_t*>(V);
    bf16_t* sk = static_cast<bf16_t*>(sketch);
    const dim3 grid((unsigned)t->n_tiles), block(kMxBlock);
    hipStream_t hs = (hipStream_t)stream;
    const size_t lds = (size_t)t->lds_bytes;
    if (p->r == 4) hipLaunchKernelGGL((k_mx_encode<4, MODE>), grid, block, lds, hs, p->d_segs, t->d_tiles, p->r, g, err, v, sk);
    else hipLaunchKernelGGL((k_mx_encode<0, MODE>), grid, block, lds, hs, p->d_segs, t->d_tiles, p->r, g, err, v, sk);
    return (int)hipGetLastError();
}

template <int MODE>
int mixed_pack(const arctopk_plan* p, const void* grad, float* err, const int32_t* rowlist, const int32_t* slotmap,
               void* packed, void* stream) {
    if (!p || !err || !rowlist || !slotmap || !packed) return ARCTOPK_EINVAL;
    // EF14 reads G for a DENSE segment only, whose X = f(G) + E is formed here; EF21 for every selected row
    if (!grad && (MODE == MX_EF21 || p->n_dense > 0)) return ARCTOPK_EINVAL;
    MxTab* t = nullptr;
    const int st = mixed_begin(p, low_bits(grad, 15) | low_bits(err, 15) | low_bits(packed, 15), &MxTab::n_chunks, &t);
    if (!t) return st;
    hipLaunchKernelGGL((k_mx_pack<MODE>), dim3((unsigned)t->n_chunks), dim3(kMxBlock), 0, (hipStream_t)stream,
                       p->d_segs, t->d_chunks, static_cast<const bf16_t*>(grad), err, rowlist,
                       static_cast<bf16_t*>(packed));
    return (int)hipGetLastError();
}

}  // namespace

namespace arctopk {
void mixed_forget(arctopk_plan* p) {
    if (!p->mx) return;
    mixed_free(static_cast<MxTab*>(p->mx));
    p->mx = nullptr;
}
bool mixed_tile_counts(const arctopk_plan* p, int64_t* vlds, int64_t* vglobal) {
    if (!p->mx) return false;
    const MxTab* t = static_cast<const MxTab*>(p->mx);
    *vlds = t->n_vlds;
    *vglobal = t->n_vglobal;
    return true;
}
}  // namespace arctopk

extern "C" int arctopk_encode_mixed(const arctopk_plan* p, const void* grad, float* err, int32_t err_in,
                                    const void* V, void* sketch, void* stream) {
    if (err_in != 0 && err_in != 1) return ARCTOPK_EINVAL;
    return err_in ? mixed_encode<MX_EF14_ADD>(p, grad, err, V, sketch, stream)
                  : mixed_encode<MX_EF14_NEW>(p, grad, err, V, sketch, stream);
}

extern "C" int arctopk_pack_mixed(const arctopk_plan* p, const void* grad, float* err, int32_t err_in,
                                  const int32_t* rowlist, const int32_t* slotmap, void* packed, void* stream) {
    if (err_in != 0 && err_in != 1) return ARCTOPK_EINVAL;
    return err_in ? mixed_pack<MX_EF14_ADD>(p, grad, err, rowlist, slotmap, packed, stream)
                  : mixed_pack<MX_EF14_NEW>(p, grad, err, rowlist, slotmap, packed, stream);
}

extern "C" int arctopk_encode_mixed21(const arctopk_plan* p, const void* grad, const float* err, const void* V,
                                      void* sketch, void* stream) {
    return mixed_encode<MX_EF21>(p, grad, err, V, sketch, stream);
}

extern "C" int arctopk_pack_mixed21(const arctopk_plan* p, const void* grad, float* err, const int32_t* rowlist,
                                    const int32_t* slotmap, void* packed, void* stream) {
    return mixed_pack<MX_EF21>(p, grad, err, rowlist, slotmap, packed, stream);
}

extern "C" int arctopk_decode_mixed21(const arctopk_plan* p, const void* packed, const int32_t* slotmap,
                                      int32_t world_size, float* gerr, void* out, void* stream) {
    if (!p || !packed || !slotmap || !gerr || !out || world_size < 1) return ARCTOPK_EINVAL;
    MxTab* t = nullptr;
    const int st = mixed_begin(p, low_bits(packed, 15) | low_bits(gerr, 15) | low_bits(out, 15), &MxTab::n_dtiles, &t);
    if (!t) return st;
    hipLaunchKernelGGL(k_mx_decode21, dim3((unsigned)t->n_dtiles), dim3(kMxBlock), 0, (hipStream_t)stream, p->d_segs,
                       t->d_dtiles, static_cast<const bf16_t*>(packed), slotmap, make_mean_scale(world_size), gerr,
                       static_cast<bf16_t*>(out));
    return (int)hipGetLastError();
}
