// EF14 with an fp32 residual under a bf16 bucket, for MI355X (gfx950): the encode and pack phases
// of a plan whose bucket, sketch, projections and packed values are bf16 while the residual E is
// kept in fp32.  With f = bf16 -> fp32 (exact) and b = fp32 -> bf16
// (round to nearest even, NaN -> 0x7FC0: cvt_pk_bf16 of common.h):
//
//   encode : X = f(G) + E (err_in = 1) or f(G) (err_in = 0), one fp32 add;  E := X
//            sketch[SKETCH seg][row][j] = b( sum_c X[row][c] * f(V[c][j]) ), fp32 sum, one rounding
//            sketch[RAW seg][e] = b(X[e]);  DENSE segments: nothing
//   pack   : selected row (every element of a DENSE segment, whose X is formed here as above):
//            packed = b(X);  E := X - f(packed), one fp32 subtract;  other rows keep E = X
//
// Select and decode are the plan's own (arctopk_select, arctopk_decode): both phases write the
// plan's sketch and packed layouts.  These are kernels of their own: nothing here is shared with
// the bf16-residual kernels of arctopk_kernels.hip but the plan's segment table.
//
// Work mapping.  A plan gets one table of encode tiles and one of pack chunks, built at its first
// call here (mixed_table; freed with the plan), so a call is two launches at most and no copy.
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
//
// The second half of the file is EF21 with both residuals in fp32: an
// encode, a pack and a decode of their own over the same tables plus one of decode tiles; see there.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <vector>

#include "common.h"

namespace {

using namespace arctopk;

constexpr int kMxBlock = 256;
constexpr int64_t kMxPackElems = 8192;   // elements per pack chunk
constexpr int64_t kMxRawElems = 4096;    // elements per RAW encode tile
constexpr int kMxUnits = 4;             // 16-B units of G (and 32 B of E) a lane loads per step
constexpr int kMxPackUnits = 1;         // ... and 32-B units of E a pack thread loads per step (headline pack:
                                        // 35.4 us with 1, 37.9 with 2, 38.7 with 4: its blocks are short)
constexpr int64_t kMxTargetBlocks = 2048;  // row tiles a bucket aims at (common.h: kEncTargetBlocks)

enum : int32_t { MX_RAW = 1, MX_VEC = 2, MX_VLDS = 4,          // encode tile flags
                 MX_SHORT = 8, MX_DENSE = 16 };                // ... and those of the EF21 decode's tiles
enum : int32_t { MXP_ROWS = 0, MXP_ROWS_VEC = 1, MXP_DENSE = 2 };  // pack chunk modes

struct MxTile {
    int32_t seg;
    int32_t flags;
    int64_t row0;    // first row (RAW: first element)
    int32_t nrows;   // rows (RAW: elements)
    int32_t lanes;   // lanes per row
    int32_t rstride; // the tile's rows are row0 + q * rstride, q < nrows: the tiles of a tensor
    int32_t pad;     //   interleave, so the blocks in flight stream one advancing window of it
};

struct MxChunk {
    int32_t seg;
    int32_t mode;
    int64_t j0;      // first selected row (DENSE: first element)
    int32_t nj;      // selected rows (DENSE: elements)
    int32_t pad;
};

struct MxTab {       // the plan's mixed work tables (device) and their sizes
    MxTile* d_tiles;
    MxChunk* d_chunks;
    MxTile* d_dtiles;  // decode tiles of the EF21 branch (k_mx_decode21)
    int n_tiles, n_chunks, n_dtiles;
    int lds_bytes;   // dynamic LDS of the encode launch
};

__device__ __forceinline__ float bf_bits_f(uint32_t u16) { return __uint_as_float(u16 << 16); }
__device__ __forceinline__ uint16_t f_to_bf(float f) { return (uint16_t)(cvt_pk_bf16(f, 0.0f) & 0xFFFFu); }

typedef float vf4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ vf4_t ld_f4_nt(const float* p) {
    return __builtin_nontemporal_load(reinterpret_cast<const vf4_t*>(p));
}
__device__ __forceinline__ void st_f4_nt(float* p, vf4_t v) {
    __builtin_nontemporal_store(v, reinterpret_cast<vf4_t*>(p));
}
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

// X of the 8 elements at g8 / e8 (16-B / 32-B aligned): f(G) + E or f(G); E := X
template <bool ERR_IN>
__device__ __forceinline__ void fold8(const bf16_t* __restrict__ g8, float* __restrict__ e8, float (&x)[8]) {
    unpack8(ld16raw<bf16_t, kEncNtLoad>(g8, 0), x);
    if constexpr (ERR_IN) {
        const vf4_t a = ld_f4_nt(e8), b = ld_f4_nt(e8 + 4);
        x[0] += a.x, x[1] += a.y, x[2] += a.z, x[3] += a.w;
        x[4] += b.x, x[5] += b.y, x[6] += b.z, x[7] += b.w;
    }
}

// ---- encode --------------------------------------------------------------------------------
// One tile of rows.  RR: the rank when it is 4, else 0 (rank r at run time, up to kMaxR).
template <int RR, bool ERR_IN, bool VEC, bool VLDS>
__device__ __forceinline__ void enc_rows(const SegDev& s, const MxTile& t, int r, const bf16_t* __restrict__ grad,
                                         float* __restrict__ err, const bf16_t* __restrict__ V,
                                         bf16_t* __restrict__ sketch, const uint16_t* __restrict__ vt) {
    constexpr int NR = RR ? RR : kMaxR;
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
                            if constexpr (ERR_IN) {
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
                        if constexpr (ERR_IN) {
                            x[0] += ea[k].x, x[1] += ea[k].y, x[2] += ea[k].z, x[3] += ea[k].w;
                            x[4] += eb[k].x, x[5] += eb[k].y, x[6] += eb[k].z, x[7] += eb[k].w;
                        }
                        float* e8 = err + base + 8 * (int64_t)u;
                        st_f4_nt(e8, vf4_t{x[0], x[1], x[2], x[3]});
                        st_f4_nt(e8 + 4, vf4_t{x[4], x[5], x[6], x[7]});
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
                    if constexpr (ERR_IN) x += err[base + c];
                    err[base + c] = x;
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

template <int RR, bool ERR_IN>
__global__ void __launch_bounds__(kMxBlock) k_mx_encode(const SegDev* __restrict__ segs,
                                                       const MxTile* __restrict__ tiles, int r,
                                                       const bf16_t* __restrict__ grad, float* __restrict__ err,
                                                       const bf16_t* __restrict__ V, bf16_t* __restrict__ sketch) {
    extern __shared__ __attribute__((aligned(16))) uint16_t mx_vt[];
    const MxTile t = tiles[blockIdx.x];
    const SegDev& s = segs[t.seg];
    if (t.flags & MX_RAW) {
        for (int i = threadIdx.x; i < t.nrows; i += kMxBlock) {
            const int64_t e = t.row0 + i;
            float x = ld1<bf16_t, kEncNtLoad>(grad + s.offset + e);
            if constexpr (ERR_IN) x += err[s.offset + e];
            err[s.offset + e] = x;
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
        if (t.flags & MX_VEC) enc_rows<RR, ERR_IN, true, true>(s, t, r, grad, err, V, sketch, mx_vt);
        else enc_rows<RR, ERR_IN, false, true>(s, t, r, grad, err, V, sketch, mx_vt);
    } else {
        if (t.flags & MX_VEC) enc_rows<RR, ERR_IN, true, false>(s, t, r, grad, err, V, sketch, mx_vt);
        else enc_rows<RR, ERR_IN, false, false>(s, t, r, grad, err, V, sketch, mx_vt);
    }
}

// ---- pack ----------------------------------------------------------------------------------
template <bool ERR_IN>
__global__ void __launch_bounds__(kMxBlock) k_mx_pack(const SegDev* __restrict__ segs,
                                                     const MxChunk* __restrict__ chunks,
                                                     const bf16_t* __restrict__ grad, float* __restrict__ err,
                                                     const int32_t* __restrict__ rowlist,
                                                     bf16_t* __restrict__ packed) {
    const MxChunk ch = chunks[blockIdx.x];
    const SegDev& s = segs[ch.seg];
    const int m = (int)s.m;
    if (ch.mode == MXP_DENSE) {
        // X is formed here (a DENSE segment has no encode work): every element is selected
        const bf16_t* g = grad + s.offset + ch.j0;
        float* e = err + s.offset + ch.j0;
        bf16_t* p = packed + s.packed_off + ch.j0;
        int done = 0;
        if (s.offset % 8 == 0 && s.packed_off % 8 == 0) {  // (chunks start at multiples of 8 elements)
            const int nu = ch.nj / 8;
            for (int u = threadIdx.x; u < nu; u += kMxBlock) {
                float x[8], y[8];
                fold8<ERR_IN>(g + 8 * u, e + 8 * u, x);
                const u4_t w = pack8(x);
                unpack8(w, y);
                __builtin_nontemporal_store(w, reinterpret_cast<u4_t*>(p + 8 * u));
                st_f4_nt(e + 8 * u, vf4_t{x[0] - y[0], x[1] - y[1], x[2] - y[2], x[3] - y[3]});
                st_f4_nt(e + 8 * u + 4, vf4_t{x[4] - y[4], x[5] - y[5], x[6] - y[6], x[7] - y[7]});
            }
            done = nu * 8;
        }
        for (int i = done + (int)threadIdx.x; i < ch.nj; i += kMxBlock) {
            float x = to_f(g[i]);
            if constexpr (ERR_IN) x += e[i];
            const uint16_t w = f_to_bf(x);
            p[i].u = w;
            e[i] = x - bf_bits_f(w);
        }
        return;
    }
    const int32_t* rl = rowlist + s.sel_off + ch.j0;
    bf16_t* p = packed + s.packed_off + ch.j0 * (int64_t)m;
    if (ch.mode == MXP_ROWS_VEC) {
        const int U = m / 8, nu = ch.nj * U;
        const bool p16 = s.packed_off % 8 == 0;  // (m % 8 == 0: every row of the segment alike)
        for (int u0 = threadIdx.x; u0 < nu; u0 += kMxBlock * kMxPackUnits) {
            float* e8[kMxPackUnits];
            vf4_t a[kMxPackUnits], b[kMxPackUnits];
#pragma unroll
            for (int k = 0; k < kMxPackUnits; ++k) {
                const int u = u0 + k * kMxBlock;
                e8[k] = nullptr;
                if (u < nu) {
                    const int jj = u / U, c8 = u - jj * U;
                    const int64_t row = rl[jj];
                    if ((uint64_t)row < (uint64_t)s.n) {  // (always, for a select's row list)
                        e8[k] = err + s.offset + row * (int64_t)m + 8 * c8;
                        a[k] = ld_f4_nt(e8[k]);
                        b[k] = ld_f4_nt(e8[k] + 4);
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < kMxPackUnits; ++k) {
                if (!e8[k]) continue;
                const int u = u0 + k * kMxBlock;
                const float x[8] = {a[k].x, a[k].y, a[k].z, a[k].w, b[k].x, b[k].y, b[k].z, b[k].w};
                float y[8];
                const u4_t w = pack8(x);
                unpack8(w, y);
                bf16_t* dst = p + 8 * (int64_t)u;
                if (p16) {
                    __builtin_nontemporal_store(w, reinterpret_cast<u4_t*>(dst));
                } else {
                    reinterpret_cast<u2_t*>(dst)[0] = u2_t{w.x, w.y};
                    reinterpret_cast<u2_t*>(dst)[1] = u2_t{w.z, w.w};
                }
                st_f4_nt(e8[k], vf4_t{x[0] - y[0], x[1] - y[1], x[2] - y[2], x[3] - y[3]});
                st_f4_nt(e8[k] + 4, vf4_t{x[4] - y[4], x[5] - y[5], x[6] - y[6], x[7] - y[7]});
            }
        }
        return;
    }
    const int ne = ch.nj * m;
    for (int i = threadIdx.x; i < ne; i += kMxBlock) {
        const int jj = i / m, c = i - jj * m;
        const int64_t row = rl[jj];
        if ((uint64_t)row >= (uint64_t)s.n) continue;
        float* e = err + s.offset + row * (int64_t)m + c;
        const float x = *e;
        const uint16_t w = f_to_bf(x);
        p[i].u = w;
        *e = x - bf_bits_f(w);
    }
}

// ---- EF21 with both residuals in fp32 ---------------------------------
//   encode : D = f(G) - E, one fp32 subtract; the sketch of D as above; E is only read
//   pack   : selected row (every element of a DENSE segment): packed = b(D);  E := E + f(packed)
//   decode : selected element: gE := gE + f(P) / ws (the mean is not rounded to bf16);
//            out = b(gE) on every element of the bucket; gE of the other rows is left as stored
// Kernels of their own over the same tables: the encode reads the tiles of k_mx_encode, the pack
// the chunks of k_mx_pack, the decode a third table (MxTab::d_dtiles) that holds the encode's row
// tiles again for rows of more than two columns, element tiles with a thread per row for RAW
// tensors and rows of one or two columns, and element tiles for DENSE segments.

// mean of the all-reduced values: x / ws correctly rounded (Scale of arctopk_kernels.hip)
struct MxScale {
    float ws, inv;
    int pow2;
    __device__ __forceinline__ float operator()(float x) const { return pow2 ? x * inv : __fdiv_rn(x, ws); }
};

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

// One tile of rows of the EF21 encode: enc_rows with D = f(G) - E and no store of E.
template <int RR, bool VEC, bool VLDS>
__device__ __forceinline__ void enc21_rows(const SegDev& s, const MxTile& t, int r, const bf16_t* __restrict__ grad,
                                           const float* __restrict__ err, const bf16_t* __restrict__ V,
                                           bf16_t* __restrict__ sketch, const uint16_t* __restrict__ vt) {
    constexpr int NR = RR ? RR : kMaxR;
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
                for (int u0 = l; u0 < m / 8; u0 += lanes * kMxUnits) {
                    u4_t graw[kMxUnits];
                    vf4_t ea[kMxUnits], eb[kMxUnits];
#pragma unroll
                    for (int k = 0; k < kMxUnits; ++k) {
                        const int u = u0 + k * lanes;
                        if (u < m / 8) {
                            graw[k] = ld16raw<bf16_t, kEncNtLoad>(grad + base + 8 * (int64_t)u, 0);
                            ea[k] = ld_f4_nt(err + base + 8 * (int64_t)u);
                            eb[k] = ld_f4_nt(err + base + 8 * (int64_t)u + 4);
                        }
                    }
#pragma unroll
                    for (int k = 0; k < kMxUnits; ++k) {
                        const int u = u0 + k * lanes;
                        if (u >= m / 8) break;
                        float x[8];
                        unpack8(graw[k], x);
                        x[0] -= ea[k].x, x[1] -= ea[k].y, x[2] -= ea[k].z, x[3] -= ea[k].w;
                        x[4] -= eb[k].x, x[5] -= eb[k].y, x[6] -= eb[k].z, x[7] -= eb[k].w;
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
                    const float x = ld1<bf16_t, kEncNtLoad>(grad + base + c) - err[base + c];
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

template <int RR>
__global__ void __launch_bounds__(kMxBlock) k_mx_encode21(const SegDev* __restrict__ segs,
                                                         const MxTile* __restrict__ tiles, int r,
                                                         const bf16_t* __restrict__ grad,
                                                         const float* __restrict__ err,
                                                         const bf16_t* __restrict__ V, bf16_t* __restrict__ sketch) {
    extern __shared__ __attribute__((aligned(16))) uint16_t mx_vt[];
    const MxTile t = tiles[blockIdx.x];
    const SegDev& s = segs[t.seg];
    if (t.flags & MX_RAW) {
        for (int i = threadIdx.x; i < t.nrows; i += kMxBlock) {
            const int64_t e = s.offset + t.row0 + i;
            sketch[s.sketch_off + t.row0 + i].u = f_to_bf(ld1<bf16_t, kEncNtLoad>(grad + e) - err[e]);
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
        if (t.flags & MX_VEC) enc21_rows<RR, true, true>(s, t, r, grad, err, V, sketch, mx_vt);
        else enc21_rows<RR, false, true>(s, t, r, grad, err, V, sketch, mx_vt);
    } else {
        if (t.flags & MX_VEC) enc21_rows<RR, true, false>(s, t, r, grad, err, V, sketch, mx_vt);
        else enc21_rows<RR, false, false>(s, t, r, grad, err, V, sketch, mx_vt);
    }
}

// D of the 8 elements at g8 / e8, packed = b(D) to p8, E := E + f(packed)
__device__ __forceinline__ void pack21_unit(const bf16_t* __restrict__ g8, float* __restrict__ e8,
                                            bf16_t* __restrict__ p8, bool p16) {
    float x[8], y[8];
    unpack8(ld16raw<bf16_t, kEncNtLoad>(g8, 0), x);
    const vf4_t a = ld_f4_nt(e8), b = ld_f4_nt(e8 + 4);
    const float e[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] -= e[i];
    const u4_t w = pack8(x);
    unpack8(w, y);
    st8bf(p8, p16, w);
    st_f4_nt(e8, vf4_t{e[0] + y[0], e[1] + y[1], e[2] + y[2], e[3] + y[3]});
    st_f4_nt(e8 + 4, vf4_t{e[4] + y[4], e[5] + y[5], e[6] + y[6], e[7] + y[7]});
}
__device__ __forceinline__ void pack21_elem(const bf16_t* __restrict__ g, float* __restrict__ e,
                                            bf16_t* __restrict__ p) {
    const float ev = *e;
    const uint16_t w = f_to_bf(to_f(*g) - ev);
    p->u = w;
    *e = ev + bf_bits_f(w);
}

__global__ void __launch_bounds__(kMxBlock) k_mx_pack21(const SegDev* __restrict__ segs,
                                                       const MxChunk* __restrict__ chunks,
                                                       const bf16_t* __restrict__ grad, float* __restrict__ err,
                                                       const int32_t* __restrict__ rowlist,
                                                       bf16_t* __restrict__ packed) {
    const MxChunk ch = chunks[blockIdx.x];
    const SegDev& s = segs[ch.seg];
    const int m = (int)s.m;
    if (ch.mode == MXP_DENSE) {  // every element is selected
        const bf16_t* g = grad + s.offset + ch.j0;
        float* e = err + s.offset + ch.j0;
        bf16_t* p = packed + s.packed_off + ch.j0;
        int done = 0;
        if (s.offset % 8 == 0 && s.packed_off % 8 == 0) {  // (chunks start at multiples of 8 elements)
            const int nu = ch.nj / 8;
            for (int u = threadIdx.x; u < nu; u += kMxBlock) pack21_unit(g + 8 * u, e + 8 * u, p + 8 * u, true);
            done = nu * 8;
        }
        for (int i = done + (int)threadIdx.x; i < ch.nj; i += kMxBlock) pack21_elem(g + i, e + i, p + i);
        return;
    }
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
            pack21_unit(grad + el, err + el, p + 8 * (int64_t)u, p16);
        }
        return;
    }
    const int ne = ch.nj * m;
    for (int i = threadIdx.x; i < ne; i += kMxBlock) {
        const int jj = i / m, c = i - jj * m;
        const int64_t row = rl[jj];
        if ((uint64_t)row >= (uint64_t)s.n) continue;
        const int64_t el = s.offset + row * (int64_t)m + c;
        pack21_elem(grad + el, err + el, p + i);
    }
}

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
int pow2_at_least(int64_t x) {
    int p = 1;
    while (p < x && p < 64) p <<= 1;
    return p;
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
            for (int64_t e = 0; e < s.n; e += kMxPackElems)
                chunks.push_back(MxChunk{i, MXP_DENSE, e, (int32_t)std::min<int64_t>(kMxPackElems, s.n - e), 0});
            const int dflags = MX_DENSE | ((s.offset % 8 == 0 && s.packed_off % 8 == 0) ? MX_VEC : 0);
            for (int64_t e = 0; e < s.n; e += kMxPackElems)
                dtiles.push_back(MxTile{i, dflags, e, (int32_t)std::min<int64_t>(kMxPackElems, s.n - e), 1, 1, 0});
            continue;
        }
        if (s.kind == ARCTOPK_SEG_RAW) {
            for (int64_t e = 0; e < s.n; e += kMxRawElems)
                tiles.push_back(MxTile{i, MX_RAW, e, (int32_t)std::min<int64_t>(kMxRawElems, s.n - e), 1, 1, 0});
        } else {
            const bool vlds = s.m * r * 4 <= (int64_t)kVLdsMaxBytes;
            const int lanes = pow2_at_least(vec ? s.m / 8 : s.m);
            const int groups = kMxBlock / lanes;
            // whole rounds of the block's groups, at least one
            int64_t per = std::max<int64_t>(1, tile_elems / s.m);
            per = std::max<int64_t>(groups, per / groups * groups);
            const int flags = (vec ? MX_VEC : 0) | (vlds ? MX_VLDS : 0);
            // tile ti holds rows ti, ti + ntiles, ...: consecutive blocks read adjacent rows
            const int64_t ntiles = (s.n + per - 1) / per;
            for (int64_t ti = 0; ti < ntiles; ++ti) {
                tiles.push_back(MxTile{i, flags, ti, (int32_t)((s.n - ti + ntiles - 1) / ntiles), lanes,
                                       (int32_t)ntiles, 0});
                if (s.m > 2) dtiles.push_back(tiles.back());  // the decode walks the same rows
            }
            if (vlds) lds = std::max<int>(lds, (int)(((s.m + 7) & ~int64_t(7)) * r * 2));
        }
        if (s.m <= 2)  // RAW tensors and rows of one or two columns: a decode thread per row
            for (int64_t e = 0; e < s.n; e += kMxRawElems)
                dtiles.push_back(MxTile{i, MX_SHORT, e, (int32_t)std::min<int64_t>(kMxRawElems, s.n - e), 1, 1, 0});
        const int64_t per = std::max<int64_t>(1, kMxPackElems / s.m);
        for (int64_t j = 0; j < s.k_rows; j += per)
            chunks.push_back(MxChunk{i, vec ? MXP_ROWS_VEC : MXP_ROWS, j,
                                     (int32_t)std::min<int64_t>(per, s.k_rows - j), 0});
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
    hipError_t e = hipSetDevice(p->device);
    if (e == hipSuccess) e = hipMalloc((void**)&t->d_tiles, std::max<size_t>(1, tiles.size()) * sizeof(MxTile));
    if (e == hipSuccess && !tiles.empty())
        e = hipMemcpy(t->d_tiles, tiles.data(), tiles.size() * sizeof(MxTile), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc((void**)&t->d_chunks, std::max<size_t>(1, chunks.size()) * sizeof(MxChunk));
    if (e == hipSuccess && !chunks.empty())
        e = hipMemcpy(t->d_chunks, chunks.data(), chunks.size() * sizeof(MxChunk), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc((void**)&t->d_dtiles, std::max<size_t>(1, dtiles.size()) * sizeof(MxTile));
    if (e == hipSuccess && !dtiles.empty())
        e = hipMemcpy(t->d_dtiles, dtiles.data(), dtiles.size() * sizeof(MxTile), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (t->d_tiles) (void)hipFree(t->d_tiles);
        if (t->d_chunks) (void)hipFree(t->d_chunks);
        if (t->d_dtiles) (void)hipFree(t->d_dtiles);
        delete t;
        return (int)e;
    }
    const_cast<arctopk_plan*>(p)->mx = t;
    *out = t;
    return 0;
}

}  // namespace

namespace arctopk {
void mixed_forget(arctopk_plan* p) {
    MxTab* t = static_cast<MxTab*>(p->mx);
    if (!t) return;
    if (t->d_tiles) (void)hipFree(t->d_tiles);
    if (t->d_chunks) (void)hipFree(t->d_chunks);
    if (t->d_dtiles) (void)hipFree(t->d_dtiles);
    delete t;
    p->mx = nullptr;
}
}  // namespace arctopk

extern "C" int arctopk_encode_mixed(const arctopk_plan* p, const void* grad, float* err, int32_t err_in,
                                    const void* V, void* sketch, void* stream) {
    if (!p || p->dtype != ARCTOPK_BF16 || !grad || !err || (err_in != 0 && err_in != 1)) return ARCTOPK_EINVAL;
    if ((p->info.v_len > 0 && !V) || (p->info.sketch_len > 0 && !sketch)) return ARCTOPK_EINVAL;
    if (((uintptr_t)grad & 15) || ((uintptr_t)err & 15) || ((uintptr_t)V & 1) || ((uintptr_t)sketch & 1))
        return ARCTOPK_EINVAL;
    MxTab* t = nullptr;
    const int st = mixed_table(p, &t);
    if (st) return st;
    if (t->n_tiles == 0) return 0;  // DENSE segments only: X is formed by the pack
    const bf16_t* g = static_cast<const bf16_t*>(grad);
    const bf16_t* v = static_cast<const bf16_t*>(V);
    bf16_t* sk = static_cast<bf16_t*>(sketch);
    const dim3 grid((unsigned)t->n_tiles), block(kMxBlock);
    hipStream_t hs = (hipStream_t)stream;
    const size_t lds = (size_t)t->lds_bytes;
    if (p->r == 4) {
        if (err_in) hipLaunchKernelGGL((k_mx_encode<4, true>), grid, block, lds, hs, p->d_segs, t->d_tiles, p->r, g, err, v, sk);
        else hipLaunchKernelGGL((k_mx_encode<4, false>), grid, block, lds, hs, p->d_segs, t->d_tiles, p->r, g, err, v, sk);
    } else {
        if (err_in) hipLaunchKernelGGL((k_mx_encode<0, true>), grid, block, lds, hs, p->d_segs, t->d_tiles, p->r, g, err, v, sk);
        else hipLaunchKernelGGL((k_mx_encode<0, false>), grid, block, lds, hs, p->d_segs, t->d_tiles, p->r, g, err, v, sk);
    }
    return (int)hipGetLastError();
}

extern "C" int arctopk_pack_mixed(const arctopk_plan* p, const void* grad, float* err, int32_t err_in,
                                  const int32_t* rowlist, const int32_t* slotmap, void* packed, void* stream) {
    if (!p || p->dtype != ARCTOPK_BF16 || !err || !rowlist || !slotmap || !packed || (err_in != 0 && err_in != 1))
        return ARCTOPK_EINVAL;
    if (p->n_dense > 0 && !grad) return ARCTOPK_EINVAL;  // a DENSE segment's X = f(G) + E is formed here
    if (((uintptr_t)grad & 15) || ((uintptr_t)err & 15) || ((uintptr_t)packed & 15)) return ARCTOPK_EINVAL;
    MxTab* t = nullptr;
    const int st = mixed_table(p, &t);
    if (st) return st;
    if (t->n_chunks == 0) return 0;
    const bf16_t* g = static_cast<const bf16_t*>(grad);
    bf16_t* pk = static_cast<bf16_t*>(packed);
    const dim3 grid((unsigned)t->n_chunks), block(kMxBlock);
    hipStream_t hs = (hipStream_t)stream;
    if (err_in) hipLaunchKernelGGL((k_mx_pack<true>), grid, block, 0, hs, p->d_segs, t->d_chunks, g, err, rowlist, pk);
    else hipLaunchKernelGGL((k_mx_pack<false>), grid, block, 0, hs, p->d_segs, t->d_chunks, g, err, rowlist, pk);
    return (int)hipGetLastError();
}

extern "C" int arctopk_encode_mixed21(const arctopk_plan* p, const void* grad, const float* err, const void* V,
                                      void* sketch, void* stream) {
    if (!p || p->dtype != ARCTOPK_BF16 || !grad || !err) return ARCTOPK_EINVAL;
    if ((p->info.v_len > 0 && !V) || (p->info.sketch_len > 0 && !sketch)) return ARCTOPK_EINVAL;
    if (((uintptr_t)grad & 15) || ((uintptr_t)err & 15) || ((uintptr_t)V & 1) || ((uintptr_t)sketch & 1))
        return ARCTOPK_EINVAL;
    MxTab* t = nullptr;
    const int st = mixed_table(p, &t);
    if (st) return st;
    if (t->n_tiles == 0) return 0;  // DENSE segments only: D is formed by the pack
    const bf16_t* g = static_cast<const bf16_t*>(grad);
    const bf16_t* v = static_cast<const bf16_t*>(V);
    bf16_t* sk = static_cast<bf16_t*>(sketch);
    const dim3 grid((unsigned)t->n_tiles), block(kMxBlock);
    hipStream_t hs = (hipStream_t)stream;
    const size_t lds = (size_t)t->lds_bytes;
    if (p->r == 4) hipLaunchKernelGGL((k_mx_encode21<4>), grid, block, lds, hs, p->d_segs, t->d_tiles, p->r, g, err, v, sk);
    else hipLaunchKernelGGL((k_mx_encode21<0>), grid, block, lds, hs, p->d_segs, t->d_tiles, p->r, g, err, v, sk);
    return (int)hipGetLastError();
}

extern "C" int arctopk_pack_mixed21(const arctopk_plan* p, const void* grad, float* err, const int32_t* rowlist,
                                    const int32_t* slotmap, void* packed, void* stream) {
    if (!p || p->dtype != ARCTOPK_BF16 || !grad || !err || !rowlist || !slotmap || !packed) return ARCTOPK_EINVAL;
    if (((uintptr_t)grad & 15) || ((uintptr_t)err & 15) || ((uintptr_t)packed & 15)) return ARCTOPK_EINVAL;
    MxTab* t = nullptr;
    const int st = mixed_table(p, &t);
    if (st) return st;
    if (t->n_chunks == 0) return 0;
    hipLaunchKernelGGL(k_mx_pack21, dim3((unsigned)t->n_chunks), dim3(kMxBlock), 0, (hipStream_t)stream, p->d_segs,
                       t->d_chunks, static_cast<const bf16_t*>(grad), err, rowlist, static_cast<bf16_t*>(packed));
    return (int)hipGetLastError();
}

extern "C" int arctopk_decode_mixed21(const arctopk_plan* p, const void* packed, const int32_t* slotmap,
                                      int32_t world_size, float* gerr, void* out, void* stream) {
    if (!p || p->dtype != ARCTOPK_BF16 || !packed || !slotmap || !gerr || !out || world_size < 1)
        return ARCTOPK_EINVAL;
    if (((uintptr_t)packed & 15) || ((uintptr_t)gerr & 15) || ((uintptr_t)out & 15)) return ARCTOPK_EINVAL;
    MxTab* t = nullptr;
    const int st = mixed_table(p, &t);
    if (st) return st;
    if (t->n_dtiles == 0) return 0;
    MxScale sc;
    sc.ws = (float)world_size;
    sc.pow2 = (world_size & (world_size - 1)) == 0;
    sc.inv = 1.0f / (float)world_size;
    hipLaunchKernelGGL(k_mx_decode21, dim3((unsigned)t->n_dtiles), dim3(kMxBlock), 0, (hipStream_t)stream, p->d_segs,
                       t->d_dtiles, static_cast<const bf16_t*>(packed), slotmap, sc, gerr, static_cast<bf16_t*>(out));
    return (int)hipGetLastError();
}
