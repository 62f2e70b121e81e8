// K1 encode for sketch ranks 16 and 32 on the matrix units of gfx950.
//
//   P[rows, r] = X[rows, m] . V[m, r],  X = G (noef) | G + E, E := X (EF14) | G - E (EF21)
//
// One block (4 waves) per tile of up to kMfTileRows rows.  The block walks the tile's columns in
// K-slabs of 64 16-B units per row.  Per slab it stages V^T [r][slab] in LDS once, then for each
// row tile of r rows: all 256 threads load the X tile coalesced (16-B units where the segment's
// offset and m allow, else element by element), apply the EF rule, store E, and write X to LDS
// in the bucket dtype; the four waves then split the slab's k-groups among them and accumulate
// P^T = V^T . X^T in fp32 with
//   fp32 buckets: v_mfma_f32_32x32x2_f32 (r = 32) / v_mfma_f32_16x16x4_f32 (r = 16),
//   bf16 buckets: v_mfma_f32_32x32x16_bf16 (r = 32) / v_mfma_f32_16x16x32_bf16 (r = 16).
// M is the rank index j, N the bucket row.  With TR = r rows per row tile and H = 64 / r, lane
// (n = lane % r, h = lane / r) reads 16-B unit kg * H + h of LDS row n of V^T (as A, j = n) and
// of X (as B): a bf16 unit is the lane's 8 K values of one MFMA; the four fp32 words of a unit
// feed four MFMAs (word i of every lane: K index h <-> column 4 (kg H + h) + i in both operands).
// Rows >= n and columns >= m are zeros in LDS, never read from memory.  The next X tile's loads
// are in flight in registers while the current one is multiplied.  At the tile's end the waves'
// partial accumulators are summed through LDS in wave order and stored (sketch in the bucket
// dtype, rounded once; fp32 partials of a column part; or the row's energy key in keys mode).
//
// bf16 operands of an fp32 bucket (arctopk_plan_set_sketch_operands; DESIGN.md 4k, "bf16 operands"):
// G, E and V stay fp32 in memory and the slab stays 256 columns, so the plan's tiles, the X prefetch
// and the E store are the fp32 kernel's; X (after the fp32 EF rule and the E store) and V are rounded
// with cvt_pk_bf16 on their way into LDS, whose rows then hold 256 bf16 (528 B with the padding, half
// the bytes) in the bf16 kernel's layout, and the walk issues the bf16 MFMAs: one per k-group of
// 8 H columns where the fp32 operands take four.
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include "encode_mfma.h"

using namespace arctopk;

namespace {

typedef float v4f __attribute__((ext_vector_type(4)));
typedef float v16f __attribute__((ext_vector_type(16)));
typedef __bf16 bf8_t __attribute__((ext_vector_type(8)));

constexpr int kSlabUnits = kMfSlabBytes / 16;  // 16-B units of G (and of E) per row per slab

template <int R> struct Acc;
template <> struct Acc<32> { typedef v16f type; static constexpr int N = 16; };
template <> struct Acc<16> { typedef v4f type; static constexpr int N = 4; };

// one k-group: the lane's unit of V^T (a) and of X (b)
template <typename T, int R>
__device__ __forceinline__ void mfma_unit(typename Acc<R>::type& c, const u4_t a, const u4_t b) {
    if constexpr (sizeof(T) == 4) {
        const float af[4] = {__uint_as_float(a.x), __uint_as_float(a.y), __uint_as_float(a.z), __uint_as_float(a.w)};
        const float bf[4] = {__uint_as_float(b.x), __uint_as_float(b.y), __uint_as_float(b.z), __uint_as_float(b.w)};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if constexpr (R == 32) c = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i], bf[i], c, 0, 0, 0);
            else c = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i], bf[i], c, 0, 0, 0);
        }
    } else {
        const bf8_t av = __builtin_bit_cast(bf8_t, a), bv = __builtin_bit_cast(bf8_t, b);
        if constexpr (R == 32) c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, bv, c, 0, 0, 0);
        else c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, bv, c, 0, 0, 0);
    }
}

// X = G (+|-) E of a 16-B unit, rounded to T as the reference's in-place add_ on a T bucket
template <typename T, int EF, bool ERR_IN>
__device__ __forceinline__ u4_t combine_unit(const u4_t g, const u4_t e) {
    constexpr bool kAdd = EF == ARCTOPK_EF14 && ERR_IN, kSub = EF == ARCTOPK_EF21;
    if constexpr (!kAdd && !kSub) return g;
    const uint32_t gw[4] = {g.x, g.y, g.z, g.w}, ew[4] = {e.x, e.y, e.z, e.w};
    uint32_t x[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if constexpr (sizeof(T) == 4) {
            const float a = __uint_as_float(gw[i]), b = __uint_as_float(ew[i]);
            x[i] = __float_as_uint(kSub ? a - b : a + b);
        } else {
            const float gl = __uint_as_float(gw[i] << 16), gh = __uint_as_float(gw[i] & 0xFFFF0000u);
            const float el = __uint_as_float(ew[i] << 16), eh = __uint_as_float(ew[i] & 0xFFFF0000u);
            x[i] = kSub ? cvt_pk_bf16(gl - el, gh - eh) : cvt_pk_bf16(gl + el, gh + eh);
        }
    }
    return u4_t{x[0], x[1], x[2], x[3]};
}

// the order key of a row's energy, formed from its r fp32 sums exactly as the select's key pass
// forms it from the stored sketch at world size 1 (arctopk_kernels.hip: energy_regs, energy_key)
template <typename T>
__device__ __forceinline__ uint32_t row_key(const float* __restrict__ p, int R) {
    const float a = rnd<T>(p[0]);
    float s = rnd<T>(__fmul_rn(a, a));
    for (int j = 1; j < R; ++j) {
        const float b = rnd<T>(p[j]);
        s = __fadd_rn(s, rnd<T>(__fmul_rn(b, b)));
    }
    s = rnd<T>(s);
    uint32_t u = __float_as_uint(s);
    if (s != s) u = 0x7FFFFFFFu;
    return u & 0x7FFFFFFFu ? u : 0u;
}

// T: the bucket's element type in memory; O: the operands' type in LDS and in the MFMA -- T itself,
// or bf16_t under an fp32 bucket (arctopk_plan_set_sketch_operands): X and V are then rounded
// on their way into LDS, E and the sums stay fp32.  At r = 32 that variant is built for three waves
// per SIMD: its 33,792 B of LDS let three blocks share a CU, which the compiler's 140 + 32 registers
// miss by four (168 with 4 VGPRs spilled under EF14 / EF21); measured 216 -> 177 us on the headline
// bucket.  0: every other instantiation is left to the compiler, as before.
template <typename T, typename O, int R, int EF, bool ERR_IN>
__global__ void __launch_bounds__(256)
__attribute__((amdgpu_waves_per_eu(sizeof(O) != sizeof(T) && R == 32 ? 3 : 0))) k_encode_mfma(const SegDev* __restrict__ segs,
                                                     const EncTile* __restrict__ tiles,
                                                     const T* __restrict__ G, T* __restrict__ E,
                                                     const T* __restrict__ V, T* __restrict__ sketch,
                                                     float* __restrict__ part_buf, uint32_t* __restrict__ keys) {
    extern __shared__ __attribute__((aligned(16))) u4_t smem[];
    constexpr int TR = R;                 // rows of a row tile (the MFMA's N)
    constexpr int H = 64 / R;             // lane groups: 16-B units of a k-group
    constexpr int NT = kMfTileRows / TR;  // row tiles of a block at most
    constexpr bool OPB = sizeof(O) != sizeof(T);  // bf16 operands of an fp32 bucket
    constexpr int EPU = 16 / (int)sizeof(T);  // elements per unit of G / E / V
    constexpr int LPU = 16 / (int)sizeof(O);  // ... and per unit of an LDS row
    constexpr int UR = LPU / EPU;             // units of G that make one LDS unit (1; OPB: 2)
    constexpr int SLAB = kSlabUnits * EPU;    // columns per slab
    constexpr int kRowUnits = SLAB / LPU + 1;  // LDS row stride in units: the slab and one unit of padding
    constexpr int kRowWords = kRowUnits * 4;
    constexpr int XU = TR / 4;                // X units per thread per row tile
    constexpr int VU = sizeof(O) == 4 ? R / 4 : R / 8;  // V work items per thread per slab
    static_assert(2 * R * kRowUnits * 16 <= 2 * R * kMfRowBytes && 4 * R * 4 <= kRowUnits * 16,
                  "V^T and X fit the plan's LDS bound; the waves' partial sums fit the X tile");
    constexpr bool LOAD_E = (EF == ARCTOPK_EF21) || (EF == ARCTOPK_EF14 && ERR_IN);
    constexpr bool WRITE_E = EF == ARCTOPK_EF14;
    typedef typename Acc<R>::type acc_t;

    u4_t* const vt = smem;                   // V^T [R][kRowUnits]
    u4_t* const xt = smem + R * kRowUnits;   // X   [TR][kRowUnits]
    float* const red = reinterpret_cast<float*>(xt);  // the waves' partial P [4][TR][R], after the walk

    const EncTile t = tiles[blockIdx.x];
    const SegDev s = segs[t.seg];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ln = lane % TR, lh = lane / TR;
    const int m = (int)s.m, c0 = t.c0, cl = t.clen;
    const bool vec = s.vec && (c0 % EPU) == 0;
    const int nslab = (cl + SLAB - 1) / SLAB;
    const int nnt = (int)((t.nrows + TR - 1) / TR);
    const int64_t row_end = t.row0 + t.nrows;
    const T* const Vs = V + s.v_off;
    const T* const Gs = G + s.offset;
    T* const Es = E + s.offset;

    acc_t acc[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int q = 0; q < Acc<R>::N; ++q) acc[i][q] = 0.f;

    // columns and LDS units (whole k-groups) of a slab
    auto slab_cols = [&](int sl) { return min(SLAB, cl - sl * SLAB); };
    auto slab_ku = [&](int sl) { return ((slab_cols(sl) + LPU - 1) / LPU + H - 1) / H * H; };

    // ---- X tile (slab sl, row tile nt): thread e = tid + 256 i takes unit e % ku of tile row e / ku
    // (units of G; OPB: a wave's lanes then write consecutive 8-B halves of LDS units, 512 B in a row)
    u4_t gx[XU], ex[XU];
    auto issue_x = [&](int sl, int nt) {
        const int cols = slab_cols(sl), ku = slab_ku(sl) * UR;
        const int units = cols / EPU;  // (vector path: cols is a multiple of EPU)
        const int64_t r0 = t.row0 + (int64_t)nt * TR;
#pragma unroll
        for (int i = 0; i < XU; ++i) {
            const int e = tid + 256 * i;
            const int rr = e / ku, u = e - rr * ku;
            gx[i] = u4_t{0u, 0u, 0u, 0u};
            ex[i] = u4_t{0u, 0u, 0u, 0u};
            if (rr < TR && u < units && r0 + rr < row_end) {
                const int64_t at = (r0 + rr) * m + c0 + sl * SLAB;  // 16-B aligned with the segment
                gx[i] = ld16raw<T, kEncNtLoad>(Gs + at, u);
                if constexpr (LOAD_E) ex[i] = ld16raw<T, kEncNtLoad>(Es + at, u);
            }
        }
    };
    auto stash_x = [&](int sl, int nt) {
        const int cols = slab_cols(sl), ku = slab_ku(sl) * UR;
        const int units = cols / EPU;
        const int64_t r0 = t.row0 + (int64_t)nt * TR;
#pragma unroll
        for (int i = 0; i < XU; ++i) {
            const int e = tid + 256 * i;
            const int rr = e / ku, u = e - rr * ku;
            if (rr >= TR) continue;
            const u4_t x = combine_unit<T, EF, ERR_IN>(gx[i], ex[i]);  // (zeros stay zeros)
            if constexpr (WRITE_E) {
                if (u < units && r0 + rr < row_end) {
                    u4_t* ep = reinterpret_cast<u4_t*>(Es + (r0 + rr) * m + c0 + sl * SLAB) + u;
                    if constexpr (kEncNtStore) __builtin_nontemporal_store(x, ep);
                    else *ep = x;
                }
            }
            if constexpr (OPB)  // (after the fp32 E store: only the operand is rounded)
                reinterpret_cast<u2_t*>(xt + rr * kRowUnits)[u] =
                    u2_t{cvt_pk_bf16(__uint_as_float(x.x), __uint_as_float(x.y)),
                         cvt_pk_bf16(__uint_as_float(x.z), __uint_as_float(x.w))};
            else
                xt[rr * kRowUnits + u] = x;
        }
    };
    // the same tile element by element (odd offsets, m no multiple of the unit): no prefetch
    auto stash_x_scalar = [&](int sl, int nt) {
        const int cols = slab_cols(sl), kuc = slab_ku(sl) * LPU;
        const int64_t r0 = t.row0 + (int64_t)nt * TR;
        O* const xl = reinterpret_cast<O*>(xt);
        for (int e = tid; e < TR * kuc; e += 256) {
            const int rr = e / kuc, cc = e - rr * kuc;
            float x = 0.f;
            if (cc < cols && r0 + rr < row_end) {
                const int64_t at = (r0 + rr) * m + c0 + sl * SLAB + cc;
                x = ld1<T, true>(Gs + at);
                if constexpr (EF == ARCTOPK_EF14 && ERR_IN) x = rnd<T>(x + ld1<T, true>(Es + at));
                else if constexpr (EF == ARCTOPK_EF21) x = rnd<T>(x - ld1<T, true>(Es + at));
                if constexpr (WRITE_E) st1<T, true>(Es + at, x);
            }
            xl[rr * (kRowUnits * LPU) + cc] = from_f<O>(x);
        }
    };

    // ---- V^T slab: V[c0 + sl SLAB + col][0..R) read in 16-B units (L2-resident), transposed into LDS.
    // fp32: item = (col, 4 ranks); bf16: item = (column pair, 8 ranks), the pair packed into one word;
    // OPB: item = (column pair, 4 fp32 ranks), each rank's pair rounded into one word
    u4_t va[VU], vb[sizeof(O) == 4 ? 1 : VU];
    auto issue_v = [&](int sl) {
        const int cols = slab_cols(sl);
        const T* vp = Vs + (int64_t)(c0 + sl * SLAB) * R;
#pragma unroll
        for (int i = 0; i < VU; ++i) {
            const int idx = tid + 256 * i;
            va[i] = u4_t{0u, 0u, 0u, 0u};
            if constexpr (sizeof(O) == 4) {
                const int col = idx / (R / 4), jq = idx % (R / 4);
                if (col < cols) va[i] = ld16raw<T, false>(vp, col * (R / 4) + jq);
            } else {
                const int cp = idx / (R / EPU), jg = idx % (R / EPU);
                vb[i] = u4_t{0u, 0u, 0u, 0u};
                if (2 * cp < cols) va[i] = ld16raw<T, false>(vp, 2 * cp * (R / EPU) + jg);
                if (2 * cp + 1 < cols) vb[i] = ld16raw<T, false>(vp, (2 * cp + 1) * (R / EPU) + jg);
            }
        }
    };
    auto stash_v = [&](int sl) {
        const int kuc = slab_ku(sl) * LPU;
        uint32_t* const vw = reinterpret_cast<uint32_t*>(vt);
#pragma unroll
        for (int i = 0; i < VU; ++i) {
            const int idx = tid + 256 * i;
            const uint32_t aw[4] = {va[i].x, va[i].y, va[i].z, va[i].w};
            if constexpr (sizeof(O) == 4) {
                const int col = idx / (R / 4), jq = idx % (R / 4);
                if (col < kuc) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) vw[(jq * 4 + q) * kRowWords + col] = aw[q];
                }
            } else {
                const int cp = idx / (R / EPU), jg = idx % (R / EPU);
                const uint32_t bw[4] = {vb[i].x, vb[i].y, vb[i].z, vb[i].w};
                if constexpr (OPB) {
                    if (2 * cp < kuc) {
#pragma unroll
                        for (int q = 0; q < 4; ++q)
                            vw[(jg * 4 + q) * kRowWords + cp] =
                                cvt_pk_bf16(__uint_as_float(aw[q]), __uint_as_float(bw[q]));
                    }
                } else if (2 * cp < kuc) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        vw[(jg * 8 + 2 * q) * kRowWords + cp] = (aw[q] & 0xFFFFu) | (bw[q] << 16);
                        vw[(jg * 8 + 2 * q + 1) * kRowWords + cp] = (aw[q] >> 16) | (bw[q] & 0xFFFF0000u);
                    }
                }
            }
        }
    };

    // ---- the walk: slabs outside, the block's row tiles inside (V^T staged once per slab)
    if (vec) issue_x(0, 0);
    for (int sl = 0; sl < nslab; ++sl) {
        issue_v(sl);
        const int ngroups = slab_ku(sl) / H;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            if (nt < nnt) {
                __syncthreads();  // the previous step's MFMAs have read their LDS operands
                if (nt == 0) stash_v(sl);
                if (vec) {
                    stash_x(sl, nt);
                    int ns = sl, nn = nt + 1;
                    if (nn == nnt) { nn = 0; ++ns; }
                    if (ns < nslab) issue_x(ns, nn);
                } else {
                    stash_x_scalar(sl, nt);
                }
                __syncthreads();
                for (int kg = wave; kg < ngroups; kg += 4) {
                    const int u = kg * H + lh;
                    mfma_unit<O, R>(acc[nt], vt[ln * kRowUnits + u], xt[ln * kRowUnits + u]);
                }
            }
        }
    }

    // ---- the waves' partial sums, added in wave order; C[j][n]: lane holds row n = lane % R and
    // ranks j = 8 (i / 4) + 4 h + i % 4 (r = 32) / 4 h + i (r = 16) in register i
    uint32_t* const kout = (keys && s.keyed) ? keys + s.row_off : nullptr;
    T* const sk_out = sketch + s.sketch_off;
    float* const pt_out = t.part < 0 ? nullptr : part_buf + s.part_off + (int64_t)t.part * s.n * R;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        if (nt < nnt) {
            __syncthreads();
#pragma unroll
            for (int i = 0; i < Acc<R>::N; ++i) {
                const int j = R == 32 ? 8 * (i / 4) + 4 * lh + (i % 4) : 4 * lh + i;
                red[(wave * TR + ln) * R + j] = acc[nt][i];
            }
            __syncthreads();
            const int64_t r0 = t.row0 + (int64_t)nt * TR;
            for (int idx = tid; idx < TR * R; idx += 256) {
                float v = red[idx];
#pragma unroll
                for (int w = 1; w < 4; ++w) v = __fadd_rn(v, red[w * TR * R + idx]);
                const int64_t row = r0 + idx / R;
                if (row >= row_end) continue;
                if (kout) red[idx] = v;
                else if (pt_out) pt_out[row * R + idx % R] = v;
                else st1<T>(sk_out + row * R + idx % R, v);
            }
            if (kout) {
                __syncthreads();
                if (tid < TR && r0 + tid < row_end) kout[r0 + tid] = row_key<T>(red + tid * R, R);
            }
        }
    }
}

template <typename K, typename... Args>
int launch(K k, int ntiles, size_t lds, hipStream_t st, hipEvent_t done, Args... args) {
    if (done) hipExtLaunchKernelGGL(k, dim3(ntiles), dim3(256), lds, st, nullptr, done, 0, args...);
    else hipLaunchKernelGGL(k, dim3(ntiles), dim3(256), lds, st, args...);
    return (int)hipGetLastError();
}

template <typename T, typename O, int R, int EF, bool ERR_IN>
int launch_k(const arctopk_plan* p, int tile0, int ntiles, const T* G, T* E, const T* V, T* sk, uint32_t* keys,
             hipStream_t st, hipEvent_t done) {
    constexpr size_t lds = 2 * (size_t)R * (kMfSlabBytes / (sizeof(T) / sizeof(O)) + 16);  // V^T and X rows of O
    if constexpr (lds > 48 * 1024) {  // (on every launch: the attribute is per device, the call is cheap)
        const hipError_t ok =
            hipFuncSetAttribute(reinterpret_cast<const void*>(&k_encode_mfma<T, O, R, EF, ERR_IN>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (ok != hipSuccess) return (int)ok;
    }
    return launch(&k_encode_mfma<T, O, R, EF, ERR_IN>, ntiles, lds, st, done, (const SegDev*)p->d_segs,
                  (const EncTile*)(p->d_enc + tile0), G, E, V, sk, p->d_part, keys);
}

template <typename T, typename O, int R>
int launch_r(const arctopk_plan* p, int tile0, int ntiles, const void* grad, void* err, int ef, int err_in,
             const void* V, void* sketch, uint32_t* keys, hipStream_t st, hipEvent_t done) {
    const T* G = static_cast<const T*>(grad);
    T* E = static_cast<T*>(err);
    const T* Vt = static_cast<const T*>(V);
    T* sk = static_cast<T*>(sketch);
    if (ef == ARCTOPK_EF_NONE) return launch_k<T, O, R, ARCTOPK_EF_NONE, false>(p, tile0, ntiles, G, E, Vt, sk, keys, st, done);
    if (ef == ARCTOPK_EF14 && err_in) return launch_k<T, O, R, ARCTOPK_EF14, true>(p, tile0, ntiles, G, E, Vt, sk, keys, st, done);
    if (ef == ARCTOPK_EF14) return launch_k<T, O, R, ARCTOPK_EF14, false>(p, tile0, ntiles, G, E, Vt, sk, keys, st, done);
    if (ef == ARCTOPK_EF21) return launch_k<T, O, R, ARCTOPK_EF21, true>(p, tile0, ntiles, G, E, Vt, sk, keys, st, done);
    return ARCTOPK_EINVAL;
}

}  // namespace

namespace arctopk {
int encode_mfma(const arctopk_plan* p, int tile0, int ntiles, const void* grad, void* err, int ef, int err_in,
                const void* V, void* sketch, uint32_t* keys, hipStream_t st, hipEvent_t done) {
    if (ntiles <= 0) return 0;
    const bool bf = p->dtype == ARCTOPK_BF16;
    const bool opb = !bf && p->sketch_op16;  // arctopk_plan_set_sketch_operands(ARCTOPK_BF16)
    if (p->r == 32)
        return bf    ? launch_r<bf16_t, bf16_t, 32>(p, tile0, ntiles, grad, err, ef, err_in, V, sketch, keys, st, done)
               : opb ? launch_r<float, bf16_t, 32>(p, tile0, ntiles, grad, err, ef, err_in, V, sketch, keys, st, done)
                     : launch_r<float, float, 32>(p, tile0, ntiles, grad, err, ef, err_in, V, sketch, keys, st, done);
    if (p->r == 16)
        return bf    ? launch_r<bf16_t, bf16_t, 16>(p, tile0, ntiles, grad, err, ef, err_in, V, sketch, keys, st, done)
               : opb ? launch_r<float, bf16_t, 16>(p, tile0, ntiles, grad, err, ef, err_in, V, sketch, keys, st, done)
                     : launch_r<float, float, 16>(p, tile0, ntiles, grad, err, ef, err_in, V, sketch, keys, st, done);
    return ARCTOPK_EINVAL;
}
}  // namespace arctopk
