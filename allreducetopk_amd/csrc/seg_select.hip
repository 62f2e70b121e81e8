// Segmented exact select for the row- and column-wise TopK / RandK hooks
// (sparse_type = "row" / "column"): every tensor [R, C] of a bucket is R row segments of C
// contiguous keys, or C column segments of R keys at element stride C, and each segment takes
// its own k_seg largest keys (TopK: |x|; RandK: rk_key(hseed(t, s), j)), ties at the threshold
// lowest position first.  Segments are uniform per tensor, so a tensor is one descriptor and the
// grids run over segments (mselect's per-item descriptors would cost a launch per 48 rows).
//
// Dispatch, per tensor (arctopk_seg_select):
//   row segments of <= kSegWaveLen keys     k_seg_rows<.., 256, true>: one wave per segment, four
//                                           segments per block (conv stems, short rows)
//   row segments of <= kSegMidLen keys      k_seg_rows<.., 256, false>: one 256-thread block each
//   row segments of <= kMSmallSel keys      k_seg_rows<.., 1024, false>: one 1,024-thread block each
//       (keys in LDS, four 8-bit radix rounds, ordered write: k_ms_small's rounds with the grid
//       striding over the segments of a tensor, at most kSegGridCap blocks per tensor)
//   longer row segments                     the multi-block ms_select, one item per segment in
//                                           batches of kMB, then k_seg_fix adds s * C to the
//                                           item-relative indices of segment s
//   column segments (C > 1), any length     k_seg_cols: a 1,024-thread block per strip of adjacent
//                                           columns (64, a lane each, from 16,384 columns on;
//                                           else 16, four lanes each, so that tall, narrow
//                                           tensors still fill the chip), per-column radix
//                                           histograms in LDS ([bin][column]); the keys are
//                                           re-read from memory in every round, so the strip
//                                           has no row limit and needs no fallback
//   a column tensor with C == 1 is one contiguous segment: it takes the row path.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "common.h"
#include "mselect.h"
#include "mselect_dev.h"

namespace {

using namespace arctopk;

constexpr int kSegBatch = 32;      // tensors per launch (kernel argument size)
constexpr int kSegWaveLen = 512;   // row segments up to this: one wave each
constexpr int kSegMidLen = 4096;   // ... up to this: one 256-thread block each (1,024 threads beyond)
constexpr int kSegGridCap = 2048;  // blocks per tensor of a row launch (grid-stride over segments)
#ifndef ARCTOPK_SEG_WIDE_STRIPS
#define ARCTOPK_SEG_WIDE_STRIPS 256  // column tensors of at least this many 64-column strips use them
#endif
constexpr int kStripWide = 64;     // columns of a wide strip (a lane per column)
constexpr int kStripNarrow = 16;   // ... of a narrow one (four lanes per column): tall, narrow tensors
                                   // then fill the chip with blocks
constexpr int kStripWaves = 16;    // waves of a strip block (each a contiguous range of rows)
constexpr int kStripBatch = 8;     // row accesses a wave keeps in flight
constexpr int strip_lds(int w) { return (256 * w + kStripWaves * 64) * 4; }  // histograms + wave partials

struct SegItem {
    int64_t off;    // element offset of the tensor in x
    int64_t koff;   // offset of the tensor's entries in idx / vals
    int32_t rows, cols;
    int32_t k;      // keys to take per segment
    int32_t t;      // the tensor's place in the bucket (hseed)
    int32_t nblk;   // row launches: blocks of this tensor
    int32_t iters;  // ... and segment groups each of them walks
};

struct SegBatch {
    SegItem it[kSegBatch];
    int32_t first[kSegBatch + 1];  // first block of each tensor; first[cnt] = blocks
    int32_t cnt;
};

// the key seed of segment s of tensor t: s = 0 is sparse_kernels.hip's rk_tensor_seed(seed, t)
__host__ __device__ inline uint32_t seg_hseed(uint64_t seed, int32_t t, int64_t s) {
    uint64_t z = seed + 0x9E3779B97F4A7C15ull * (uint64_t)(t + 1) + 0xD1B54A32D192ED03ull * (uint64_t)s;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (uint32_t)(z ^ (z >> 31));
}

__device__ __forceinline__ bool seg_locate(const SegBatch& b, int* t, int* r) {
    const int x = (int)blockIdx.x;
    if (x >= b.first[b.cnt]) return false;
    int lo = 0, hi = b.cnt - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (b.first[mid] <= x) lo = mid;
        else hi = mid - 1;
    }
    *t = lo;
    *r = x - b.first[lo];
    return true;
}

// bf16 |x| keys are the 16 value bits widened: their low 16 bits are zero, so the two low radix
// rounds would find digit 0 with every candidate in it and change nothing
template <int SRC> constexpr int kLastShift = SRC == 2 ? 16 : 0;

template <int SRC>
__device__ __forceinline__ void seg_store_zero(void* zero_x, int64_t i) {
    if constexpr (SRC == 1 || SRC == 3) static_cast<float*>(zero_x)[i] = 0.f;
    else static_cast<uint16_t*>(zero_x)[i] = (uint16_t)0;
}

// Row segments with their keys in LDS.  WAVESEG: each wave of the block owns a segment (its own
// slice of the key array and its own histogram); else the block owns one.  Every block of a
// tensor walks the same number of segment groups (it.iters), so the barriers stay uniform.
template <int SRC, int NT, bool WAVESEG>
__global__ void __launch_bounds__(NT) k_seg_rows(SegBatch b, uint64_t seed, const void* __restrict__ x,
                                                 int32_t* __restrict__ out_idx, void* __restrict__ out_val,
                                                 void* zero_x, int cap) {
    constexpr int NW = NT / 64, NG = WAVESEG ? NW : 1, GS = WAVESEG ? 64 : NT;
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    __shared__ uint32_t hist[NG][256];
    __shared__ uint32_t s_w[2][NW];
    __shared__ uint32_t s_digit[NG], s_acc[NG];
    int ti, bi;
    if (!seg_locate(b, &ti, &bi)) return;
    const SegItem it = b.it[ti];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = WAVESEG ? wave : 0, gt = WAVESEG ? lane : tid;
    const uint64_t lt = lane ? (~0ull >> (64 - lane)) : 0ull;
    uint32_t* skeys = smem + (size_t)g * cap;
    const int n = it.cols;
    for (int iter = 0; iter < it.iters; ++iter) {
        const int64_t s = ((int64_t)iter * it.nblk + bi) * NG + g;
        const bool act = s < it.rows;
        const int64_t base = it.off + s * n;
        const uint32_t hs = SRC >= 3 ? seg_hseed(seed, it.t, s) : 0u;
        if (act) {
            for (int i = gt; i < n; i += GS) {
                if constexpr (SRC >= 3) skeys[i] = rk_key(hs, i);
                else skeys[i] = key_of<SRC>(load_bits<SRC>(nullptr, x, base + i));
            }
        }
        __syncthreads();
        uint32_t prefix = 0u, mask = 0u;
        int64_t kk = it.k;
        for (int shift = 24; shift >= kLastShift<SRC>; shift -= 8) {
            for (int j = gt; j < 256; j += GS) hist[g][j] = 0u;
            __syncthreads();
            if (act) {
                for (int i = gt; i < n; i += GS) {
                    const uint32_t k = skeys[i];
                    if ((k & mask) == prefix) atomicAdd(&hist[g][(k >> shift) & 255u], 1u);
                }
            }
            __syncthreads();
            if (WAVESEG || tid < 64) {  // lane l: bins 255 - 4l .. 252 - 4l, scanned from the top
                uint32_t c[4], tot = 0u;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    c[q] = hist[g][255 - (4 * lane + q)];
                    tot += c[q];
                }
                uint32_t incl = tot;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const uint32_t y = __shfl_up(incl, o, 64);
                    if (lane >= o) incl += y;
                }
                const uint64_t excl = incl - tot;
                if (excl < (uint64_t)kk && excl + tot >= (uint64_t)kk) {
                    uint64_t acc = excl;
                    int q = 0;
                    for (; q < 3; ++q) {
                        if (acc + c[q] >= (uint64_t)kk) break;
                        acc += c[q];
                    }
                    s_digit[g] = (uint32_t)(255 - (4 * lane + q));
                    s_acc[g] = (uint32_t)acc;
                }
            }
            __syncthreads();
            prefix |= s_digit[g] << shift;
            mask |= 255u << shift;
            kk -= (int64_t)s_acc[g];
            __syncthreads();  // s_digit / s_acc / hist are rewritten by the next round
        }
        const uint32_t T = prefix;
        const uint32_t take_eq = (uint32_t)kk;  // threshold-equal keys to take, lowest position first
        uint32_t run = 0u, eq_run = 0u;
        for (int c0 = 0; c0 < n; c0 += GS) {
            const int i = c0 + gt;
            const bool valid = act && i < n;
            const uint32_t key = valid ? skeys[i] : 0u;
            const bool gtT = valid && key > T, eq = valid && key == T;
            const uint64_t beq = __ballot(eq);
            uint32_t eq_before = popc64(beq & lt), eq_tot = popc64(beq);
            if constexpr (!WAVESEG) {
                if (lane == 0) s_w[0][wave] = eq_tot;
                __syncthreads();
                eq_tot = 0u;
#pragma unroll
                for (int w = 0; w < NW; ++w) {
                    eq_before += w < wave ? s_w[0][w] : 0u;
                    eq_tot += s_w[0][w];
                }
            }
            const bool sel = gtT || (eq && eq_run + eq_before < take_eq);
            const uint64_t bsel = __ballot(sel);
            uint32_t sel_before = popc64(bsel & lt), sel_tot = popc64(bsel);
            if constexpr (!WAVESEG) {
                if (lane == 0) s_w[1][wave] = sel_tot;
                __syncthreads();
                sel_tot = 0u;
#pragma unroll
                for (int w = 0; w < NW; ++w) {
                    sel_before += w < wave ? s_w[1][w] : 0u;
                    sel_tot += s_w[1][w];
                }
            }
            const uint32_t pos = run + sel_before;
            if (sel && pos < (uint32_t)it.k) {  // bound: never past the segment's k entries
                const int64_t o = it.koff + s * it.k + pos;
                out_idx[o] = (int32_t)(s * n + i);
                if (x) {
                    if (out_val) store_val<SRC>(out_val, o, load_bits<SRC>(nullptr, x, base + i));
                    if (zero_x) seg_store_zero<SRC>(zero_x, base + i);
                }
            }
            run += sel_tot;
            eq_run += eq_tot;
            if constexpr (!WAVESEG) __syncthreads();  // s_w is rewritten by the next chunk
        }
        __syncthreads();  // skeys are rewritten by the next segment group
    }
}

// Column segments: block = strip of W adjacent columns.  A wave covers 64 / W consecutive rows of
// the strip per access (lane = sub * W + column: W = 64 is one coalesced 256-B row per access,
// W = 16 four 64-B row pieces), wave w owns rows [w * rpw, (w + 1) * rpw) and keeps kStripBatch
// accesses in flight.  Four 8-bit rounds re-read the strip into per-column histograms
// hist[bin][column] (lanes of different columns never share a word); the digit of each column is
// found by every wave for its own lanes from per-wave partial sums of 16 bins.  Ordered write:
// per-lane counts of keys above / at the threshold, prefixed over the waves (and the lanes of a
// column), then each wave walks its rows in order with the column's running counts replicated in
// the lanes of that column and advanced by ballots.  Entry j of column c goes to
// koff + j * C + c (the reference's [k_seg, C] layout).
template <int SRC, int W>
__global__ void __launch_bounds__(kStripWaves * 64) k_seg_cols(SegBatch b, uint64_t seed, const void* __restrict__ x,
                                                               int32_t* __restrict__ out_idx,
                                                               void* __restrict__ out_val, void* zero_x) {
    constexpr int NW = kStripWaves, BPW = 256 / NW, NT = NW * 64, SUB = 64 / W, U = kStripBatch;
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    uint32_t* hist = smem;             // [256][W]
    uint32_t* s_part = smem + 256 * W;  // [NW][64]
    int ti, bi;
    if (!seg_locate(b, &ti, &bi)) return;
    const SegItem it = b.it[ti];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & (W - 1), sub = lane / W;
    const int R = it.rows, C = it.cols;
    const int c = bi * W + col;
    const bool cact = c < C;
    const int rpw = (R + NW - 1) / NW;
    const int r0 = min(R, wave * rpw), r1 = min(R, r0 + rpw);
    const uint32_t hs = SRC >= 3 ? seg_hseed(seed, it.t, c) : 0u;
    const int64_t cbase = it.off + c;
    uint64_t colmask = 0ull;  // the lanes of this lane's column
#pragma unroll
    for (int j = 0; j < SUB; ++j) colmask |= 1ull << (col + W * j);
    const uint64_t lt = colmask & (lane ? (~0ull >> (64 - lane)) : 0ull);
    auto key_at = [&](int r) -> uint32_t {
        if constexpr (SRC >= 3) return rk_key(hs, r);
        else return key_of<SRC>(load_bits<SRC>(nullptr, x, cbase + (int64_t)r * C));
    };
    uint32_t prefix = 0u, mask = 0u, kk = (uint32_t)it.k;
    for (int shift = 24; shift >= kLastShift<SRC>; shift -= 8) {
        for (int j = tid; j < 256 * W; j += NT) hist[j] = 0u;
        __syncthreads();
        for (int base = r0 + sub; base < r1; base += SUB * U) {
            uint32_t kv[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int r = base + u * SUB;
                kv[u] = cact && r < r1 ? key_at(r) : 0u;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (cact && base + u * SUB < r1 && (kv[u] & mask) == prefix)
                    atomicAdd(&hist[((kv[u] >> shift) & 255u) * W + col], 1u);
            }
        }
        __syncthreads();
        uint32_t part = 0u;  // wave w: bins 255 - w * BPW downwards
#pragma unroll
        for (int q = 0; q < BPW; ++q) part += hist[(255 - wave * BPW - q) * W + col];
        s_part[wave * 64 + lane] = part;
        __syncthreads();
        uint32_t acc = 0u;
        int ow = 0;
        bool found = false;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const uint32_t p = s_part[w * 64 + lane];
            const bool hit = !found && acc + p >= kk;
            if (hit) ow = w;
            found = found || hit;
            if (!found) acc += p;
        }
        uint32_t digit = 0u;
        found = false;
#pragma unroll
        for (int q = 0; q < BPW; ++q) {
            const int bin = 255 - ow * BPW - q;
            const uint32_t cnt = hist[bin * W + col];
            const bool hit = !found && acc + cnt >= kk;
            if (hit) digit = (uint32_t)bin;
            found = found || hit;
            if (!found) acc += cnt;
        }
        prefix |= digit << shift;
        mask |= 255u << shift;
        kk -= cact ? acc : 0u;
        __syncthreads();  // hist / s_part are rewritten by the next round
    }
    const uint32_t T = prefix, take_eq = kk;
    uint32_t* s_cgt = smem;  // [NW][64] each (the histograms are done)
    uint32_t* s_ceq = smem + NW * 64;
    uint32_t cgt = 0u, ceq = 0u;
    for (int base = r0 + sub; base < r1; base += SUB * U) {
        uint32_t kv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int r = base + u * SUB;
            kv[u] = cact && r < r1 ? key_at(r) : 0u;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool valid = cact && base + u * SUB < r1;
            cgt += valid && kv[u] > T ? 1u : 0u;
            ceq += valid && kv[u] == T ? 1u : 0u;
        }
    }
    s_cgt[wave * 64 + lane] = cgt;
    s_ceq[wave * 64 + lane] = ceq;
    __syncthreads();
    uint32_t gtb = 0u, eqb = 0u;  // the column's keys in the waves before this one
    for (int w = 0; w < wave; ++w) {
#pragma unroll
        for (int j = 0; j < SUB; ++j) {
            gtb += s_cgt[w * 64 + col + W * j];
            eqb += s_ceq[w * 64 + col + W * j];
        }
    }
    uint32_t eq_run = eqb, sel_run = gtb + min(eqb, take_eq);
    for (int base = r0; base < r1; base += SUB * U) {  // (wave-uniform: the ballots see every lane)
        uint32_t bv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int r = base + u * SUB + sub;
            if constexpr (SRC >= 3) bv[u] = 0u;
            else bv[u] = cact && r < r1 ? load_bits<SRC>(nullptr, x, cbase + (int64_t)r * C) : 0u;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int r = base + u * SUB + sub;
            const bool valid = cact && r < r1;
            const uint32_t k = SRC >= 3 ? rk_key(hs, r) : key_of<SRC>(bv[u]);
            const bool eq = valid && k == T;
            const uint64_t beq = __ballot(eq);
            const bool sel = valid && (k > T || (eq && eq_run + popc64(beq & lt) < take_eq));
            const uint64_t bsel = __ballot(sel);
            const uint32_t pos = sel_run + popc64(bsel & lt);
            if (sel && pos < (uint32_t)it.k) {  // bound: never past the column's k entries
                const int64_t gi = cbase + (int64_t)r * C;
                const int64_t o = it.koff + (int64_t)pos * C + c;
                out_idx[o] = (int32_t)((int64_t)r * C + c);
                if (x) {
                    if (out_val) store_val<SRC>(out_val, o, SRC >= 3 ? load_bits<SRC>(nullptr, x, gi) : bv[u]);
                    if (zero_x) seg_store_zero<SRC>(zero_x, gi);
                }
            }
            eq_run += popc64(beq & colmask);
            sel_run += popc64(bsel & colmask);
        }
    }
}

// ms_select writes indices relative to its item: segment s of a row tensor adds s * C
__global__ void __launch_bounds__(256) k_seg_fix(int32_t* __restrict__ idx, int64_t koff, int32_t k, int64_t nseg,
                                                 int32_t cols) {
    const int64_t tot = nseg * k;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x + k; e < tot; e += (int64_t)gridDim.x * 256)
        idx[koff + e] += (int32_t)((e / k) * cols);
}

struct SegGeom {  // one tensor as the kernels see it
    int64_t nseg, len;
    bool strip;   // column strips; else contiguous row segments
};

SegGeom seg_geom(int64_t rows, int64_t cols, bool by_column) {
    if (by_column && cols > 1) return {cols, rows, true};
    if (by_column) return {1, rows, false};  // one column: a contiguous segment
    return {rows, cols, false};
}

bool seg_valid(int32_t nt, const int64_t* rows, const int64_t* cols, const int64_t* k_seg, bool by_column) {
    if (nt < 1 || !rows || !cols || !k_seg) return false;
    for (int32_t j = 0; j < nt; ++j) {
        if (rows[j] < 1 || cols[j] < 1 || rows[j] >= (1ll << 31) || cols[j] >= (1ll << 31)) return false;
        if (rows[j] * cols[j] >= (1ll << 31)) return false;
        const SegGeom g = seg_geom(rows[j], cols[j], by_column);
        if (k_seg[j] < 1 || k_seg[j] > g.len) return false;
    }
    return true;
}

// candidate slots ms_select needs for the long row segments (> kMSmallSel keys): the largest
// per-batch sum, batches of kMB segments in (tensor, segment) order
int64_t seg_cap_total(int32_t nt, const int64_t* rows, const int64_t* cols, bool by_column) {
    int64_t best = 0, cap = 0;
    int inb = 0;
    for (int32_t j = 0; j < nt; ++j) {
        const SegGeom g = seg_geom(rows[j], cols[j], by_column);
        if (g.strip || g.len <= kMSmallSel) continue;
        MItem it{};
        it.n = g.len;
        ms_item_geometry(it);
        for (int64_t s = 0; s < g.nseg; ++s) {
            if (inb == kMB) {
                inb = 0;
                cap = 0;
            }
            cap += it.cand_cap;
            ++inb;
            best = std::max(best, cap);
        }
    }
    return best;
}

template <int SRC>
int launch_rows(const SegBatch& b, int cls, int maxlen, uint64_t seed, const void* x, int32_t* idx, void* vals,
                void* zero_x, hipStream_t st) {
    const dim3 grid(b.first[b.cnt]);
    if (cls == 0)
        hipLaunchKernelGGL((k_seg_rows<SRC, 256, true>), grid, dim3(256), (size_t)maxlen * 16, st, b, seed, x, idx,
                           vals, zero_x, maxlen);
    else if (cls == 1)
        hipLaunchKernelGGL((k_seg_rows<SRC, 256, false>), grid, dim3(256), (size_t)maxlen * 4, st, b, seed, x, idx,
                           vals, zero_x, maxlen);
    else
        hipLaunchKernelGGL((k_seg_rows<SRC, 1024, false>), grid, dim3(1024), (size_t)maxlen * 4, st, b, seed, x, idx,
                           vals, zero_x, maxlen);
    return (int)hipGetLastError();
}

template <int SRC>
int launch_cols(const SegBatch& b, bool wide, uint64_t seed, const void* x, int32_t* idx, void* vals, void* zero_x,
                hipStream_t st) {
    if (!wide) {
        hipLaunchKernelGGL((k_seg_cols<SRC, kStripNarrow>), dim3(b.first[b.cnt]), dim3(kStripWaves * 64),
                           strip_lds(kStripNarrow), st, b, seed, x, idx, vals, zero_x);
        return (int)hipGetLastError();
    }
    // 68 KiB of dynamic LDS: above the 64 KiB a kernel gets without the attribute
    static const hipError_t ok = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_seg_cols<SRC, kStripWide>),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize,
                                                     strip_lds(kStripWide));
    if (ok != hipSuccess) return (int)ok;
    hipLaunchKernelGGL((k_seg_cols<SRC, kStripWide>), dim3(b.first[b.cnt]), dim3(kStripWaves * 64),
                       strip_lds(kStripWide), st, b, seed, x, idx, vals, zero_x);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" int64_t arctopk_seg_workspace_bytes(int32_t nt, const int64_t* rows, const int64_t* cols,
                                               const int64_t* k_seg, int32_t by_column) {
    if (!seg_valid(nt, rows, cols, k_seg, by_column != 0)) return -(int64_t)ARCTOPK_EINVAL;
    const int64_t cap = seg_cap_total(nt, rows, cols, by_column != 0);
    return cap ? ms_workspace_bytes(cap) : 256;
}

extern "C" int arctopk_seg_select(void* x, int32_t nt, const int64_t* offsets, const int64_t* rows,
                                  const int64_t* cols, const int64_t* k_seg, const int64_t* k_off,
                                  int32_t by_column, int32_t hashed, uint64_t seed, int32_t* idx, void* vals,
                                  void* workspace, int32_t dtype, int32_t zero_selected, void* stream) {
    if (!k_off || !idx || !workspace) return ARCTOPK_EINVAL;
    if (x ? (!offsets || !vals) : (!hashed || vals != nullptr || zero_selected)) return ARCTOPK_EINVAL;
    if (dtype != ARCTOPK_F32 && dtype != ARCTOPK_BF16) return ARCTOPK_EINVAL;
    const bool bycol = by_column != 0;
    if (!seg_valid(nt, rows, cols, k_seg, bycol)) return ARCTOPK_EINVAL;
    for (int32_t j = 0; j < nt; ++j)
        if (k_off[j] < 0 || (x && offsets[j] < 0)) return ARCTOPK_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const bool bf16 = dtype == ARCTOPK_BF16;
    void* zero_x = zero_selected ? x : nullptr;
    const int src = hashed ? (bf16 ? 4 : 3) : (bf16 ? 2 : 1);

    // classes 0..2: row kernels by segment length; 3 / 4: narrow / wide column strips; long rows go
    // to ms_select
    std::vector<int32_t> cls[5], longs;
    for (int32_t j = 0; j < nt; ++j) {
        const SegGeom g = seg_geom(rows[j], cols[j], bycol);
        if (g.strip) cls[g.nseg >= (int64_t)ARCTOPK_SEG_WIDE_STRIPS * kStripWide ? 4 : 3].push_back(j);
        else if (g.len <= kSegWaveLen) cls[0].push_back(j);
        else if (g.len <= kSegMidLen) cls[1].push_back(j);
        else if (g.len <= kMSmallSel) cls[2].push_back(j);
        else longs.push_back(j);
    }
    for (int c = 0; c < 5; ++c) {
        for (size_t a = 0; a < cls[c].size(); a += kSegBatch) {
            SegBatch b{};
            b.cnt = (int32_t)std::min(cls[c].size() - a, (size_t)kSegBatch);
            int maxlen = 1;
            for (int i = 0; i < b.cnt; ++i) {
                const int32_t j = cls[c][a + i];
                const SegGeom g = seg_geom(rows[j], cols[j], bycol);
                SegItem& it = b.it[i];
                it.off = x ? offsets[j] : 0;
                it.koff = k_off[j];
                it.rows = (int32_t)(g.strip ? rows[j] : g.nseg);
                it.cols = (int32_t)(g.strip ? cols[j] : g.len);
                it.k = (int32_t)k_seg[j];
                it.t = j;
                if (g.strip) {
                    const int w = c == 4 ? kStripWide : kStripNarrow;
                    it.nblk = (int32_t)((g.nseg + w - 1) / w);
                    it.iters = 1;
                } else {
                    const int64_t per = c == 0 ? 4 : 1;  // segments per block
                    const int64_t groups = (g.nseg + per - 1) / per;
                    it.nblk = (int32_t)std::min<int64_t>(groups, kSegGridCap);
                    it.iters = (int32_t)((groups + it.nblk - 1) / it.nblk);
                }
                b.first[i] = i ? b.first[i - 1] + b.it[i - 1].nblk : 0;
                maxlen = std::max(maxlen, (int)it.cols);
            }
            b.first[b.cnt] = b.first[b.cnt - 1] + b.it[b.cnt - 1].nblk;
            int e;
#define SEG_LAUNCH(S) (c >= 3 ? launch_cols<S>(b, c == 4, seed, x, idx, vals, zero_x, st) \
                              : launch_rows<S>(b, c, maxlen, seed, x, idx, vals, zero_x, st))
            if (src == 1) e = SEG_LAUNCH(1);
            else if (src == 2) e = SEG_LAUNCH(2);
            else if (src == 3) e = SEG_LAUNCH(3);
            else e = SEG_LAUNCH(4);
#undef SEG_LAUNCH
            if (e) return e;
        }
    }
    if (longs.empty()) return 0;

    const int64_t cap_total = seg_cap_total(nt, rows, cols, bycol);
    MWorkspace* ws = static_cast<MWorkspace*>(workspace);
    MBatch mb;
    mb.cnt = 0;
    int64_t cap = 0, maxn = 0;
    auto flush = [&]() -> int {
        if (mb.cnt == 0) return 0;
        const int e = ms_select(mb, maxn, nullptr, x, bf16, false, ws, cap_total, idx, vals, nullptr, zero_x, st,
                                hashed != 0, 0, nullptr);
        mb.cnt = 0;
        cap = 0;
        maxn = 0;
        return e;
    };
    for (int32_t j : longs) {
        const SegGeom g = seg_geom(rows[j], cols[j], bycol);
        for (int64_t s = 0; s < g.nseg; ++s) {
            if (mb.cnt == kMB)
                if (int e = flush()) return e;
            MItem& it = mb.it[mb.cnt++];
            it = MItem{};
            it.key_off = x ? offsets[j] + s * g.len : 0;
            it.n = g.len;
            it.k = k_seg[j];
            it.out_off = k_off[j] + s * k_seg[j];
            ms_item_geometry(it);
            it.hseed = hashed ? seg_hseed(seed, j, s) : 0u;
            it.cand_off = cap;
            cap += it.cand_cap;
            maxn = std::max(maxn, g.len);
        }
    }
    if (int e = flush()) return e;
    for (int32_t j : longs) {
        const SegGeom g = seg_geom(rows[j], cols[j], bycol);
        if (g.nseg < 2) continue;
        const int64_t tot = g.nseg * k_seg[j];
        const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(2048, (tot + 255) / 256));
        hipLaunchKernelGGL(k_seg_fix, dim3(grid), dim3(256), 0, st, idx, k_off[j], (int32_t)k_seg[j], g.nseg,
                           (int32_t)g.len);
    }
    return (int)hipGetLastError();
}
