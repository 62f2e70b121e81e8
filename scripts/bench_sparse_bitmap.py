#!/usr/bin/env python3
"""TopK with its indices as a per-tensor bitmap on the wire (SparseState.index_wire = "bitmap", DESIGN.md
section 4j) on one GPU, against the int32-index kernels and the idx16 ones, in one process, interleaved,
on the same indices -- the method and the helpers of scripts/bench_sparse_idx16.py and
scripts/bench_sparse_wire16.py, at ratio 0.2 and at 0.05 (below the formats' crossover).

    bytes    the index bytes of one rank's payload, int32 / idx16 / bitmap, at ratios 0.01, 0.08, 0.2
    pack     arctopk_sparse_idx16_pack against arctopk_sparse_bitmap_pack
    decode   arctopk_sparse_decode (fp32 values, accumulate 1) or arctopk_sparse_decode_wire16 (bf16 values),
             arctopk_sparse_decode_idx16 and arctopk_sparse_decode_bitmap on the same payloads, at
             nranks = world size 1, 2, 4 and 8, without gE and with it (EF21)
    unpack   a bf16 bucket: arctopk_sparse_decode (bf16) alone against arctopk_sparse_bitmap_unpack + it
    hook     sparse_hook_sync (world size 1), TopK, EF14 and EF21, fp32 buckets: index_wire None / idx16 / bitmap

    python scripts/bench_sparse_bitmap.py
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_sparse_wire16 as B16  # noqa: E402  (RATIO lives there: Layout reads it)
from bench_sparse_idx16 import Idx16Layout  # noqa: E402
from bench_sparse_wire16 import DEV, MAX_RANKS, REPO, SETS, ab, cell, loads  # noqa: E402

from allreducetopk_amd import _native as N  # noqa: E402
from allreducetopk_amd.bucket import SyntheticBucket, bucket_numel  # noqa: E402
from allreducetopk_amd.comm_hooks import sparse_hook as SH  # noqa: E402

FMT = "%-20s %-13s %-5s | %-24s | %-24s | %-24s | %s"


class BitmapLayout(Idx16Layout):
    """bench_sparse_idx16's buffers, plus every rank's indices as a bitmap."""

    def __init__(self, shapes, gen, sid):
        super().__init__(shapes, gen, sid)
        L = N.lib()
        self.bm_bytes = int(L.arctopk_sparse_bitmap_bytes(*self.lay))
        self.bm = torch.empty(MAX_RANKS * self.bm_bytes, dtype=torch.uint8, device=DEV)
        for r in range(MAX_RANKS):
            N.check(L.arctopk_sparse_bitmap_pack(*self.lay, self.idx[r * self.sum_k:].data_ptr(),
                                                 self.bm[r * self.bm_bytes:].data_ptr(), sid), "arctopk_sparse_bitmap_pack")
        self.scratch_bm = torch.empty(self.bm_bytes, dtype=torch.uint8, device=DEV)
        torch.cuda.synchronize()


def emit(lines, what, name, ratio, t):
    """One row: the median (min..max) of each path, and idx16 / today, bitmap / today, bitmap / idx16."""
    med = {k: statistics.median(v) for k, v in t.items()}
    rel = ["%.2f" % (med[p] / med[q]) if p in med and q in med else "-" for p, q in (("b", "a"), ("c", "a"), ("c", "b"))]
    lines.append(FMT % (what, name, ratio, *[cell(t[k]) if k in t else "-" for k in "abc"], " ".join(rel)))
    print(lines[-1], flush=True)


def byte_rows(name, buckets, lines):
    L = N.lib()
    for ratio in (0.01, 0.08, 0.2):
        size = {"a": 0, "b": 0, "c": 0}
        for shapes in buckets:
            numels = [bucket_numel([s]) for s in shapes]
            ks = [max(1, int(m * ratio)) for m in numels]
            a = [N.i64_array([sum(v[:i]) for i in range(len(v))]) for v in (numels, ks)]
            lay = (sum(numels), len(numels), a[0], N.i64_array(ks), a[1])
            size["a"] += 4 * sum(ks)
            size["b"] += int(L.arctopk_sparse_idx16_bytes(*lay))
            size["c"] += int(L.arctopk_sparse_bitmap_bytes(*lay))
        lines.append(FMT % ("index bytes", name, ratio, size["a"], size["b"], size["c"],
                            "%.3f %.3f %.3f" % (size["b"] / size["a"], size["c"] / size["a"], size["c"] / size["b"])))
        print(lines[-1], flush=True)


def kernel_rows(name, buckets, ratio, args, gen, sid, lines):
    L = N.lib()
    lay = [BitmapLayout(shapes, gen, sid) for shapes in buckets]

    def each(fn):
        return lambda i: [fn(x, i % SETS) for x in lay]

    def pack(fmt):  # the indices rotate with the rank: every call reads other memory
        entry = getattr(L, "arctopk_sparse_%s_pack" % fmt)
        return lambda x, s: N.check(entry(*x.lay, x.idx[(s % MAX_RANKS) * x.sum_k:].data_ptr(),
                                          (x.scratch_wire if fmt == "idx16" else x.scratch_bm).data_ptr(), sid), fmt)

    def ge_ptr(x, s, ge):
        return x.gE[s].data_ptr() if ge else None

    def today(nr, ge, dt):
        if dt == N.F32:
            return lambda x, s: N.check(L.arctopk_sparse_decode(
                x.out[s].data_ptr(), *x.lay, x.sum_k, x.idx.data_ptr(), x.vals32.data_ptr(), nr, nr, 1, ge_ptr(x, s, ge),
                1.0, N.F32, sid), "arctopk_sparse_decode")
        return lambda x, s: N.check(L.arctopk_sparse_decode_wire16(
            x.out[s].data_ptr(), *x.lay, x.sum_k, x.idx.data_ptr(), x.vals16.data_ptr(), nr, nr, 1, ge_ptr(x, s, ge), 1.0,
            sid), "arctopk_sparse_decode_wire16")

    def compact(fmt, nr, ge, dt):
        entry = getattr(L, "arctopk_sparse_decode_%s" % fmt)
        return lambda x, s: N.check(entry(
            x.out[s].data_ptr(), *x.lay, x.sum_k, *((x.wire.data_ptr(), x.bytes) if fmt == "idx16" else
                                                    (x.bm.data_ptr(), x.bm_bytes)),
            (x.vals32 if dt == N.F32 else x.vals16).data_ptr(), dt, nr, nr, ge_ptr(x, s, ge), 1.0, sid), fmt)

    def dec_bf16(nr, unpack):
        def fn(x, s):
            idx = x.idx
            if unpack:
                N.check(L.arctopk_sparse_bitmap_unpack(*x.lay, x.sum_k, x.bm.data_ptr(), x.bm_bytes, nr,
                                                       x.unpacked.data_ptr(), sid), "arctopk_sparse_bitmap_unpack")
                idx = x.unpacked
            N.check(L.arctopk_sparse_decode(x.out16[s].data_ptr(), *x.lay, x.sum_k, idx.data_ptr(), x.vals16.data_ptr(), nr,
                                            nr, 1, None, 1.0, N.BF16, sid), "arctopk_sparse_decode")
        return fn

    emit(lines, "pack", name, ratio, ab({"b": each(pack("idx16")), "c": each(pack("bitmap"))}, args))
    if args.pack_only:
        return
    for vals, dt in (("fp32", N.F32), ("bf16", N.BF16)):
        for ge in (False, True):
            for nr in (1, 2, 4, 8):
                emit(lines, "decode %s%s nr=%d" % (vals, " ef21" if ge else "", nr), name, ratio,
                     ab({"a": each(today(nr, ge, dt)), "b": each(compact("idx16", nr, ge, dt)),
                         "c": each(compact("bitmap", nr, ge, dt))}, args))
    for nr in (1, 2, 4, 8):
        emit(lines, "unpack+bf16 nr=%d" % nr, name, ratio,
             ab({"a": each(dec_bf16(nr, False)), "c": each(dec_bf16(nr, True))}, args))


def hook_rows(name, buckets, ratio, args, gen, lines):
    nb = len(buckets)
    for ef in ("ef14", "ef21"):
        states, bks = {}, {}
        for k, wire in (("a", None), ("b", "idx16"), ("c", "bitmap")):
            st = states[k] = SH.SparseState(None, compress_ratio=ratio, start_compress_iter=0, sparse_type="tensor",
                                            use_error_feedback=ef)
            st.index_wire = wire
            bks[k] = [[SyntheticBucket(torch.randn(bucket_numel(s), device=DEV, generator=gen), s,
                                       index=q * nb + j, is_last=(j == nb - 1)) for j, s in enumerate(buckets)]
                      for q in range(SETS)]

        def step(k):
            def fn(i, st=states[k], sets=bks[k]):
                for bk in sets[i % SETS]:
                    SH.sparse_hook_sync(st, bk).wait()
            return fn
        for k in states:  # EF21's dense first call of every bucket is not a compressed one
            for i in range(SETS):
                step(k)(i)
        emit(lines, "hook topk %s" % ef, name, ratio, ab({k: step(k) for k in states}, args))
        assert states["c"].bitmap_calls > 0 and states["b"].bitmap_calls == 0 and states["a"].idx16_calls == 0
        del states, bks
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--loads", default="headline,resnet50_ddp")
    ap.add_argument("--ratios", default="0.2,0.05")
    ap.add_argument("--no-hook", action="store_true")
    ap.add_argument("--pack-only", action="store_true", help="of the kernel rows, the pack row alone (span variants)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sparse_bitmap", "table.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sparse_bitmap.py needs a GPU")
    from parity import ensure_group
    ensure_group("nccl")
    gen = torch.Generator(device=DEV).manual_seed(1000)
    sid = torch.cuda.current_stream().cuda_stream
    lines = ["# library: %s; us per call: median (min..max) of %d repetitions' medians of %d calls after %d warm-ups, "
             "the paths alternating; %d disjoint sets of buffers in rotation; fp32 buckets unless the row says bf16; one "
             "draw of ascending indices per rank, the same on every path; last column: idx16 / int32, bitmap / int32, "
             "bitmap / idx16" % (N.lib().arctopk_version().decode(), args.repeats, args.calls, args.warmup, SETS),
             FMT % ("what", "workload", "ratio", "int32 indices (today)", "idx16", "bitmap", "ratios")]
    all_loads = loads()
    names = [w for w in args.loads.split(",") if w]
    for name in names:
        byte_rows(name, all_loads[name], lines)
    for ratio in [float(r) for r in args.ratios.split(",")]:
        B16.RATIO = ratio
        for name in names:
            kernel_rows(name, all_loads[name], ratio, args, gen, sid, lines)
            torch.cuda.empty_cache()
            if not args.no_hook:
                hook_rows(name, all_loads[name], ratio, args, gen, lines)
    lines.append("# index bytes: one rank's payload, every bucket of the workload, the formats' padding included; decode "
                 "fp32 rows: today is arctopk_sparse_decode (fp32, accumulate 1); decode bf16 rows: today is "
                 "arctopk_sparse_decode_wire16's merged route; unpack+bf16 rows: a bf16 bucket, arctopk_sparse_decode alone "
                 "against arctopk_sparse_bitmap_unpack followed by it; hook rows: sparse_hook_sync at world size 1, TopK, a "
                 "call is every bucket of the workload")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
