#!/usr/bin/env python3
"""TopK with its indices as 16-bit block offsets on the wire (SparseState.index_wire = "idx16",
DESIGN.md section 4i) on one GPU, against the int32-index kernels it is an option beside, in one
process, interleaved, on the same indices -- the method and the helpers of
scripts/bench_sparse_wire16.py (cold buffers in rotation, device-scope timed events, medians of
--calls calls after --warmup, --repeats repetitions with the paths alternating).

    bytes    the index bytes of one rank's payload, int32 against the format, at ratios 0.01, 0.08, 0.2
    pack     arctopk_sparse_idx16_pack alone (today has no counterpart: the int32 indices travel)
    decode   arctopk_sparse_decode (fp32 values, accumulate 1) and arctopk_sparse_decode_wire16 (bf16
             values, merged route) against arctopk_sparse_decode_idx16 on the same payloads, at
             nranks = world size 1, 2, 4 and 8, without gE and with it (EF21)
    unpack   a bf16 bucket: arctopk_sparse_decode (bf16) alone against arctopk_sparse_idx16_unpack + it
    hook     sparse_hook_sync (world size 1), TopK, EF14 and EF21, fp32 buckets, the option off and on

    python scripts/bench_sparse_idx16.py
"""
import argparse
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from allreducetopk_amd import _native as N  # noqa: E402
from allreducetopk_amd.bucket import SyntheticBucket, bucket_numel  # noqa: E402
from allreducetopk_amd.comm_hooks import sparse_hook as SH  # noqa: E402
from bench_sparse_wire16 import DEV, MAX_RANKS, RATIO, SETS, Layout, ab, cell, loads  # noqa: E402

BF16 = torch.bfloat16
FMT = "%-18s %-13s | %-26s | %-26s | %s"


class Idx16Layout(Layout):
    """bench_sparse_wire16's buffers, plus every rank's indices in the format and a bf16 bucket."""

    def __init__(self, shapes, gen, sid):
        super().__init__(shapes, gen, sid)
        L = N.lib()
        self.lay = (self.n, self.nt, self.a_off, self.a_k, self.a_ko)
        self.bytes = int(L.arctopk_sparse_idx16_bytes(*self.lay))
        self.wire = torch.empty(MAX_RANKS * self.bytes, dtype=torch.uint8, device=DEV)
        for r in range(MAX_RANKS):
            N.check(L.arctopk_sparse_idx16_pack(*self.lay, self.idx[r * self.sum_k:].data_ptr(),
                                                self.wire[r * self.bytes:].data_ptr(), sid), "arctopk_sparse_idx16_pack")
        self.scratch_wire = torch.empty(self.bytes, dtype=torch.uint8, device=DEV)
        self.unpacked = torch.empty(MAX_RANKS * self.sum_k, dtype=torch.int32, device=DEV)
        self.out16 = [torch.empty(self.n, dtype=BF16, device=DEV) for _ in range(SETS)]
        torch.cuda.synchronize()


def byte_rows(name, buckets, lines):
    L = N.lib()
    for ratio in (0.01, 0.08, 0.2):
        int32 = fmt = 0
        for shapes in buckets:
            numels = [bucket_numel([s]) for s in shapes]
            ks = [max(1, int(m * ratio)) for m in numels]
            a = [N.i64_array([sum(v[:i]) for i in range(len(v))]) for v in (numels, ks)]
            int32 += 4 * sum(ks)
            fmt += int(L.arctopk_sparse_idx16_bytes(sum(numels), len(numels), a[0], N.i64_array(ks), a[1]))
        lines.append(FMT % ("index bytes r=%s" % ratio, name, int32, fmt, "%.3f" % (fmt / int32)))
        print(lines[-1], flush=True)


def kernel_rows(name, buckets, args, gen, sid, lines):
    L = N.lib()
    lay = [Idx16Layout(shapes, gen, sid) for shapes in buckets]

    def each(fn):
        def call(i):
            for x in lay:
                fn(x, i % SETS)
        return call

    def ck(rc, what):
        N.check(rc, what)

    def row(what, t):
        ma, mb = statistics.median(t["a"]), statistics.median(t["b"])
        lines.append(FMT % (what, name, cell(t["a"]) if ma else "-", cell(t["b"]), "%.2f" % (mb / ma) if ma else "-"))
        print(lines[-1], flush=True)

    def pack(x, s):  # the indices rotate with the rank: every call reads other memory
        ck(L.arctopk_sparse_idx16_pack(*x.lay, x.idx[(s % MAX_RANKS) * x.sum_k:].data_ptr(), x.scratch_wire.data_ptr(),
                                       sid), "arctopk_sparse_idx16_pack")

    def ge_ptr(x, s, ge):
        return x.gE[s].data_ptr() if ge else None

    def dec32(nr, ge):
        return lambda x, s: ck(L.arctopk_sparse_decode(x.out[s].data_ptr(), x.n, x.nt, x.a_off, x.a_k, x.a_ko, x.sum_k,
                                                       x.idx.data_ptr(), x.vals32.data_ptr(), nr, nr, 1, ge_ptr(x, s, ge),
                                                       1.0, N.F32, sid), "arctopk_sparse_decode")

    def dec16(nr, ge):
        return lambda x, s: ck(L.arctopk_sparse_decode_wire16(x.out[s].data_ptr(), x.n, x.nt, x.a_off, x.a_k, x.a_ko,
                                                              x.sum_k, x.idx.data_ptr(), x.vals16.data_ptr(), nr, nr, 1,
                                                              ge_ptr(x, s, ge), 1.0, sid), "arctopk_sparse_decode_wire16")

    def dec_idx16(nr, ge, dt):
        return lambda x, s: ck(L.arctopk_sparse_decode_idx16(x.out[s].data_ptr(), *x.lay, x.sum_k, x.wire.data_ptr(),
                                                             x.bytes, (x.vals32 if dt == N.F32 else x.vals16).data_ptr(),
                                                             dt, nr, nr, ge_ptr(x, s, ge), 1.0, sid),
                                "arctopk_sparse_decode_idx16")

    def dec_bf16(nr, unpack):
        def fn(x, s):
            idx = x.idx
            if unpack:
                ck(L.arctopk_sparse_idx16_unpack(*x.lay, x.sum_k, x.wire.data_ptr(), x.bytes, nr, x.unpacked.data_ptr(),
                                                 sid), "arctopk_sparse_idx16_unpack")
                idx = x.unpacked
            ck(L.arctopk_sparse_decode(x.out16[s].data_ptr(), x.n, x.nt, x.a_off, x.a_k, x.a_ko, x.sum_k, idx.data_ptr(),
                                       x.vals16.data_ptr(), nr, nr, 1, None, 1.0, N.BF16, sid), "arctopk_sparse_decode")
        return fn

    t = ab({"b": each(pack)}, args)
    row("pack", dict(t, a=[0.0]))
    for vals, today, dt in (("fp32", dec32, N.F32), ("bf16", dec16, N.BF16)):
        for ge in (False, True):
            for nr in (1, 2, 4, 8):
                row("decode %s%s nr=%d" % (vals, " ef21" if ge else "", nr),
                    ab({"a": each(today(nr, ge)), "b": each(dec_idx16(nr, ge, dt))}, args))
    for nr in (1, 2, 4, 8):
        row("unpack+bf16 nr=%d" % nr, ab({"a": each(dec_bf16(nr, False)), "b": each(dec_bf16(nr, True))}, args))
    del lay
    torch.cuda.empty_cache()


def hook_rows(name, buckets, args, gen, lines):
    nb = len(buckets)
    for ef in ("ef14", "ef21"):
        states, bks = {}, {}
        for k in ("a", "b"):
            st = SH.SparseState(None, compress_ratio=RATIO, start_compress_iter=0, sparse_type="tensor",
                                use_error_feedback=ef)
            st.index_wire = "idx16" if k == "b" else None
            states[k] = st
            bks[k] = [[SyntheticBucket(torch.randn(bucket_numel(s), device=DEV, generator=gen), s,
                                       index=q * nb + j, is_last=(j == nb - 1)) for j, s in enumerate(buckets)]
                      for q in range(SETS)]

        def step(k):
            def fn(i, st=states[k], sets=bks[k]):
                for bk in sets[i % SETS]:
                    SH.sparse_hook_sync(st, bk).wait()
            return fn
        for k in ("a", "b"):  # EF21's dense first call of every bucket is not a compressed one
            for i in range(SETS):
                step(k)(i)
        t = ab({"a": step("a"), "b": step("b")}, args)
        assert states["b"].idx16_calls > 0 and states["a"].idx16_calls == 0
        lines.append(FMT % ("hook topk %s" % ef, name, cell(t["a"]), cell(t["b"]),
                            "%.2f" % (statistics.median(t["b"]) / statistics.median(t["a"]))))
        print(lines[-1], flush=True)
        del states, bks
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--loads", default="headline,resnet50_ddp")
    ap.add_argument("--no-hook", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sparse_idx16", "table.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sparse_idx16.py needs a GPU")
    from parity import ensure_group
    ensure_group("nccl")
    gen = torch.Generator(device=DEV).manual_seed(1000)
    sid = torch.cuda.current_stream().cuda_stream
    lines = ["# library: %s; us per call: median (min..max) of %d repetitions' medians of %d calls after %d warm-ups, "
             "the paths alternating; %d disjoint sets of buffers in rotation; ratio %s (kernel and hook rows), fp32 "
             "buckets unless the row says bf16; one draw of ascending indices per rank, the same on both paths"
             % (N.lib().arctopk_version().decode(), args.repeats, args.calls, args.warmup, SETS, RATIO),
             FMT % ("what", "workload", "int32 indices (today)", "idx16 (option)", "option / today")]
    all_loads = loads()
    names = [w for w in args.loads.split(",") if w]
    for name in names:
        byte_rows(name, all_loads[name], lines)
    for name in names:
        kernel_rows(name, all_loads[name], args, gen, sid, lines)
    lines.append("# index bytes: one rank's payload, every bucket of the workload, the format's padding included; decode "
                 "fp32 rows: today is arctopk_sparse_decode (fp32, accumulate 1); decode bf16 rows: today is "
                 "arctopk_sparse_decode_wire16's merged route; unpack+bf16 rows: a bf16 bucket, arctopk_sparse_decode "
                 "alone against arctopk_sparse_idx16_unpack followed by it")
    if not args.no_hook:
        for name in names:
            hook_rows(name, all_loads[name], args, gen, lines)
        lines.append("# hook rows: sparse_hook_sync at world size 1, TopK; a call is every bucket of the workload; the "
                     "option adds the pack and changes the decode")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
