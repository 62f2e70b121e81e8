#!/usr/bin/env python3
"""TopK / RandK with bf16 values on the wire of an fp32 bucket (SparseState.wire_dtype =
torch.bfloat16) on one GPU, against the fp32-wire path it is an option
beside, in one process, interleaved -- the method of scripts/bench_sparse_mixed.py.

Kernels, each call between two of the library's device-scope timed events, four disjoint sets of
bucket-sized buffers in rotation (no call finds its data in the Infinity Cache):

    pack    arctopk_sparse_residual (fp32) against arctopk_sparse_pack_wire16, EF14 and EF21, at the
            ascending indices of the device RandK draw (uniform over every tensor)
    decode  arctopk_sparse_decode (fp32, accumulate 1) against arctopk_sparse_decode_wire16's merged
            route (accumulate 1) and its scattered route (accumulate 3) on the same indices, at
            nranks = world size 1, 2, 4 and 8 (payloads built locally, one draw per rank: no
            collective), without gE and with it (EF21).  GB/s of the merged route: the bytes it has
            to move per element of the bucket -- 4 B written, under EF21 8 B of gE as well -- over
            the median; with --stream FILE (scripts/stream_mixed's output, same session) also as a
            share of the best rate in the file

Per repetition: --warmup calls, then the median of --calls calls; the paths alternate, --repeats
repetitions each; the table gives the median and the min..max of the repetitions' medians.

Whole call: sparse_hook_sync (world size 1) on fp32 buckets, a state with the option against a
default one, TopK and RandK "hash", EF14 and EF21; a call is one bucket of the headline, or one
backward's buckets of the ResNet-50 DDP set.

    python scripts/bench_sparse_wire16.py --stream profiles/sparse_wire16/stream_mixed.txt
"""
import argparse
import os
import re
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from allreducetopk_amd import _native as N  # noqa: E402
from allreducetopk_amd.bucket import SyntheticBucket, bucket_numel  # noqa: E402
from allreducetopk_amd.comm_hooks import sparse_hook as SH  # noqa: E402
from workloads import DDP_MODELS, HEADLINE, ddp_buckets  # noqa: E402

DEV = "cuda:0"
SETS = 4
BF16 = torch.bfloat16
F32 = torch.float32
RATIO = 0.2
MAX_RANKS = 8


def loads():
    """name -> the buckets of one call (a list of shape lists)."""
    return {"headline": [HEADLINE], "resnet50_ddp": ddp_buckets(DDP_MODELS["resnet50_ddp"][1](), elem_bytes=4)}


def timed_calls(fn, calls, warmup):
    """Median us of `calls` calls of fn(i), each between two device-scope timed events."""
    stream = torch.cuda.current_stream().cuda_stream
    for i in range(warmup):
        fn(i)
    ev = [(N.DeviceEvent(timing=True), N.DeviceEvent(timing=True)) for _ in range(calls)]
    for i, (e0, e1) in enumerate(ev):
        e0.record(stream)
        fn(warmup + i)
        e1.record(stream)
    torch.cuda.synchronize()
    return statistics.median(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev)


def ab(fns, args):
    t = {k: [] for k in fns}
    for _ in range(args.repeats):
        for k, fn in fns.items():
            t[k].append(timed_calls(fn, args.calls, args.warmup))
    return t


def cell(v):
    return "%.1f (%.1f..%.1f)" % (statistics.median(v), min(v), max(v))


class Layout:
    """One bucket's host arrays and device buffers: SETS of each bucket-sized one, and MAX_RANKS
    payloads (each rank its own ascending draw) as fp32 and as bf16 values."""

    def __init__(self, shapes, gen, sid):
        L = N.lib()
        self.n = n = bucket_numel(shapes)
        numels = [bucket_numel([s]) for s in shapes]
        ks = [max(1, int(m * RATIO)) for m in numels]
        self.nt, self.sum_k = len(shapes), sum(ks)
        offs = [sum(numels[:i]) for i in range(len(numels))]
        koff = [sum(ks[:i]) for i in range(len(ks))]
        self.a_off, self.a_n, self.a_k, self.a_ko = (N.i64_array(offs), N.i64_array(numels), N.i64_array(ks),
                                                     N.i64_array(koff))
        rnd = lambda s=1.0: [torch.randn(n, device=DEV, generator=gen) * s for _ in range(SETS)]  # noqa: E731
        self.E, self.gE = rnd(0.1), rnd(0.1)
        self.out = [torch.empty(n, device=DEV) for _ in range(SETS)]
        self.vals32 = torch.randn(MAX_RANKS * self.sum_k, device=DEV, generator=gen)
        self.vals16 = self.vals32.to(BF16)
        self.pack16 = torch.empty(self.sum_k, dtype=BF16, device=DEV)
        self.idx = torch.empty(MAX_RANKS * self.sum_k, dtype=torch.int32, device=DEV)
        nb = int(L.arctopk_sparse_workspace_bytes(self.nt, self.a_n))
        ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
        for r in range(MAX_RANKS):
            N.check(L.arctopk_randk_select(None, self.nt, None, self.a_n, self.a_k, self.a_ko, 7 + r,
                                           self.idx[r * self.sum_k:].data_ptr(), None, ws.data_ptr(), N.F32, 0, sid),
                    "arctopk_randk_select")
        torch.cuda.synchronize()


def kernel_rows(name, buckets, args, gen, sid, ceiling, lines):
    L = N.lib()
    lay = [Layout(shapes, gen, sid) for shapes in buckets]
    n = sum(x.n for x in lay)

    def each(fn):
        def call(i):
            for x in lay:
                fn(x, i % SETS)
        return call

    def ck(rc, what):
        N.check(rc, what)

    def residual(ef):
        return lambda x, s: ck(L.arctopk_sparse_residual(x.E[s].data_ptr(), x.nt, x.a_off, x.a_k, x.a_ko, x.idx.data_ptr(),
                                                         x.vals32.data_ptr(), ef, 1.0, N.F32, sid), "arctopk_sparse_residual")

    def pack(ef):
        return lambda x, s: ck(L.arctopk_sparse_pack_wire16(x.vals32.data_ptr(), x.E[s].data_ptr(), x.n, x.nt, x.a_off,
                                                            x.a_k, x.a_ko, x.idx.data_ptr(), x.pack16.data_ptr(), ef, 1.0,
                                                            sid), "arctopk_sparse_pack_wire16")

    def dec32(nr, ge):
        return lambda x, s: ck(L.arctopk_sparse_decode(x.out[s].data_ptr(), x.n, x.nt, x.a_off, x.a_k, x.a_ko, x.sum_k,
                                                       x.idx.data_ptr(), x.vals32.data_ptr(), nr, nr, 1,
                                                       x.gE[s].data_ptr() if ge else None, 1.0, N.F32, sid),
                                "arctopk_sparse_decode")

    def dec16(nr, ge, acc):
        return lambda x, s: ck(L.arctopk_sparse_decode_wire16(x.out[s].data_ptr(), x.n, x.nt, x.a_off, x.a_k, x.a_ko,
                                                              x.sum_k, x.idx.data_ptr(), x.vals16.data_ptr(), nr, nr, acc,
                                                              x.gE[s].data_ptr() if ge else None, 1.0, sid),
                                "arctopk_sparse_decode_wire16")

    def row(what, t, nbytes):
        ma, mb = statistics.median(t["a"]), statistics.median(t["b"])
        gb, share = "      -", "        -"
        if nbytes:
            gb = "%7.0f" % (nbytes / mb / 1e3)
            if ceiling:
                share = "%8.0f%%" % (100.0 * nbytes / mb / 1e3 / ceiling)
        c = cell(t["c"]) if "c" in t else "-"
        lines.append("%-16s %-13s | %-26s | %-26s %s %s | %.2f | %-26s" %
                     (what, name, cell(t["a"]), cell(t["b"]), gb, share, mb / ma, c))
        print(lines[-1], flush=True)

    for ef, tag in ((N.EF14, "pack ef14"), (N.EF21, "pack ef21")):
        row(tag, ab({"a": each(residual(ef)), "b": each(pack(ef))}, args), None)
    for ge in (False, True):
        for nr in (1, 2, 4, 8):
            t = ab({"a": each(dec32(nr, ge)), "b": each(dec16(nr, ge, 1)), "c": each(dec16(nr, ge, 3))}, args)
            row("decode%s nr=%d" % (" ef21" if ge else "", nr), t, n * (12 if ge else 4))
    del lay
    torch.cuda.empty_cache()


def hook_rows(name, buckets, args, gen, lines):
    nb = len(buckets)
    for kind, ef in (("topk", "ef14"), ("topk", "ef21"), ("randk", "ef14"), ("randk", "ef21")):
        states, bks = {}, {}
        for k in ("a", "b"):
            st = SH.SparseState(None, compress_ratio=RATIO, start_compress_iter=0, sparse_type="tensor",
                                random=kind == "randk", use_error_feedback=ef, random_seed=1234, index_source="hash")
            st.wire_dtype = BF16 if k == "b" else None
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
        assert states["b"].wire16_calls > 0 and states["a"].wire16_calls == 0
        ma, mb = statistics.median(t["a"]), statistics.median(t["b"])
        lines.append("%-16s %-13s | %-26s | %-26s %s %s | %.2f | %-26s" %
                     ("%s %s" % (kind, ef), name, cell(t["a"]), cell(t["b"]), "      -", "        -", mb / ma, "-"))
        print(lines[-1], flush=True)
        del states, bks
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--loads", default="headline,resnet50_ddp")
    ap.add_argument("--stream", default=None, help="output of scripts/stream_mixed (the plain-stream ceiling)")
    ap.add_argument("--no-hook", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sparse_wire16", "table.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sparse_wire16.py needs a GPU")
    from parity import ensure_group
    ensure_group("nccl")
    L = N.lib()
    ceiling = None
    if args.stream and os.path.exists(args.stream):
        with open(args.stream) as fh:
            rates = [float(x) for x in re.findall(r"cold grid\s+\d+:\s+(\d+) GB/s", fh.read())]
        ceiling = max(rates) if rates else None
    gen = torch.Generator(device=DEV).manual_seed(1000)
    sid = torch.cuda.current_stream().cuda_stream
    lines = ["# library: %s; us per call: median (min..max) of %d repetitions' medians of %d calls after %d warm-ups, "
             "the paths alternating; %d disjoint sets of buffers in rotation; ratio %s, fp32 buckets; GB/s (decode rows): "
             "4 B per bucket element, 12 B under EF21, over the merged route's median; plain stream "
             "(scripts/stream_mixed, cold): %s GB/s"
             % (L.arctopk_version().decode(), args.repeats, args.calls, args.warmup, SETS, RATIO,
                "%.0f" % ceiling if ceiling else "not measured"),
             "%-16s %-13s | %-26s | %-26s %7s %9s | %s | %-26s" %
             ("what", "workload", "fp32 wire (today)", "bf16 wire (option)", "GB/s", "of stream", "time x",
              "bf16 wire, scattered route")]
    all_loads = loads()
    names = [w for w in args.loads.split(",") if w]
    for name in names:
        kernel_rows(name, all_loads[name], args, gen, sid, ceiling, lines)
    lines.append("# pack rows: today's column is arctopk_sparse_residual alone (the values are already gathered on both "
                 "paths); decode rows: nranks = world size, today's column is arctopk_sparse_decode (fp32, accumulate 1), "
                 "the option's is the merged route (accumulate 1), the last column the scattered route (accumulate 3) on "
                 "the same payloads; time x: option / today")
    if not args.no_hook:
        for name in names:
            hook_rows(name, all_loads[name], args, gen, lines)
        lines.append("# hook rows: sparse_hook_sync at world size 1, index_source 'hash' for RandK; a call is every bucket "
                     "of the workload; the fold and the select are the same on both paths")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
