#!/usr/bin/env python3
"""TopK / RandK with fp32 residuals under a bf16 bucket (SparseState.error_dtype = torch.float32,
DESIGN.md section 4g) on one GPU, against the bf16-residual path it is an option beside, in one
process, interleaved -- the method of scripts/bench_mixed_ef.py.

Kernels, each call between two of the library's device-scope timed events, four disjoint sets of
buffers in rotation (no call finds its data in the Infinity Cache):

    fold    arctopk_ef14_fold (bf16, err_in = 1) / arctopk_ef_apply (bf16, EF21) against
            arctopk_sparse_fold_mixed; bytes per element 2 + 2 + 2 against 2 + 4 + 4
    pack    arctopk_sparse_gather + arctopk_sparse_residual (bf16) against arctopk_sparse_pack_mixed,
            at the ascending indices of the device RandK draw (uniform over every tensor)
    decode  EF21, one payload: arctopk_sparse_decode (bf16, gerr) against arctopk_sparse_decode_mixed21

Per repetition: --warmup calls, then the median of --calls calls; the two alternate, --repeats
repetitions each; the table gives the median and the min..max of the repetitions' medians.

The bar: the fold's byte pattern is scripts/stream_mixed.hip's.  With --stream FILE (that program's
output, same session) the fold's GB/s is given as a share of the best rate in the file, next to the
share arctopk_encode_mixed (the same bytes plus a sketch) reaches in this
process on the headline bucket.

Whole call: sparse_hook_sync (world size 1) on bf16 buckets, a state with the option against a
default one, TopK and RandK "hash", EF14 and EF21; a call is one bucket of the headline, or one
backward's buckets of the ResNet-50 DDP set.

    python scripts/bench_sparse_mixed.py --stream profiles/sparse_mixed/stream_mixed.txt
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
from allreducetopk_amd.comm_hooks import group_topk_hook_no_reshape as G  # noqa: E402
from allreducetopk_amd.comm_hooks import sparse_hook as SH  # noqa: E402
from workloads import DDP_MODELS, HEADLINE, ddp_buckets  # noqa: E402

DEV = "cuda:0"
SETS = 4
BF16 = torch.bfloat16
F32 = torch.float32
RATIO = 0.2


def loads():
    """name -> the buckets of one call (a list of shape lists)."""
    return {"headline_bf16": [HEADLINE],
            "resnet50_ddp_bf16": ddp_buckets(DDP_MODELS["resnet50_ddp"][1](), elem_bytes=2)}


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
    """One bucket's host arrays and device buffers, SETS of each."""

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
        rnd = lambda dt, s=1.0: [(torch.randn(n, device=DEV, generator=gen) * s).to(dt) for _ in range(SETS)]  # noqa: E731
        self.G, self.E16, self.gE16 = rnd(BF16), rnd(BF16, 0.1), rnd(BF16, 0.1)
        self.E32, self.gE32, self.D32 = rnd(F32, 0.1), rnd(F32, 0.1), rnd(F32)
        self.out16 = [torch.empty(n, dtype=BF16, device=DEV) for _ in range(SETS)]
        self.vals = torch.empty(self.sum_k, dtype=BF16, device=DEV)
        self.idx = torch.empty(self.sum_k, dtype=torch.int32, device=DEV)
        nb = int(L.arctopk_sparse_workspace_bytes(self.nt, self.a_n))
        ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
        N.check(L.arctopk_randk_select(None, self.nt, None, self.a_n, self.a_k, self.a_ko, 7, self.idx.data_ptr(),
                                       None, ws.data_ptr(), N.F32, 0, sid), "arctopk_randk_select")
        torch.cuda.synchronize()


def kernel_rows(name, buckets, args, gen, sid, ceiling, lines):
    L = N.lib()
    lay = [Layout(shapes, gen, sid) for shapes in buckets]
    n = sum(x.n for x in lay)
    sel = sum(x.sum_k for x in lay)

    def each(fn):
        def call(i):
            for x in lay:
                fn(x, i % SETS)
        return call

    def ck(rc, what):
        N.check(rc, what)

    rows = []
    t = ab({"a": each(lambda x, s: ck(L.arctopk_ef14_fold(x.G[s].data_ptr(), x.E16[s].data_ptr(), x.n, 1, N.BF16, sid),
                                      "arctopk_ef14_fold")),
            "b": each(lambda x, s: ck(L.arctopk_sparse_fold_mixed(x.G[s].data_ptr(), x.E32[s].data_ptr(), None, x.n,
                                                                  N.EF14, 1, sid), "arctopk_sparse_fold_mixed"))}, args)
    rows.append(("fold ef14", t, n * 6, n * 10))
    t = ab({"a": each(lambda x, s: ck(L.arctopk_ef_apply(x.G[s].data_ptr(), x.E16[s].data_ptr(), x.n, N.EF21, 1, N.BF16,
                                                         sid), "arctopk_ef_apply")),
            "b": each(lambda x, s: ck(L.arctopk_sparse_fold_mixed(x.G[s].data_ptr(), x.E32[s].data_ptr(),
                                                                  x.D32[s].data_ptr(), x.n, N.EF21, 1, sid),
                                      "arctopk_sparse_fold_mixed"))}, args)
    rows.append(("fold ef21", t, n * 6, n * 10))

    def pack16(ef):
        def fn(x, s):
            src = x.E16[s] if ef == N.EF14 else x.G[s]
            ck(L.arctopk_sparse_gather(src.data_ptr(), x.nt, x.a_off, x.a_k, x.a_ko, x.idx.data_ptr(),
                                       x.vals.data_ptr(), N.BF16, sid), "arctopk_sparse_gather")
            ck(L.arctopk_sparse_residual(x.E16[s].data_ptr(), x.nt, x.a_off, x.a_k, x.a_ko, x.idx.data_ptr(),
                                         x.vals.data_ptr(), ef, 1.0, N.BF16, sid), "arctopk_sparse_residual")
        return fn

    def pack32(ef):
        def fn(x, s):
            src = x.E32[s] if ef == N.EF14 else x.D32[s]
            ck(L.arctopk_sparse_pack_mixed(src.data_ptr(), x.E32[s].data_ptr(), x.n, x.nt, x.a_off, x.a_k, x.a_ko,
                                           x.idx.data_ptr(), x.vals.data_ptr(), ef, 1.0, sid),
               "arctopk_sparse_pack_mixed")
        return fn

    for ef, tag in ((N.EF14, "pack ef14"), (N.EF21, "pack ef21")):
        t = ab({"a": each(pack16(ef)), "b": each(pack32(ef))}, args)
        rows.append((tag, t, None, None))

    def dec16(x, s):
        ck(L.arctopk_sparse_decode(x.out16[s].data_ptr(), x.n, x.nt, x.a_off, x.a_k, x.a_ko, x.sum_k, x.idx.data_ptr(),
                                   x.vals.data_ptr(), 1, 1, 1, x.gE16[s].data_ptr(), 1.0, N.BF16, sid),
           "arctopk_sparse_decode")

    def dec32(x, s):
        ck(L.arctopk_sparse_decode_mixed21(x.out16[s].data_ptr(), x.gE32[s].data_ptr(), x.D32[s].data_ptr(), x.n, x.nt,
                                           x.a_off, x.a_k, x.a_ko, x.sum_k, x.idx.data_ptr(), x.vals.data_ptr(), 1, 1,
                                           1.0, sid), "arctopk_sparse_decode_mixed21")

    t = ab({"a": each(dec16), "b": each(dec32)}, args)
    rows.append(("decode ef21", t, None, None))
    fold_share = None
    for what, t, b16, b32 in rows:
        ma, mb = statistics.median(t["a"]), statistics.median(t["b"])
        ga = "%7.0f" % (b16 / ma / 1e3) if b16 else "      -"
        gb = "%7.0f" % (b32 / mb / 1e3) if b32 else "      -"
        share = "        -"
        if b32 and ceiling:
            share = "%8.0f%%" % (100.0 * b32 / mb / 1e3 / ceiling)
            if what == "fold ef14":
                fold_share = [100.0 * b32 / v / 1e3 / ceiling for v in t["b"]]
        lines.append("%-12s %-17s | %-26s %s | %-26s %s %9s | %.2f" %
                     (what, name, cell(t["a"]), ga, cell(t["b"]), gb, share, mb / ma))
        print(lines[-1], flush=True)
    del lay
    torch.cuda.empty_cache()
    return fold_share, sel


def encode_mixed_share(args, gen, sid, ceiling, lines):
    """arctopk_encode_mixed (ARC-TopK's fp32-residual encode, EF14, err_in = 1) on the headline
    bucket: the kernel whose share of the plain stream the fold has to reach."""
    L = N.lib()
    n = bucket_numel(HEADLINE)
    plan = G.BucketPlan([tuple(s) for s in HEADLINE], 4, RATIO, BF16, DEV, 0)
    Gs = [torch.randn(n, device=DEV, generator=gen).to(BF16) for _ in range(SETS)]
    E32 = [torch.randn(n, device=DEV, generator=gen) * 0.1 for _ in range(SETS)]
    V = plan.V_ring[0]
    N.check(L.arctopk_draw_projections(plan.handle, 7, V.data_ptr(), sid), "draw")

    def enc(i):
        N.check(L.arctopk_encode_mixed(plan.handle, Gs[i % SETS].data_ptr(), E32[i % SETS].data_ptr(), 1, V.data_ptr(),
                                       plan.sketch.data_ptr(), sid), "arctopk_encode_mixed")
    t = [timed_calls(enc, args.calls, args.warmup) for _ in range(args.repeats)]
    m = statistics.median(t)
    share = [100.0 * n * 10 / v / 1e3 / ceiling for v in t] if ceiling else None
    lines.append("%-12s %-17s | %-26s %s | %-26s %7.0f %9s |" %
                 ("encode_mixed", "headline_bf16", "-", "      -", cell(t), n * 10 / m / 1e3,
                  "%8.0f%%" % statistics.median(share) if share else "        -"))
    print(lines[-1], flush=True)
    del plan, Gs, E32
    torch.cuda.empty_cache()
    return share


def hook_rows(name, buckets, args, gen, lines):
    nb = len(buckets)
    n = sum(bucket_numel(s) for s in buckets)
    for kind, ef in (("topk", "ef14"), ("topk", "ef21"), ("randk", "ef14"), ("randk", "ef21")):
        states, bks = {}, {}
        for k in ("a", "b"):
            st = SH.SparseState(None, compress_ratio=RATIO, start_compress_iter=0, sparse_type="tensor",
                                random=kind == "randk", use_error_feedback=ef, random_seed=1234, index_source="hash")
            st.error_dtype = F32 if k == "b" else None
            states[k] = st
            bks[k] = [[SyntheticBucket(torch.randn(bucket_numel(s), device=DEV, generator=gen).to(BF16), s,
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
        assert states["b"].mixed_calls > 0 and states["a"].mixed_calls == 0
        ma, mb = statistics.median(t["a"]), statistics.median(t["b"])
        lines.append("%-12s %-17s | %-26s %7.0f | %-26s %7.0f %9s | %.2f" %
                     ("%s %s" % (kind, ef), name, cell(t["a"]), n * 2 / ma / 1e3, cell(t["b"]), n * 2 / mb / 1e3,
                      "        -", mb / ma))
        print(lines[-1], flush=True)
        del states, bks
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--loads", default="headline_bf16,resnet50_ddp_bf16")
    ap.add_argument("--stream", default=None, help="output of scripts/stream_mixed (the plain-stream ceiling)")
    ap.add_argument("--no-hook", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sparse_mixed", "table.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sparse_mixed.py needs a GPU")
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
             "the two paths alternating; %d disjoint sets of buffers in rotation; ratio %s; GB/s: algorithmic bytes / "
             "median (hook rows: bucket bytes / median); plain stream of the fold's bytes, cold: %s GB/s"
             % (L.arctopk_version().decode(), args.repeats, args.calls, args.warmup, SETS, RATIO,
                "%.0f" % ceiling if ceiling else "not measured"),
             "%-12s %-17s | %-26s %7s | %-26s %7s %9s | %s" %
             ("what", "workload", "bf16 residual (today)", "GB/s", "fp32 residual (option)", "GB/s", "of stream", "time x")]
    all_loads = loads()
    fold_share = None
    for name in [w for w in args.loads.split(",") if w]:
        share, _ = kernel_rows(name, all_loads[name], args, gen, sid, ceiling, lines)
        if name == "headline_bf16":
            fold_share = share
    if "headline_bf16" in args.loads.split(","):
        enc_share = encode_mixed_share(args, gen, sid, ceiling, lines)
        if fold_share and enc_share:
            spread = max(max(fold_share) - min(fold_share), max(enc_share) - min(enc_share))
            lines.append("# the bar (headline): fold ef14 %.1f%% of the stream (%.1f..%.1f), arctopk_encode_mixed %.1f%% "
                         "(%.1f..%.1f), run-to-run spread %.1f points: the fold %s"
                         % (statistics.median(fold_share), min(fold_share), max(fold_share),
                            statistics.median(enc_share), min(enc_share), max(enc_share), spread,
                            "reaches it" if statistics.median(fold_share) >= statistics.median(enc_share) - spread
                            else "falls short"))
            print(lines[-1], flush=True)
    if not args.no_hook:
        for name in [w for w in args.loads.split(",") if w]:
            hook_rows(name, all_loads[name], args, gen, lines)
        lines.append("# hook rows: sparse_hook_sync at world size 1, index_source 'hash' for RandK; a call is every bucket "
                     "of the workload; both paths select, the option's on fp32 keys")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
