#!/usr/bin/env python3
"""EF14 with an fp32 residual under a bf16 bucket (GroupTopKState.error_dtype = torch.float32,
DESIGN.md section 4d) on one GPU, against the bf16-residual path it is an option beside, in one
process, interleaved.

Kernels: arctopk_encode (bf16, EF14, err_in = 1) against arctopk_encode_mixed, and arctopk_pack
(EF14) against arctopk_pack_mixed, each call between two of the library's device-scope timed
events, four disjoint sets of bucket and residual in rotation (no call finds its data in the
Infinity Cache).  Per repetition: --warmup calls, then the median of --calls calls; the two
alternate, --repeats repetitions each; the table gives the median and the min..max of the
repetitions' medians.  Bytes are algorithmic: encode 2 + 2 + 2 B per element against 2 + 4 + 4;
pack, per selected element, 2 + 2 + 2 B against 4 + 4 + 2.  With --stream FILE (the output of
scripts/stream_mixed: a plain stream of the new encode's bytes, cold) the new kernels' GB/s are
also given as a share of the best rate in that file.

Whole call: group_topk_hook (EF14, r 4, world size 1) on bf16 buckets, a state with the option
against a default one (one-call step, deferred decodes), a call being one backward of four
buckets; reported as the option's cost.

    python scripts/bench_mixed_ef.py --stream profiles/mixed_ef/stream_mixed.txt --out profiles/mixed_ef/table.txt
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
from allreducetopk_amd.comm_hooks import group_topk_hook_no_reshape_c4 as G4  # noqa: E402
from workloads import HEADLINE, WORKLOADS  # noqa: E402

DEV = "cuda:0"
SETS = 4
BF16 = torch.bfloat16
# name -> (shapes, ratio, plan flags, c4 hook)
LOADS = {
    "headline_bf16": (HEADLINE, 0.2, 0, False),
    "llama_layer_c4": (WORKLOADS["llama_layer_mixed"][1], 0.2, N.PLAN_DENSE_1D, True),
}


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--loads", default=",".join(LOADS))
    ap.add_argument("--stream", default=None, help="output of scripts/stream_mixed (the plain-stream ceiling)")
    ap.add_argument("--no-hook", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mixed_ef", "table.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mixed_ef.py needs a GPU")
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
             "the two kernels (states) alternating; %d disjoint sets of bucket and residual in rotation; GB/s: "
             "algorithmic bytes / median; plain stream of the fp32-residual encode's bytes, cold: %s GB/s"
             % (L.arctopk_version().decode(), args.repeats, args.calls, args.warmup, SETS,
                "%.0f" % ceiling if ceiling else "not measured"),
             "%-7s %-15s | %-24s %7s | %-24s %7s %9s | %s" %
             ("what", "workload", "bf16 residual (today)", "GB/s", "fp32 residual (option)", "GB/s", "of stream", "time x")]
    for name in [w for w in args.loads.split(",") if w]:
        shapes, ratio, flags, c4 = LOADS[name]
        n = bucket_numel(shapes)
        plan = G.BucketPlan([tuple(s) for s in shapes], 4, ratio, BF16, DEV, flags)
        Gs = [torch.randn(n, device=DEV, generator=gen).to(BF16) for _ in range(SETS)]
        E16 = [(torch.randn(n, device=DEV, generator=gen) * 0.1).to(BF16) for _ in range(SETS)]
        E32 = [torch.randn(n, device=DEV, generator=gen) * 0.1 for _ in range(SETS)]
        V = plan.V_ring[0]
        N.check(L.arctopk_draw_projections(plan.handle, 7, V.data_ptr(), sid), "draw")
        sk, rl, sm, pk = plan.sketch.data_ptr(), plan.rowlist.data_ptr(), plan.slotmap.data_ptr(), plan.packed.data_ptr()

        def enc16(i):
            N.check(L.arctopk_encode(plan.handle, Gs[i % SETS].data_ptr(), E16[i % SETS].data_ptr(), N.EF14, 1,
                                     V.data_ptr(), sk, sid), "arctopk_encode")

        def enc32(i):
            N.check(L.arctopk_encode_mixed(plan.handle, Gs[i % SETS].data_ptr(), E32[i % SETS].data_ptr(), 1,
                                           V.data_ptr(), sk, sid), "arctopk_encode_mixed")

        def pack16(i):
            N.check(L.arctopk_pack(plan.handle, Gs[i % SETS].data_ptr(), E16[i % SETS].data_ptr(), N.EF14, rl, sm,
                                   pk, sid), "arctopk_pack")

        def pack32(i):
            N.check(L.arctopk_pack_mixed(plan.handle, Gs[i % SETS].data_ptr(), E32[i % SETS].data_ptr(), 1, rl, sm,
                                         pk, sid), "arctopk_pack_mixed")

        t = ab({"a": enc16, "b": enc32}, args)
        enc_el = sum(s.n * s.m for s in plan.segments if s.kind != N.SEG_DENSE)  # (DENSE: no encode work)
        rows = [("encode", t, enc_el * 6, enc_el * 10)]
        enc32(0)
        plan.select(1, sid)  # the rows both packs gather
        torch.cuda.synchronize()
        t = ab({"a": pack16, "b": pack32}, args)
        sel = int(plan.info.values_len)
        dense = sum(s.n for s in plan.segments if s.kind == N.SEG_DENSE)  # (their X is formed by the pack: + G)
        rows.append(("pack", t, sel * 6 + dense * 2, sel * 10 + dense * 2))
        for what, t, b16, b32 in rows:
            ma, mb = statistics.median(t["a"]), statistics.median(t["b"])
            share = "%8.0f%%" % (100.0 * b32 / mb / 1e3 / ceiling) if ceiling else "        -"
            lines.append("%-7s %-15s | %-24s %7.0f | %-24s %7.0f %9s | %.2f" %
                         (what, name, cell(t["a"]), b16 / ma / 1e3, cell(t["b"]), b32 / mb / 1e3, share, mb / ma))
            print(lines[-1], flush=True)
        del plan, Gs, E16, E32, enc16, enc32, pack16, pack32
        torch.cuda.empty_cache()
    if not args.no_hook:
        for name in [w for w in args.loads.split(",") if w]:
            shapes, ratio, flags, c4 = LOADS[name]
            mod = G4 if c4 else G
            n = bucket_numel(shapes)
            states, buckets = {}, {}
            for k in ("a", "b"):
                kw = dict(gradual_compression=False) if c4 else {}
                st = mod.GroupTopKState(None, r=4, compress_ratio=ratio, start_compress_iter=0,
                                        use_error_feedback="ef14", seed=1234, **kw)
                st.defer_decode = True  # the step waits every Future after the last bucket, as DDP's finalize does
                st.error_dtype = torch.float32 if k == "b" else None
                states[k] = st
                buckets[k] = [SyntheticBucket(torch.randn(n, device=DEV, generator=gen).to(BF16), shapes, index=i,
                                              is_last=(i == 3)) for i in range(4)]

            def step(k):
                def fn(i, st=states[k], bks=buckets[k]):
                    for f in [mod.group_topk_hook(st, bk) for bk in bks]:
                        f.wait()
                return fn
            t = ab({"a": step("a"), "b": step("b")}, args)
            assert states["b"].mixed_calls > 0 and states["a"].mixed_calls == 0
            ma, mb = statistics.median(t["a"]), statistics.median(t["b"])
            lines.append("%-7s %-15s | %-24s %7.0f | %-24s %7.0f %9s | %.2f" %
                         ("hook x4", name, cell(t["a"]), 4 * n * 2 / ma / 1e3, cell(t["b"]), 4 * n * 2 / mb / 1e3,
                          "        -", mb / ma))
            print(lines[-1], flush=True)
            del states, buckets
            torch.cuda.empty_cache()
        lines.append("# hook rows: one backward of four bf16 buckets; GB/s = bucket bytes / median (bench.py's figure of "
                     "merit); today's path is the one-call step with deferred decodes, the option's runs phase by phase")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
