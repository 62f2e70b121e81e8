#!/usr/bin/env python3
"""The packed values of an fp32 bucket sent as bf16 (GroupTopKState.wire_dtype = torch.bfloat16,
DESIGN.md section 4f) on one GPU, against the fp32 path it is an option beside, in one process,
interleaved.

Kernels: arctopk_pack (fp32; EF14, EF21) against arctopk_pack_wire16, and arctopk_decode (fp32;
EF14, EF21) against arctopk_decode_wire16, each call between two of the library's device-scope
timed events, four disjoint sets of bucket, residuals and output in rotation (no call finds its data
in the Infinity Cache).  Per repetition: --warmup calls, then the median of --calls calls; the two
alternate, --repeats repetitions each; the table gives the median and the min..max of the
repetitions' medians.  Bytes are algorithmic, K selected elements of N: pack EF14 12 K against
10 K, EF21 16 K against 14 K; decode 4 N + 4 K against 4 N + 2 K (EF21: 8 N + 8 K against
8 N + 6 K).  With --stream FILE (the output of scripts/stream_wire16: plain streams of the new
kernels' bytes, cold) the new kernels' GB/s are also given as a share of the best rate of their
pattern in that file.

Whole call: one backward of four headline buckets through group_topk_hook (EF14, r 4) beside the
emulated 8-rank wire (emulate_wire = dict(ranks=8, busbw_gbs=350)): the default pipelined path, the
default path with async_exchange = False (inline, like for like), wire_dtype = bf16 (inline) and
wire_dtype = bf16 with wire_exchange = "step" (the bf16 wire through the exchange step: pipelined).

Scatter: arctopk_decode_wire16 (noef / EF14, the whole decode: 4 N + 2 K bytes) against
arctopk_decode_wire16_scatter (the zero-ahead drain's decode into a zeroed bucket: 6 K bytes), the
same way as the other kernel rows.

    python scripts/bench_wire16.py --stream profiles/wire16/stream_wire16.txt --out profiles/wire16/table.txt
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
from workloads import HEADLINE, WORKLOADS  # noqa: E402

DEV = "cuda:0"
SETS = 4
BF16 = torch.bfloat16
LOADS = {"headline": (HEADLINE, 0.2), "resnet18_conv": (WORKLOADS["resnet18_conv"][1], 0.2)}


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
    ap.add_argument("--stream", default=None, help="output of scripts/stream_wire16 (the plain-stream ceilings)")
    ap.add_argument("--no-hook", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "wire16", "table.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_wire16.py needs a GPU")
    from parity import ensure_group
    ensure_group("nccl")
    L = N.lib()
    ceil = {}
    if args.stream and os.path.exists(args.stream):
        with open(args.stream) as fh:
            for name, rate in re.findall(r"^(\w+)\s+cold grid\s+\d+:\s+(\d+) GB/s", fh.read(), flags=re.M):
                ceil[name] = max(ceil.get(name, 0.0), float(rate))
    gen = torch.Generator(device=DEV).manual_seed(1000)
    sid = torch.cuda.current_stream().cuda_stream
    lines = ["# library: %s; us per call: median (min..max) of %d repetitions' medians of %d calls after %d warm-ups, "
             "the two kernels (states) alternating; %d disjoint buffer sets in rotation; GB/s: algorithmic bytes / "
             "median; plain streams, cold: %s"
             % (L.arctopk_version().decode(), args.repeats, args.calls, args.warmup, SETS,
                ", ".join("%s %.0f GB/s" % kv for kv in sorted(ceil.items())) or "not measured"),
             "%-11s %-14s | %-24s %7s | %-24s %7s %9s | %s" %
             ("what", "workload", "fp32 values (today)", "GB/s", "bf16 values (option)", "GB/s", "of stream", "time x")]
    for name in [w for w in args.loads.split(",") if w]:
        shapes, ratio = LOADS[name]
        n = bucket_numel(shapes)
        plan = G.BucketPlan([tuple(s) for s in shapes], 4, ratio, torch.float32, DEV)
        Gs = [torch.randn(n, device=DEV, generator=gen) for _ in range(SETS)]
        Es = [torch.randn(n, device=DEV, generator=gen) * 0.1 for _ in range(SETS)]
        Os = [torch.empty(n, device=DEV) for _ in range(SETS)]
        P32 = [torch.zeros(max(1, plan.info.packed_len), device=DEV) for _ in range(SETS)]
        P16 = [torch.zeros(max(1, plan.info.packed_len), device=DEV, dtype=BF16) for _ in range(SETS)]
        V = plan.V_ring[0]
        N.check(L.arctopk_draw_projections(plan.handle, 7, V.data_ptr(), sid), "draw")
        rl, sm = plan.rowlist.data_ptr(), plan.slotmap.data_ptr()
        plan.encode(Gs[0], Es[0], N.EF14, True, V, sid)
        plan.select(1, sid)  # the rows every pack gathers and every decode scatters
        torch.cuda.synchronize()
        k = int(plan.info.values_len)

        def pack32(ef):
            return lambda i: N.check(L.arctopk_pack(plan.handle, Gs[i % SETS].data_ptr(), Es[i % SETS].data_ptr(), ef,
                                                    rl, sm, P32[i % SETS].data_ptr(), sid), "arctopk_pack")

        def pack16(ef):
            return lambda i: N.check(L.arctopk_pack_wire16(plan.handle, Gs[i % SETS].data_ptr(),
                                                           Es[i % SETS].data_ptr(), ef, 1, rl, sm,
                                                           P16[i % SETS].data_ptr(), sid), "arctopk_pack_wire16")

        def dec32(ef):
            return lambda i: N.check(L.arctopk_decode(plan.handle, P32[i % SETS].data_ptr(), sm, 1, ef,
                                                      Es[i % SETS].data_ptr() if ef == N.EF21 else None,
                                                      Os[i % SETS].data_ptr(), sid), "arctopk_decode")

        def dec16(ef):
            return lambda i: N.check(L.arctopk_decode_wire16(plan.handle, P16[i % SETS].data_ptr(), sm, 1, ef,
                                                             Es[i % SETS].data_ptr() if ef == N.EF21 else None,
                                                             Os[i % SETS].data_ptr(), sid), "arctopk_decode_wire16")

        def scat16(i):
            N.check(L.arctopk_decode_wire16_scatter(plan.handle, P16[i % SETS].data_ptr(), rl, sm, 1,
                                                    Os[i % SETS].data_ptr(), sid), "arctopk_decode_wire16_scatter")

        rows = [("pack ef14", pack32(N.EF14), pack16(N.EF14), 12 * k, 10 * k, "rw8w2"),
                ("pack ef21", pack32(N.EF21), pack16(N.EF21), 16 * k, 14 * k, "r4rw8w2"),
                ("decode ef14", dec32(N.EF14), dec16(N.EF14), 4 * n + 4 * k, 4 * n + 2 * k, "w4r2"),
                ("decode ef21", dec32(N.EF21), dec16(N.EF21), 8 * n + 8 * k, 8 * n + 6 * k, None),
                # (left: the whole bf16-wire decode; right: the scatter of the same packed values)
                ("w16 scatter", dec16(N.EF14), scat16, 4 * n + 2 * k, 6 * k, "r2w4")]
        for what, fa, fb, ba, bb, pat in rows:
            t = ab({"a": fa, "b": fb}, args)
            ma, mb = statistics.median(t["a"]), statistics.median(t["b"])
            share = "%8.0f%%" % (100.0 * bb / mb / 1e3 / ceil[pat]) if pat in ceil else "        -"
            lines.append("%-11s %-14s | %-24s %7.0f | %-24s %7.0f %9s | %.2f" %
                         (what, name, cell(t["a"]), ba / ma / 1e3, cell(t["b"]), bb / mb / 1e3, share, mb / ma))
            print(lines[-1], flush=True)
        del plan, Gs, Es, Os, P32, P16, rows
        torch.cuda.empty_cache()
    if not args.no_hook:
        shapes, ratio = LOADS["headline"]
        n = bucket_numel(shapes)
        configs = {"pipelined": dict(), "inline": dict(async_exchange=False), "wire16": dict(wire_dtype=BF16),
                   "wire16_step": dict(wire_dtype=BF16, wire_exchange="step")}
        states, buckets = {}, {}
        for kname, kw in configs.items():
            st = G.GroupTopKState(None, r=4, compress_ratio=ratio, start_compress_iter=0, use_error_feedback="ef14",
                                  seed=1234)
            st.defer_decode = True  # the step waits every Future after the last bucket, as DDP's finalize does
            st.emulate_wire = dict(ranks=8, busbw_gbs=350)
            for key, v in kw.items():
                setattr(st, key, v)
            states[kname] = st
            buckets[kname] = [SyntheticBucket(torch.randn(n, device=DEV, generator=gen), shapes, index=i,
                                              is_last=(i == 3)) for i in range(4)]

        def step(kname):
            def fn(i, st=states[kname], bks=buckets[kname]):
                for f in [G.group_topk_hook(st, bk) for bk in bks]:
                    f.wait()
            return fn
        t = ab({kname: step(kname) for kname in configs}, args)
        assert states["wire16"].wire16_calls > 0 and states["pipelined"].wire16_calls == 0
        assert states["wire16_step"].wire16_step_calls == states["wire16_step"].wire16_calls > 0
        assert states["wire16"].wire16_step_calls == 0
        base = statistics.median(t["pipelined"])
        lines.append("# one backward of four headline fp32 buckets (EF14) beside the emulated wire (8 ranks, 350 GB/s "
                     "busBW); GB/s = bucket bytes / median (bench.py's figure of merit); x: time against the pipelined default")
        for kname in configs:
            m = statistics.median(t[kname])
            lines.append("%-11s %-14s | %-24s %7.0f | x %.2f" % ("hook x4", kname, cell(t[kname]), 4 * n * 4 / m / 1e3,
                                                               m / base))
            print(lines[-1], flush=True)
        mi, mw = statistics.median(t["inline"]), statistics.median(t["wire16"])
        lines.append("# the inline bf16-wire branch %s the pipelined default beside the wire (%.0f us against %.0f us); "
                     "against the inline default it takes %.2f of the time"
                     % ("beats" if mw < base else "does not beat", mw, base, mw / mi))
        ts = t["wire16_step"]
        ms = statistics.median(ts)
        spread = max(max(ts) - min(ts), max(t["wire16"]) - min(t["wire16"]))
        lines.append("# the bf16 wire through the exchange step: %.1f us against the inline bf16-wire branch's %.1f us "
                     "(margin %.1f us, the larger of the two lines' max - min %.1f us); against the pipelined default "
                     "x %.2f (its minimum %.1f us)" % (ms, mw, mw - ms, spread, ms / base, min(t["pipelined"])))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
