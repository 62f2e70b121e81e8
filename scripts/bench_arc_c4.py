#!/usr/bin/env python3
"""The c4 ARC-TopK hook (dense 1-D tensors) against the base hook, one GPU, world size 1.

Both hooks at the same ratio (0.2), EF14, fp32, r = 4, device projections; the c4 hook past its
ramp (gradual_compression=False, warmup_iters=0, start_compress_iter=0), so the two differ only in
how 1-D tensors travel: RAW segments (sketch copy, a place in the sketch, a select item each)
against DENSE ones.  One process; per workload and path (the world-size-1 step path, and the
exchange step over one-rank communicators: force_exchange) three states step the same buckets
-- base, c4 and a second base state, whose difference from the first is the spread two runs of
the same hook show here -- alternating window by window, their order rotating from repeat to
repeat (the states share one set of side streams: the process's four hardware queues do not serve
three sets); every state is warmed up, every window
holds --steps backward passes (all of the workload's buckets, Futures waited after the last, as
DDP's finalize does) between two device events; median and min..max over --repeats windows.

    python scripts/bench_arc_c4.py --out profiles/arc_c4/table.txt
    # one hook alone, for a kernel trace of its own:
    rocprofv3 --kernel-trace --stats ... -- python scripts/bench_arc_c4.py --trace c4 --workloads resnet50_ddp
"""
import argparse
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from allreducetopk_amd.bucket import SyntheticBucket, bucket_numel  # noqa: E402
from allreducetopk_amd.comm_hooks import group_topk_hook_no_reshape as G  # noqa: E402
from allreducetopk_amd.comm_hooks import group_topk_hook_no_reshape_c4 as G4  # noqa: E402
from workloads import DDP_MODELS, WORKLOADS, ddp_buckets  # noqa: E402

DEV = "cuda:0"
RATIO, EF = 0.2, "ef14"


def layouts_of(name):
    if name in DDP_MODELS:
        return ddp_buckets(DDP_MODELS[name][1]())
    return [WORKLOADS[name][1]] * 4  # bench.py's default: four buckets per backward


def make_stepper(kind, layouts, force_exchange, share=None):
    if kind == "c4":
        st = G4.GroupTopKState(None, r=4, compress_ratio=RATIO, start_compress_iter=0, use_error_feedback=EF,
                               seed=1234, gradual_compression=False, warmup_iters=0)
        hook = G4.group_topk_hook
    else:
        st = G.GroupTopKState(None, r=4, compress_ratio=RATIO, start_compress_iter=0, use_error_feedback=EF,
                              seed=1234)
        hook = G.group_topk_hook
    st.force_exchange = force_exchange
    st.defer_decode = True  # step() waits every Future after the last bucket
    if share is not None:
        # one set of side streams for every state of the process: a process has four hardware
        # queues, and each state's own select / all-reduce / copy streams would share them with the
        # other states' (measured: the second and third state of a process ran up to 3x slower)
        for table in ("_sel_streams", "_ar_streams", "_copy_streams", "_side_streams"):
            setattr(st, table, getattr(share, table))
    if force_exchange:
        st.init_exchange_comms(torch.device(DEV))
    g = torch.Generator(device=DEV).manual_seed(1000)
    nb = len(layouts)
    buckets = [SyntheticBucket(torch.randn(bucket_numel(sh), device=DEV, generator=g), sh, index=i,
                               is_last=(i == nb - 1)) for i, sh in enumerate(layouts)]

    def step():
        futs = [hook(st, bk) for bk in buckets]
        return [f.wait() for f in futs]
    return step, st


def window(step, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        step()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / steps  # us per step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=6)
    ap.add_argument("--workloads", default="resnet50_ddp,resnet18_ddp,llama_layer_mixed,headline")
    ap.add_argument("--paths", default="step,exchange")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "arc_c4", "table.txt"))
    ap.add_argument("--create", default="base,c4,base2",
                    help="order in which the three states (and their buckets, residuals and plan buffers) "
                         "are created: where a state's memory lies differs with it")
    ap.add_argument("--trace", default="", choices=["", "base", "c4"],
                    help="run this hook alone (for a kernel trace of its own): no table")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_arc_c4.py needs a GPU")
    from parity import ensure_group
    ensure_group("nccl")
    names = [w for w in args.workloads.split(",") if w]
    if args.trace:
        for name in names:
            step, _ = make_stepper(args.trace, layouts_of(name), False)
            for _ in range(5):
                step()
            torch.cuda.synchronize()
            print(name, args.trace, "%.1f us per step" % window(step, args.steps))
        return
    lines = ["# us per backward (all buckets of the workload): median (min..max) over %d windows of %d steps; "
             "ratio 0.2, EF14, fp32, r 4, world size 1; base2 = a second state of the base hook in the same "
             "process (base vs base2 = the spread of two runs of one hook); GB/s = bucket bytes / median; "
             "states created in the order %s" % (args.repeats, args.steps, args.create),
             "%-18s %-8s %4s %5s | %-26s | %-26s | %-26s | %8s %8s | %9s %9s" %
             ("workload", "path", "bkts", "1-D", "base", "c4", "base2", "base GB/s", "c4 GB/s", "c4/base", "base2/base")]
    for name in names:
        layouts = layouts_of(name)
        nbytes = 4 * sum(bucket_numel(sh) for sh in layouts)
        n1d = sum(1 for sh in layouts for s in sh if len(s) == 1)
        nt = sum(len(sh) for sh in layouts)
        for path in [p for p in args.paths.split(",") if p]:
            fe = path == "exchange"
            steppers, first = {}, None
            for k in args.create.split(","):
                steppers[k], st = make_stepper("c4" if k == "c4" else "base", layouts, fe, share=first)
                first = first or st
            for fn in steppers.values():  # warm-up of every state at this workload
                for _ in range(5):
                    fn()
            torch.cuda.synchronize()
            t = {k: [] for k in steppers}
            order = ["base", "c4", "base2"]
            for rep_ in range(args.repeats):  # the order of the states rotates from repeat to repeat:
                for k in order[rep_ % 3:] + order[:rep_ % 3]:  # no state always follows the same one
                    t[k].append(window(steppers[k], args.steps))

            def cell(k):
                return "%.1f (%.1f..%.1f)" % (statistics.median(t[k]), min(t[k]), max(t[k]))
            mb, mc, m2 = (statistics.median(t[k]) for k in ("base", "c4", "base2"))
            lines.append("%-18s %-8s %4d %5s | %-26s | %-26s | %-26s | %8.1f %8.1f | %9.3f %9.3f" %
                         (name, path, len(layouts), "%d/%d" % (n1d, nt), cell("base"), cell("c4"), cell("base2"),
                          nbytes / mb / 1e3, nbytes / mc / 1e3, mc / mb, m2 / mb))
            print(lines[-1], flush=True)
            del steppers
            torch.cuda.synchronize()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
