#!/usr/bin/env python3
"""The momentum fold (HookState.accumulate_momentum_on_bucket) on one GPU: the native
arctopk_momentum_fold against the torch loop it replaces (ARCTOPK_MOMENTUM_NATIVE=0), in one
process, interleaved.

Fold alone: every call sits between two of the library's device-scope timed events; a call is
one backward's folds (the headline: one bucket; a DDP model: all of its buckets).  Four disjoint
sets of buckets and moments take turns, so no call finds its data in the Infinity Cache.  Per
repetition: --warmup calls, then the median of --calls calls; native and torch alternate,
--repeats repetitions each; the table gives the median and the min..max of the repetitions'
medians.  Bytes are algorithmic: read G, read M, write G.

Whole hook: group_topk_hook (EF14, ratio 0.2, r 4, world size 1) with momentum compression on,
one state, the switch flipped between windows; a call is one backward (the headline: four
buckets, as bench.py steps them).

    python scripts/bench_momentum.py --out profiles/momentum/table.txt
    # a load/store-hint variant of the library (scripts/build_variants.py), fold and hook on the headline:
    ARCTOPK_LIB=allreducetopk_amd/lib/var/libarctopk_mom_plain.so python scripts/bench_momentum.py \
        --workloads headline_fp32 --hooks headline --label plain --out profiles/momentum/ab_plain.txt
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
from allreducetopk_amd.comm_hooks import group_topk_hook_no_reshape as G  # noqa: E402
from allreducetopk_amd.comm_hooks.utils import HookState  # noqa: E402
from workloads import DDP_MODELS, HEADLINE, ddp_buckets  # noqa: E402

DEV = "cuda:0"
BETA1 = 0.9
SETS = 4
F32, BF16 = torch.float32, torch.bfloat16
# name -> (bucket layouts of one backward, bucket dtype, moment dtype)
FOLDS = {
    "headline_fp32": ([HEADLINE], F32, F32),
    "headline_bf16": ([HEADLINE], BF16, BF16),
    "headline_bf16_m32": ([HEADLINE], BF16, F32),
    "resnet50_ddp": (ddp_buckets(DDP_MODELS["resnet50_ddp"][1]()), F32, F32),
}
HOOKS = {"headline": [HEADLINE] * 4, "resnet50_ddp": FOLDS["resnet50_ddp"][0]}


def make_backward(layouts, gdt, mdt, gen, param_state, index0=0):
    """One backward's buckets (indices from index0) with a parameter and a moment (its own
    allocation) per tensor."""
    buckets = []
    for i, shapes in enumerate(layouts):
        params = [torch.nn.Parameter(torch.empty(0)) for _ in shapes]
        for p, s in zip(params, shapes):
            param_state[p] = {"exp_avg": torch.randn(s, device=DEV, generator=gen).to(mdt)}
        buf = torch.randn(bucket_numel(shapes), device=DEV, generator=gen).to(gdt)
        buckets.append(SyntheticBucket(buf, shapes, index=index0 + i, is_last=(i == len(layouts) - 1),
                                       parameters=params))
    return buckets


def set_native(on):
    os.environ["ARCTOPK_MOMENTUM_NATIVE"] = "1" if on else "0"


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


def ab(fn, args):
    """native / torch medians of --repeats interleaved repetitions; fn(i) is one call."""
    t = {"native": [], "torch": []}
    for _ in range(args.repeats):
        for mode in ("native", "torch"):
            set_native(mode == "native")
            t[mode].append(timed_calls(fn, args.calls, args.warmup))
    set_native(True)
    return t


def cell(v):
    return "%.1f (%.1f..%.1f)" % (statistics.median(v), min(v), max(v))


def verdict(t):
    return "faster" if max(t["native"]) < min(t["torch"]) else "NOT faster"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--workloads", default=",".join(FOLDS))
    ap.add_argument("--hooks", default=",".join(HOOKS))
    ap.add_argument("--label", default="product", help="which library build this is (ARCTOPK_LIB variants)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "momentum", "table.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_momentum.py needs a GPU")
    from parity import ensure_group
    ensure_group("nccl")
    gen = torch.Generator(device=DEV).manual_seed(1000)
    lines = ["# library: %s (%s); us per call: median (min..max) of %d repetitions' medians of %d calls after %d "
             "warm-ups, native and torch (ARCTOPK_MOMENTUM_NATIVE=0) alternating; beta1 %.1f; fold: %d disjoint "
             "sets of buckets and moments in rotation; GB/s: (read G, read M, write G) / native median"
             % (args.label, N.lib().arctopk_version().decode(), args.repeats, args.calls, args.warmup, BETA1, SETS),
             "%-6s %-18s %5s %5s | %-26s | %-28s | %8s %7s | %s" %
             ("what", "workload", "bkts", "tens", "native", "torch loop", "GB/s", "torch/n", "native is")]
    for name in [w for w in args.workloads.split(",") if w]:
        layouts, gdt, mdt = FOLDS[name]
        st = HookState(None)
        st.init_momentum_field({}, BETA1)
        # every set's buckets get indices of their own: one cache entry per bucket
        sets = [make_backward(layouts, gdt, mdt, gen, st.param_state, index0=s * len(layouts))
                for s in range(SETS)]

        def fold(i, sets=sets, st=st):
            for bk in sets[i % SETS]:
                st.accumulate_momentum_on_bucket(bk)
        t = ab(fold, args)
        numel = sum(bucket_numel(sh) for sh in layouts)
        esz_g, esz_m = torch.finfo(gdt).bits // 8, torch.finfo(mdt).bits // 8
        nbytes = numel * (2 * esz_g + esz_m)
        mn, mt = statistics.median(t["native"]), statistics.median(t["torch"])
        lines.append("%-6s %-18s %5d %5d | %-26s | %-28s | %8.1f %7.2f | %s" %
                     ("fold", name, len(layouts), sum(len(sh) for sh in layouts), cell(t["native"]), cell(t["torch"]),
                      nbytes / mn / 1e3, mt / mn, verdict(t)))
        print(lines[-1], flush=True)
        assert st.momentum_native_calls == args.repeats * (args.calls + args.warmup) * len(layouts)
        del sets, st, fold
        torch.cuda.empty_cache()
    for name in [w for w in args.hooks.split(",") if w]:
        layouts = HOOKS[name]
        st = G.GroupTopKState(None, r=4, compress_ratio=0.2, start_compress_iter=0, use_error_feedback="ef14",
                              seed=1234)
        st.defer_decode = True  # the step waits every Future after the last bucket, as DDP's finalize does
        st.init_momentum_field({}, BETA1)
        buckets = make_backward(layouts, F32, F32, gen, st.param_state)

        def step(i, st=st, buckets=buckets):
            for f in [G.group_topk_hook(st, bk) for bk in buckets]:
                f.wait()
        t = ab(step, args)
        numel = sum(bucket_numel(sh) for sh in layouts)
        mn, mt = statistics.median(t["native"]), statistics.median(t["torch"])
        lines.append("%-6s %-18s %5d %5d | %-26s | %-28s | %8.1f %7.2f | %s" %
                     ("hook", name, len(layouts), sum(len(sh) for sh in layouts), cell(t["native"]), cell(t["torch"]),
                      4 * numel / mn / 1e3, mt / mn, verdict(t)))
        print(lines[-1], flush=True)
        del buckets, st, step
        torch.cuda.empty_cache()
    lines.append("# hook rows: GB/s = bucket bytes / native median (bench.py's figure of merit)")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
