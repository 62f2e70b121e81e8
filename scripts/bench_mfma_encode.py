#!/usr/bin/env python3
"""The encode kernel at sketch ranks 8, 16 and 32 on the headline bucket (16 x [2048, 2048], ratio
0.2, EF14 with a residual), fp32 and bf16, on one GPU in one process.

r = 8 runs k_encode, r = 16 and 32 the matrix encode (csrc/encode_mfma.hip).  Each arctopk_encode
call sits between two of the library's device-scope timed events; four disjoint sets of bucket and
residual rotate, so no call finds its data in the Infinity Cache.  Per repetition: --warmup calls,
then the median of --calls calls; the configurations alternate, --repeats repetitions each; the
table gives the median and the min..max of the repetitions' medians.  Bytes are algorithmic: G and
E read, E written (3 x the bucket) plus the sketch.  "fp32/op16" rows: the fp32 bucket at r = 16 and
32 with bf16 operands (arctopk_plan_set_sketch_operands), on the fp32 rows' buffers; their last
column is the fp32-operand encode of the same rank in the same run over this one.

    python scripts/bench_mfma_encode.py --out profiles/mfma_encode_bf16op/table.txt
"""
import argparse
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from allreducetopk_amd import _native as N  # noqa: E402
from allreducetopk_amd.comm_hooks.group_topk_hook_no_reshape import BucketPlan  # noqa: E402

DEV = "cuda:0"
SETS = 4
HEADLINE = [(2048, 2048)] * 16
NUMEL = 16 * 2048 * 2048


def median_us(fn, calls, warmup):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ranks", type=int, nargs="+", default=[8, 16, 32])
    ap.add_argument("--dtypes", nargs="+", default=["fp32", "bf16"])
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    stream = torch.cuda.current_stream().cuda_stream
    runs = {}
    for name in a.dtypes:
        dtype = torch.float32 if name == "fp32" else torch.bfloat16
        gen = torch.Generator(device=DEV).manual_seed(1)
        Gs = [torch.randn(NUMEL, device=DEV, generator=gen).to(dtype) for _ in range(SETS)]
        Es = [torch.zeros(NUMEL, device=DEV, dtype=dtype) for _ in range(SETS)]
        for r in a.ranks:
            plan = BucketPlan(HEADLINE, r, 0.2, dtype, DEV)
            V = torch.randn(plan.info.v_len, device=DEV, generator=gen).to(dtype)
            nbytes = NUMEL * 3 * Gs[0].element_size() + plan.info.sketch_len * Gs[0].element_size()
            runs[name, r] = (plan, V, Gs, Es, nbytes)
            if name == "fp32" and r in (16, 32):
                op16 = BucketPlan(HEADLINE, r, 0.2, dtype, DEV)
                N.check(N.lib().arctopk_plan_set_sketch_operands(op16.handle, N.BF16), "arctopk_plan_set_sketch_operands")
                runs["fp32/op16", r] = (op16, V, Gs, Es, nbytes)
    med = {k: [] for k in runs}
    for _ in range(a.repeats):
        for k, (plan, V, Gs, Es, _) in runs.items():  # the configurations alternate
            med[k].append(median_us(lambda i: plan.encode(Gs[i % SETS], Es[i % SETS], N.EF14, True, V, stream),
                                    a.calls, a.warmup))
    lines = [f"encode, EF14 err_in 1, 16 x [2048, 2048]; median (min..max) of {a.repeats} repetitions' medians "
             f"of {a.calls} calls", "dtype      r   us                        GB/s   vs r = 8 (op16: vs fp32 operands)"]
    for (name, r), m in med.items():
        us, base = statistics.median(m), statistics.median(med[("fp32", r) if name == "fp32/op16" else (name, a.ranks[0])])
        lines.append(f"{name:9s} {r:3d}  {us:7.1f} ({min(m):.1f}..{max(m):.1f})  {runs[name, r][4] / us / 1e3:7.0f}   "
                     f"{base / us:.2f}x")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
