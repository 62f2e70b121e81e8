#!/usr/bin/env python3
"""Row- / column-wise selection on the GPU: the segmented select (arctopk_seg_select) alone and
the whole hook call at world size 1, against two stand-ins timed in the same process:

  (a) what the shipped library offered before: the same segments passed to arctopk_topk_select
      (RandK: arctopk_randk_select) as separate tensors; column mode: x.t().contiguous() first
  (b) the reference's own ops on the GPU: torch.topk(x.abs(), k, dim) and a gather (TopK only)

Every shape is warmed up, every timed window holds --calls calls between two device events, the
variants alternate inside one process and the median and the min..max spread over --repeats
windows are reported.  Bytes per call are algorithmic: one read of the tensor plus the payload
write (int32 index + value per entry); the share is of the 8 TB/s HBM peak.

    python scripts/bench_rowcol.py --out profiles/rowcol/select_table.txt
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
from allreducetopk_amd.bucket import SyntheticBucket  # noqa: E402
from allreducetopk_amd.comm_hooks import sparse_hook  # noqa: E402

HBM_PEAK = 8.0e12
SHAPES = [([2048, 2048], torch.float32), ([5461, 2048], torch.float32), ([2048, 5461], torch.float32),
          ([2048, 5461], torch.bfloat16), ([32000, 2048], torch.float32), ([512, 512, 3, 3], torch.float32),
          ([64, 3, 7, 7], torch.float32), ([1000, 2048], torch.float32)]
RATIOS = [0.2, 0.01]
VARIANTS = [("topk", "row"), ("topk", "column"), ("randk", "row")]
DEV = "cuda:0"


def view(shape):
    n = 1
    for d in shape:
        n *= d
    return shape[0], n // shape[0]


def timed(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls  # us per call


def make_new(x, r, c, k, mode, random, dtype):
    L, a = N.lib(), N.i64_array
    nseg = c if mode == "column" else r
    rows, cols, ks, zero = a([r]), a([c]), a([k]), a([0])
    nb = int(L.arctopk_seg_workspace_bytes(1, rows, cols, ks, int(mode == "column")))
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    idx = torch.empty(nseg * k, dtype=torch.int32, device=DEV)
    vals = torch.empty(nseg * k, dtype=dtype, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    dt = N.DTYPE_CODE[dtype]

    def run():
        N.check(L.arctopk_seg_select(x.data_ptr(), 1, zero, rows, cols, ks, zero, int(mode == "column"),
                                     int(random), 12345, idx.data_ptr(), vals.data_ptr(), ws.data_ptr(), dt, 0, st),
                "arctopk_seg_select")
    return run


def make_old(x, r, c, k, mode, random, dtype):
    """(a): every segment as a tensor of its own through the per-tensor select."""
    L, a = N.lib(), N.i64_array
    nseg, seg_len = (c, r) if mode == "column" else (r, c)
    numels, ks = a([seg_len] * nseg), a([k] * nseg)
    offs, koff = a([s * seg_len for s in range(nseg)]), a([s * k for s in range(nseg)])
    nb = int(L.arctopk_sparse_workspace_bytes(nseg, numels))
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    idx = torch.empty(nseg * k, dtype=torch.int32, device=DEV)
    vals = torch.empty(nseg * k, dtype=dtype, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    dt = N.DTYPE_CODE[dtype]
    x2 = x.view(r, c)

    def run():
        src = x2.t().contiguous() if mode == "column" else x2
        if random:
            N.check(L.arctopk_randk_select(src.data_ptr(), nseg, offs, numels, ks, koff, 12345, idx.data_ptr(),
                                           vals.data_ptr(), ws.data_ptr(), dt, 0, st), "arctopk_randk_select")
        else:
            N.check(L.arctopk_topk_select(src.data_ptr(), nseg, offs, numels, ks, koff, idx.data_ptr(),
                                          vals.data_ptr(), ws.data_ptr(), dt, 0, st), "arctopk_topk_select")
    return run


def make_torch(x, r, c, k, mode):
    x2 = x.view(r, c)
    dim = 0 if mode == "column" else 1

    def run():
        _, i = torch.topk(x2.abs(), k, dim=dim, sorted=False)
        torch.gather(x2, dim, i)
    return run


def make_hook(x, shape, ratio, mode, random):
    st = sparse_hook.SparseState(None, compress_ratio=ratio, start_compress_iter=0, sparse_type=mode,
                                 random=random, use_error_feedback="ef14", index_source="hash")
    g = x.clone()

    def run():
        sparse_hook.sparse_hook_sync(st, SyntheticBucket(g, [shape])).wait()
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "rowcol", "select_table.txt"))
    ap.add_argument("--only", default="", help="comma list of shape indices")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rowcol.py needs a GPU")
    from parity import ensure_group
    ensure_group("nccl")
    only = {int(v) for v in args.only.split(",") if v}
    lines = ["# us per call: median (min..max) over %d windows of %d calls; new = arctopk_seg_select; "
             "(a) = per-segment tensors through the per-tensor select; (b) = torch.topk + gather; "
             "hook = sparse_hook_sync, EF14, world size 1; GB/s and %% of 8 TB/s: algorithmic bytes "
             "(tensor read + payload write) over new" % (args.repeats, args.calls),
             "%-18s %-5s %-6s %-6s %5s | %-24s | %-26s | %-24s | %-24s | %7s %6s | %s" %
             ("shape", "dtype", "kind", "mode", "ratio", "new", "(a)", "(b)", "hook", "GB/s", "%HBM", "new vs")]
    for si, (shape, dtype) in enumerate(SHAPES):
        if only and si not in only:
            continue
        r, c = view(shape)
        x = torch.randn(r * c, generator=torch.Generator().manual_seed(si)).to(dtype).to(DEV)
        for kind, mode in VARIANTS:
            for ratio in RATIOS:
                seg_len, nseg = (r, c) if mode == "column" else (c, r)
                k = max(1, int(seg_len * ratio))
                random = kind == "randk"
                fns = {"new": make_new(x, r, c, k, mode, random, dtype),
                       "a": make_old(x, r, c, k, mode, random, dtype),
                       "hook": make_hook(x, shape, ratio, mode, random)}
                if not random:
                    fns["b"] = make_torch(x, r, c, k, mode)
                for fn in fns.values():  # warm-up of every variant at this shape
                    timed(fn, 3)
                t = {name: [] for name in fns}
                for _ in range(args.repeats):
                    for name, fn in fns.items():
                        t[name].append(timed(fn, args.calls))

                def cell(name):
                    if name not in t:
                        return "n/a"
                    v = t[name]
                    return "%.1f (%.1f..%.1f)" % (statistics.median(v), min(v), max(v))
                esz = x.element_size()
                nbytes = r * c * esz + nseg * k * (4 + esz)
                new = statistics.median(t["new"])
                gbs = nbytes / (new * 1e-6) / 1e9
                verdict = []
                for name in ("a", "b"):
                    if name in t:
                        faster = max(t["new"]) < min(t[name])
                        verdict.append("%s: %s %.1fx" % (name, "faster" if faster else "NOT faster",
                                                         statistics.median(t[name]) / new))
                lines.append("%-18s %-5s %-6s %-6s %5.2f | %-24s | %-26s | %-24s | %-24s | %7.1f %5.1f%% | %s" %
                             (str(shape), "bf16" if dtype == torch.bfloat16 else "fp32", kind, mode, ratio,
                              cell("new"), cell("a"), cell("b"), cell("hook"), gbs, 100.0 * nbytes /
                              (new * 1e-6) / HBM_PEAK, "; ".join(verdict)))
                print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
