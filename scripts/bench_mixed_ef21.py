#!/usr/bin/env python3
"""EF21 with both residuals in fp32 under a bf16 bucket (GroupTopKState.ef21_error_dtype =
torch.float32) on one GPU, against the bf16-residual path it is an option
beside, in one process, interleaved: the method of scripts/bench_mixed_ef.py.

Kernels: arctopk_encode / arctopk_pack / arctopk_decode (bf16, EF21) against arctopk_encode_mixed21 /
arctopk_pack_mixed21 / arctopk_decode_mixed21, each call between two of the library's device-scope
timed events, four disjoint sets of bucket and residuals in rotation (no call finds its data in the
Infinity Cache).  Per repetition: --warmup calls, then the median of --calls calls; the two
alternate, --repeats repetitions each; the table gives the median and the min..max of the
repetitions' medians.  Bytes are algorithmic, per element e of the phase's pass and per selected
element s: encode 4 e (read G, E) against 6 e; pack 8 s (read G, E; write packed, E) against 12 s;
decode 4 e + 4 s (read gE, write out; read packed, write gE) against 6 e + 6 s.  With --stream FILE
(the output of scripts/stream_mixed21, cold) the new kernels' GB/s are also given as a share of a
plain stream of the same bytes: r6 for the encode, rw12 for the pack, and for the decode the time
r4w2 needs for the unselected elements plus rw12's for the selected ones.

Whole call: group_topk_hook (EF21, r 4, world size 1) on bf16 buckets, a state with the option
against a default one (one-call step, deferred decodes), a call being one backward of four
buckets; reported as the option's cost.

    python scripts/bench_mixed_ef21.py --stream profiles/mixed_ef21/stream_mixed21.txt --out profiles/mixed_ef21/table.txt
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
sys.path.insert(0, os.path.join(REPO, "scripts"))

from allreducetopk_amd import _native as N  # noqa: E402
from allreducetopk_amd.bucket import SyntheticBucket, bucket_numel  # noqa: E402
from allreducetopk_amd.comm_hooks import group_topk_hook_no_reshape as G  # noqa: E402
from allreducetopk_amd.comm_hooks import group_topk_hook_no_reshape_c4 as G4  # noqa: E402
from bench_mixed_ef import DEV, LOADS, SETS, ab, cell  # noqa: E402

BF16 = torch.bfloat16


def stream_rates(path):
    """{pattern: best GB/s} of a scripts/stream_mixed21 output, or {}."""
    if not path or not os.path.exists(path):
        return {}
    best = {}
    with open(path) as fh:
        for name, rate in re.findall(r"^(\w+)\s+cold grid\s+\d+:\s+(\d+) GB/s", fh.read(), re.M):
            best[name] = max(best.get(name, 0.0), float(rate))
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--loads", default=",".join(LOADS))
    ap.add_argument("--stream", default=None, help="output of scripts/stream_mixed21 (the plain-stream ceilings)")
    ap.add_argument("--no-hook", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mixed_ef21", "table.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mixed_ef21.py needs a GPU")
    from parity import ensure_group
    ensure_group("nccl")
    L = N.lib()
    rates = stream_rates(args.stream)
    gen = torch.Generator(device=DEV).manual_seed(1000)
    sid = torch.cuda.current_stream().cuda_stream
    lines = ["# library: %s; us per call: median (min..max) of %d repetitions' medians of %d calls after %d warm-ups, "
             "the two kernels (states) alternating; %d disjoint sets of bucket and residuals in rotation; GB/s: "
             "algorithmic bytes / median; plain streams, cold, GB/s: %s"
             % (L.arctopk_version().decode(), args.repeats, args.calls, args.warmup, SETS,
                ", ".join("%s %.0f" % kv for kv in sorted(rates.items())) or "not measured"),
             "%-7s %-15s | %-24s %7s | %-24s %7s %9s | %s" %
             ("what", "workload", "bf16 residuals (today)", "GB/s", "fp32 residuals (option)", "GB/s", "of stream", "time x")]
    for name in [w for w in args.loads.split(",") if w]:
        shapes, ratio, flags, c4 = LOADS[name]
        n = bucket_numel(shapes)
        plan = G.BucketPlan([tuple(s) for s in shapes], 4, ratio, BF16, DEV, flags)
        Gs = [torch.randn(n, device=DEV, generator=gen).to(BF16) for _ in range(SETS)]
        E16 = [(torch.randn(n, device=DEV, generator=gen) * 0.1).to(BF16) for _ in range(SETS)]
        g16 = [(torch.randn(n, device=DEV, generator=gen) * 0.1).to(BF16) for _ in range(SETS)]
        E32 = [torch.randn(n, device=DEV, generator=gen) * 0.1 for _ in range(SETS)]
        g32 = [torch.randn(n, device=DEV, generator=gen) * 0.1 for _ in range(SETS)]
        V = plan.V_ring[0]
        N.check(L.arctopk_draw_projections(plan.handle, 7, V.data_ptr(), sid), "draw")
        sk, rl, sm, pk = plan.sketch.data_ptr(), plan.rowlist.data_ptr(), plan.slotmap.data_ptr(), plan.packed.data_ptr()

        def enc16(i):
            N.check(L.arctopk_encode(plan.handle, Gs[i % SETS].data_ptr(), E16[i % SETS].data_ptr(), N.EF21, 1,
                                     V.data_ptr(), sk, sid), "arctopk_encode")

        def enc32(i):
            N.check(L.arctopk_encode_mixed21(plan.handle, Gs[i % SETS].data_ptr(), E32[i % SETS].data_ptr(),
                                             V.data_ptr(), sk, sid), "arctopk_encode_mixed21")

        def pack16(i):
            N.check(L.arctopk_pack(plan.handle, Gs[i % SETS].data_ptr(), E16[i % SETS].data_ptr(), N.EF21, rl, sm,
                                   pk, sid), "arctopk_pack")

        def pack32(i):
            N.check(L.arctopk_pack_mixed21(plan.handle, Gs[i % SETS].data_ptr(), E32[i % SETS].data_ptr(), rl, sm,
                                           pk, sid), "arctopk_pack_mixed21")

        def dec16(i):  # (the bucket itself is the output, as in the hook)
            N.check(L.arctopk_decode(plan.handle, pk, sm, 1, N.EF21, g16[i % SETS].data_ptr(),
                                     Gs[i % SETS].data_ptr(), sid), "arctopk_decode")

        def dec32(i):
            N.check(L.arctopk_decode_mixed21(plan.handle, pk, sm, 1, g32[i % SETS].data_ptr(),
                                             Gs[i % SETS].data_ptr(), sid), "arctopk_decode_mixed21")

        enc_el = sum(s.n * s.m for s in plan.segments if s.kind != N.SEG_DENSE)  # (DENSE: no encode work)
        sel = int(plan.info.values_len)
        t = ab({"a": enc16, "b": enc32}, args)
        rows = [("encode", t, enc_el * 4, enc_el * 6, enc_el * 6 / rates["r6"] if "r6" in rates else None)]
        enc32(0)
        plan.select(1, sid)  # the rows the packs gather and the decodes scatter
        torch.cuda.synchronize()
        t = ab({"a": pack16, "b": pack32}, args)
        rows.append(("pack", t, sel * 8, sel * 12, sel * 12 / rates["rw12"] if "rw12" in rates else None))
        pack16(0)  # (the bf16 decode reads what the plan's last pack left for it)
        t = ab({"a": dec16, "b": dec32}, args)
        floor = ((n - sel) * 6 / rates["r4w2"] + sel * 12 / rates["rw12"]) if {"r4w2", "rw12"} <= set(rates) else None
        rows.append(("decode", t, n * 4 + sel * 4, n * 6 + sel * 6, floor))
        for what, t, b16, b32, floor in rows:
            ma, mb = statistics.median(t["a"]), statistics.median(t["b"])
            share = "%8.0f%%" % (100.0 * floor / 1e3 / mb) if floor else "        -"  # (bytes / (GB/s) / 1e3 = us)
            lines.append("%-7s %-15s | %-24s %7.0f | %-24s %7.0f %9s | %.2f" %
                         (what, name, cell(t["a"]), b16 / ma / 1e3, cell(t["b"]), b32 / mb / 1e3, share, mb / ma))
            print(lines[-1], flush=True)
        del plan, Gs, E16, E32, g16, g32, enc16, enc32, pack16, pack32, dec16, dec32
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
                                        use_error_feedback="ef21", seed=1234, **kw)
                st.defer_decode = True  # the step waits every Future after the last bucket, as DDP's finalize does
                st.ef21_error_dtype = torch.float32 if k == "b" else None
                states[k] = st
                buckets[k] = [SyntheticBucket(torch.randn(n, device=DEV, generator=gen).to(BF16), shapes, index=i,
                                              is_last=(i == 3)) for i in range(4)]

            def step(k):
                def fn(i, st=states[k], bks=buckets[k]):  # (the first call of a state is EF21's dense one: a warm-up)
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
