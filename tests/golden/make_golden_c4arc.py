"""Generate the golden vectors of the c4 ARC-TopK hook (tests/golden/c4arc_*.npz).

RUNS ONLY IN THE BUILD CONTAINER, like make_golden.py (whose bucket, gradients and capture it
uses): it imports the reference's comm_hooks/group_topk_hook_no_reshape_c4.py from
``/root/reference`` and drives it on CPU over a gloo group of 1 or 2 ranks.  Only the data
written next to this script travels (inputs and expected outputs; no reference source).

Captured per bucket call: make_golden.py's keys out, bits, iter_after, seed and topk_j (the
norms on rank 0 only: they are the same on every rank), ``V_t`` -- the projection of every 2-D /
ND tensor, drawn by ``V.normal_(...)`` (:37-39, :75-77) -- and ``ratio`` -- the compress ratio in
force during the call (``get_current_compress_ratio()`` as the hook read it, :261; -1 for a dense
warm-up call).  To keep every file below 1 MiB the gradient G and the residuals E / gE are pinned
by their SHA-256 (``G_sha``, ``E_sha``, ``gE_sha``: tests/arc_c4_oracle.py's ``digest``) -- G is
make_golden.make_grad's seeded randn, restated as ``arc_c4_oracle.bucket_grad`` -- and E / gE are
stored in full after the last call only (gE never: an EF21 call returns it as ``out``); ``out``
is stored for rank 0 and pinned by ``out_sha`` on every rank; the all-reduce results are not stored.

Every top-k threshold of the fp32 cases must have a relative gap of at least 1e-4 between the
k-th and the (k+1)-th energy (asserted here): the condition under which the GPU's rows must
equal the reference's exactly (its sketch sums differ from CPU sgemm's by ~4e-7 relative).

Also writes c4arc_ef21_1d_error.json: how the reference fails with EF21 and a 1-D tensor, and
c4arc_ratio_schedule.json: the reference state's ``get_current_compress_ratio()`` and ``cal_k`` per
iteration at warmup_iters 0, 1 and 2 (start 1, ratio 0.2), before and after compression starts.

Usage:  python tests/golden/make_golden_c4arc.py   (writes tests/golden/c4arc_*)
"""
from __future__ import annotations

import json
import os
import sys
import tempfile
from contextlib import contextmanager

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))  # tests/: arc_c4_oracle

import make_golden as MG  # noqa: E402
from make_golden import GMIX, REFERENCE, SyntheticBucket, _np, free_port, make_grad  # noqa: E402
from arc_c4_oracle import bucket_grad, digest  # noqa: E402

G2D = [s for s in GMIX if len(s) > 1]  # GMIX without its 1-D tensors

MIN_GAP = 1e-4

CASES = [
    dict(name="c4arc_gmix_noef_ws1", shapes=GMIX, ef="noef", ws=1, warmup=2, iters=6),
    dict(name="c4arc_gmix_ef14_ws1", shapes=GMIX, ef="ef14", ws=1, warmup=2, iters=6),
    dict(name="c4arc_g2d_ef21_ws1", shapes=G2D, ef="ef21", ws=1, warmup=2, iters=6),
    dict(name="c4arc_gmix_ef14_ws2", shapes=GMIX, ef="ef14", ws=2, warmup=1, iters=5),
    dict(name="c4arc_g2d_ef21_ws2", shapes=G2D, ef="ef21", ws=2, warmup=1, iters=5),
    dict(name="c4arc_gmix_noef_bf16_ws1", shapes=GMIX, ef="noef", ws=1, warmup=2, iters=6, dtype="bf16"),
]
for c in CASES:
    c.update(hook="arc_c4", ratio=0.2, r=4, start=1, seed=4321)


@contextmanager
def capture_normal(rec):
    """The projections: V.normal_(generator=g) / V.normal_() on a fresh torch.empty(m, r)."""
    orig = torch.Tensor.normal_

    def normal_(self, *a, **k):
        out = orig(self, *a, **k)
        if self.dim() == 2:
            rec.setdefault("V", []).append(self.detach().clone())
        return out

    torch.Tensor.normal_ = normal_
    try:
        yield rec
    finally:
        torch.Tensor.normal_ = orig


def make_state(case):
    from comm_hooks.group_topk_hook_no_reshape_c4 import GroupTopKState, group_topk_hook
    st = GroupTopKState(process_group=None, r=case["r"], compress_ratio=case["ratio"],
                        start_compress_iter=case["start"], use_error_feedback=case["ef"], seed=case["seed"],
                        gradual_compression=True, warmup_iters=case["warmup"])
    return st, group_topk_hook


def run_rank(rank, ws, case, port, outdir):
    sys.path.insert(0, REFERENCE)
    os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
    sys.dont_write_bytecode = True
    torch.set_num_threads(max(1, 8 // ws))
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=ws)
    state, hook = make_state(case)
    ratios = []
    orig_ratio = state.get_current_compress_ratio
    state.get_current_compress_ratio = lambda: ratios.append(orig_ratio()) or ratios[-1]
    arrays = {}
    min_gap = float("inf")
    for it in range(case["iters"]):
        G = make_grad(case, it, rank)
        bucket = SyntheticBucket(G.clone(), case["shapes"], index=0, is_last=True)
        rec = {}
        del ratios[:]
        with MG.capture(rec), capture_normal(rec):
            out = hook(state, bucket).wait()
        p = f"it{it}_"
        assert torch.equal(G, bucket_grad(G.numel(), it, rank, G.dtype)), "bucket_grad restates make_grad"
        last = it == case["iters"] - 1
        arrays[p + "G_sha"] = np.array(digest(G))
        arrays[p + "out_sha"] = np.array(digest(out))
        if rank == 0:
            arrays[p + "out"] = _np(out.clone())
        for key, table in (("E", state.error_dict), ("gE", state.global_error_dict)):
            if 0 in table:
                arrays[p + key + "_sha"] = np.array(digest(table[0]))
                if last and key == "E":
                    arrays[p + key] = _np(table[0].clone())
        arrays[p + "bits"] = np.array(int(state.comm_bits_this_round), dtype=np.int64)
        arrays[p + "iter_after"] = np.array(int(state.iter), dtype=np.int64)
        arrays[p + "ratio"] = np.array(ratios[0] if ratios else -1.0, dtype=np.float64)
        assert len(set(ratios)) <= 1, "one ratio per call"
        if "seed" in rec:
            arrays[p + "seed"] = np.array(rec["seed"], dtype=np.int64)
        for j, v in enumerate(rec.get("V", [])):
            arrays[p + f"V{j}"] = _np(v)
        for j, (inp, k, idx) in enumerate(rec.get("topk", [])):
            if rank == 0:
                arrays[p + f"topk{j}_in"] = _np(inp)
            arrays[p + f"topk{j}_k"] = np.array(k, dtype=np.int64)
            arrays[p + f"topk{j}_idx"] = idx.numpy()
            if case.get("dtype") != "bf16" and k < inp.numel():
                top = torch.sort(inp.double(), descending=True).values
                min_gap = min(min_gap, float((top[k - 1] - top[k]) / top[k - 1]))
    assert min_gap >= MIN_GAP, f"{case['name']}: top-k threshold gap {min_gap:.3g} < {MIN_GAP}: pick other seeds"
    arrays["min_gap"] = np.array(min_gap, dtype=np.float64)
    np.savez(os.path.join(outdir, f"rank{rank}.npz"), **arrays)
    dist.barrier()
    dist.destroy_process_group()


def ef21_1d_error(rank, port, outdir):
    """EF21 with a 1-D tensor in the bucket: the first compressed call after the EF21 init."""
    sys.path.insert(0, REFERENCE)
    sys.dont_write_bytecode = True
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    case = dict(CASES[0], ef="ef21", start=0)
    state, hook = make_state(case)
    res = dict(raises="no-error", call=None)
    for it in range(2):
        bucket = SyntheticBucket(make_grad(case, it, 0), case["shapes"], index=0, is_last=True)
        try:
            hook(state, bucket).wait()
        except Exception as e:  # noqa: BLE001 -- recorded as the reference's behaviour
            res = dict(raises=type(e).__name__, message=str(e), call=it)
            break
    res["iter_after"] = int(state.iter)
    with open(os.path.join(outdir, "err.json"), "w") as f:
        json.dump(res, f)
    dist.destroy_process_group()


SCHEDULE_SHAPES = [[7], [40, 16], [16, 8, 3, 3], [16, 8, 1, 1], [96, 40]]


def ratio_schedule():
    """The state's schedule alone (no hook call): ratio and cal_k per iteration."""
    sys.path.insert(0, REFERENCE)
    sys.dont_write_bytecode = True
    from comm_hooks.group_topk_hook_no_reshape_c4 import cal_k
    out = []
    for warmup in (0, 1, 2):
        st, _ = make_state(dict(CASES[0], warmup=warmup))
        rows = []
        for started in (False, True):
            st.compression_started = started
            for it in range(0, 8):
                st.iter = it
                rows.append(dict(started=started, iter=it, ratio=st.get_current_compress_ratio(),
                                 cal_k=[int(cal_k(st, torch.empty(s))) for s in SCHEDULE_SHAPES]))
        out.append(dict(warmup_iters=warmup, start=CASES[0]["start"], ratio=CASES[0]["ratio"],
                        warmup_field=int(st.warmup_iters), calls=rows))
    return out


def main():
    meta_common = dict(torch=torch.__version__, cpu_capability=torch.backends.cpu.get_cpu_capability(),
                       reference="Aris-ma/AllreduceTopK @ /root/reference (read-only)")
    only = set(sys.argv[1:])
    for case in CASES:
        if only and case["name"] not in only:
            continue
        with tempfile.TemporaryDirectory() as td:
            mp.spawn(run_rank, args=(case["ws"], case, free_port(), td), nprocs=case["ws"], join=True)
            merged = {}
            for rk in range(case["ws"]):
                with np.load(os.path.join(td, f"rank{rk}.npz")) as z:
                    for k in z.files:
                        merged[f"r{rk}_{k}"] = z[k]
        merged["meta"] = np.array(json.dumps(dict(meta_common, **case)))
        path = os.path.join(HERE, case["name"] + ".npz")
        np.savez_compressed(path, **merged)
        assert os.path.getsize(path) < (1 << 20), f"{path}: {os.path.getsize(path)} bytes"
        print("wrote", case["name"], os.path.getsize(path), "bytes, min gap", float(merged["r0_min_gap"]))
    if not only or "c4arc_ratio_schedule" in only:
        with open(os.path.join(HERE, "c4arc_ratio_schedule.json"), "w") as f:
            json.dump(dict(meta_common, shapes=SCHEDULE_SHAPES, schedules=ratio_schedule()), f, indent=1)
    if not only:
        with tempfile.TemporaryDirectory() as td:
            mp.spawn(ef21_1d_error, args=(free_port(), td), nprocs=1, join=True)
            with open(os.path.join(td, "err.json")) as f:
                res = json.load(f)
        with open(os.path.join(HERE, "c4arc_ef21_1d_error.json"), "w") as f:
            json.dump(dict(meta_common, shapes=GMIX, ef="ef21", **res), f, indent=1)


if __name__ == "__main__":
    main()
