"""Which native calls and collectives the TopK / RandK hooks make, on the CPU (sparse_hook_rig): the
call table of sparse_hook's docstring restated per variant -- the sequence of names and, per call,
``ef``, ``err_in``, the dtype code, the zero flag, ``nranks``, ``world_size``, ``accumulate``, which
pointer is which buffer (or NULL), the int64 arrays and the collectives -- and what a call leaves in
the state.  The expectations are written from the table, not from a recorded run.

(What the kernels compute: tests/test_gpu_sparse*.py, tests/test_gpu_rowcol.py.)"""
import pytest
import torch

import sparse_hook_rig as R
from allreducetopk_amd import _native as N

TOTAL = 5 + 16 * 64 + 3 * 7 + 8 * 4 * 3 * 3
NUMELS = [5, 1024, 21, 288]
OFFSETS = [0, 5, 1029, 1050]
VIEWS = [(1, 5), (16, 64), (3, 7), (8, 36)]  # [rows, cols]: 1-D is one row, N-D is [shape[0], rest]


def layout(sparse_type, ratio):
    """ks, k offsets and (row / column) rows, cols, k_seg of the rig's bucket."""
    rows = cols = k_seg = None
    if sparse_type == "tensor":
        ks = [max(1, int(n * ratio)) for n in NUMELS]
    else:
        col = sparse_type == "column"
        views = [(c, r) if col and r == 1 else (r, c) for r, c in VIEWS]  # a 1-D tensor is one column of n rows
        rows, cols = [r for r, _ in views], [c for _, c in views]
        k_seg = [max(1, int((r if col else c) * ratio)) for r, c in views]
        ks = [k * (c if col else r) for k, (r, c) in zip(k_seg, views)]
    k_off = [sum(ks[:i]) for i in range(len(ks))]
    return ks, k_off, rows, cols, k_seg


def expected(kind, source, ef, sparse_type, variant, ws, call, ratio=R.RATIO):
    """(calls and collectives in order, each a name and the fields that must match; bits the call
    adds; whether it is EF21's dense first call)."""
    random, hashed = kind == "randk", source == "hash"
    refdraw = random and not hashed
    seg, by_col = sparse_type != "tensor", sparse_type == "column"
    f32 = variant.startswith("fp32")
    dt = N.F32 if f32 else N.BF16
    mixed = variant == "bf16+error_dtype" and ef != "noef"
    wire16 = variant == "fp32+wire_dtype"
    efc = N.EF_CODE[ef]
    ks, k_off, rows, cols, k_seg = layout(sparse_type, ratio)
    sum_k = sum(ks)
    lay = dict(ntensors=4, offsets=OFFSETS, ks=ks, k_off=k_off)
    # the shared reseed: one draw from the state's generator (seed 7) per compressed RandK call
    g = torch.Generator().manual_seed(7)
    seed = [int(torch.randint(0, 1_000_000_000, (1,), generator=g)) for _ in range(call + 1)][call - (ef == "ef21")]
    E, gE = "error_dict[b]", "global_error_dict[b]"
    if ef == "ef21" and call == 0:  # the dense call: no native call, one all-reduce at any world size
        return [("all_reduce", dict(dtype="f32" if f32 else "bf16", numel=TOTAL, buf="bucket"))], 0, True

    seq = []
    # ---- the EF pre-apply
    select_folds = not seg and ef == "ef14" and not mixed and (hashed if random else f32)
    if mixed:
        seq.append(("arctopk_sparse_fold_mixed", dict(g="bucket", E=E, D="scratch" if ef == "ef21" else "NULL",
                                                      numel=TOTAL, ef=efc, err_in=call if ef == "ef14" else 1)))
    elif ef == "ef14" and not select_folds:
        seq.append(("arctopk_ef14_fold", dict(x="bucket", E=E, numel=TOTAL, err_in=call, dtype=dt)))
    elif ef == "ef21":
        seq.append(("arctopk_ef_apply", dict(x="bucket", E=E, numel=TOTAL, ef=N.EF21, err_in=1, dtype=dt)))
    # ---- select or draw: where the pre-compression bucket lives, and the select's own values
    src = ("scratch" if ef == "ef21" else E) if mixed else E if ef == "ef14" else "bucket"
    sel_dt = N.F32 if mixed else dt
    zero = int(ef == "ef14" and not mixed)
    idx = f"indices.i32[{sum_k}]"
    sel_vals = f"values.{'f32' if f32 or mixed else 'bf16'}[{sum_k}]"
    if refdraw:
        if not mixed:  # the draws are torch's; then the gather
            seq.append(("arctopk_sparse_gather", dict(x=src, idx=idx, vals=sel_vals, dtype=dt, **lay)))
    elif seg:
        seq.append(("arctopk_seg_select", dict(x=src, ntensors=4, offsets=OFFSETS, rows=rows, cols=cols, k_seg=k_seg,
                                               k_off=k_off, by_column=int(by_col), hashed=int(hashed),
                                               seed=seed if hashed else 0, idx=idx,
                                               vals=sel_vals, workspace="workspace", dtype=sel_dt,
                                               zero_selected=zero)))
    elif mixed and hashed:  # indices only
        seq.append(("arctopk_randk_select", dict(x="NULL", offsets="NULL", numels=NUMELS, ks=ks, k_off=k_off, seed=seed,
                                                 idx=idx,
                                                 vals="NULL", workspace="workspace", dtype=N.F32, zero_selected=0)))
    elif select_folds:
        name = "arctopk_randk_select_ef14" if random else "arctopk_topk_select_ef14"
        seq.append((name, dict(g="bucket", E=E, err_in=call, numels=NUMELS, idx=idx, vals=sel_vals,
                               workspace="workspace", dtype=dt, **({"seed": seed} if random else {}), **lay)))
    else:
        name = "arctopk_randk_select" if random else "arctopk_topk_select"
        seq.append((name, dict(x=src, numels=NUMELS, idx=idx, vals=sel_vals, workspace="workspace", dtype=sel_dt,
                               zero_selected=zero, **({"seed": seed} if random else {}), **lay)))
    # ---- pack or residual
    wire_vals, vbits = sel_vals, 32 if f32 else 16
    if wire16:
        wire_vals, vbits = f"values.bf16[{sum_k}]", 16
        seq.append(("arctopk_sparse_pack_wire16", dict(values=sel_vals, E="NULL" if ef == "noef" else E, numel=TOTAL,
                                                       idx=idx, vals16=wire_vals, ef=efc, decay=R.DECAY, **lay)))
    elif mixed:
        wire_vals = f"values.bf16[{sum_k}]"
        seq.append(("arctopk_sparse_pack_mixed", dict(src=src, E=E, numel=TOTAL, idx=idx, vals=wire_vals, ef=efc,
                                                      decay=R.DECAY, **lay)))
    elif ef == "ef21" or (ef == "ef14" and refdraw):  # EF14's E[idx] = 0 is the select's otherwise
        seq.append(("arctopk_sparse_residual", dict(E=E, idx=idx, vals=sel_vals, ef=efc, decay=R.DECAY, dtype=dt,
                                                    **lay)))
    # ---- exchange
    wdt = wire_vals.split(".")[1].split("[")[0]
    dec_idx, dec_vals = idx, wire_vals
    if random:
        bits = 2 * (ws - 1) * sum_k * vbits
        if ws > 1:
            seq.append(("all_reduce", dict(dtype=wdt, numel=sum_k, buf=wire_vals)))
        nranks, accumulate = 1, 2 if hashed and not by_col else 0
    else:
        bits = (ws - 1) * ws * sum_k * (vbits + 32)
        if ws > 1:
            seq.append(("all_gather", dict(dtype=wdt, numel=sum_k, out_numel=ws * sum_k, buf=wire_vals)))
            seq.append(("all_gather", dict(dtype="i32", numel=sum_k, out_numel=ws * sum_k, buf=idx)))
            dec_idx, dec_vals = f"indices.i32[{ws * sum_k}]", f"values.{wdt}[{ws * sum_k}]"
        nranks, accumulate = ws, 3 if by_col else 1
    # ---- decode
    dec = dict(out="bucket", numel=TOTAL, packed_len=sum_k, idx=dec_idx, nranks=nranks, world_size=ws,
               decay=R.DECAY, **lay)
    if wire16:
        seq.append(("arctopk_sparse_decode_wire16", dict(vals16=dec_vals, accumulate=accumulate,
                                                         gE=gE if ef == "ef21" else "NULL", **dec)))
    elif mixed and ef == "ef21":
        seq.append(("arctopk_sparse_decode_mixed21", dict(vals=dec_vals, gE=gE, scratch="scratch", **dec)))
    else:
        seq.append(("arctopk_sparse_decode", dict(vals=dec_vals, accumulate=accumulate, dtype=dt,
                                                  gerr=gE if ef == "ef21" and not mixed else "NULL", **dec)))
    return seq, bits, False


def check_trace(trace, seq, where):
    """The recorded calls are ``seq``: same names in the same order, every stated field equal.  The
    two *_workspace_bytes queries are cached per layout, so they may or may not appear."""
    got = [t for t in trace if not t.get("call", "").endswith("_workspace_bytes") and "state" not in t]
    names = [t.get("call") or t.get("coll") or "raised" for t in got]
    assert names == [n for n, _ in seq], where
    for t, (name, fields) in zip(got, seq):
        for key, want in fields.items():
            assert t[key] == want, f"{where}: {name}.{key} is {t[key]!r}, not {want!r}"
        if "stream" in t:
            assert t["stream"] == "stream", f"{where}: {name}"
        assert "unknown" not in t.values(), f"{where}: {name} got a pointer that is no buffer of the call: {t}"


def check_state(snap, prev, kind, ef, variant, bits, dense, ks, where, count_bits=True):
    f32 = variant.startswith("fp32")
    mixed = variant == "bf16+error_dtype" and ef != "noef"
    assert snap["iter"] == prev["iter"] + 1, where
    assert snap["comm_bits_this_round"] == prev["comm_bits_this_round"] + (bits if count_bits else 0), where
    assert snap["mixed_calls"] == prev["mixed_calls"] + int(mixed and not dense), where
    assert snap["wire16_calls"] == prev["wire16_calls"] + int(variant == "fp32+wire_dtype" and not dense), where
    if not dense:
        assert snap["last_k"] == ks, where
    res = "f32" if f32 or mixed else "bf16"
    assert snap["error_dtype"] == ({} if ef == "noef" else {0: res}), where
    assert snap["global_error_dtype"] == ({0: res} if ef == "ef21" else {}), where
    assert snap["mixed_buckets"] == ([0] if mixed else []), where
    # one draw from state.rng per compressed RandK call (the shared reseed), none otherwise; the CPU
    # generator is reseeded then, and "torch" (on CPU tensors) and "host" draw from it
    assert (snap["state_rng"] != prev["state_rng"]) == (kind == "randk" and not dense), where
    assert (snap["cpu_rng"] != prev["cpu_rng"]) == (kind == "randk" and not dense), where


def _fresh(case):
    st = R.make_state(case["kind"], case["source"], case["ef"], case["sparse_type"], case["variant"], case["ws"],
                      c4=case.get("c4", False))
    torch.manual_seed(1234)
    return R.snapshot(st)


MATRIX = [(cid, kw) for cid, kw in R.matrix() if not cid.startswith(("large_batch", "c4"))]


@pytest.mark.parametrize("cid,case", MATRIX, ids=[cid for cid, _ in MATRIX])
def test_matrix(cid, case):
    traces = R.run_case(**case)
    prev = _fresh(case)
    for call, trace in enumerate(traces):
        seq, bits, dense = expected(call=call, **case)
        where = f"{cid} call {call}"
        check_trace(trace, seq, where)
        snap = trace[-1]["state"]
        check_state(snap, prev, case["kind"], case["ef"], case["variant"], bits, dense,
                    layout(case["sparse_type"], R.RATIO)[0], where)
        prev = snap


def test_the_torch_and_host_draws_differ_only_in_where_they_are_made():
    """On CPU tensors "torch" and "host" draw from the same generator in the same order: the whole
    trace, generator states included, is the same."""
    for sp in R.SPARSE_TYPES:
        a = R.run_case("randk", "torch", "ef14", sp, "fp32", 1)
        b = R.run_case("randk", "host", "ef14", sp, "fp32", 1)
        assert a == b, sp


C4 = [(cid, kw) for cid, kw in R.matrix() if cid.startswith("c4")]


@pytest.mark.parametrize("cid,case", C4, ids=[cid for cid, _ in C4])
def test_c4_state_selects_at_the_ramp_ratio(cid, case):
    """The c4 state: the same calls, with every call's layout at that call's ratio (0.8 at the
    first compressed call, one step of 0.55 / 100 down at the second)."""
    traces = R.run_case(**case)
    prev = _fresh(case)
    kw = {k: v for k, v in case.items() if k != "c4"}
    for call, trace in enumerate(traces):
        ratio = 0.8 - (0.8 - R.RATIO) * (call / 100)
        seq, bits, dense = expected(call=call, ratio=ratio, **kw)
        check_trace(trace, seq, f"{cid} call {call}")
        snap = trace[-1]["state"]
        check_state(snap, prev, kw["kind"], kw["ef"], kw["variant"], bits, dense,
                    layout(kw["sparse_type"], ratio)[0], f"{cid} call {call}")
        prev = snap
    assert layout("row", 0.8)[0] != layout("row", R.RATIO)[0]


def test_large_batch_init():
    """The large-batch EF21 hook (start_compress_iter 2): TypeError at iteration 0, a dense
    accumulating call, then compressed calls at ``compress_ratio`` with alpha 1 in the residual,
    ``error_decay`` in the decode, no bits counted and the values handed to the diff log."""
    (cid, case), = [(c, k) for c, k in R.matrix() if c.startswith("large_batch")]
    t0, t1, t2, t3 = R.run_case(**case)
    assert [t.get("raised") for t in t0[:-1]] == ["TypeError"] and t0[-1]["state"]["iter"] == 1
    check_trace(t1, [("all_reduce", dict(dtype="bf16", numel=TOTAL, buf="bucket"))], "warm-up")
    assert t1[-1]["state"]["iter"] == 2 and t1[-1]["state"]["error_dtype"] == {0: "bf16"}
    ks, k_off, *_ = layout("tensor", R.RATIO)
    sum_k = sum(ks)
    lay = dict(ntensors=4, offsets=OFFSETS, ks=ks, k_off=k_off)
    idx, vals = f"indices.i32[{sum_k}]", f"values.bf16[{sum_k}]"
    seq = [("arctopk_ef_apply", dict(x="bucket", E="error_dict[b]", numel=TOTAL, ef=N.EF21, err_in=1, dtype=N.BF16)),
           ("arctopk_topk_select", dict(x="bucket", numels=NUMELS, idx=idx, vals=vals, workspace="workspace",
                                        dtype=N.BF16, zero_selected=0, **lay)),
           ("arctopk_sparse_residual", dict(E="error_dict[b]", idx=idx, vals=vals, ef=N.EF21, decay=1.0,
                                            dtype=N.BF16, **lay)),
           ("all_gather", dict(dtype="bf16", numel=sum_k, out_numel=2 * sum_k, buf=vals)),
           ("all_gather", dict(dtype="i32", numel=sum_k, out_numel=2 * sum_k, buf=idx)),
           ("arctopk_sparse_decode", dict(out="bucket", numel=TOTAL, packed_len=sum_k, idx=f"indices.i32[{2 * sum_k}]",
                                          vals=f"values.bf16[{2 * sum_k}]", nranks=2, world_size=2, accumulate=1,
                                          gerr="global_error_dict[b]", decay=R.DECAY, dtype=N.BF16, **lay))]
    for i, t in enumerate((t2, t3)):
        check_trace(t, seq, f"compressed call {i}")
        assert t[-1]["state"]["iter"] == 3 + i and t[-1]["state"]["last_k"] == ks
    assert t3[-1]["state"]["comm_bits_this_round"] == 0  # this hook counts none
    assert t3[-1]["state"]["mixed_calls"] == 0 and t3[-1]["state"]["wire16_calls"] == 0
