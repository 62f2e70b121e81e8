"""An fp32 bucket whose packed values travel as bf16, on an MI355X (run with -m gpu): the two phase
entry points (arctopk_pack_wire16, arctopk_decode_wire16) and the hook branch that
``GroupTopKState.wire_dtype = torch.bfloat16`` selects, against the CPU restatement (wire16_oracle)
given the rows the device's own select chose.

Bars: the packed values (pads included), the residuals and the decoded bucket are bit-exact; encode
and select are the existing ones and are checked by their own tests.
"""
import ctypes
import os
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import wire16_oracle as W
from allreducetopk_amd import _native as N
from allreducetopk_amd.bucket import SyntheticBucket, bucket_numel
from allreducetopk_amd.comm_hooks import group_topk_hook_no_reshape as H
from allreducetopk_amd.comm_hooks import group_topk_hook_no_reshape_c4 as H4
from allreducetopk_amd.comm_hooks.group_topk_hook_no_reshape import BucketPlan
from oracle import arctopk as A
from parity import assert_bitwise, ensure_group, rendezvous

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
DEV = "cuda:0"
BF16 = torch.bfloat16
F32 = torch.float32
# [16, 64]: 16-B units; [5]: RAW, and every later offset odd (element by element); [64, 128],
# [100, 72]: wide rows; [9, 100]: odd offset; m = 18 (ND) and m = 2 (1x1 conv): short rows;
# [4, 5461]: an odd wide m; [7]: RAW
MIXA = [[16, 64], [5], [64, 128], [100, 72], [9, 100], [8, 4, 3, 3], [16, 8, 1, 1], [8, 40], [4, 5461], [7]]
MIXA9 = [s for s in MIXA if s != [4, 5461]]
# every tensor on the vector path; [4, 4] (k = 1: 4 values) leaves the next segment's packed_off
# = 4 (mod 8): 8-B and 16-B packed stores both run
ALIGNB = [[4, 4], [32, 2048], [6, 24], [10, 24], [16, 64]]
LAYOUTS = {"mixa": (MIXA, False), "alignb": (ALIGNB, False), "mixa_dense": (MIXA, True)}
MODES = {"noef": ("noef", 1), "ef14_new": ("ef14", 0), "ef14_add": ("ef14", 1), "ef21": ("ef21", 1)}
GUARD = 64  # elements around a buffer: a write outside it is seen
SENT = 12345.0


@pytest.fixture(scope="module", autouse=True)
def group():
    ensure_group("nccl")
    yield


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _guarded(t0: torch.Tensor):
    """t0 (CPU) on the device inside a buffer of sentinels; (whole buffer, view of the values)."""
    buf = torch.full((t0.numel() + 2 * GUARD,), SENT, dtype=t0.dtype, device=DEV)
    view = buf[GUARD:GUARD + t0.numel()]
    view.copy_(t0)
    assert view.data_ptr() % 16 == 0
    return buf, view


def _guards_intact(*bufs):
    return all(bool((b_[:GUARD] == SENT).all() and (b_[-GUARD:] == SENT).all()) for b_ in bufs)


def _rows(plan):
    rl = plan.rowlist.cpu()
    return [rl[s.sel_off:s.sel_off + s.k_rows].long() for s in plan.segments]


def _packed_layout(plan, vals: torch.Tensor) -> torch.Tensor:
    """Values in oracle.arctopk's layout (segments back to back) laid out as the plan's packed
    buffer: every segment at its packed_off, zeros in the pads."""
    full = torch.zeros(max(1, plan.info.packed_len), dtype=vals.dtype)
    off = 0
    for s in plan.segments:
        k = int(s.k_rows * s.m)
        full[s.packed_off:s.packed_off + k] = vals[off:off + k]
        off += k
    assert off == vals.numel()
    return full


def _pack(plan, Gd, Ed, ef, err_in, p16):
    return N.lib().arctopk_pack_wire16(plan.handle, N.ptr(Gd), N.ptr(Ed), N.EF_CODE[ef], int(err_in),
                                       plan.rowlist.data_ptr(), plan.slotmap.data_ptr(), p16.data_ptr(), _stream())


def _decode(plan, p16, ws, ef, gEd, outd):
    return N.lib().arctopk_decode_wire16(plan.handle, p16.data_ptr(), plan.slotmap.data_ptr(), ws, N.EF_CODE[ef],
                                         N.ptr(gEd), outd.data_ptr(), _stream())


def _selected(layout, mode, seed):
    """A plan after the existing encode and select on the device; the inputs and what the encode
    left, on the CPU, with the restatement's segments and the device's rows."""
    shapes, dense = LAYOUTS[layout]
    ef, err_in = MODES[mode]
    g = torch.Generator().manual_seed(seed)
    n = bucket_numel(shapes)
    G = torch.randn(n, generator=g)
    E0 = torch.randn(n, generator=g) * 0.37 if (ef == "ef21" or err_in) else torch.zeros(n)
    plan = BucketPlan([tuple(s) for s in shapes], 4, 0.25, F32, DEV, flags=N.PLAN_DENSE_1D if dense else 0)
    V = torch.randn(max(1, plan.info.v_len), generator=g)
    Gd = G.to(DEV)
    ebuf = Ed = None
    if ef != "noef":
        ebuf, Ed = _guarded(E0)
    plan.encode(Gd, Ed, N.EF_CODE[ef], bool(err_in), V.to(DEV), _stream())
    plan.select(1, _stream())
    torch.cuda.synchronize()
    segs = W.segments(shapes, 0.25, dense)
    rows = W.full_rows(_rows(plan), segs)
    for r_, s in zip(rows, plan.segments):
        assert torch.equal(r_, r_.sort().values) and int(r_.max()) < s.n
    E_in = None if ef == "noef" or (ef == "ef14" and not err_in) else E0
    return dict(plan=plan, G=G, Gd=Gd, E_in=E_in, ebuf=ebuf, Ed=Ed, segs=segs, rows=rows, ef=ef, err_in=err_in, n=n,
                gen=g)


def test_layouts_cover_the_paths():
    p = BucketPlan([tuple(s) for s in ALIGNB], 4, 0.25, F32, DEV)
    assert all(s.m % 4 == 0 and s.offset % 4 == 0 and s.packed_off % 4 == 0 for s in p.segments)
    assert p.segments[0].k_rows * p.segments[0].m == 4
    assert {int(s.packed_off % 8) for s in p.segments} == {0, 4}, "8-B and 16-B packed stores"
    q = BucketPlan([tuple(s) for s in MIXA], 4, 0.25, F32, DEV)
    assert any(s.offset % 4 for s in q.segments) and any(s.m % 4 == 0 and s.offset % 4 == 0 for s in q.segments)
    assert {N.SEG_RAW, N.SEG_SKETCH} == {s.kind for s in q.segments}
    assert {18, 2, 5461} <= {int(s.m) for s in q.segments}


# ---- 1. pack -----------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_pack_phase(layout, mode):
    c = _selected(layout, mode, 23)
    plan, ef = c["plan"], c["ef"]
    rl0, sm0 = plan.rowlist.clone(), plan.slotmap.clone()
    pbuf, p16 = _guarded(torch.zeros(max(1, plan.info.packed_len), dtype=BF16))
    assert _pack(plan, c["Gd"], c["Ed"], ef, c["err_in"], p16) == 0
    torch.cuda.synchronize()
    assert torch.equal(plan.rowlist, rl0) and torch.equal(plan.slotmap, sm0)
    assert _guards_intact(pbuf) and (ef == "noef" or _guards_intact(c["ebuf"])), "a write outside a buffer"
    vals, E_new = W.pack(c["G"], c["E_in"], ef, c["rows"], c["segs"])
    assert_bitwise(p16, _packed_layout(plan, vals), f"{layout} {mode}: packed = b(X), zero pads")
    if ef != "noef":
        assert_bitwise(c["Ed"], E_new, f"{layout} {mode}: E")
    assert torch.equal(c["Gd"].cpu(), c["G"]), "the bucket is only read"


# ---- 2. decode ---------------------------------------------------------------------------
@pytest.mark.parametrize("ws", [1, 2, 3])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_decode_phase(layout, mode, ws):
    c = _selected(layout, mode, 29)
    plan, ef, n, g = c["plan"], c["ef"], c["n"], c["gen"]
    vals = [W.pack(c["G"], c["E_in"], ef, c["rows"], c["segs"])[0]]
    for _ in range(1, ws):  # the other ranks' values: any bf16 values do
        vals.append(W.b(torch.randn(vals[0].numel(), generator=g) * 1.7))
    vsum = W.wire_sum(vals)
    gE0 = torch.randn(n, generator=g) * 0.11
    gE0[::5] = -0.0
    want_out, want_gE = W.decode(vsum, ws, c["rows"], c["segs"], n, ef, gE0 if ef == "ef21" else None)
    pbuf, p16 = _guarded(_packed_layout(plan, vsum))
    gbuf = gEd = None
    if ef == "ef21":
        gbuf, gEd = _guarded(gE0)
    obuf, outd = _guarded(torch.full((n,), 777.0))
    assert _decode(plan, p16, ws, ef, gEd, outd) == 0
    torch.cuda.synchronize()
    assert _guards_intact(pbuf, obuf) and (gbuf is None or _guards_intact(gbuf)), "a write outside a buffer"
    assert not (outd == 777.0).any(), "every element of out is written"
    assert_bitwise(outd, want_out, f"{layout} {mode} ws{ws}: out")
    assert_bitwise(p16, _packed_layout(plan, vsum), "the packed values are only read")
    if ef == "ef21":
        assert_bitwise(gEd, want_gE, f"{layout} {mode} ws{ws}: gE")
        sel = A.decode(torch.ones(vsum.numel()), 1, c["rows"], c["segs"], n, F32) != 0
        assert torch.equal(gEd.cpu().view(torch.int32)[~sel], gE0.view(torch.int32)[~sel]), "unselected gE kept"
        gEd.copy_(gE0)
    # out aliasing the bucket
    assert _decode(plan, p16, ws, ef, gEd, c["Gd"]) == 0
    torch.cuda.synchronize()
    assert_bitwise(c["Gd"], want_out, f"{layout} {mode} ws{ws}: out is the bucket")
    if ef == "ef21":
        assert_bitwise(gEd, want_gE, f"{layout} {mode} ws{ws}: gE, out is the bucket")


# ---- 3. refusals -------------------------------------------------------------------------
def test_entry_points_refuse():
    L = N.lib()
    sent = lambda n, dt=F32: torch.full((n,), SENT, dtype=dt, device=DEV)  # noqa: E731
    p16 = BucketPlan([(4, 64)], 4, 0.25, BF16, DEV)
    p32 = BucketPlan([(4, 64)], 4, 0.25, F32, DEV)
    pd = BucketPlan([(4, 64), (8,)], 4, 0.25, F32, DEV, flags=N.PLAN_DENSE_1D)
    x, e, ge, out, pk = sent(264), sent(264), sent(264), sent(264), sent(264, BF16)
    for p in (p32, pd, p16):
        p.rowlist.zero_(), p.slotmap.zero_()

    def pack(p, g, e_, ef, err_in):
        return L.arctopk_pack_wire16(p.handle, N.ptr(g), N.ptr(e_), ef, err_in, p.rowlist.data_ptr(),
                                     p.slotmap.data_ptr(), pk.data_ptr(), _stream())

    def dec(p, ef, ge_, ws=1):
        return L.arctopk_decode_wire16(p.handle, pk.data_ptr(), p.slotmap.data_ptr(), ws, ef, N.ptr(ge_),
                                       out.data_ptr(), _stream())

    assert pack(p16, x, e, N.EF14, 1) == N.EINVAL and dec(p16, N.EF14, None) == N.EINVAL  # a bf16 plan
    assert pack(p32, x, e, N.EF14, 2) == N.EINVAL                                         # no zero rows here
    assert pack(p32, x, e, 3, 1) == N.EINVAL and dec(p32, 3, ge) == N.EINVAL
    assert dec(p32, N.EF21, None) == N.EINVAL                                             # gerr under EF21
    assert dec(p32, N.EF14, None, ws=0) == N.EINVAL
    assert pack(pd, None, e, N.EF14, 1) == N.EINVAL                                       # DENSE: X formed from G
    assert pack(p32, None, e, N.EF21, 1) == N.EINVAL and pack(p32, None, None, N.EF_NONE, 1) == N.EINVAL
    assert pack(p32, x, None, N.EF14, 1) == N.EINVAL and pack(p32, x, None, N.EF21, 1) == N.EINVAL
    assert pack(p32, x[1:], e, N.EF14, 1) == N.EINVAL and pack(p32, x, e[2:], N.EF14, 1) == N.EINVAL
    assert L.arctopk_pack_wire16(p32.handle, x.data_ptr(), e.data_ptr(), N.EF14, 1, p32.rowlist.data_ptr(),
                                 p32.slotmap.data_ptr(), pk[1:].data_ptr(), _stream()) == N.EINVAL
    assert L.arctopk_decode_wire16(p32.handle, pk.data_ptr(), p32.slotmap.data_ptr(), 1, N.EF14, None,
                                   out[1:].data_ptr(), _stream()) == N.EINVAL
    torch.cuda.synchronize()
    for t in (x, e, ge, out, pk):
        assert bool((t == SENT).all()), "nothing was launched"
    assert pack(p32, None, e, N.EF14, 1) == 0  # EF14 without DENSE segments reads no G
    torch.cuda.synchronize()


# ---- 4. the hook -------------------------------------------------------------------------
def _hook_state(c4, ef, seed, wire=True, **kw):
    if c4:  # two ramp calls (restarted draws, ratios 0.8 and 0.525), then steady ones
        st = H4.GroupTopKState(None, r=4, compress_ratio=0.25, start_compress_iter=0, use_error_feedback=ef,
                               seed=seed, warmup_iters=2)
    else:
        st = H.GroupTopKState(None, r=4, compress_ratio=0.25, start_compress_iter=0, use_error_feedback=ef, seed=seed)
    st.wire_dtype = BF16 if wire else None
    for k, v in kw.items():
        setattr(st, k, v)
    return st


_HOOK_CASES = [(c4, ef, proj, False) for c4 in (False, True) for ef in ("noef", "ef14", "ef21")
               for proj in ("device", "host")] + [(False, "ef14", "device", True), (False, "ef21", "device", True)]


@pytest.mark.parametrize("c4,ef,projections,force_exchange", _HOOK_CASES)
def test_hook_vs_restatement(c4, ef, projections, force_exchange):
    st = _hook_state(c4, ef, 91, projections=projections, force_exchange=force_exchange)
    hook = H4.group_topk_hook if c4 else H.group_topk_hook
    o = W.Wire16Oracle(1, MIXA, 0.25, ef, c4=c4, warmup_iters=2)
    n = bucket_numel(MIXA)
    ratios, compressed = [], 0
    for it in range(4):
        G = torch.randn(n, generator=torch.Generator().manual_seed(500 + it)) * 3.0
        fut = hook(st, SyntheticBucket(G.to(DEV), MIXA, index=0, is_last=True))
        assert fut.done()
        out = fut.wait()
        torch.cuda.synchronize()
        what = f"c4={c4} {ef} {projections} fx={force_exchange} it{it}"
        if ef == "ef21" and it == 0:  # the dense fp32 call
            res = o.call([G])
            assert not st._plans and st.wire16_calls == 0
        else:
            plan = st._plans[0][1]
            res = o.call([G], _rows(plan))
            compressed += 1
            assert plan.ratio == res["ratio"] and bool(plan.flags & N.PLAN_DENSE_1D) == c4, what
            assert plan.packed16.dtype == BF16 and plan.packed16.numel() == max(1, plan.info.packed_len)
            ratios.append(plan.ratio)
        assert out.dtype == F32
        assert_bitwise(out, res["out"], what + " out")
        if ef != "noef":
            assert st.error_dict[0].dtype == F32
            assert_bitwise(st.error_dict[0], o.Es[0], what + " E")
        if ef == "ef21":
            assert_bitwise(st.global_error_dict[0], o.gE, what + " gE")
        assert st.comm_bits_this_round == o.bits and st.iter == o.iter, what
        assert st.wire16_calls == compressed and not st._x_pend
    if c4:
        assert ratios[0] > ratios[1] and ratios[-1] == 0.25
    else:
        assert set(ratios) == {0.25}
    if force_exchange:
        assert st._comms is not None and st._comms[3].kind == "rccl" and st._comms[3].size == 1


# ---- 5. the identities -------------------------------------------------------------------
@pytest.mark.parametrize("c4", [False, True])
def test_identities_through_the_hook(c4):
    hook = H4.group_topk_hook if c4 else H.group_topk_hook
    s14, s21 = _hook_state(c4, "ef14", 5), _hook_state(c4, "ef21", 5)
    n = bucket_numel(MIXA)
    E_old = torch.zeros(n)
    for it in range(4):
        G = torch.randn(n, generator=torch.Generator().manual_seed(900 + it)) * 10.0 ** (it - 2)
        out = hook(s14, SyntheticBucket(G.to(DEV), MIXA, index=0, is_last=True)).wait()
        out21 = hook(s21, SyntheticBucket(G.to(DEV), MIXA, index=0, is_last=True)).wait()
        torch.cuda.synchronize()
        E_new = s14.error_dict[0].cpu().clone()
        assert torch.equal(out.cpu() + E_new, G + E_old), f"EF14 conservation, call {it}"
        E_old = E_new
        assert_bitwise(s21.global_error_dict[0], s21.error_dict[0].cpu(), f"EF21 gE == E, call {it}")
        assert_bitwise(out21, s21.global_error_dict[0].cpu(), f"EF21 out == gE, call {it}")
    assert s14.wire16_calls == 4 and s21.wire16_calls == 3


# ---- 6. the default path's rows ----------------------------------------------------------
@pytest.mark.parametrize("ef", ["noef", "ef14"])
def test_same_rows_as_the_default_path(ef):
    n = bucket_numel(MIXA)
    G = torch.randn(n, generator=torch.Generator().manual_seed(61)) * 2.0
    got = {}
    for wire in (False, True):
        st = _hook_state(False, ef, 13, wire=wire)
        out = H.group_topk_hook(st, SyntheticBucket(G.to(DEV), MIXA, index=0, is_last=True)).wait()
        torch.cuda.synchronize()
        plan = st._plans[0][1]
        got[wire] = (plan.rowlist.cpu().clone(), out.cpu().clone(), st.wire16_calls)
    assert got[False][2] == 0 and got[True][2] == 1
    assert torch.equal(got[False][0], got[True][0]), "the selection is the default path's"
    assert_bitwise(got[True][1], got[False][1].to(BF16).float(), f"{ef}: out = f(b(out_default))")
    assert got[False][1].count_nonzero() > 0


# ---- 7. two ranks ------------------------------------------------------------------------
def _two_rank_worker(rank, ws, port, ef):
    sys.path.insert(0, REPO)
    sys.path.insert(0, HERE)
    torch.set_num_threads(2)
    dist.init_process_group("gloo", init_method=port, rank=rank, world_size=ws)
    st = _hook_state(False, ef, 77)
    plain = _hook_state(False, ef, 77, wire=False)
    o = W.Wire16Oracle(ws, MIXA9, 0.25, ef)
    n = bucket_numel(MIXA9)
    segs = W.segments(MIXA9, 0.25)
    for it in range(3):
        Gl = torch.randn(n, generator=torch.Generator().manual_seed(1000 * it + rank))
        allg = [torch.empty(n) for _ in range(ws)]
        dist.all_gather(allg, Gl)
        H.group_topk_hook(plain, SyntheticBucket(Gl.to(DEV), MIXA9)).wait()
        out = H.group_topk_hook(st, SyntheticBucket(Gl.to(DEV), MIXA9)).wait()
        torch.cuda.synchronize()
        if ef == "ef21" and it == 0:
            res = o.call(allg)
        else:
            plan = st._plans[0][1]
            rl = plan.rowlist.cpu()
            other = [torch.empty_like(rl) for _ in range(ws)]
            dist.all_gather(other, rl)
            assert torch.equal(other[0], other[1]), "ranks selected different rows"
            pk = st._comms[3]
            assert pk.kind == "callback" and pk.size == ws
            assert pk._views[plan.packed16.data_ptr()].dtype == BF16, "the packed all-reduce carried bf16"
            res = o.call(allg, _rows(plan))
        assert_bitwise(out, res["out"], f"{ef} it{it} rank{rank} out")
        assert_bitwise(st.error_dict[0], o.Es[rank], f"{ef} it{it} rank{rank} E")
        if ef == "ef21":
            assert_bitwise(st.global_error_dict[0], o.gE, f"{ef} it{it} rank{rank} gE")
        assert st.comm_bits_this_round == o.bits > 0
    compressed = 3 if ef == "ef14" else 2
    k = sum(s.k for s in segs)
    first = n * 32 if ef == "ef21" else 0
    assert st.comm_bits_this_round == first + compressed * 2 * (ws - 1) * (W.sketch_elems(segs, 4) * 32 + k * 16)
    assert plain.comm_bits_this_round - st.comm_bits_this_round == compressed * 2 * (ws - 1) * k * 16 > 0
    assert st.wire16_calls == compressed and plain.wire16_calls == 0
    plain.flush_exchange()
    torch.cuda.synchronize()
    dist.destroy_process_group()


@pytest.mark.parametrize("ef", ["ef14", "ef21"])
def test_two_ranks_one_gpu(ef):
    mp.spawn(_two_rank_worker, args=(2, rendezvous(), ef), nprocs=2, join=True)


# ---- 8. the option unset -----------------------------------------------------------------
def test_option_unset_is_todays_path():
    """An fp32 bucket without the option: the existing step, bit for bit the base restatement's
    given the rows, and the zero-rows encode still runs (it never does on the bf16-wire branch)."""
    shapes = [[64, 256], [128], [200, 96]]
    st = H.GroupTopKState(None, r=4, compress_ratio=0.2, start_compress_iter=0, use_error_feedback="ef14", seed=4)
    assert st.wire_dtype is None
    ost = A.OracleState(seed=4)
    n = bucket_numel(shapes)
    E = None
    for it in range(3):
        G = torch.randn(n, generator=torch.Generator().manual_seed(40 + it))
        out = H.group_topk_hook(st, SyntheticBucket(G.to(DEV), shapes, index=0, is_last=True)).wait()
        torch.cuda.synchronize()
        plan = st._plans[0][1]
        res = A.simulate_step([G], [E], None, shapes, 0.2, 4, "ef14", ost.next_seed(), rows_override=_rows(plan),
                              proj_device=DEV)
        assert_bitwise(out, res["out"], f"it{it} out")
        assert_bitwise(st.error_dict[0], res["E_new"][0], f"it{it} E")
        E = res["E_new"][0]
    c = ctypes.c_int64(-1)
    N.check(N.lib().arctopk_diag_zero_row_encodes(plan.handle, ctypes.byref(c)), "arctopk_diag_zero_row_encodes")
    assert c.value >= 1 and st.wire16_calls == 0 and plan.packed16 is None
    # ... and with it, on the same layout: never
    st2 = H.GroupTopKState(None, r=4, compress_ratio=0.2, start_compress_iter=0, use_error_feedback="ef14", seed=4)
    st2.wire_dtype = BF16
    for it in range(3):
        G = torch.randn(n, generator=torch.Generator().manual_seed(40 + it))
        H.group_topk_hook(st2, SyntheticBucket(G.to(DEV), shapes, index=0, is_last=True)).wait()
    torch.cuda.synchronize()
    N.check(N.lib().arctopk_diag_zero_row_encodes(st2._plans[0][1].handle, ctypes.byref(c)), "diag")
    assert c.value == 0 and st2.wire16_calls == 3
