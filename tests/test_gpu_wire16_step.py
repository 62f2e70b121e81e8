"""The bf16 wire through the exchange step, on an MI355X (run with -m gpu):
``GroupTopKState.wire_exchange = "step"`` sends a bf16-wire bucket (``wire_dtype = torch.bfloat16``)
through arctopk_exchange_step on a plan bound with arctopk_plan_bind_wire16 -- deferral, the
all-reduce stream, ExchangeFutures -- and the backward's last large EF14 / noef bucket through the
zero-ahead scatter (arctopk_decode_wire16_scatter).

Bars: everything is bit-exact -- the scatter against arctopk_decode_wire16 and the CPU restatement
(wire16_oracle); the step branch against the inline branch (the phase-by-phase call) and against
the restatement given the rows the device's own select chose.

Layouts (the ones tests/test_gpu_wire16.py justifies, the smallest that reach every store width and
row path): MIXA has odd offsets (element by element), m = 18 and m = 2 (short rows), an odd wide m
and RAW tensors; ALIGNB has every tensor on the vector path with packed_off % 8 in {0, 4}, so 8-B
and 16-B packed accesses both run; MIXA under PLAN_DENSE_1D has DENSE segments.  Ratio 0.25, r = 4.
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
from parity import assert_bitwise, ensure_group, rendezvous

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
DEV = "cuda:0"
BF16 = torch.bfloat16
F32 = torch.float32
MIXA = [[16, 64], [5], [64, 128], [100, 72], [9, 100], [8, 4, 3, 3], [16, 8, 1, 1], [8, 40], [4, 5461], [7]]
MIXA9 = [s for s in MIXA if s != [4, 5461]]
ALIGNB = [[4, 4], [32, 2048], [6, 24], [10, 24], [16, 64]]
LAYOUTS = {"mixa": (MIXA, False), "alignb": (ALIGNB, False), "mixa_dense": (MIXA, True)}
GUARD = 64  # elements around a buffer: a write outside it is seen
SENT = 12345.0
EFS = ("noef", "ef14", "ef21")


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


def _scatters(plan) -> int:
    c = ctypes.c_int64(-1)
    N.check(N.lib().arctopk_diag_wire16_scatters(plan.handle, ctypes.byref(c)), "arctopk_diag_wire16_scatters")
    return c.value


# ---- 1. the scatter kernel, phase level ------------------------------------------------------
def _scatter(plan, p16, ws, outd, rowlist=True):
    return N.lib().arctopk_decode_wire16_scatter(plan.handle, p16.data_ptr(),
                                                 plan.rowlist.data_ptr() if rowlist else None,
                                                 plan.slotmap.data_ptr(), ws, outd.data_ptr(), _stream())


@pytest.mark.parametrize("ws", [1, 2, 3])
@pytest.mark.parametrize("ef", ["noef", "ef14"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_scatter_phase(layout, ef, ws):
    shapes, dense = LAYOUTS[layout]
    L = N.lib()
    g = torch.Generator().manual_seed(31)
    n = bucket_numel(shapes)
    G = torch.randn(n, generator=g)
    E0 = torch.randn(n, generator=g) * 0.37 if ef == "ef14" else None
    plan = BucketPlan([tuple(s) for s in shapes], 4, 0.25, F32, DEV, flags=N.PLAN_DENSE_1D if dense else 0)
    V = torch.randn(max(1, plan.info.v_len), generator=g)
    Gd = G.to(DEV)
    Ed = None if E0 is None else E0.to(DEV)
    plan.encode(Gd, Ed, N.EF_CODE[ef], True, V.to(DEV), _stream())
    plan.select(1, _stream())
    pbuf, p16 = _guarded(torch.zeros(max(1, plan.info.packed_len), dtype=BF16))
    assert L.arctopk_pack_wire16(plan.handle, Gd.data_ptr(), N.ptr(Ed), N.EF_CODE[ef], 1, plan.rowlist.data_ptr(),
                                 plan.slotmap.data_ptr(), p16.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    segs = W.segments(shapes, 0.25, dense)
    rows = W.full_rows(_rows(plan), segs)
    vals = [W.pack(G, E0, ef, rows, segs)[0]]
    assert_bitwise(p16, _packed_layout(plan, vals[0]), f"{layout} {ef}: the device's pack")
    for _ in range(1, ws):  # the other ranks' values: any bf16 values do
        vals.append(W.b(torch.randn(vals[0].numel(), generator=g) * 1.7))
    vsum = W.wire_sum(vals)
    p16.copy_(_packed_layout(plan, vsum))
    want, _ = W.decode(vsum, ws, rows, segs, n, ef, None)
    obuf, outd = _guarded(torch.zeros(n))  # the zeroed bucket
    rbuf, refd = _guarded(torch.full((n,), 777.0))
    rl0 = plan.rowlist.clone()
    assert _scatter(plan, p16, ws, outd) == 0
    assert L.arctopk_decode_wire16(plan.handle, p16.data_ptr(), plan.slotmap.data_ptr(), ws, N.EF_CODE[ef], None,
                                   refd.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    assert _guards_intact(pbuf, obuf, rbuf), "a write outside a buffer"
    assert torch.equal(plan.rowlist, rl0)
    assert_bitwise(p16, _packed_layout(plan, vsum), "the packed values are only read")
    assert_bitwise(outd, refd, f"{layout} {ef} ws{ws}: scatter == arctopk_decode_wire16")
    assert_bitwise(outd, want, f"{layout} {ef} ws{ws}: scatter == the restatement's decode")
    assert outd.count_nonzero() > 0
    # it touches nothing else: an unselected element keeps what it held
    o2buf, out2 = _guarded(torch.full((n,), 555.0))
    assert _scatter(plan, p16, ws, out2) == 0
    torch.cuda.synchronize()
    sel = W.decode(W.b(torch.ones(vsum.numel())), 1, rows, segs, n, ef, None)[0] != 0
    assert torch.equal(out2.cpu()[~sel], torch.full((n,), 555.0)[~sel]) and _guards_intact(o2buf)
    assert_bitwise(out2.cpu()[sel], want[sel], "selected elements")


def test_scatter_refuses():
    sent = lambda n, dt=F32: torch.full((n,), SENT, dtype=dt, device=DEV)  # noqa: E731
    p16 = BucketPlan([(4, 64)], 4, 0.25, BF16, DEV)
    p32 = BucketPlan([(4, 64)], 4, 0.25, F32, DEV)
    for p in (p16, p32):
        p.rowlist.zero_(), p.slotmap.zero_()
    out, pk = sent(264), sent(264, BF16)
    assert _scatter(p16, pk, 1, out) == N.EINVAL            # a bf16 plan
    assert _scatter(p32, pk, 1, out[1:]) == N.EINVAL        # a misaligned out
    assert _scatter(p32, pk, 1, out, rowlist=False) == N.EINVAL  # a NULL row list
    assert _scatter(p32, pk, 0, out) == N.EINVAL
    assert _scatter(p32, pk[1:], 1, out) == N.EINVAL
    torch.cuda.synchronize()
    assert bool((out == SENT).all()) and bool((pk == SENT).all()), "nothing was launched"
    assert _scatter(p32, pk, 1, out) == 0
    torch.cuda.synchronize()


# ---- 2. step equals inline, bit for bit --------------------------------------------------------
def _hook_state(c4, ef, seed, wire=True, exchange="step", **kw):
    if c4:  # two ramp calls (restarted draws, ratios 0.8 and 0.525), then steady ones
        st = H4.GroupTopKState(None, r=4, compress_ratio=0.25, start_compress_iter=0, use_error_feedback=ef,
                               seed=seed, warmup_iters=2)
    else:
        st = H.GroupTopKState(None, r=4, compress_ratio=0.25, start_compress_iter=0, use_error_feedback=ef, seed=seed)
    st.wire_dtype = BF16 if wire else None
    st.wire_exchange = exchange
    st.defer_decode = True
    for k, v in kw.items():
        setattr(st, k, v)
    return st


COMMS = {"none": {}, "force": dict(force_exchange=True), "wire": dict(emulate_wire=dict(ranks=8, busbw_gbs=350))}
BUCKETS3 = [MIXA, ALIGNB, MIXA]  # indices 0 .. 2, is_last only on the third


def _grad(shapes, tag: int) -> torch.Tensor:
    return torch.randn(bucket_numel(shapes), generator=torch.Generator().manual_seed(tag)) * 3.0


def _backward(st, hook, buckets, it, wire=None, check_pend=False):
    """One backward: the hook for every bucket (the last is_last), Futures waited at the end as DDP's
    finalize does.  wire: per bucket, the state's wire_dtype for that call.  Returns the outputs."""
    futs, last = [], len(buckets) - 1
    for b, shapes in enumerate(buckets):
        if wire is not None:
            st.wire_dtype = wire[b]
        calls0 = st.wire16_step_calls
        futs.append(hook(st, SyntheticBucket(_grad(shapes, 1000 * it + b).to(DEV), shapes, index=b,
                                             is_last=(b == last))))
        if check_pend and b != last and st.wire16_step_calls > calls0:
            assert st._x_pend and not futs[-1].done(), f"backward {it} bucket {b}: the step call is deferred"
    assert not st._x_pend and all(f.done() for f in futs), "the last bucket finishes everything pending"
    outs = [f.wait() for f in futs]
    torch.cuda.synchronize()
    return outs


@pytest.mark.parametrize("ef,comms,c4", [(ef, c, False) for ef in EFS for c in COMMS] + [(ef, "none", True) for ef in EFS])
def test_step_equals_inline(ef, comms, c4):
    hook = H4.group_topk_hook if c4 else H.group_topk_hook
    s_in = _hook_state(c4, ef, 91, exchange="inline", **COMMS[comms])
    s_st = _hook_state(c4, ef, 91, exchange="step", **COMMS[comms])
    orc = [W.Wire16Oracle(1, shapes, 0.25, ef, c4=c4, warmup_iters=2) for shapes in BUCKETS3]
    compressed = 0
    for it in range(3):
        o_in = _backward(s_in, hook, BUCKETS3, it)
        o_st = _backward(s_st, hook, BUCKETS3, it, check_pend=True)
        for b, shapes in enumerate(BUCKETS3):
            what = f"{ef} {comms} c4={c4} backward {it} bucket {b}"
            G = _grad(shapes, 1000 * it + b)
            if ef == "ef21" and it == 0:  # the dense fp32 call
                res = orc[b].call([G])
            else:
                res = orc[b].call([G], _rows(s_st._plans[b][1]))
                compressed += 1
                assert s_st._plans[b][1].wire16_bound and not s_in._plans[b][1].wire16_bound
            assert_bitwise(o_st[b], o_in[b], what + ": out, step vs inline")
            assert_bitwise(o_st[b], res["out"], what + ": out vs the restatement")
            if ef != "noef":
                assert_bitwise(s_st.error_dict[b], s_in.error_dict[b], what + ": E, step vs inline")
                assert_bitwise(s_st.error_dict[b], orc[b].Es[0], what + ": E vs the restatement")
            if ef == "ef21":
                assert_bitwise(s_st.global_error_dict[b], s_in.global_error_dict[b], what + ": gE, step vs inline")
                assert_bitwise(s_st.global_error_dict[b], orc[b].gE, what + ": gE vs the restatement")
        assert s_st.comm_bits_this_round == s_in.comm_bits_this_round == sum(o.bits for o in orc)
        assert s_st.iter == s_in.iter == it + 1 == orc[0].iter
        assert s_st.wire16_step_calls == s_st.wire16_calls == compressed
        assert s_in.wire16_step_calls == 0 and s_in.wire16_calls == compressed
    assert compressed == (6 if ef == "ef21" else 9)
    if comms != "none":
        assert s_st._comms is not None and s_st._plans[0][1].packed16_registered is s_st._comms[3]


# ---- 3. mixed pend -----------------------------------------------------------------------------
# D: a default-path call (wire_dtype None), W: a bf16-wire step.  With collectives the decode riding
# in a call's select is the one two calls back, without them the previous call's:
#   force D W D      : the issue's case (W finished by the last step, D riding in D)
#   force D D W W D D: D riding in a W step, W riding in a D step (a separate launch, never select_ride)
#   none  D W D      : the same two at world size 1 without communicators (depth 1)
_MIXED = {"force_dwd": ("force", "DWD"), "force_ddwwdd": ("force", "DDWWDD"), "none_dwd": ("none", "DWD")}


@pytest.mark.parametrize("ef", ["ef14", "ef21"])
@pytest.mark.parametrize("case", list(_MIXED))
def test_mixed_pend(case, ef):
    comms, modes = _MIXED[case]
    buckets = [MIXA if i % 2 == 0 else ALIGNB for i in range(len(modes))]
    wire = [BF16 if m == "W" else None for m in modes]
    mixed = _hook_state(False, ef, 17, **COMMS[comms])
    only_d = _hook_state(False, ef, 17, wire=False, **COMMS[comms])
    only_w = _hook_state(False, ef, 17, **COMMS[comms])
    for it in range(3):
        o_m = _backward(mixed, H.group_topk_hook, buckets, it, wire=wire, check_pend=True)
        o_d = _backward(only_d, H.group_topk_hook, buckets, it)
        o_w = _backward(only_w, H.group_topk_hook, buckets, it)
        for b, m in enumerate(modes):
            ref_o, ref = (o_w, only_w) if m == "W" else (o_d, only_d)
            what = f"{case} {ef} backward {it} bucket {b} ({m})"
            assert_bitwise(o_m[b], ref_o[b], what + ": out")
            assert_bitwise(mixed.error_dict[b], ref.error_dict[b], what + ": E")
            if ef == "ef21":
                assert_bitwise(mixed.global_error_dict[b], ref.global_error_dict[b], what + ": gE")
    n_w = modes.count("W") * (2 if ef == "ef21" else 3)
    assert mixed.wire16_step_calls == mixed.wire16_calls == n_w and only_d.wire16_calls == 0
    assert [mixed._plans[b][1].wire16_bound for b in range(len(modes))] == [m == "W" for m in modes]


def test_option_changes_on_one_bucket():
    """The same bucket as a bf16-wire step, then a default step, then a bf16-wire step again: the
    plan is bound and unbound between its steps, each result the single-mode state's."""
    wire = [BF16, None, BF16, None]
    mixed, only_d, only_w = (_hook_state(False, "ef21", 3, wire=w, force_exchange=True) for w in (True, False, True))
    for it in range(4):
        mixed.wire_dtype = wire[it]
        o_m = _backward(mixed, H.group_topk_hook, [ALIGNB], it)
        o_d = _backward(only_d, H.group_topk_hook, [ALIGNB], it)
        o_w = _backward(only_w, H.group_topk_hook, [ALIGNB], it)
        if it == 0:
            continue  # (the dense call)
        # E and gE carry over between modes, so only the first compressed call has a single-mode twin
        if it == 1:
            assert_bitwise(o_m[0], o_d[0], "a default step on a plan that was never bound")
        assert mixed._plans[0][1].wire16_bound == (wire[it] is BF16)
    assert mixed.wire16_step_calls == 1 and only_w.wire16_step_calls == 3 and o_w[0].dtype == F32


# ---- 4. two ranks on one GPU -------------------------------------------------------------------
def _two_rank_worker(rank, ws, port, ef):
    sys.path.insert(0, REPO)
    sys.path.insert(0, HERE)
    torch.set_num_threads(2)
    dist.init_process_group("gloo", init_method=port, rank=rank, world_size=ws)
    buckets = [MIXA9, ALIGNB, MIXA9]
    st = _hook_state(False, ef, 77)
    inl = _hook_state(False, ef, 77, exchange="inline")
    orc = [W.Wire16Oracle(ws, shapes, 0.25, ef) for shapes in buckets]
    for it in range(3):
        allg, futs, futs_in = [], [], []
        for b, shapes in enumerate(buckets):
            Gl = torch.randn(bucket_numel(shapes), generator=torch.Generator().manual_seed(1000 * it + 10 * b + rank))
            parts = [torch.empty_like(Gl) for _ in range(ws)]
            dist.all_gather(parts, Gl)
            allg.append(parts)
            last = b == len(buckets) - 1
            futs_in.append(H.group_topk_hook(inl, SyntheticBucket(Gl.to(DEV), shapes, index=b, is_last=last)))
            futs.append(H.group_topk_hook(st, SyntheticBucket(Gl.to(DEV), shapes, index=b, is_last=last)))
            if not last and not (ef == "ef21" and it == 0):
                assert len(st._x_pend) == b + 1, "three buckets in flight"
        assert not st._x_pend and all(f.done() for f in futs)
        outs, outs_in = [f.wait() for f in futs], [f.wait() for f in futs_in]
        torch.cuda.synchronize()
        for b, shapes in enumerate(buckets):
            what = f"{ef} it{it} rank{rank} bucket{b}"
            if ef == "ef21" and it == 0:
                res = orc[b].call(allg[b])
            else:
                plan = st._plans[b][1]
                rl = plan.rowlist.cpu()
                other = [torch.empty_like(rl) for _ in range(ws)]
                dist.all_gather(other, rl)
                assert torch.equal(other[0], other[1]), what + ": ranks selected different rows"
                pk = st._comms[3]
                assert pk.kind == "callback" and pk.size == ws
                assert pk._views[plan.packed16.data_ptr()].dtype == BF16, "the packed all-reduce carried bf16"
                res = orc[b].call(allg[b], _rows(plan))
            assert_bitwise(outs[b], res["out"], what + " out")
            assert_bitwise(outs[b], outs_in[b], what + " out, step vs inline")
            assert_bitwise(st.error_dict[b], orc[b].Es[rank], what + " E")
            if ef == "ef21":
                assert_bitwise(st.global_error_dict[b], orc[b].gE, what + " gE")
        assert st.comm_bits_this_round == inl.comm_bits_this_round == sum(o.bits for o in orc) > 0
    compressed = 3 * (3 if ef == "ef14" else 2)
    assert st.wire16_step_calls == st.wire16_calls == compressed and inl.wire16_step_calls == 0
    dist.destroy_process_group()


@pytest.mark.parametrize("ef", ["ef14", "ef21"])
def test_two_ranks_one_gpu(ef):
    mp.spawn(_two_rank_worker, args=(2, rendezvous(), ef), nprocs=2, join=True)


# ---- 5. inside DDP -----------------------------------------------------------------------------
class _DdpNet(torch.nn.Module):
    """Conv (ND, m = 18), linear weights (2-D) and biases (1-D): several DDP buckets at a 0.5 MB cap."""

    def __init__(self):
        super().__init__()
        self.body = torch.nn.Sequential(torch.nn.Conv2d(3, 16, 3), torch.nn.ReLU(), torch.nn.Flatten(),
                                        torch.nn.Linear(16 * 6 * 6, 512), torch.nn.ReLU(),
                                        torch.nn.Linear(512, 512), torch.nn.ReLU(),
                                        torch.nn.Linear(512, 10))

    def forward(self, x):
        return self.body(x)


def test_inside_ddp():
    from torch.nn.parallel import DistributedDataParallel as DDP
    x = torch.randn(8, 3, 8, 8, generator=torch.Generator().manual_seed(5)).to(DEV)
    grads, states = {}, {}
    for mode in ("inline", "step"):
        torch.manual_seed(0)
        model = DDP(_DdpNet().cuda(), device_ids=[0], bucket_cap_mb=0.5)
        # (one dense warm-up backward, after which DDP rebuilds its buckets; then three compressed ones)
        st = H.GroupTopKState(None, r=4, compress_ratio=0.25, start_compress_iter=1, use_error_feedback="ef14", seed=3)
        st.wire_dtype, st.wire_exchange, st.force_exchange = BF16, mode, True
        model.register_comm_hook(st, H.group_topk_hook)
        grads[mode] = []
        for _ in range(4):
            model.zero_grad()
            model(x).pow(2).mean().backward()
            torch.cuda.synchronize()
            assert not st._x_pend
            grads[mode].append([p.grad.detach().clone() for p in model.parameters()])
        states[mode] = st
    for it in range(4):
        for i, (a, b_) in enumerate(zip(grads["step"][it], grads["inline"][it])):
            assert_bitwise(a, b_, f"backward {it} parameter {i}: step vs inline")
        assert any(bool(g.count_nonzero()) for g in grads["step"][it])
    st = states["step"]
    assert len(st._plans) >= 2, "several buckets"
    assert st.wire16_step_calls == st.wire16_calls == states["inline"].wire16_calls >= 3 * 2
    assert states["inline"].wire16_step_calls == 0
    assert st._comms[3].kind == "rccl" and st.comm_bits_this_round == states["inline"].comm_bits_this_round


# ---- 6. the zero-ahead drain through the hook --------------------------------------------------
@pytest.mark.parametrize("ef", EFS)
def test_zero_ahead_drain(ef):
    """Two 64 MiB buckets per backward (the zero-ahead threshold holds), forced exchange: the
    backward's last bucket decodes through the scatter under noef / EF14, never under EF21.  Two
    backwards; EF21 runs a third, its first being the dense call."""
    big = [[4096, 4096]]
    n = bucket_numel(big)
    s_in = _hook_state(False, ef, 11, exchange="inline", force_exchange=True)
    s_st = _hook_state(False, ef, 11, exchange="step", force_exchange=True)
    gen = torch.Generator(device=DEV)
    backwards = 3 if ef == "ef21" else 2
    for it in range(backwards):
        outs = {}
        for st in (s_in, s_st):
            futs = []
            for b in range(2):
                gen.manual_seed(100 * it + b)
                G = torch.randn(n, generator=gen, device=DEV)
                futs.append(H.group_topk_hook(st, SyntheticBucket(G, big, index=b, is_last=(b == 1))))
            assert not st._x_pend
            outs[st] = [f.wait() for f in futs]
            torch.cuda.synchronize()
        for b in range(2):
            what = f"{ef} backward {it} bucket {b}"
            assert torch.equal(outs[s_st][b], outs[s_in][b]), what + ": out"
            if ef != "noef":
                assert torch.equal(s_st.error_dict[b], s_in.error_dict[b]), what + ": E"
            if ef == "ef21":
                assert torch.equal(s_st.global_error_dict[b], s_in.global_error_dict[b]), what + ": gE"
        assert bool(outs[s_st][1].count_nonzero())
    compressed = backwards - (ef == "ef21")
    assert s_st.wire16_step_calls == 2 * compressed
    assert _scatters(s_st._plans[1][1]) == (0 if ef == "ef21" else compressed), "the last bucket's decode"
    assert _scatters(s_st._plans[0][1]) == 0, "a deferred step keeps the whole decode"
    assert _scatters(s_in._plans[1][1]) == 0


# ---- 7. refusals of the step -------------------------------------------------------------------
def _native_step(plan, x, e, ef, err_in, seed, sel_stream=None, trail=None):
    """arctopk_exchange_step at world size 1 without communicators, nothing deferred."""
    return N.lib().arctopk_exchange_step(plan.handle, x.data_ptr(), N.ptr(e), None, ef, err_in, 1, seed, None, 0,
                                         None, None, _stream(), None, 0, None, None, None, None, 0, None, None,
                                         sel_stream, trail)


def test_step_refusals_leave_the_plan_usable():
    L = N.lib()
    shapes = [tuple(s) for s in ALIGNB]
    n = bucket_numel(ALIGNB)
    plan = BucketPlan(shapes, 4, 0.25, F32, DEV)
    p16 = torch.zeros(max(1, plan.info.packed_len), dtype=BF16, device=DEV)
    assert L.arctopk_plan_bind_wire16(plan.handle, p16[1:].data_ptr()) == N.EINVAL  # 8-B aligned
    pb = BucketPlan([(4, 64)], 4, 0.25, BF16, DEV)
    assert L.arctopk_plan_bind_wire16(pb.handle, p16.data_ptr()) == N.EINVAL        # an fp32 plan only
    assert L.arctopk_plan_bind_wire16(plan.handle, p16.data_ptr()) == 0
    # a small bound plan with a trailing step recorded (single-block selects: it qualifies as one)
    small = BucketPlan([(16, 64), (8, 40)], 4, 0.25, F32, DEV)
    s16 = torch.zeros(max(1, small.info.packed_len), dtype=BF16, device=DEV)
    xs = torch.randn(bucket_numel([(16, 64), (8, 40)]), device=DEV)
    es = torch.zeros_like(xs)
    assert L.arctopk_plan_bind_wire16(small.handle, s16.data_ptr()) == 0
    assert L.arctopk_exchange_trail(small.handle, xs.data_ptr(), es.data_ptr(), None, N.EF14, 0, 1, 5, None,
                                    _stream()) == 0
    assert L.arctopk_plan_bind_wire16(small.handle, None) == N.EINVAL  # a step trailing: no rebinding

    G = torch.randn(n, generator=torch.Generator().manual_seed(8))
    E0 = torch.randn(n, generator=torch.Generator().manual_seed(9)) * 0.3
    x, e = G.to(DEV), E0.to(DEV)
    other = torch.cuda.Stream()
    assert _native_step(plan, x, e, N.EF14, N.ERR_IN_ZERO_ROWS, 7) == N.EINVAL          # err_in = 2
    assert _native_step(plan, x, e, N.EF14, 1, 7, sel_stream=other.cuda_stream) == N.EINVAL  # a foreign select stream
    assert _native_step(plan, x, e, N.EF14, 1, 7, trail=small.handle) == N.EINVAL        # a bf16-wire trail
    assert _native_step(plan, x[1:], e, N.EF14, 1, 7) == N.EINVAL                        # 16-B aligned bucket
    assert _native_step(plan, x, e[2:], N.EF14, 1, 7) == N.EINVAL
    torch.cuda.synchronize()
    assert torch.equal(x.cpu(), G) and torch.equal(e.cpu(), E0) and not p16.any(), "nothing was enqueued"
    # the plan is still usable: a correct step on it succeeds and matches the restatement
    assert _native_step(plan, x, e, N.EF14, 1, 7) == 0
    torch.cuda.synchronize()
    segs = W.segments(ALIGNB, 0.25)
    res = W.simulate_step([G], [E0], None, ALIGNB, 0.25, 4, "ef14", _rows(plan))
    assert_bitwise(x, res["out"], "out after the refusals")
    assert_bitwise(e, res["E_new"][0], "E after the refusals")
    assert_bitwise(p16, _packed_layout(plan, res["values_sum"]), "the bound buffer holds the packed values")
    assert len(segs) == len(plan.segments)
    # the trailing step is still recorded on its plan: finished on its own (the default path's decode)
    N.check(L.arctopk_exchange_finish(small.handle, _stream(), None), "arctopk_exchange_finish")
    torch.cuda.synchronize()
    assert L.arctopk_plan_bind_wire16(small.handle, None) == 0
    assert L.arctopk_plan_bind_wire16(plan.handle, None) == 0


# ---- 8. the option unset -----------------------------------------------------------------------
def test_option_unset_is_the_inline_branch():
    st = H.GroupTopKState(None, r=4, compress_ratio=0.25, start_compress_iter=0, use_error_feedback="ef14", seed=91)
    st.wire_dtype = BF16
    assert st.wire_exchange == "inline" and st.state_dict()["wire_exchange"] == "inline"
    o = W.Wire16Oracle(1, MIXA, 0.25, "ef14")
    for it in range(3):
        G = _grad(MIXA, 70 + it)
        fut = H.group_topk_hook(st, SyntheticBucket(G.to(DEV), MIXA, index=0, is_last=True))
        assert fut.done() and not st._x_pend
        out = fut.wait()
        torch.cuda.synchronize()
        plan = st._plans[0][1]
        res = o.call([G], _rows(plan))
        assert_bitwise(out, res["out"], f"it{it} out")
        assert_bitwise(st.error_dict[0], o.Es[0], f"it{it} E")
        assert not plan.wire16_bound
    assert st.wire16_step_calls == 0 and st.wire16_calls == 3
