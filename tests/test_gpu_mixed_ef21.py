"""EF21 with both residuals in fp32 under a bf16 bucket on an MI355X (run with -m gpu): the three
phase entry points (arctopk_encode_mixed21, arctopk_pack_mixed21, arctopk_decode_mixed21) and the
hook branch that ``GroupTopKState.ef21_error_dtype = torch.float32`` selects, against the CPU
restatement (mixed_ef21_oracle) given the rows the device's own select chose.

Bars: both residuals, the packed values and the decoded bucket are bit-exact; the sketch of a 2-D /
ND tensor is within 2^-7 * (|D| @ |V|) of the restatement (one bf16 rounding of a sum formed in
another order than CPU `mm`, the bar of tests/test_gpu_mixed_ef.py::test_encode_phase); a RAW
tensor's sketch is b(D) exactly.
"""
import os
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import mixed_ef21_oracle as M21
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
FP32 = torch.float32
# [16, 64]: 16-B units, 8 lanes per row; [5]: RAW, and every later offset odd (element by element);
# [64, 128], [100, 72]: wave per row; [9, 100]: m % 8 != 0; m = 18 (ND) and m = 2 (1x1 conv): short
# rows; [4, 5461]: V past the 64 KiB LDS bound (read from global memory), odd m
MIX10 = [[16, 64], [5], [64, 128], [100, 72], [9, 100], [8, 4, 3, 3], [16, 8, 1, 1], [8, 40], [4, 5461], [7]]
MIX9 = [s for s in MIX10 if s != [4, 5461]]
# every tensor on the 16-B path: V past the LDS bound with m % 8 == 0, a wave per row with four
# units per lane, 4 lanes per row (m = 24) after a [3] + [21] that restore the alignment and leave
# the packed offsets behind them multiples of 4 but not of 8 (8-B packed accesses)
ALIGNED = [[4, 5464], [32, 2048], [3], [21], [6, 24], [10, 24], [16, 64]]
LAYOUTS = ["mix10", "aligned", "mix10_dense", "aligned_dense"]
GUARD = 64  # floats around a residual: a write outside it is seen


@pytest.fixture(scope="module", autouse=True)
def group():
    ensure_group("nccl")
    yield


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _guarded(E0: torch.Tensor):
    """E0 (fp32, CPU) on the device inside a buffer of sentinels; (whole buffer, view of E)."""
    buf = torch.full((E0.numel() + 2 * GUARD,), 12345.0, device=DEV)
    view = buf[GUARD:GUARD + E0.numel()]
    view.copy_(E0)
    assert view.data_ptr() % 16 == 0
    return buf, view


def _guards_intact(buf):
    return bool((buf[:GUARD] == 12345.0).all() and (buf[-GUARD:] == 12345.0).all())


def _encode(plan, G, Ed, V):
    N.check(N.lib().arctopk_encode_mixed21(plan.handle, G.data_ptr(), Ed.data_ptr(), V.data_ptr(),
                                           plan.sketch.data_ptr(), _stream()), "arctopk_encode_mixed21")


def _pack(plan, G, Ed):
    N.check(N.lib().arctopk_pack_mixed21(plan.handle, G.data_ptr(), Ed.data_ptr(), plan.rowlist.data_ptr(),
                                         plan.slotmap.data_ptr(), plan.packed.data_ptr(), _stream()),
            "arctopk_pack_mixed21")


def _decode(plan, ws, gEd, out):
    N.check(N.lib().arctopk_decode_mixed21(plan.handle, plan.packed.data_ptr(), plan.slotmap.data_ptr(), ws,
                                           gEd.data_ptr(), out.data_ptr(), _stream()), "arctopk_decode_mixed21")


def _layout(name):
    return (ALIGNED if name.startswith("aligned") else MIX10), name.endswith("_dense")


def _setup(name, seed):
    """(shapes, dense, G, E0, V, plan, restatement's segments) of a layout, seeded."""
    shapes, dense = _layout(name)
    g = torch.Generator().manual_seed(seed)
    n = bucket_numel(shapes)
    G = torch.randn(n, generator=g).to(BF16)
    E0 = torch.randn(n, generator=g) * 0.37  # fp32: low bits set
    plan = BucketPlan([tuple(s) for s in shapes], 4, 0.25, BF16, DEV, flags=N.PLAN_DENSE_1D if dense else 0)
    V = torch.randn(max(1, plan.info.v_len), generator=g).to(BF16)
    return shapes, dense, G, E0, V, plan, M21.segments(shapes, 0.25, dense)


def _plan_Vs(plan, V):
    return [V[s.v_off:s.v_off + s.m * plan.r].view(s.m, plan.r) if s.kind == N.SEG_SKETCH else None
            for s in plan.segments]


def _rows(plan, segs=None):
    rl = plan.rowlist.cpu()
    rows = [rl[s.sel_off:s.sel_off + s.k_rows].long() for s in plan.segments]
    if segs is not None:
        rows = [torch.arange(o.n) if o.kind == M21.DENSE else r for o, r in zip(segs, rows)]
    return rows


def _selected_mask(segs, rows, n):
    sent = torch.zeros(n, dtype=torch.bool)
    for s, idx in zip(segs, rows):
        sent[s.offset:s.offset + s.numel].view(s.n, s.m)[idx] = True
    return sent


# ---- 1. encode ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", LAYOUTS)
def test_encode_phase(name):
    shapes, dense, G, E0, V, plan, segs = _setup(name, 17)
    buf, Ed = _guarded(E0)
    plan.sketch.fill_(-7.0)
    _encode(plan, G.to(DEV), Ed, V.to(DEV))
    torch.cuda.synchronize()
    D, Ps = M21.encode(G, E0, segs, _plan_Vs(plan, V))
    assert _guards_intact(buf), "a write outside the residual"
    assert_bitwise(Ed, E0, f"{name}: the encode only reads E")
    sk = plan.sketch.cpu()
    assert sk.numel() == max(1, plan.info.sketch_len)
    for s, o, P in zip(plan.segments, segs, Ps):
        if s.kind == N.SEG_DENSE:
            assert P is None
            continue
        if s.kind == N.SEG_RAW:
            assert_bitwise(sk[s.sketch_off:s.sketch_off + s.n], P, f"{name} RAW [{s.n}] sketch = b(D)")
            continue
        d = D[o.offset:o.offset + o.numel].view(s.n, s.m)
        v = V[s.v_off:s.v_off + s.m * 4].view(s.m, 4).float()
        got = sk[s.sketch_off:s.sketch_off + s.n * 4].view(s.n, 4).float()
        scale = (d.abs() @ v.abs()).clamp_min(1e-30)
        worst = ((got - P.float()).abs() / scale).max().item()
        print(f"{name} [{s.n}, {s.m}]: worst sketch deviation {worst:.3e} of |D| @ |V| (bar 2^-7)")
        bad = ((got - P.float()).abs() > 2.0 ** -7 * scale).sum().item()
        assert bad == 0, f"{name} [{s.n}, {s.m}]: {bad} sketch entries off by more than one rounding"
    if dense:  # nothing of a DENSE segment reaches the sketch: its length is the other segments'
        assert plan.info.sketch_len == sum(s.n * 4 for s in plan.segments if s.kind == N.SEG_SKETCH)


@pytest.mark.parametrize("shapes", [[[4, 64]], [[3], [4, 64]], [[4, 5464]], [[1], [4, 5461]]])
def test_encode_pairs_columns_with_projections(shapes):
    """G[row][c] = 2 (c + 1), E[row][c] = c + 1 (c < 64, else both 0) and V[c][j] = [c == j]  ->
    sketch[row][j] = j + 1, on the 16-B path, the element path (odd offset) and the rows whose V is
    read from global memory."""
    plan = BucketPlan([tuple(s) for s in shapes], 4, 0.25, BF16, DEV)
    s = plan.segments[-1]
    m = int(s.m)
    row = torch.zeros(m)
    row[:64] = torch.arange(64, dtype=torch.float32) + 1
    G = torch.zeros(plan.info.numel)
    E = torch.zeros(plan.info.numel)
    G[s.offset:] = (2 * row).repeat(4)
    E[s.offset:] = row.repeat(4)
    Vi = torch.zeros(m, 4)
    for j in range(4):
        Vi[j, j] = 1.0
    buf, Ed = _guarded(E)
    _encode(plan, G.to(BF16).to(DEV), Ed, Vi.flatten().to(BF16).to(DEV))
    torch.cuda.synchronize()
    want = torch.tensor([1.0, 2.0, 3.0, 4.0]).repeat(4, 1)
    got = plan.sketch[s.sketch_off:s.sketch_off + 16].view(4, 4).float().cpu()
    assert torch.equal(got, want), got
    assert _guards_intact(buf) and torch.equal(Ed.cpu(), E)


# ---- 2. pack -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", LAYOUTS)
def test_pack_phase(name):
    """Rows from arctopk_select on the device's own sketch; packed values and E bit-exact given
    them; unselected rows of E, the row list and the slot map untouched."""
    shapes, dense, G, E0, V, plan, segs = _setup(name, 23)
    buf, Ed = _guarded(E0)
    Gd = G.to(DEV)
    _encode(plan, Gd, Ed, V.to(DEV))
    plan.select(1, _stream())
    torch.cuda.synchronize()
    rl0, sm0 = plan.rowlist.clone(), plan.slotmap.clone()
    _pack(plan, Gd, Ed)
    torch.cuda.synchronize()
    assert torch.equal(plan.rowlist, rl0) and torch.equal(plan.slotmap, sm0)
    assert _guards_intact(buf), "a write outside the residual"
    assert_bitwise(Gd, G, f"{name}: the bucket is only read")
    rows = _rows(plan, segs)
    for r_, s in zip(rows, plan.segments):
        assert torch.equal(r_, r_.sort().values) and int(r_.max()) < s.n
    D, _ = M21.encode(G, E0, segs, _plan_Vs(plan, V))
    vals, E_new = M21.pack(D, E0, rows, segs)
    assert_bitwise(plan.packed_values(), vals, f"{name}: packed = b(D)")
    assert_bitwise(Ed, E_new, f"{name}: E + f(packed) on the rows, E elsewhere")
    sent = _selected_mask(segs, rows, G.numel())
    assert sent.any() and not sent.all()
    assert torch.equal(Ed.cpu()[~sent], E0[~sent]), "unselected rows of E are untouched"
    used = torch.zeros(plan.packed.numel(), dtype=torch.bool)
    for s in plan.segments:
        used[s.packed_off:s.packed_off + s.k_rows * s.m] = True
    assert not plan.packed.cpu()[~used].any(), "the alignment pads of the packed buffer stay zero"


# ---- 3. decode ---------------------------------------------------------------------------
@pytest.mark.parametrize("ws", [1, 2, 3])
@pytest.mark.parametrize("name", LAYOUTS)
def test_decode_phase(name, ws):
    """A packed buffer of 'all-reduced' values and the select's slot map: gE and the bucket bit-exact
    (ws = 3: the true division), gE of unselected rows unchanged, the output written over the
    bucket itself."""
    shapes, dense, G, E0, V, plan, segs = _setup(name, 29)
    Gd = G.to(DEV)
    _encode(plan, Gd, E0.to(DEV), V.to(DEV))
    plan.select(1, _stream())
    torch.cuda.synchronize()
    g = torch.Generator().manual_seed(31 + ws)
    plan.packed.copy_((torch.randn(plan.packed.numel(), generator=g) * 3.0).to(BF16))
    gE0 = torch.randn(G.numel(), generator=g) * 0.61
    buf, gEd = _guarded(gE0)
    sm0, pk0 = plan.slotmap.clone(), plan.packed.clone()
    _decode(plan, ws, gEd, Gd)  # out aliases the bucket
    torch.cuda.synchronize()
    assert _guards_intact(buf), "a write outside the global residual"
    assert torch.equal(plan.slotmap, sm0) and torch.equal(plan.packed, pk0)
    rows = _rows(plan, segs)
    out, gE_new = M21.decode(plan.packed_values().cpu(), ws, rows, segs, gE0)
    assert_bitwise(gEd, gE_new, f"{name} ws {ws}: gE + f(P) / ws on the rows")
    assert_bitwise(Gd, out, f"{name} ws {ws}: out = b(gE)")
    sent = _selected_mask(segs, rows, G.numel())
    assert torch.equal(gEd.cpu()[~sent], gE0[~sent]), "gE of unselected rows is left as stored"
    assert (gEd.cpu()[sent] != gE0[sent]).any()


# ---- 4. refusals -------------------------------------------------------------------------
def test_entry_points_refuse_other_plans_and_pointers():
    L = N.lib()
    n = 256

    def enc(p, g, e, v, sk):
        return L.arctopk_encode_mixed21(p.handle, g, e, v, sk, _stream())

    def pack(p, g, e, rl, sm, pk):
        return L.arctopk_pack_mixed21(p.handle, g, e, rl, sm, pk, _stream())

    def dec(p, pk, sm, ws, ge, out):
        return L.arctopk_decode_mixed21(p.handle, pk, sm, ws, ge, out, _stream())

    x16 = torch.zeros(n + 8, dtype=BF16, device=DEV)
    e32 = torch.zeros(n + 8, device=DEV)
    for dtype in (FP32, BF16):
        p = BucketPlan([(4, 64)], 4, 0.25, dtype, DEV)
        g, e = x16.data_ptr(), e32.data_ptr()
        v, sk, rl, sm, pk = (p.V_ring[0].data_ptr(), p.sketch.data_ptr(), p.rowlist.data_ptr(),
                             p.slotmap.data_ptr(), p.packed.data_ptr())
        if dtype == FP32:  # not a bf16 plan
            assert enc(p, g, e, v, sk) == N.EINVAL
            assert pack(p, g, e, rl, sm, pk) == N.EINVAL
            assert dec(p, pk, sm, 1, e, g) == N.EINVAL
            continue
        g1, e1 = x16[1:].data_ptr(), e32[1:].data_ptr()  # 2 B and 4 B past a 16-B boundary
        assert g1 % 16 == 2 and e1 % 16 == 4
        for st in (enc(p, None, e, v, sk), enc(p, g, None, v, sk), enc(p, g, e, None, sk), enc(p, g, e, v, None),
                   enc(p, g1, e, v, sk), enc(p, g, e1, v, sk),
                   pack(p, None, e, rl, sm, pk), pack(p, g, None, rl, sm, pk), pack(p, g, e, None, sm, pk),
                   pack(p, g, e, rl, None, pk), pack(p, g, e, rl, sm, None),
                   pack(p, g1, e, rl, sm, pk), pack(p, g, e1, rl, sm, pk), pack(p, g, e, rl, sm, pk + 2),
                   dec(p, None, sm, 1, e, g), dec(p, pk, None, 1, e, g), dec(p, pk, sm, 1, None, g),
                   dec(p, pk, sm, 1, e, None), dec(p, pk + 2, sm, 1, e, g), dec(p, pk, sm, 1, e1, g),
                   dec(p, pk, sm, 1, e, g1), dec(p, pk, sm, 0, e, g), dec(p, pk, sm, -1, e, g)):
            assert st == N.EINVAL
    torch.cuda.synchronize()
    assert not x16.any() and not e32.any()


# ---- 5. the hook -------------------------------------------------------------------------
def _hook_state(c4, seed, option=FP32, **kw):
    if c4:  # two ramp calls (restarted draws, ratios 0.617 and 0.433), then a steady one
        st = H4.GroupTopKState(None, r=4, compress_ratio=0.25, start_compress_iter=0, use_error_feedback="ef21",
                               seed=seed, warmup_iters=3)
    else:
        st = H.GroupTopKState(None, r=4, compress_ratio=0.25, start_compress_iter=0, use_error_feedback="ef21",
                              seed=seed)
    st.ef21_error_dtype = option
    for k, v in kw.items():
        setattr(st, k, v)
    return st


@pytest.mark.parametrize("c4,projections,force_exchange", [(False, "device", False), (False, "host", False),
                                                           (True, "device", False), (True, "host", False),
                                                           (False, "device", True), (True, "device", True)])
def test_hook_vs_restatement(c4, projections, force_exchange):
    st = _hook_state(c4, 91, projections=projections, force_exchange=force_exchange)
    hook = H4.group_topk_hook if c4 else H.group_topk_hook
    o = M21.Mixed21Oracle(1, MIX10, 0.25, seed=91, c4=c4, warmup_iters=3)
    n = bucket_numel(MIX10)
    ratios = []
    for it in range(4):  # the dense first call, then three compressed ones
        G = (torch.randn(n, generator=torch.Generator().manual_seed(500 + it)) * 3.0).to(BF16)
        fut = hook(st, SyntheticBucket(G.to(DEV), MIX10, index=0, is_last=True))
        assert fut.done()
        out = fut.wait()
        torch.cuda.synchronize()
        what = f"c4={c4} {projections} fx={force_exchange} it{it}"
        if it == 0:
            res = o.call([G])
            assert 0 not in st._plans and st.mixed_calls == 0
        else:
            plan = st._plans[0][1]
            res = o.call([G], _rows(plan), proj_device=DEV if projections == "device" else None)
            assert plan.ratio == res["ratio"] and bool(plan.flags & N.PLAN_RESTART_DRAWS) == res["restart"], what
            assert bool(plan.flags & N.PLAN_DENSE_1D) == c4
            ratios.append(plan.ratio)
        assert out.dtype == BF16
        assert st.error_dict[0].dtype == FP32 and st.global_error_dict[0].dtype == FP32
        assert_bitwise(out, res["out"], what + " out")
        assert_bitwise(st.error_dict[0], o.Es[0], what + " E")
        assert_bitwise(st.global_error_dict[0], o.gE, what + " gE")
        assert st.comm_bits_this_round == o.bits and st.iter == o.iter == it + 1
    assert st.mixed_calls == 3 and st._mixed_buckets == {0} and not st._x_pend
    assert (ratios[0] > ratios[1] > ratios[2] == 0.25) if c4 else ratios == [0.25] * 3
    if force_exchange:
        assert st._comms is not None and st._comms[3].kind == "rccl" and st._comms[3].size == 1


# ---- 6. the invariant at world size one --------------------------------------------------
@pytest.mark.parametrize("c4", [False, True])
def test_global_residual_equals_local_at_world_size_one(c4):
    st = _hook_state(c4, 5)
    hook = H4.group_topk_hook if c4 else H.group_topk_hook
    n = bucket_numel(MIX10)
    for it in range(4):
        G = (torch.randn(n, generator=torch.Generator().manual_seed(900 + it)) * 10.0 ** (it - 2)).to(BF16)
        out = hook(st, SyntheticBucket(G.to(DEV), MIX10, index=0, is_last=True)).wait()
        torch.cuda.synchronize()
        E, gE = st.error_dict[0], st.global_error_dict[0]
        assert E.data_ptr() != gE.data_ptr()
        assert_bitwise(gE, E.cpu(), f"call {it}: gE == E")
        assert_bitwise(out, gE.cpu().to(BF16), f"call {it}: out == b(gE)")
    assert st.mixed_calls == 3


# ---- 7. two ranks ------------------------------------------------------------------------
def _two_rank_worker(rank, ws, port):
    sys.path.insert(0, REPO)
    sys.path.insert(0, HERE)
    torch.set_num_threads(2)
    dist.init_process_group("gloo", init_method=port, rank=rank, world_size=ws)
    st = H.GroupTopKState(None, r=4, compress_ratio=0.25, start_compress_iter=0, use_error_feedback="ef21", seed=77)
    st.ef21_error_dtype = FP32
    o = M21.Mixed21Oracle(ws, MIX9, 0.25, seed=77)
    n = bucket_numel(MIX9)
    for it in range(4):  # the dense first call (gloo's all-reduce of the bf16 bucket), then three compressed ones
        Gl = torch.randn(n, generator=torch.Generator().manual_seed(1000 * it + rank)).to(BF16)
        parts = [torch.empty(n) for _ in range(ws)]
        dist.all_gather(parts, Gl.float())
        allg = [p.to(BF16) for p in parts]
        out = H.group_topk_hook(st, SyntheticBucket(Gl.to(DEV), MIX9)).wait()
        torch.cuda.synchronize()
        if it == 0:
            res = o.call(allg)
            assert 0 not in st._plans
        else:
            plan = st._plans[0][1]
            rl = plan.rowlist.cpu()
            other = [torch.empty_like(rl) for _ in range(ws)]
            dist.all_gather(other, rl)
            assert torch.equal(other[0], other[1]), "ranks selected different rows"
            assert st._comms is not None and st._comms[3].kind == "callback" and st._comms[3].size == ws
            res = o.call(allg, _rows(plan), proj_device=DEV)
        assert_bitwise(out, res["out"], f"it{it} rank{rank} out")
        assert_bitwise(st.error_dict[0], o.Es[rank], f"it{it} rank{rank} E")
        assert_bitwise(st.global_error_dict[0], o.gE, f"it{it} rank{rank} gE")
        assert st.error_dict[0].dtype == FP32 and st.global_error_dict[0].dtype == FP32
        assert st.comm_bits_this_round == o.bits > 0
    assert st.mixed_calls == 3
    dist.destroy_process_group()


def test_two_ranks_one_gpu():
    mp.spawn(_two_rank_worker, args=(2, rendezvous()), nprocs=2, join=True)


# ---- 8. the drift ------------------------------------------------------------------------
def _drift_worker(rank, ws, port, fp32, want):
    sys.path.insert(0, REPO)
    sys.path.insert(0, HERE)
    torch.set_num_threads(2)
    dist.init_process_group("gloo", init_method=port, rank=rank, world_size=ws)
    st = H.GroupTopKState(None, r=4, compress_ratio=0.25, start_compress_iter=0, use_error_feedback="ef21", seed=8)
    st.ef21_error_dtype = FP32 if fp32 else None
    G0 = torch.full((4, 64), 0.125)
    G0[0] = 1024.0
    # the dense first call: E_0 = G, gE_0 = the mean, 1024 and 0.125 on both ranks
    out = H.group_topk_hook(st, SyntheticBucket(G0.flatten().to(BF16).to(DEV), [[4, 64]])).wait()
    torch.cuda.synchronize()
    assert torch.equal(out.float().cpu().view(4, 64), G0) and 0 not in st._plans
    for t in range(1, 17):
        G = G0.clone()
        if rank == 0:
            G[0] = 1024.0 + 8 * t
        out = H.group_topk_hook(st, SyntheticBucket(G.flatten().to(BF16).to(DEV), [[4, 64]])).wait()
        torch.cuda.synchronize()
        assert _rows(st._plans[0][1])[0].tolist() == [0], f"call {t}: row 0 carries the only change"
    out = out.float().cpu().view(4, 64)
    E = st.error_dict[0].float().cpu().view(4, 64)
    gE = st.global_error_dict[0].float().cpu().view(4, 64)
    print(f"rank {rank} fp32={fp32}: out[0][0] {out[0, 0].item()} gE[0][0] {gE[0, 0].item()} E[0][0] {E[0, 0].item()}")
    assert torch.equal(E[0], torch.full((64,), 1152.0 if rank == 0 else 1024.0))  # E tracks G on both paths
    assert torch.equal(gE[0], torch.full((64,), want)), gE[0, :4]
    assert torch.equal(out[0], torch.full((64,), want)), out[0, :4]
    assert torch.equal(out[1:], torch.full((3, 64), 0.125)) and torch.equal(gE[1:], torch.full((3, 64), 0.125))
    assert st.mixed_calls == (16 if fp32 else 0)
    assert st.global_error_dict[0].dtype == (FP32 if fp32 else BF16)
    dist.destroy_process_group()


@pytest.mark.parametrize("option,want", [(torch.float32, 1088.0), (None, 1024.0)])
def test_global_residual_drifts_in_bf16_and_not_in_fp32(option, want):
    """Two ranks, [[4, 64]], k = 1: rank 0's row 0 is 1024 + 8 t at call t, rank 1's stays 1024, rows
    1-3 are 0.125 on both.  The mean of the ranks' E is 1088 after 16 calls.  Each call's mean step
    is 4, half a bf16 ulp at 1024: the bf16 gE rounds every one away (today's behaviour: that half
    passes without the option), the fp32 gE adds them and b(1088) = 1088 comes out."""
    mp.spawn(_drift_worker, args=(2, rendezvous(), option is torch.float32, want), nprocs=2, join=True)


# ---- 9. the option unset -----------------------------------------------------------------
def test_option_unset_is_todays_path():
    """A bf16 EF21 bucket without the option: bf16 residuals and the existing step, bit for bit the
    base restatement's given the rows."""
    shapes = [[64, 256], [128], [200, 96]]
    st = _hook_state(False, 4, option=None)
    assert st.ef21_error_dtype is None
    ost = A.OracleState(seed=4)
    n = bucket_numel(shapes)
    E = gE = None
    for it in range(4):
        G = torch.randn(n, generator=torch.Generator().manual_seed(40 + it)).to(BF16)
        out = H.group_topk_hook(st, SyntheticBucket(G.to(DEV), shapes, index=0, is_last=True)).wait()
        torch.cuda.synchronize()
        assert st.error_dict[0].dtype == BF16 and st.global_error_dict[0].dtype == BF16
        if it == 0:
            assert_bitwise(out, G, "the dense first call")
            E, gE = G.clone(), G.clone()
        else:
            res = A.simulate_step([G], [E], gE, shapes, 0.25, 4, "ef21", ost.next_seed(),
                                  rows_override=_rows(st._plans[0][1]), proj_device=DEV)
            assert_bitwise(out, res["out"], f"it{it} out")
            E, gE = res["E_new"][0], res["gE_new"]
        assert_bitwise(st.error_dict[0], E, f"it{it} E")
        assert_bitwise(st.global_error_dict[0], gE, f"it{it} gE")
    assert st.mixed_calls == 0 and not st._mixed_buckets
