"""EF14 with an fp32 residual under a bf16 bucket on an MI355X (run with -m gpu): the two phase
entry points (arctopk_encode_mixed, arctopk_pack_mixed) and the hook branch that
``GroupTopKState.error_dtype = torch.float32`` selects, against the CPU restatement
(mixed_ef_oracle) given the rows the device's own select chose.

Bars: the residual, the packed values and the decoded bucket are bit-exact; the sketch of a 2-D /
ND tensor is within the bar tests/test_gpu_arctopk.py::test_row_path_sketch_matches_fp32_accumulation
applies to bf16, 2^-7 * (|x| @ |v|) (another summation order than CPU `mm`: within one bf16
rounding of the sum's magnitude); a RAW tensor's sketch is b(X) exactly.
"""
import ctypes
import os
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import mixed_ef_oracle as MX
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
# [16, 64]: 16-B units, 8 lanes per row; [5]: RAW, and every later offset odd (element by element);
# [64, 128], [100, 72]: wave per row; [9, 100]: m % 8 != 0; m = 18 (ND) and m = 2 (1x1 conv): short
# rows; [4, 5461]: V past the 64 KiB LDS bound (read from global memory), odd m
MIX10 = [[16, 64], [5], [64, 128], [100, 72], [9, 100], [8, 4, 3, 3], [16, 8, 1, 1], [8, 40], [4, 5461], [7]]
MIX9 = [s for s in MIX10 if s != [4, 5461]]
# every tensor on the 16-B path: V past the LDS bound with m % 8 == 0, a wave per row with four
# units per lane, 4 lanes per row (m = 24) after a [3] + [21] that restore the alignment and leave
# the packed offsets behind them multiples of 4 but not of 8 (8-B packed stores)
ALIGNED = [[4, 5464], [32, 2048], [3], [21], [6, 24], [10, 24], [16, 64]]
GUARD = 64  # floats around the residual: a write outside it is seen


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


def _encode(plan, G, Ed, err_in, V):
    N.check(N.lib().arctopk_encode_mixed(plan.handle, G.data_ptr(), Ed.data_ptr(), int(err_in), V.data_ptr(),
                                         plan.sketch.data_ptr(), _stream()), "arctopk_encode_mixed")


def _pack(plan, G, Ed, err_in):
    N.check(N.lib().arctopk_pack_mixed(plan.handle, N.ptr(G), Ed.data_ptr(), int(err_in), plan.rowlist.data_ptr(),
                                       plan.slotmap.data_ptr(), plan.packed.data_ptr(), _stream()),
            "arctopk_pack_mixed")


def _inputs(shapes, seed):
    g = torch.Generator().manual_seed(seed)
    n = bucket_numel(shapes)
    G = torch.randn(n, generator=g).to(BF16)
    E0 = torch.randn(n, generator=g) * 0.37  # fp32: low bits set
    return G, E0, g


def _plan_Vs(plan, V):
    return [V[s.v_off:s.v_off + s.m * plan.r].view(s.m, plan.r) if s.kind == N.SEG_SKETCH else None
            for s in plan.segments]


def _rows(plan):
    rl = plan.rowlist.cpu()
    return [rl[s.sel_off:s.sel_off + s.k_rows].long() for s in plan.segments]


# ---- 1. encode ---------------------------------------------------------------------------
@pytest.mark.parametrize("err_in", [0, 1])
@pytest.mark.parametrize("name", ["mix10", "aligned"])
def test_encode_phase(name, err_in):
    shapes = MIX10 if name == "mix10" else ALIGNED
    G, E0, g = _inputs(shapes, 17)
    plan = BucketPlan([tuple(s) for s in shapes], 4, 0.25, BF16, DEV)
    V = torch.randn(plan.info.v_len, generator=g).to(BF16)
    buf, Ed = _guarded(E0)
    plan.sketch.fill_(-7.0)
    _encode(plan, G.to(DEV), Ed, err_in, V.to(DEV))
    torch.cuda.synchronize()
    segs = MX.segments(shapes, 0.25)
    X, Ps = MX.encode(G, E0 if err_in else None, segs, _plan_Vs(plan, V))
    assert _guards_intact(buf), "a write outside the residual"
    assert_bitwise(Ed, X, f"{name} err_in {err_in}: E := X")
    sk = plan.sketch.cpu()
    assert sk.numel() == max(1, plan.info.sketch_len)
    for s, o, P in zip(plan.segments, segs, Ps):
        if s.kind == N.SEG_RAW:
            assert_bitwise(sk[s.sketch_off:s.sketch_off + s.n], P, f"{name} RAW [{s.n}] sketch = b(X)")
            continue
        x = X[o.offset:o.offset + o.numel].view(s.n, s.m)
        v = V[s.v_off:s.v_off + s.m * 4].view(s.m, 4).float()
        d = sk[s.sketch_off:s.sketch_off + s.n * 4].view(s.n, 4).float()
        scale = (x.abs() @ v.abs()).clamp_min(1e-30)
        worst = ((d - P.float()).abs() / scale).max().item()
        print(f"{name} err_in {err_in} [{s.n}, {s.m}]: worst sketch deviation {worst:.3e} of |x| @ |v| (bar 2^-7)")
        bad = ((d - P.float()).abs() > 2.0 ** -7 * scale).sum().item()
        assert bad == 0, f"{name} [{s.n}, {s.m}]: {bad} sketch entries off by more than one rounding"


@pytest.mark.parametrize("shapes", [[[4, 64]], [[3], [4, 64]], [[4, 5464]], [[1], [4, 5461]]])
def test_encode_pairs_columns_with_projections(shapes):
    """G[row][c] = c + 1 (c < 64, else 0) and V[c][j] = [c == j]  ->  sketch[row][j] = j + 1, on the
    16-B path, the element path (odd offset) and the rows whose V is read from global memory."""
    plan = BucketPlan([tuple(s) for s in shapes], 4, 0.25, BF16, DEV)
    s = plan.segments[-1]
    m = int(s.m)
    row = torch.zeros(m)
    row[:64] = torch.arange(64, dtype=torch.float32) + 1
    G = torch.zeros(plan.info.numel)
    G[s.offset:] = row.repeat(4)
    Vi = torch.zeros(m, 4)
    for j in range(4):
        Vi[j, j] = 1.0
    buf, Ed = _guarded(torch.zeros(plan.info.numel))
    _encode(plan, G.to(BF16).to(DEV), Ed, 1, Vi.flatten().to(BF16).to(DEV))
    torch.cuda.synchronize()
    want = torch.tensor([1.0, 2.0, 3.0, 4.0]).repeat(4, 1)
    got = plan.sketch[s.sketch_off:s.sketch_off + 16].view(4, 4).float().cpu()
    assert torch.equal(got, want), got
    assert _guards_intact(buf)


def test_entry_points_refuse_other_plans():
    L = N.lib()
    p32 = BucketPlan([(4, 64)], 4, 0.25, torch.float32, DEV)
    x = torch.zeros(256, device=DEV)
    for st in (L.arctopk_encode_mixed(p32.handle, x.data_ptr(), x.data_ptr(), 0, p32.V_ring[0].data_ptr(),
                                      p32.sketch.data_ptr(), _stream()),
               L.arctopk_pack_mixed(p32.handle, x.data_ptr(), x.data_ptr(), 0, p32.rowlist.data_ptr(),
                                    p32.slotmap.data_ptr(), p32.packed.data_ptr(), _stream())):
        assert st == N.EINVAL
    p16 = BucketPlan([(4, 64)], 4, 0.25, BF16, DEV)
    assert L.arctopk_encode_mixed(p16.handle, x.data_ptr(), x.data_ptr(), 2, p16.V_ring[0].data_ptr(),
                                  p16.sketch.data_ptr(), _stream()) == N.EINVAL  # no zero rows here
    assert L.arctopk_encode_mixed(p16.handle, x.data_ptr(), None, 0, p16.V_ring[0].data_ptr(),
                                  p16.sketch.data_ptr(), _stream()) == N.EINVAL
    torch.cuda.synchronize()


# ---- 2. pack -----------------------------------------------------------------------------
@pytest.mark.parametrize("err_in", [0, 1])
@pytest.mark.parametrize("name", ["mix10", "aligned", "mix10_dense"])
def test_pack_phase(name, err_in):
    """Rows from arctopk_select on the device's own sketch; packed values and E bit-exact given
    them; the row list and the slot map untouched; then the plan's own decode."""
    dense = name.endswith("_dense")
    shapes = ALIGNED if name == "aligned" else MIX10
    G, E0, g = _inputs(shapes, 23)
    plan = BucketPlan([tuple(s) for s in shapes], 4, 0.25, BF16, DEV, flags=N.PLAN_DENSE_1D if dense else 0)
    V = torch.randn(plan.info.v_len, generator=g).to(BF16)
    buf, Ed = _guarded(E0 if err_in else torch.zeros_like(E0))
    Gd = G.to(DEV)
    _encode(plan, Gd, Ed, err_in, V.to(DEV))
    plan.select(1, _stream())
    torch.cuda.synchronize()
    rl0, sm0 = plan.rowlist.clone(), plan.slotmap.clone()
    _pack(plan, Gd, Ed, err_in)
    torch.cuda.synchronize()
    assert torch.equal(plan.rowlist, rl0) and torch.equal(plan.slotmap, sm0)
    assert _guards_intact(buf), "a write outside the residual"
    segs = MX.segments(shapes, 0.25, dense)
    rows = [torch.arange(o.n) if o.kind == MX.DENSE else r for o, r in zip(segs, _rows(plan))]
    for r_, s in zip(rows, plan.segments):
        assert torch.equal(r_, r_.sort().values) and int(r_.max()) < s.n
    X, _ = MX.encode(G, E0 if err_in else None, segs, _plan_Vs(plan, V))
    vals, E_new = MX.pack(X, rows, segs)
    assert_bitwise(plan.packed_values(), vals, f"{name} err_in {err_in}: packed = b(X)")
    assert_bitwise(Ed, E_new, f"{name} err_in {err_in}: E = X - f(packed) on the rows, X elsewhere")
    used = torch.zeros(plan.packed.numel(), dtype=torch.bool)
    for s in plan.segments:
        used[s.packed_off:s.packed_off + s.k_rows * s.m] = True
    assert not plan.packed.cpu()[~used].any(), "the alignment pads of the packed buffer stay zero"
    out = torch.full((plan.info.numel,), 3.0, dtype=BF16, device=DEV)
    plan.decode(1, N.EF14, None, out, _stream())
    torch.cuda.synchronize()
    assert_bitwise(out, A.decode(vals, 1, rows, segs, plan.info.numel, BF16), f"{name}: the plan's decode")
    assert torch.equal(out.float().cpu() + Ed.cpu(), X), "f(out) + E_new == f(G) + E_old"


@pytest.mark.parametrize("err_in", [0, 1])
@pytest.mark.parametrize("name", ["mix10", "aligned"])
def test_pack_without_grad(name, err_in):
    """arctopk_pack_mixed takes grad = NULL for a plan without DENSE segments (a selected row's X is
    the E the encode stored: G is not read): packed values and E bit-exact as in test_pack_phase."""
    shapes = ALIGNED if name == "aligned" else MIX10
    G, E0, g = _inputs(shapes, 23)
    plan = BucketPlan([tuple(s) for s in shapes], 4, 0.25, BF16, DEV)
    V = torch.randn(plan.info.v_len, generator=g).to(BF16)
    buf, Ed = _guarded(E0 if err_in else torch.zeros_like(E0))
    _encode(plan, G.to(DEV), Ed, err_in, V.to(DEV))
    plan.select(1, _stream())
    st = N.lib().arctopk_pack_mixed(plan.handle, None, Ed.data_ptr(), err_in, plan.rowlist.data_ptr(),
                                    plan.slotmap.data_ptr(), plan.packed.data_ptr(), _stream())
    assert st == 0
    torch.cuda.synchronize()
    assert _guards_intact(buf), "a write outside the residual"
    segs = MX.segments(shapes, 0.25)
    X, _ = MX.encode(G, E0 if err_in else None, segs, _plan_Vs(plan, V))
    vals, E_new = MX.pack(X, _rows(plan), segs)
    assert_bitwise(plan.packed_values(), vals, f"{name} err_in {err_in}, grad = NULL: packed = b(X)")
    assert_bitwise(Ed, E_new, f"{name} err_in {err_in}, grad = NULL: E = X - f(packed) on the rows, X elsewhere")


@pytest.mark.parametrize("err_in", [0, 1])
def test_pack_without_grad_refused_with_dense_segments(err_in):
    """A DENSE segment's X = f(G) + E is formed by the pack: grad = NULL is EINVAL (a host check)."""
    plan = BucketPlan([tuple(s) for s in MIX10], 4, 0.25, BF16, DEV, flags=N.PLAN_DENSE_1D)
    Ed = torch.zeros(plan.info.numel, device=DEV)
    st = N.lib().arctopk_pack_mixed(plan.handle, None, Ed.data_ptr(), err_in, plan.rowlist.data_ptr(),
                                    plan.slotmap.data_ptr(), plan.packed.data_ptr(), _stream())
    assert st == N.EINVAL
    torch.cuda.synchronize()
    assert not Ed.any() and not plan.packed.any(), "nothing was launched"


# ---- 3. the hook -------------------------------------------------------------------------
def _hook_state(c4, seed, **kw):
    if c4:  # two ramp calls (restarted draws, ratios 0.8 and 0.525), then steady ones
        st = H4.GroupTopKState(None, r=4, compress_ratio=0.25, start_compress_iter=0, use_error_feedback="ef14",
                               seed=seed, warmup_iters=2)
    else:
        st = H.GroupTopKState(None, r=4, compress_ratio=0.25, start_compress_iter=0, use_error_feedback="ef14",
                              seed=seed)
    st.error_dtype = torch.float32
    for k, v in kw.items():
        setattr(st, k, v)
    return st


@pytest.mark.parametrize("c4,projections,force_exchange", [(False, "device", False), (False, "host", False),
                                                           (True, "device", False), (True, "host", False),
                                                           (False, "device", True), (True, "device", True)])
def test_hook_vs_restatement(c4, projections, force_exchange):
    st = _hook_state(c4, 91, projections=projections, force_exchange=force_exchange)
    hook = H4.group_topk_hook if c4 else H.group_topk_hook
    o = MX.MixedOracle(1, MIX10, 0.25, seed=91, c4=c4, warmup_iters=2)
    n = bucket_numel(MIX10)
    ratios = []
    for it in range(4):
        G = (torch.randn(n, generator=torch.Generator().manual_seed(500 + it)) * 3.0).to(BF16)
        fut = hook(st, SyntheticBucket(G.to(DEV), MIX10, index=0, is_last=True))
        assert fut.done()
        out = fut.wait()
        torch.cuda.synchronize()
        plan = st._plans[0][1]
        res = o.call([G], _rows(plan), proj_device=DEV if projections == "device" else None)
        what = f"c4={c4} {projections} fx={force_exchange} it{it}"
        assert plan.ratio == res["ratio"] and bool(plan.flags & N.PLAN_RESTART_DRAWS) == res["restart"], what
        assert bool(plan.flags & N.PLAN_DENSE_1D) == c4
        ratios.append(plan.ratio)
        assert out.dtype == BF16 and st.error_dict[0].dtype == torch.float32
        assert_bitwise(out, res["out"], what + " out")
        assert_bitwise(st.error_dict[0], o.Es[0], what + " E")
        assert st.comm_bits_this_round == o.bits and st.iter == o.iter
    assert st.mixed_calls == 4 and not st._x_pend
    assert (ratios[0] > ratios[1] > ratios[2] == 0.25) if c4 else ratios == [0.25] * 4
    if force_exchange:
        assert st._comms is not None and st._comms[3].kind == "rccl" and st._comms[3].size == 1


# ---- 4. conservation ---------------------------------------------------------------------
@pytest.mark.parametrize("c4", [False, True])
def test_conservation_at_world_size_one(c4):
    st = _hook_state(c4, 5)
    hook = H4.group_topk_hook if c4 else H.group_topk_hook
    n = bucket_numel(MIX10)
    E_old = torch.zeros(n)
    for it in range(4):
        G = (torch.randn(n, generator=torch.Generator().manual_seed(900 + it)) * 10.0 ** (it - 2)).to(BF16)
        out = hook(st, SyntheticBucket(G.to(DEV), MIX10, index=0, is_last=True)).wait()
        torch.cuda.synchronize()
        E_new = st.error_dict[0].cpu().clone()
        assert torch.equal(out.float().cpu() + E_new, G.float() + E_old), f"call {it}"
        E_old = E_new


# ---- 5. the stall ------------------------------------------------------------------------
@pytest.mark.parametrize("error_dtype,want", [(torch.float32, 37.5), (None, 32.0)])
def test_unselected_rows_stall_in_bf16_and_not_in_fp32(error_dtype, want):
    """[[4, 64]], k = 1: row 0 is 1024 everywhere, rows 1-3 are 0.125.  Rows constant across the
    columns have energies in the ratio of their squares whatever V is, so row 0 is selected every
    call and rows 1-3 accumulate: to 300 * 0.125 = 37.5 in fp32; the bf16 residual stops at
    2^8 * 0.125 = 32 (today's behaviour: that half passes without the option)."""
    st = H.GroupTopKState(None, r=4, compress_ratio=0.25, start_compress_iter=0, use_error_feedback="ef14", seed=8)
    st.error_dtype = error_dtype
    G = torch.full((4, 64), 0.125)
    G[0] = 1024.0
    Gd = G.flatten().to(BF16).to(DEV)
    for _ in range(300):
        out = H.group_topk_hook(st, SyntheticBucket(Gd.clone(), [[4, 64]], index=0, is_last=True)).wait()
    torch.cuda.synchronize()
    E = st.error_dict[0].float().cpu().view(4, 64)
    assert _rows(st._plans[0][1])[0].tolist() == [0]
    assert torch.equal(out.float().cpu().view(4, 64)[0], torch.full((64,), 1024.0))
    assert not E[0].any()
    assert torch.equal(E[1:], torch.full((3, 64), want)), E[1:, :4]


# ---- 6. two ranks ------------------------------------------------------------------------
def _two_rank_worker(rank, ws, port):
    sys.path.insert(0, REPO)
    sys.path.insert(0, HERE)
    torch.set_num_threads(2)
    dist.init_process_group("gloo", init_method=port, rank=rank, world_size=ws)
    st = H.GroupTopKState(None, r=4, compress_ratio=0.25, start_compress_iter=0, use_error_feedback="ef14", seed=77)
    st.error_dtype = torch.float32
    o = MX.MixedOracle(ws, MIX9, 0.25, seed=77)
    n = bucket_numel(MIX9)
    for it in range(3):
        Gl = torch.randn(n, generator=torch.Generator().manual_seed(1000 * it + rank)).to(BF16)
        parts = [torch.empty(n) for _ in range(ws)]
        dist.all_gather(parts, Gl.float())
        allg = [p.to(BF16) for p in parts]
        out = H.group_topk_hook(st, SyntheticBucket(Gl.to(DEV), MIX9)).wait()
        torch.cuda.synchronize()
        plan = st._plans[0][1]
        rl = plan.rowlist.cpu()
        other = [torch.empty_like(rl) for _ in range(ws)]
        dist.all_gather(other, rl)
        assert torch.equal(other[0], other[1]), "ranks selected different rows"
        assert st._comms is not None and st._comms[3].kind == "callback" and st._comms[3].size == ws
        res = o.call(allg, _rows(plan), proj_device=DEV)
        assert_bitwise(out, res["out"], f"it{it} rank{rank} out")
        assert_bitwise(st.error_dict[0], o.Es[rank], f"it{it} rank{rank} E")
        assert st.error_dict[0].dtype == torch.float32
        assert st.comm_bits_this_round == o.bits > 0
    assert st.mixed_calls == 3
    dist.destroy_process_group()


def test_two_ranks_one_gpu():
    mp.spawn(_two_rank_worker, args=(2, rendezvous()), nprocs=2, join=True)


# ---- 7. the option unset -----------------------------------------------------------------
def test_option_unset_is_todays_path():
    """A bf16 bucket without the option: the bf16 residual of the existing step, bit for bit the
    base restatement's given the rows, and the zero-rows encode still runs (it never does on the
    fp32-residual branch)."""
    shapes = [[64, 256], [128], [200, 96]]
    st = H.GroupTopKState(None, r=4, compress_ratio=0.2, start_compress_iter=0, use_error_feedback="ef14", seed=4)
    assert st.error_dtype is None
    ost = A.OracleState(seed=4)
    n = bucket_numel(shapes)
    E = None
    for it in range(3):
        G = torch.randn(n, generator=torch.Generator().manual_seed(40 + it)).to(BF16)
        out = H.group_topk_hook(st, SyntheticBucket(G.to(DEV), shapes, index=0, is_last=True)).wait()
        torch.cuda.synchronize()
        plan = st._plans[0][1]
        res = A.simulate_step([G], [E], None, shapes, 0.2, 4, "ef14", ost.next_seed(), rows_override=_rows(plan),
                              proj_device=DEV)
        assert st.error_dict[0].dtype == BF16
        assert_bitwise(out, res["out"], f"it{it} out")
        assert_bitwise(st.error_dict[0], res["E_new"][0], f"it{it} E")
        E = res["E_new"][0]
    c = ctypes.c_int64(-1)
    N.check(N.lib().arctopk_diag_zero_row_encodes(plan.handle, ctypes.byref(c)), "arctopk_diag_zero_row_encodes")
    assert c.value >= 1 and st.mixed_calls == 0
    # ... and with it, on the same layout: never
    st2 = _hook_state(False, 4)
    for it in range(3):
        G = torch.randn(n, generator=torch.Generator().manual_seed(40 + it)).to(BF16)
        H.group_topk_hook(st2, SyntheticBucket(G.to(DEV), shapes, index=0, is_last=True)).wait()
    torch.cuda.synchronize()
    N.check(N.lib().arctopk_diag_zero_row_encodes(st2._plans[0][1].handle, ctypes.byref(c)), "diag")
    assert c.value == 0 and st2.mixed_calls == 3 and st2.error_dict[0].dtype == torch.float32
