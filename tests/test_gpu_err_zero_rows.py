"""EF14 zero rows (err_in = 2): the encode skips the residual rows the previous step zeroed and
computes the same bits (MI355X, -m gpu).

Buckets (ratio 0.2, r 4; one hook state with ``err_zero_rows`` on, one with it off, same inputs):

  A  [[64, 256], [37, 1000], [4096, 64], [8, 8192], [5, 67], [32, 4, 3, 3], [300]]
       wave-per-row tiles of whole rows; 128 interleaved tiles (rstride 128) for [4096, 64]; a
       column-split tensor (two parts of 4096 columns); scalar rows (m = 67); thread-per-row
       tiles (m = 36); a 1-D tensor.  Every 2-D offset is a multiple of 8 elements, so the same
       tensors take the vector paths in bf16.
  B  [[2048, 128], [16, 2048], [1, 512]]
       the last tensor has one row: k = n, every row selected on every call.
  C  [[540672, 64]] bf16: 264 rows per tile, 66 per wave -- a wave walks past the 64 rows one
       slot-map lookup covers.

``arctopk_diag_zero_row_encodes`` counts the encode launches of a plan that ran the zero-rows
kernel: it proves below that the path was taken, or refused.  Outputs and residuals are compared
as bit patterns (-0.0 differs from +0.0, a NaN equals itself).
"""
import ctypes

import pytest
import torch

from allreducetopk_amd import _native as N
from allreducetopk_amd.bucket import SyntheticBucket, bucket_numel
from allreducetopk_amd.comm_hooks.group_topk_hook_no_reshape import BucketPlan, GroupTopKState, group_topk_hook
from oracle import arctopk as A
from parity import ensure_group

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES_A = [[64, 256], [37, 1000], [4096, 64], [8, 8192], [5, 67], [32, 4, 3, 3], [300]]
SHAPES_B = [[2048, 128], [16, 2048], [1, 512]]
SHAPES_C = [[540672, 64]]
BUCKETS = [SHAPES_A, SHAPES_B]


@pytest.fixture(scope="module", autouse=True)
def group():
    ensure_group("nccl")
    yield


def _bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16).cpu()


def same_bits(a, b, what):
    a, b = _bits(a), _bits(b)
    assert a.shape == b.shape, what
    if not torch.equal(a, b):
        i = int(torch.nonzero(a != b)[0])
        raise AssertionError(f"{what}: {int((a != b).sum())} elements differ, first at {i}: "
                             f"{int(a[i]):#x} vs {int(b[i]):#x}")


def zr_count(plan) -> int:
    c = ctypes.c_int64(-1)
    N.check(N.lib().arctopk_diag_zero_row_encodes(plan.handle, ctypes.byref(c)), "arctopk_diag_zero_row_encodes")
    return int(c.value)


def make_state(on, force_exchange=False, seed=1234, ratio=0.2, r=4):
    st = GroupTopKState(None, r=r, compress_ratio=ratio, start_compress_iter=0, use_error_feedback="ef14",
                        seed=seed)
    st.force_exchange = force_exchange
    st.defer_decode = True  # Futures waited after the backward's last bucket, as DDP does
    st.err_zero_rows = on
    return st


def backward(st, grads, buckets=BUCKETS):
    """One backward: bucket j = grads[j]; returns the outputs and residuals (copies)."""
    futs = []
    for j, (shapes, G) in enumerate(zip(buckets, grads)):
        futs.append(group_topk_hook(st, SyntheticBucket(G.to(DEV).clone(), shapes, index=j,
                                                         is_last=(j == len(grads) - 1))))
    outs = [f.wait().clone() for f in futs]
    torch.cuda.synchronize()
    return outs, [st.error_dict[j].clone() for j in range(len(grads))]


def randn_grads(seed, dtype=torch.float32, buckets=BUCKETS):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(bucket_numel(s), generator=g).to(dtype) for s in buckets]


def plans(st, n=2):
    return [st._plans[j][1] for j in range(n)]


def rows_of(plan):
    rl = plan.rowlist.cpu()
    return [rl[s.sel_off:s.sel_off + s.k_rows].long() for s in plan.segments]


def compare(on, off, grads, what, buckets=BUCKETS):
    o1, e1 = backward(on, grads, buckets)
    o0, e0 = backward(off, grads, buckets)
    for j in range(len(grads)):
        same_bits(o1[j], o0[j], f"{what}: bucket {j} output")
        same_bits(e1[j], e0[j], f"{what}: bucket {j} residual")
    return o1, e1


@pytest.mark.parametrize("force_exchange", [False, True], ids=["step", "exchange"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_same_bits_as_with_the_feature_off(dtype, force_exchange):
    on, off = make_state(True, force_exchange), make_state(False, force_exchange)
    for it in range(4):
        compare(on, off, randn_grads(100 + it, dtype), f"backward {it}")
        # every call from the second on ran the zero-rows encode; none with the feature off
        assert [zr_count(p) for p in plans(on)] == [it, it]
        assert [zr_count(p) for p in plans(off)] == [0, 0]


def test_signed_zero_nan_inf_and_moving_selections():
    """-0.0, NaN and +-inf in G inside rows the previous step selected; a tensor whose previous
    selection does not repeat; a tensor with every row selected ([1, 512] of bucket B)."""
    on, off = make_state(True), make_state(False)
    compare(on, off, randn_grads(1), "backward 0")
    segs = plans(on)[0].segments
    sel1 = rows_of(plans(on)[0])
    # backward 1: -0.0 over every row of [64, 256] and [4096, 64] (segments 0 and 2) selected at
    # backward 0: X = -0.0 + 0 must be stored as +0.0; their energy is 0, so the selection moves
    # to other rows entirely
    g = randn_grads(2)
    for si in (0, 2):
        s = segs[si]
        g[0][s.offset:s.offset + s.n * s.m].view(s.n, s.m)[sel1[si]] = -0.0
    _, e = compare(on, off, g, "backward 1 (-0.0)")
    sel2 = rows_of(plans(on)[0])
    for si in (0, 2):
        s = segs[si]
        assert not set(sel1[si].tolist()) & set(sel2[si].tolist()), "the selection was to move"
        rows = e[0][s.offset:s.offset + s.n * s.m].view(s.n, s.m)[sel1[si].to(DEV)]
        assert torch.all(_bits(rows) == 0), "-0.0 + 0 is +0.0"
    assert [zr_count(p) for p in plans(on)] == [1, 1]
    # backward 2: NaN and +-inf in rows selected at backward 1 (wave-per-row, column-split and
    # the one-row tensor)
    g = randn_grads(3)
    for si, vals in ((0, (float("nan"), float("inf"))), (3, (float("-inf"), float("nan"))), (1, (float("inf"),))):
        s = segs[si]
        view = g[0][s.offset:s.offset + s.n * s.m].view(s.n, s.m)
        for k, v in enumerate(vals):
            view[sel2[si][k % len(sel2[si])], (7 * k + 3) % s.m::5] = v
    g[1][-512:][::3] = float("nan")  # the [1, 512] tensor of bucket B: k = n
    g[1][-512:][1::3] = -0.0
    compare(on, off, g, "backward 2 (NaN, inf)")
    compare(on, off, randn_grads(4), "backward 3")
    assert [zr_count(p) for p in plans(on)] == [3, 3]
    assert plans(on)[1].segments[2].k_rows == plans(on)[1].segments[2].n == 1


def test_rows_past_one_lookup_bf16():
    """Bucket C: 66 rows per wave, two slot-map lookups."""
    on, off = make_state(True), make_state(False)
    n = bucket_numel(SHAPES_C)
    for it in range(3):
        G = torch.randn(n, device=DEV, generator=torch.Generator(DEV).manual_seed(40 + it)).to(torch.bfloat16)
        compare(on, off, [G], f"backward {it}", buckets=[SHAPES_C])
        assert zr_count(plans(on, 1)[0]) == it
    assert zr_count(plans(off, 1)[0]) == 0


@pytest.mark.parametrize("force_exchange", [False, True], ids=["step", "exchange"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_against_the_oracle(dtype, force_exchange):
    """Every call replayed through the CPU oracle given the rows the device selected (read from the
    plan's row list; no select is re-run on the plan, which would end the zero-rows record), on
    the step path and on the N > 1 code path over one-rank communicators."""
    st = make_state(True, force_exchange, seed=77)
    ost = A.OracleState(r=4, compress_ratio=0.2, start_compress_iter=0, use_error_feedback="ef14", seed=77)
    E = [None, None]
    for it in range(4):
        grads = randn_grads(300 + it, dtype)
        outs, errs = backward(st, grads)
        for j, shapes in enumerate(BUCKETS):
            seed = ost.next_seed()
            plan = plans(st)[j]
            rows = rows_of(plan)
            res = A.simulate_step([grads[j]], [E[j]], None, shapes, 0.2, 4, "ef14", seed, rows_override=rows,
                                  proj_device=DEV)
            same_bits(outs[j], res["out"], f"backward {it} bucket {j} output")
            same_bits(errs[j], res["E_new"][0], f"backward {it} bucket {j} residual")
            E[j] = res["E_new"][0]
        assert [zr_count(p) for p in plans(st)] == [it, it]


# ---- refusals: the call after the disturbance reads the whole residual (counter unchanged for
# ---- that bucket) and computes what the "off" state computes; the call after it skips again

def _warm():
    on, off = make_state(True), make_state(False)
    for it in range(2):
        compare(on, off, randn_grads(10 + it), f"backward {it}")
    assert [zr_count(p) for p in plans(on)] == [1, 1]
    return on, off


def test_refused_after_in_place_edit_of_the_residual():
    on, off = _warm()
    for st in (on, off):
        st.error_dict[0].add_(1.0)  # non-zero values into the rows the last step zeroed
    compare(on, off, randn_grads(20), "after the edit")
    assert [zr_count(p) for p in plans(on)] == [1, 2]  # bucket 0 refused (by the hook), bucket 1 not
    compare(on, off, randn_grads(21), "one later")
    assert [zr_count(p) for p in plans(on)] == [2, 3]


def test_refused_after_a_select_on_another_sketch():
    on, off = _warm()
    for st in (on, off):
        p = plans(st)[0]
        p.sketch.normal_()
        p.select(1, torch.cuda.current_stream().cuda_stream)  # rewrites the row list and slot map
    torch.cuda.synchronize()
    compare(on, off, randn_grads(22), "after the select")
    assert [zr_count(p) for p in plans(on)] == [1, 2]  # refused by the library's own record
    compare(on, off, randn_grads(23), "one later")
    assert [zr_count(p) for p in plans(on)] == [2, 3]


def test_refused_after_a_checkpoint_reload():
    on, off = _warm()
    for st in (on, off):
        st.load_state_dict(st.state_dict())
    compare(on, off, randn_grads(24), "after the reload")
    assert [zr_count(p) for p in plans(on)] == [1, 1]
    compare(on, off, randn_grads(25), "one later")
    assert [zr_count(p) for p in plans(on)] == [2, 2]


def test_refused_after_a_changed_ratio():
    on, off = _warm()
    old = plans(on)
    for st in (on, off):
        st.compress_ratio = 0.3
    compare(on, off, randn_grads(26), "new plans")
    assert all(a is not b for a, b in zip(old, plans(on)))
    assert [zr_count(p) for p in plans(on)] == [0, 0]
    compare(on, off, randn_grads(27), "one later")
    assert [zr_count(p) for p in plans(on)] == [1, 1]


def test_refused_on_another_stream():
    on, off = _warm()
    other = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(other):
        o1, e1 = backward(on, randn_grads(28))
    o0, e0 = backward(off, randn_grads(28))
    for j in range(2):
        same_bits(o1[j], o0[j], f"other stream: bucket {j} output")
        same_bits(e1[j], e0[j], f"other stream: bucket {j} residual")
    # the finalizes of backward 1 ran on the default stream: nothing orders this stream after them
    assert [zr_count(p) for p in plans(on)] == [1, 1]
    with torch.cuda.stream(other):  # ... but it is the stream of backward 2's own finalizes
        backward(on, randn_grads(29))
    assert [zr_count(p) for p in plans(on)] == [2, 2]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_refused_on_a_freshly_bound_plan_c_api(dtype):
    """arctopk_encode(err_in = 2) on a plan no pack or finalize has run on: it reads all of E,
    whatever the bound slot map holds."""
    n = bucket_numel(SHAPES_B)
    gen = torch.Generator().manual_seed(9)
    G = torch.randn(n, generator=gen).to(dtype).to(DEV)
    E0 = torch.randn(n, generator=gen).to(dtype).to(DEV)
    res, Vh = [], None
    for err_in in (N.ERR_IN_ZERO_ROWS, N.ERR_IN_READ):
        plan = BucketPlan(SHAPES_B, 4, 0.2, dtype, torch.device(DEV))
        plan.slotmap.zero_()  # "every row selected", were it believed
        if Vh is None:
            Vh = torch.randn(plan.V_ring[0].numel(), generator=gen).to(dtype)
        V = plan.V_ring[0].copy_(Vh)
        E = E0.clone()
        plan.encode(G, E, N.EF14, err_in, V, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert zr_count(plan) == 0
        res.append((E, plan.sketch.clone()))
    same_bits(res[0][0], res[1][0], "residual")
    same_bits(res[0][1], res[1][1], "sketch")
