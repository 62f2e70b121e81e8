"""The fp32 EF14 zero-rows encode's row walk (a ring of step buffers, DEPTH - 1 steps' loads issued
ahead, the first of them before the V^T staging) at its prologue and epilogue (MI355X, -m gpu).

A step of the walk is 1,024 fp32 columns (64 lanes x 4 units of 16 B); a wave walks the (row, step)
pairs of its tile's rows w, w + 4, ...  One bucket holds every [rows, m] of

  m    64 (a partial step), 1024 (one step), 1028 (one and a 4-column tail), 2048, 3072 (2, 3), 5120
  rows 1, 3, 4, 5, 9, 70

and [8, 8192].  A tile row holds at most 4,096 columns (the V^T slice in LDS), so the plan splits
m = 5120 into two column parts of 2,560 (2.5 steps: three, the last half empty) and [8, 8192] into
two of 4,096 (4 steps, the most a tile row has).  A tensor of fewer than 8 rows is one
tile, so its waves hold 0, 1 or 2 rows; [9, 64] is one tile (3, 2, 2, 2 rows), [70, 64] two of 35 rows
(9 or 8 a wave): a wave holds 0 to 10 pairs, on both sides of any ring depth up to 5, and clamped
lanes in every last step of m = 64 and 1028.  ``encode_tiles`` shows below that every tile of
the bucket is a wave-per-row (vector) tile.

Per ratio (0.2; 0.01: one row selected per tensor; 1.0: every row, no load from E at all) four
hook calls run on a state with ``err_zero_rows`` on and on one with it off (the err_in = 1 kernel),
and are replayed through the CPU oracle given the rows the device selected.  The third call's G has
-0.0 over whole rows and NaNs inside rows the second call zeroed.  Outputs and residuals are compared
as bit patterns.
"""
import ctypes

import pytest
import torch

from allreducetopk_amd import _native as N
from allreducetopk_amd.bucket import SyntheticBucket, bucket_numel
from allreducetopk_amd.comm_hooks.group_topk_hook_no_reshape import GroupTopKState, group_topk_hook
from oracle import arctopk as A
from parity import ensure_group

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MS = [64, 1024, 1028, 2048, 3072, 5120]
ROWS = [1, 3, 4, 5, 9, 70]
SPLIT = [8, 8192]
SHAPES = [[n, m] for m in MS for n in ROWS] + [SPLIT]
SEED = 4242


@pytest.fixture(scope="module", autouse=True)
def group():
    ensure_group("nccl")
    yield


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


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


def make_state(on, ratio):
    st = GroupTopKState(None, r=4, compress_ratio=ratio, start_compress_iter=0, use_error_feedback="ef14",
                        seed=SEED)
    st.defer_decode = True
    st.err_zero_rows = on
    return st


def call(st, G):
    out = group_topk_hook(st, SyntheticBucket(G.to(DEV).clone(), SHAPES, index=0, is_last=True)).wait().clone()
    torch.cuda.synchronize()
    return out, st.error_dict[0].clone()


def plan_of(st):
    return st._plans[0][1]


def rows_of(plan):
    rl = plan.rowlist.cpu()
    return [rl[s.sel_off:s.sel_off + s.k_rows].long() for s in plan.segments]


@pytest.fixture(scope="module")
def grads():
    g = torch.Generator().manual_seed(7)
    return [torch.randn(bucket_numel(SHAPES), generator=g) for _ in range(4)]


@pytest.mark.parametrize("ratio", [0.2, 0.01, 1.0], ids=["rho0.2", "one_row", "every_row"])
def test_ring_walk_same_bits_as_full_read_and_oracle(ratio, grads):
    on, off = make_state(True, ratio), make_state(False, ratio)
    ost = A.OracleState(r=4, compress_ratio=ratio, start_compress_iter=0, use_error_feedback="ef14", seed=SEED)
    E = None
    for it in range(4):
        G = grads[it].clone()
        if it == 2:
            # rows the last call selected (all zeros in E now): -0.0 over the whole row of every
            # second tensor (X = -0.0 + 0 is stored as +0.0), NaNs inside the row of the others
            for si, (s, sel) in enumerate(zip(plan_of(on).segments, rows_of(plan_of(on)))):
                row = G[s.offset:s.offset + s.n * s.m].view(s.n, s.m)[int(sel[0])]
                if si % 2:
                    row[:] = -0.0
                else:
                    row[(3 * si) % s.m::97] = float("nan")
        o1, e1 = call(on, G)
        o0, e0 = call(off, G)
        same_bits(o1, o0, f"call {it}: output, zero rows on / off")
        same_bits(e1, e0, f"call {it}: residual, zero rows on / off")
        plan = plan_of(on)
        if it == 0:
            t = plan.encode_tiles()
            assert t["row_vec"] > 0 and t["raw"] == t["tile"] == t["row_scalar"] == 0, t
            assert t["n_split"] == len(ROWS) + 1, t  # every m = 5120 tensor and [8, 8192]
            ks = [s.k_rows for s in plan.segments]
            if ratio == 0.01:
                assert set(ks) == {1}
            if ratio == 1.0:
                assert ks == [s.n for s in plan.segments]
        res = A.simulate_step([G], [E], None, SHAPES, ratio, 4, "ef14", ost.next_seed(), rows_override=rows_of(plan),
                              proj_device=DEV)
        same_bits(o1, res["out"], f"call {it}: output against the oracle")
        same_bits(e1, res["E_new"][0], f"call {it}: residual against the oracle")
        E = res["E_new"][0]
        same_bits(plan.slotmap, plan_of(off).slotmap, f"call {it}: slot map")
        # every call from the second on ran the zero-rows kernel; none with the feature off
        assert zr_count(plan) == it and zr_count(plan_of(off)) == 0
