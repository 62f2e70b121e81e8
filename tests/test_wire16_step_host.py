"""``GroupTopKState.wire_exchange`` on CPU, the native library stubbed: the option and its
validation, which native calls a bf16-wire bucket makes with ``wire_exchange="step"`` (the plan
bound to its bf16 buffer, then ONE arctopk_exchange_step, deferred like the default path's), the
scatter of the zero-ahead drain restated in torch ops against wire16_oracle's whole decode, and the
new entry points' declarations against their ctypes bindings.

(The kernels and the hook on a GPU: tests/test_gpu_wire16_step.py.)"""
import os
import re

import pytest
import torch

import arc_hook_rig as R
import wire16_oracle as W
from allreducetopk_amd import _native as N
from allreducetopk_amd.bucket import bucket_numel
from allreducetopk_amd.comm_hooks import group_topk_hook_no_reshape as H
from allreducetopk_amd.comm_hooks import group_topk_hook_no_reshape_c4 as H4
from arc_hook_rig import SHAPES, rig as base_rig  # noqa: F401

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16 = torch.bfloat16
MIXA = [[16, 64], [5], [64, 128], [100, 72], [9, 100], [8, 4, 3, 3], [16, 8, 1, 1], [8, 40], [4, 5461], [7]]
ALIGNB = [[4, 4], [32, 2048], [6, 24], [10, 24], [16, 64]]
LAYOUTS = {"mixa": (MIXA, False), "alignb": (ALIGNB, False), "mixa_dense": (MIXA, True)}


# what the tests below compare of each record (the rest of it: tests/test_arc_hook_calls_host.py)
FIELDS = {"exchange_step": ("err_in", "defer", "sel_stream", "trail"), "plan_bind_wire16": ("packed_bf16",),
          "encode": ("ef", "err_in"), "select": ("world_size",), "pack_wire16": ("ef", "err_in"),
          "decode_wire16": ("ef", "world_size"), "comm_allreduce": ("count", "dtype")}


@pytest.fixture()
def rig(base_rig):  # noqa: F811
    """``call``: one hook call of an fp32 bucket: (its Future, the calls it made, by FIELDS)."""
    step = base_rig.call

    def call(st, dtype=torch.float32, b=0, hook=H.group_topk_hook, is_last=True):
        fut, trace = step(st, dtype=dtype, b=b, hook=hook, is_last=is_last)
        return fut, R.brief(trace, FIELDS)

    base_rig.call = call
    return base_rig


# ---- 1. the option -----------------------------------------------------------------------------
def test_default_and_environment(rig, monkeypatch):
    st = rig.make()
    assert st.wire_exchange == "inline" and st.wire16_step_calls == 0
    assert st.state_dict()["wire_exchange"] == "inline"
    monkeypatch.setenv("ARCTOPK_WIRE_EXCHANGE", "step")
    assert rig.make().wire_exchange == "step"
    assert rig.make(H4.GroupTopKState).wire_exchange == "step"  # the c4 state inherits it
    assert rig.make().state_dict()["wire_exchange"] == "step"
    for bad in ("inline", "1", "STEP", "exchange"):
        monkeypatch.setenv("ARCTOPK_WIRE_EXCHANGE", bad)
        with pytest.raises(ValueError, match="ARCTOPK_WIRE_EXCHANGE"):
            rig.make()


@pytest.mark.parametrize("bad", ["Step", "", None, True, 1, "pipelined"])
def test_other_values_raise_at_the_first_compressed_call(rig, bad):
    st = rig.make()
    st.wire_dtype = BF16
    st.wire_exchange = bad
    with pytest.raises(ValueError, match="wire_exchange"):
        rig.call(st)
    assert not st.error_dict and not rig.rec.trace


def test_no_effect_without_the_bf16_wire(rig):
    st = rig.make()
    st.wire_exchange = "step"
    fut, calls = rig.call(st)  # wire_dtype None: today's default step, no binding
    assert fut.done() and calls == [("exchange_step", N.ERR_IN_NONE, 0, "NULL", "NULL")]
    st.wire_dtype = BF16
    fut, calls = rig.call(st, dtype=BF16, b=1)  # a bf16 bucket ignores both options
    assert calls == [("exchange_step", N.ERR_IN_NONE, 0, "NULL", "NULL")]
    assert st.wire16_calls == st.wire16_step_calls == 0 and st.error_dict[1].dtype == BF16


def test_host_staged_takes_precedence(rig):
    st = rig.make()
    st.wire_dtype, st.wire_exchange, st.host_staged = BF16, "step", True
    with pytest.raises(ValueError, match="host_staged"):
        rig.call(st)
    assert not st.error_dict and not rig.rec.trace


def test_inline_is_untouched(rig):
    st = rig.make()
    st.wire_dtype = BF16
    fut, calls = rig.call(st)
    assert fut.done() and [c[0] for c in calls] == ["encode", "select", "pack_wire16", "decode_wire16"]
    assert st.wire16_calls == 1 and st.wire16_step_calls == 0


# ---- 2. the step branch ------------------------------------------------------------------------
@pytest.mark.parametrize("ef,code", [("noef", N.EF_NONE), ("ef14", N.EF14)])
def test_step_branch_makes_one_native_call(rig, ef, code):
    st = rig.make(ef=ef)
    st.wire_dtype, st.wire_exchange = BF16, "step"
    st.err_zero_rows = True
    first = N.ERR_IN_NONE if ef == "ef14" else N.ERR_IN_READ
    fut, calls = rig.call(st)
    assert fut.done() and calls == [("plan_bind_wire16", "packed16"), ("exchange_step", first, 0, "NULL", "NULL")]
    plan = rig.plan(st)
    assert plan.wire16_bound and plan.packed16.dtype == BF16 and plan.packed16.numel() == 80 and not plan.packed16.any()
    # bound once; the residual is read from the second call on; zero rows (err_in = 2) are never claimed
    for _ in range(2):
        assert rig.call(st)[1] == [("exchange_step", N.ERR_IN_READ, 0, "NULL", "NULL")]
    assert st.wire16_step_calls == st.wire16_calls == 3 and not st._zr and not st._x_pend
    assert st.comm_bits_this_round == 0 and st.iter == 3
    # the option can change between calls: the default step unbinds the plan, and may claim zero rows again
    st.wire_dtype = None
    assert rig.call(st)[1] == [("plan_bind_wire16", "NULL"), ("exchange_step", N.ERR_IN_READ, 0, "NULL", "NULL")]
    assert not plan.wire16_bound and st.wire16_calls == 3
    if ef == "ef14":
        assert rig.call(st)[1] == [("exchange_step", N.ERR_IN_ZERO_ROWS, 0, "NULL", "NULL")]
        st.wire_dtype = BF16  # ... whose record a bf16-wire step drops
        assert rig.call(st)[1] == [("plan_bind_wire16", "packed16"), ("exchange_step", N.ERR_IN_READ, 0, "NULL", "NULL")]
        st.wire_dtype = None
        assert rig.call(st)[1] == [("plan_bind_wire16", "NULL"), ("exchange_step", N.ERR_IN_READ, 0, "NULL", "NULL")]


def test_step_branch_defers_like_the_default_path(rig):
    st = rig.make()
    st.wire_dtype, st.wire_exchange, st.defer_decode = BF16, "step", True
    f0, c0 = rig.call(st, b=0, is_last=False)
    assert isinstance(f0, H.ExchangeFuture) and not f0.done() and len(st._x_pend) == 1
    assert c0 == [("plan_bind_wire16", "packed16"), ("exchange_step", N.ERR_IN_NONE, 1, "NULL", "NULL")]
    f1, c1 = rig.call(st, b=1, is_last=True)  # the backward's last bucket finishes everything pending
    assert c1 == [("plan_bind_wire16", "packed16"), ("exchange_step", N.ERR_IN_NONE, 0, "NULL", "NULL")]
    assert f0.done() and f1.done() and not st._x_pend and st.wire16_step_calls == 2
    f2, _ = rig.call(st, b=0, is_last=False)
    assert not f2.done()
    st.flush_exchange()
    assert f2.done() and not st._x_pend and rig.rec.trace[-1]["call"] == "arctopk_exchange_finish"
    # the c4 hook inherits the branch
    st4 = rig.make(H4.GroupTopKState)
    st4.wire_dtype, st4.wire_exchange = BF16, "step"
    assert [c[0] for c in rig.call(st4, hook=H4.group_topk_hook)[1]] == ["plan_bind_wire16", "exchange_step"]


def test_step_branch_takes_no_groups_select_stream_or_trail(rig):
    st = rig.make(ws=2)
    st.wire_dtype, st.wire_exchange, st.defer_decode = BF16, "step", True
    st.exchange_groups, st.select_streams, st.trail_bytes = "all", "on", 1 << 30
    fut, calls = rig.call(st, is_last=False)  # (a grouped bucket would make one step per group)
    assert calls == [("plan_bind_wire16", "packed16"), ("exchange_step", N.ERR_IN_NONE, 1, "NULL", "NULL")]
    assert st.trail_calls == 0 and st._trail is None and len(st._x_pend) == 1
    # bits: the sketch in fp32, the selected values in bf16; the bf16 buffer is registered
    segs = W.segments(SHAPES, 0.2)
    assert st.comm_bits_this_round == 2 * (2 - 1) * W.bits_per_call(segs, 4)
    plan = rig.plan(st)
    assert any(t is plan.packed16 for t in st._comms[3].registered) and plan.packed16_registered is st._comms[3]
    st.flush_exchange()
    assert fut.done()


# ---- 3. the scatter restated -------------------------------------------------------------------
def _scatter(vsum: torch.Tensor, ws: int, rows, segs, numel: int) -> torch.Tensor:
    """The zero-ahead drain in torch ops: zero the bucket, then write the selected rows' means."""
    out = torch.zeros(numel)
    off = 0
    for s, idx in zip(segs, rows):
        out[s.offset:s.offset + s.numel].view(s.n, s.m)[idx] = (W.f(vsum[off:off + s.k]) / ws).view(-1, s.m)
        off += s.k
    assert off == vsum.numel()
    return out


@pytest.mark.parametrize("ws", [1, 2, 3])
@pytest.mark.parametrize("ef", ["noef", "ef14"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_scatter_restatement_is_the_whole_decode(layout, ef, ws):
    shapes, dense = LAYOUTS[layout]
    segs = W.segments(shapes, 0.25, dense)
    g = torch.Generator().manual_seed(7)
    n = bucket_numel(shapes)
    rows = W.full_rows([torch.randperm(s.n, generator=g)[:s.k_rows].sort().values for s in segs], segs)
    G = torch.randn(n, generator=g)
    E = torch.randn(n, generator=g) * 0.4 if ef == "ef14" else None
    vals = [W.pack(G, E, ef, rows, segs)[0]] + [W.b(torch.randn(sum(s.k for s in segs), generator=g)) for _ in range(1, ws)]
    vsum = W.wire_sum(vals)
    want, _ = W.decode(vsum, ws, rows, segs, n, ef, None)
    got = _scatter(vsum, ws, rows, segs, n)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert 0 < got.count_nonzero() < n or dense


# ---- 4. the C ABI ------------------------------------------------------------------------------
def _declared_args(name: str) -> int:
    with open(os.path.join(REPO, "include", "arctopk.h")) as fh:
        text = fh.read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in include/arctopk.h"
    return len([a for a in m.group(1).split(",") if a.strip()])


@pytest.mark.parametrize("name,nargs", [("arctopk_plan_bind_wire16", 2), ("arctopk_decode_wire16_scatter", 7),
                                        ("arctopk_diag_wire16_scatters", 2)])
def test_entry_points_are_declared_and_bound(name, nargs):
    assert _declared_args(name) == nargs
    restype, argtypes = N._SIGS[name]
    assert restype is N.c_int32 and len(argtypes) == nargs
