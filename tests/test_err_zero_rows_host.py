"""The hook's EF14 zero-rows bookkeeping on CPU, the native step stubbed: which ``err_in`` reaches
``arctopk_exchange_step`` across a first call, steady state, an in-place edit of the residual,
``residual_touched``, a checkpoint reload, a plan rebuild, the switch and an exception.

(What the library itself then does with ``err_in = 2`` -- its own record of the slot map, the pack
or finalize and the stream -- is tests/test_gpu_err_zero_rows.py.)"""
import pytest

from allreducetopk_amd import _native as N
from allreducetopk_amd.comm_hooks import group_topk_hook_no_reshape as H
from allreducetopk_amd.comm_hooks import group_topk_hook_no_reshape_c4 as H4
from arc_hook_rig import rig as base_rig  # noqa: F401


@pytest.fixture()
def rig(base_rig):  # noqa: F811
    """``call``: one hook call on bucket b, waited for; the err_in its step got."""
    step = base_rig.call

    def call(st, b=0, hook=H.group_topk_hook):
        fut, trace = step(st, b=b, hook=hook)
        fut.wait()
        return [t["err_in"] for t in trace if t.get("call") == "arctopk_exchange_step"][-1]

    base_rig.call = call
    return base_rig


def test_first_call_then_steady_state(rig):
    st = rig.make()
    assert rig.call(st) == N.ERR_IN_NONE
    assert rig.call(st) == N.ERR_IN_ZERO_ROWS
    assert rig.call(st) == N.ERR_IN_ZERO_ROWS
    assert rig.call(st, b=1) == N.ERR_IN_NONE  # buckets are vouched for one by one
    assert rig.call(st, b=1) == N.ERR_IN_ZERO_ROWS
    assert rig.call(st, b=0) == N.ERR_IN_ZERO_ROWS


def test_in_place_edit_turns_it_off_for_one_call(rig):
    st = rig.make()
    rig.call(st), rig.call(st)
    st.error_dict[0].mul_(0.5)  # bumps _version
    assert rig.call(st) == N.ERR_IN_READ
    assert rig.call(st) == N.ERR_IN_ZERO_ROWS
    st.error_dict[0] = st.error_dict[0].clone()  # another tensor
    assert rig.call(st) == N.ERR_IN_READ
    assert rig.call(st) == N.ERR_IN_ZERO_ROWS
    rig.plan(st).slotmap.add_(1)  # a torch op on the slot map
    assert rig.call(st) == N.ERR_IN_READ
    assert rig.call(st) == N.ERR_IN_ZERO_ROWS


def test_residual_touched(rig):
    st = rig.make()
    for b in (0, 1):
        rig.call(st, b), rig.call(st, b)
    st.residual_touched(1)
    assert rig.call(st, 0) == N.ERR_IN_ZERO_ROWS
    assert rig.call(st, 1) == N.ERR_IN_READ
    st.residual_touched()
    assert rig.call(st, 0) == N.ERR_IN_READ
    assert rig.call(st, 1) == N.ERR_IN_READ
    assert rig.call(st, 1) == N.ERR_IN_ZERO_ROWS


def test_reload_resets(rig):
    st = rig.make()
    rig.call(st), rig.call(st)
    st.load_state_dict(st.state_dict())
    assert rig.call(st) == N.ERR_IN_READ
    assert rig.call(st) == N.ERR_IN_ZERO_ROWS


def test_plan_rebuild_resets(rig):
    st = rig.make()
    rig.call(st), rig.call(st)
    st.compress_ratio = 0.5  # another plan for the bucket
    assert rig.call(st) == N.ERR_IN_READ
    assert rig.call(st) == N.ERR_IN_ZERO_ROWS


def test_c4_ramp_moves_the_plan_every_iteration(rig):
    st = rig.make(H4.GroupTopKState, gradual_compression=True, warmup_iters=10)
    seen = [rig.call(st, hook=H4.group_topk_hook) for _ in range(4)]
    assert seen == [N.ERR_IN_NONE, N.ERR_IN_READ, N.ERR_IN_READ, N.ERR_IN_READ]  # the ratio moved
    st.gradual_compression = False
    rig.call(st, hook=H4.group_topk_hook)
    assert rig.call(st, hook=H4.group_topk_hook) == N.ERR_IN_ZERO_ROWS


def test_switch_and_environment(rig, monkeypatch):
    st = rig.make()
    assert st.err_zero_rows is True
    st.err_zero_rows = False
    assert [rig.call(st) for _ in range(3)] == [N.ERR_IN_NONE, N.ERR_IN_READ, N.ERR_IN_READ]
    st.err_zero_rows = True
    assert rig.call(st) == N.ERR_IN_ZERO_ROWS
    monkeypatch.setenv("ARCTOPK_ERR_ZERO_ROWS", "0")
    assert rig.make().err_zero_rows is False


def test_other_ef_modes_never_pass_it(rig):
    st = rig.make(ef="noef")
    assert [rig.call(st) for _ in range(3)] == [1, 1, 1]  # (err_in is unused without EF14)


def test_failed_step_resets(rig):
    st = rig.make()
    rig.call(st), rig.call(st)
    rig.rec.status["arctopk_exchange_step"] = N.EINVAL
    with pytest.raises(Exception):
        rig.call(st)
    rig.rec.status["arctopk_exchange_step"] = 0
    assert rig.call(st) == N.ERR_IN_READ
    assert rig.call(st) == N.ERR_IN_ZERO_ROWS
