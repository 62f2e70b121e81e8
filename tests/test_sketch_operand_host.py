"""``GroupTopKState.sketch_operand_dtype`` on CPU: the switch, its validation and the decision the hook
takes per bucket, and the setter's refusal of a null plan.  (The kernel, the other refusals and the hook
on a GPU: tests/test_gpu_sketch_operand.py.)"""
import pytest
import torch

from allreducetopk_amd import _native as N
from allreducetopk_amd.comm_hooks import group_topk_hook_no_reshape_c4 as H4
from arc_hook_rig import rig  # noqa: F401

F32, BF16 = torch.float32, torch.bfloat16


def test_env_default_and_bad_values(rig, monkeypatch):  # noqa: F811
    st = rig.make(r=32)
    assert st.sketch_operand_dtype is None and st.state_dict()["sketch_operand_dtype"] is None
    assert st._sketch_op16(F32) is False
    monkeypatch.setenv("ARCTOPK_SKETCH_OPERAND_DTYPE", "bf16")
    st = rig.make(H4.GroupTopKState, r=16)  # the c4 state inherits it
    assert st.sketch_operand_dtype is BF16 and st.state_dict()["sketch_operand_dtype"] == "bf16"
    assert st._sketch_op16(F32) is True and st._sketch_op16(BF16) is False  # a bf16 bucket: nothing to do
    for bad in ("fp32", "bfloat16", "1"):
        monkeypatch.setenv("ARCTOPK_SKETCH_OPERAND_DTYPE", bad)
        with pytest.raises(ValueError, match="ARCTOPK_SKETCH_OPERAND_DTYPE"):
            rig.make()


@pytest.mark.parametrize("r,value", [(32, torch.float16), (16, "bf16"), (16, True), (4, BF16), (8, BF16)])
def test_other_values_and_ranks_raise_before_any_call(rig, r, value):  # noqa: F811
    st = rig.make(r=r)
    st.sketch_operand_dtype = value
    with pytest.raises(ValueError, match="sketch_operand_dtype"):
        rig.call(st)
    assert not st.error_dict and not rig.rec.trace
    if value is BF16:
        with pytest.raises(ValueError, match="sketch_operand_dtype"):
            rig.call(st, dtype=BF16)  # the rank is refused whatever the bucket


def test_setter_refuses_a_null_plan_without_a_device():
    assert "arctopk_plan_set_sketch_operands" in N.EXPORTS
    assert N.lib().arctopk_plan_set_sketch_operands(None, N.BF16) == N.EINVAL
