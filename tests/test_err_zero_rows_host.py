"""The hook's EF14 zero-rows bookkeeping on CPU, the native step stubbed: which ``err_in`` reaches
``arctopk_exchange_step`` across a first call, steady state, an in-place edit of the residual,
``residual_touched``, a checkpoint reload, a plan rebuild, the switch and an exception.

(What the library itself then does with ``err_in = 2`` -- its own record of the slot map, the pack
or finalize and the stream -- is tests/test_gpu_err_zero_rows.py.)"""
import types

import pytest
import torch

from allreducetopk_amd import _native as N
from allreducetopk_amd.bucket import SyntheticBucket, bucket_numel
from allreducetopk_amd.comm_hooks import group_topk_hook_no_reshape as H
from allreducetopk_amd.comm_hooks import group_topk_hook_no_reshape_c4 as H4

SHAPES = [[8, 64], [16]]


class _Lib:
    """Stands in for libarctopk: records the err_in of every step, fails on request."""

    def __init__(self):
        self.err_in = []
        self.fail = 0

    def arctopk_exchange_step(self, handle, x, e, g, ef, err_in, *rest):
        self.err_in.append(err_in)
        return self.fail

    def arctopk_exchange_finish(self, *a):
        return 0


class _Plan:
    """What the hook touches of a BucketPlan on the native path."""

    def __init__(self):
        self.handle = object()
        self.slotmap = torch.zeros(24, dtype=torch.int32)
        self.bits_sum = 0
        self.philox_advance = 0
        self.comm_registered = None


@pytest.fixture()
def rig(monkeypatch):
    lib = _Lib()
    monkeypatch.setattr(H, "_LIB", [lib])
    monkeypatch.setattr(N, "lib", lambda: lib)
    monkeypatch.setattr(H, "_reseed_global", lambda *a, **k: None)
    monkeypatch.setattr(H, "_current_raw_stream", lambda dix: 0)
    monkeypatch.setattr(H, "_claim_projections", lambda *a, **k: False)
    monkeypatch.setattr(H, "_predraw_target", lambda *a, **k: (None, 0))
    group = types.SimpleNamespace(size=lambda: 1)  # (the hook only asks a group for its size here)
    plans = {}

    def make(cls=H.GroupTopKState, ef="ef14", **kw):
        st = cls(group, r=4, compress_ratio=0.2, start_compress_iter=0, use_error_feedback=ef, **kw)
        st.select_streams = "off"
        st.defer_decode = False
        st.trail_bytes = 0
        st._plan_for = lambda bucket, buf=None: plans.setdefault((bucket.index(), st._plan_ratio()), _Plan())
        return st

    def call(st, b=0, hook=H.group_topk_hook):
        G = torch.ones(bucket_numel(SHAPES))
        hook(st, SyntheticBucket(G, SHAPES, index=b)).wait()
        return lib.err_in[-1]

    return types.SimpleNamespace(lib=lib, make=make, call=call, plans=plans)


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
    rig.plans[(0, 0.2)].slotmap.add_(1)  # a torch op on the slot map
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
    rig.lib.fail = N.EINVAL
    with pytest.raises(Exception):
        rig.call(st)
    rig.lib.fail = 0
    assert rig.call(st) == N.ERR_IN_READ
    assert rig.call(st) == N.ERR_IN_ZERO_ROWS
