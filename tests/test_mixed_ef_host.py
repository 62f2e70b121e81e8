"""``GroupTopKState.error_dtype`` on CPU, the native library stubbed: the switch and its
validation, which native calls the compressed call of a bf16 bucket makes with it, the EF21
refusal, checkpoints, and the arithmetic the option exists for (the bf16 residual's stall at
2^8 g, the restatement's conservation identity).

(The kernels and the hook on a GPU: tests/test_gpu_mixed_ef.py.)"""
import types

import pytest
import torch

import mixed_ef_oracle as MX
from allreducetopk_amd import _native as N
from allreducetopk_amd.bucket import SyntheticBucket, bucket_numel
from allreducetopk_amd.comm_hooks import group_topk_hook_no_reshape as H
from allreducetopk_amd.comm_hooks import group_topk_hook_no_reshape_c4 as H4

SHAPES = [[8, 64], [16]]
BF16 = torch.bfloat16


class _Lib:
    """Stands in for libarctopk: records the native calls of a hook call in order."""

    def __init__(self):
        self.calls = []

    def arctopk_exchange_step(self, handle, x, e, g, ef, err_in, *rest):
        self.calls.append(("exchange_step", err_in))
        return 0

    def arctopk_exchange_finish(self, *a):
        return 0

    def arctopk_encode_mixed(self, handle, g, e, err_in, v, sk, stream):
        self.calls.append(("encode_mixed", err_in))
        return 0

    def arctopk_pack_mixed(self, handle, g, e, err_in, rl, sm, pk, stream):
        self.calls.append(("pack_mixed", err_in))
        return 0


class _Plan:
    """What the hook touches of a BucketPlan."""

    def __init__(self, lib):
        self.lib = lib
        self.handle = object()
        self.slotmap = torch.zeros(24, dtype=torch.int32)
        self.rowlist = torch.zeros(24, dtype=torch.int32)
        self.sketch = torch.zeros(64, dtype=BF16)
        self.packed = torch.zeros(64, dtype=BF16)
        self.V_ring = [torch.zeros(256, dtype=BF16)]
        self.info = types.SimpleNamespace(sketch_len=48, packed_len=64, v_len=256)
        self.bits_sum = 1000
        self.philox_advance = 0
        self.comm_registered = None

    def select(self, ws, stream, *a):
        self.lib.calls.append(("select", ws))

    def decode(self, ws, ef, gerr, out, stream):
        self.lib.calls.append(("decode", ef))


@pytest.fixture()
def rig(monkeypatch):
    lib = _Lib()
    monkeypatch.delenv("ARCTOPK_ERROR_DTYPE", raising=False)
    monkeypatch.setattr(H, "_LIB", [lib])
    monkeypatch.setattr(N, "lib", lambda: lib)
    monkeypatch.setattr(H, "_reseed_global", lambda *a, **k: None)
    monkeypatch.setattr(H, "_current_raw_stream", lambda dix: 0)
    monkeypatch.setattr(H, "_claim_projections", lambda *a, **k: False)
    monkeypatch.setattr(H, "_predraw_target", lambda *a, **k: (None, 0))
    group = types.SimpleNamespace(size=lambda: 1)
    plans = {}

    def make(cls=H.GroupTopKState, ef="ef14", **kw):
        st = cls(group, r=4, compress_ratio=0.2, start_compress_iter=0, use_error_feedback=ef, **kw)
        st.select_streams = "off"
        st.defer_decode = False
        st.trail_bytes = 0
        st._plan_for = lambda bucket, buf=None: plans.setdefault((bucket.index(), st._plan_ratio()), _Plan(lib))
        return st

    def call(st, dtype=BF16, b=0, hook=H.group_topk_hook):
        del lib.calls[:]
        G = torch.ones(bucket_numel(SHAPES), dtype=dtype)
        fut = hook(st, SyntheticBucket(G, SHAPES, index=b))
        assert fut.done()
        return list(lib.calls)

    return types.SimpleNamespace(lib=lib, make=make, call=call, plans=plans)


def test_default_and_environment(rig, monkeypatch):
    assert rig.make().error_dtype is None
    monkeypatch.setenv("ARCTOPK_ERROR_DTYPE", "fp32")
    assert rig.make().error_dtype is torch.float32
    assert rig.make(H4.GroupTopKState).error_dtype is torch.float32  # the c4 state inherits it
    for bad in ("bf16", "float32", "1"):
        monkeypatch.setenv("ARCTOPK_ERROR_DTYPE", bad)
        with pytest.raises(ValueError):
            rig.make()


@pytest.mark.parametrize("bad", [torch.bfloat16, torch.float16, torch.float64, "fp32", True])
def test_other_values_raise(rig, bad):
    st = rig.make()
    st.error_dtype = bad
    with pytest.raises(ValueError):
        rig.call(st)
    assert not st.error_dict and not rig.lib.calls


def test_option_unset_is_the_existing_path(rig):
    st = rig.make()
    assert rig.call(st) == [("exchange_step", N.ERR_IN_NONE)]
    assert rig.call(st) == [("exchange_step", N.ERR_IN_ZERO_ROWS)]
    assert st.error_dict[0].dtype == BF16 and st.mixed_calls == 0


def test_bf16_bucket_takes_the_branch(rig):
    st = rig.make()
    st.error_dtype = torch.float32
    assert rig.call(st) == [("encode_mixed", 0), ("select", 1), ("pack_mixed", 0), ("decode", N.EF14)]
    E = st.error_dict[0]
    assert E.dtype == torch.float32 and E.numel() == bucket_numel(SHAPES) and not E.any()
    # the residual is read from the second call on; zero rows (err_in = 2) are never claimed
    for _ in range(3):
        assert rig.call(st) == [("encode_mixed", 1), ("select", 1), ("pack_mixed", 1), ("decode", N.EF14)]
    assert st.error_dict[0] is E and st.mixed_calls == 4 and not st._zr
    assert st.comm_bits_this_round == 0 and st.iter == 4  # world size 1: 2 (ws - 1) bits_sum = 0
    # the c4 hook inherits the branch
    st4 = rig.make(H4.GroupTopKState)
    st4.error_dtype = torch.float32
    assert [c[0] for c in rig.call(st4, hook=H4.group_topk_hook)] == ["encode_mixed", "select", "pack_mixed", "decode"]


def test_fp32_bucket_and_noef_ignore_it(rig):
    st = rig.make()
    st.error_dtype = torch.float32
    assert rig.call(st, dtype=torch.float32) == [("exchange_step", N.ERR_IN_NONE)]  # same dtype: existing path
    assert st.error_dict[0].dtype == torch.float32 and st.mixed_calls == 0
    st = rig.make(ef="noef")
    st.error_dtype = torch.float32
    assert [c[0] for c in rig.call(st)] == ["exchange_step"] and not st.error_dict
    st = rig.make(ef="ef21")  # EF21 on an fp32 bucket: fp32 residuals as ever (its first call needs a
    st.error_dtype = torch.float32  # process group: only the check is exercised here)
    assert st._mixed_residual(torch.float32, N.EF21) is False


def test_ef21_on_a_bf16_bucket_is_refused(rig):
    st = rig.make(ef="ef21")
    st.error_dtype = torch.float32
    with pytest.raises(ValueError, match="ef14"):
        rig.call(st)
    assert not st.error_dict and not st.global_error_dict and not rig.lib.calls


def test_switching_mid_run_is_an_error_not_a_reinterpretation(rig):
    st = rig.make()
    rig.call(st)  # a bf16 residual exists
    st.error_dtype = torch.float32
    with pytest.raises(RuntimeError, match="error_dtype"):
        rig.call(st)
    st = rig.make()
    st.error_dtype = torch.float32
    rig.call(st)
    st.error_dtype = None
    with pytest.raises(RuntimeError, match="float32"):
        rig.call(st)


def test_state_dict_round_trip_and_conversion(rig, tmp_path):
    st = rig.make()
    st.error_dtype = torch.float32
    rig.call(st)
    st.error_dict[0].copy_(torch.randn(st.error_dict[0].numel()))
    torch.save(st.state_dict(), tmp_path / "ck.pt")
    sd = torch.load(tmp_path / "ck.pt", weights_only=True)
    assert sd["error_dtype"] == "fp32" and sd["mixed_buckets"] == [0]
    st2 = rig.make()
    st2.error_dtype = torch.float32
    st2.load_state_dict(sd)
    assert st2.error_dict[0].dtype == torch.float32 and torch.equal(st2.error_dict[0], st.error_dict[0])
    assert rig.call(st2)[0] == ("encode_mixed", 1)
    # fp32 residuals of bf16 buckets into a state without the option: refused, nothing loaded
    st3 = rig.make()
    with pytest.raises(ValueError, match="error_dtype"):
        st3.load_state_dict(sd)
    assert not st3.error_dict
    # bf16 residuals into a state with the option: converted, exactly
    old = rig.make()
    rig.call(old)
    old.error_dict[0].copy_(torch.randn(old.error_dict[0].numel()))
    sd_old = old.state_dict()
    assert sd_old["error_dtype"] is None and sd_old["mixed_buckets"] == []
    st4 = rig.make()
    st4.error_dtype = torch.float32
    st4.load_state_dict(sd_old)
    assert st4.error_dict[0].dtype == torch.float32
    assert torch.equal(st4.error_dict[0].to(BF16), old.error_dict[0])
    assert rig.call(st4)[0] == ("encode_mixed", 1)
    assert st4.state_dict()["mixed_buckets"] == [0]


def test_stall_arithmetic():
    """An unselected element that receives g every step: the bf16 residual stops at 2^8 g (the next
    sum is a tie that rounds to even, back to 2^8 g), the fp32 rule carries all of it."""
    g = torch.tensor(2.0 ** -3, dtype=BF16)
    e16 = torch.zeros((), dtype=BF16)
    e32 = torch.zeros((), dtype=torch.float32)
    for _ in range(300):
        e16 = e16 + g                  # one bf16 add, rounded to nearest even
        e32 = MX.f(g) + e32            # one fp32 add
    assert e16.item() == 256 * 0.125 == 32.0
    assert e32.item() == 300 * 0.125 == 37.5
    assert (torch.tensor(32.0, dtype=BF16) + g).item() == 32.0  # the tie itself


@pytest.mark.parametrize("dense_1d", [False, True])
def test_oracle_conservation(dense_1d):
    """f(out) + E_new == f(G) + E_old on every element at world size 1, whatever the rows."""
    shapes = [(16, 64), (5,), (9, 100), (8, 4, 3, 3), (7,)]
    gen = torch.Generator().manual_seed(3)
    n = bucket_numel(shapes)
    segs = MX.segments(shapes, 0.25, dense_1d)
    E = None
    for it in range(3):
        G = (torch.randn(n, generator=gen) * 10.0 ** (it - 1)).to(BF16)
        rows = [torch.randperm(s.n, generator=gen)[:s.k_rows].sort().values for s in segs]
        res = MX.simulate_step([G], [E], shapes, 0.25, 4, 11 + it, rows, dense_1d=dense_1d)
        X = MX.f(G) if E is None else MX.f(G) + E
        assert torch.equal(MX.f(res["out"]) + res["E_new"][0], X)
        sent = MX.f(res["out"]) != 0
        assert torch.equal(res["E_new"][0][~sent], X[~sent])
        assert (res["E_new"][0][sent].abs() <= X[sent].abs() * 2.0 ** -8).all()  # the rounding remainder
        E = res["E_new"][0]
    # the bf16-residual rule cannot: it rounds X before it stores it
    Xb = G + E.to(BF16)
    assert not torch.equal(MX.f(Xb), MX.f(G) + E)


# ---- the branch's collectives, pending deferred steps and bits ---------------------------------
class _Comm:
    handle = 1

    def __init__(self):
        self.registered = []

    def register(self, t):
        self.registered.append(t)

    def check(self, status, what):
        assert status == 0

    def raise_if_failed(self):
        pass


def _with_comms(rig, st, ws=1):
    """Stub exchange communicators for `st`, a group of `ws` ranks, and an all-reduce entry point
    that records itself."""
    st._test_comms = (_Comm(), _Comm())
    st._exchange_comms = lambda group, dev: st._test_comms
    st.process_group = types.SimpleNamespace(size=lambda: ws)
    rig.lib.arctopk_comm_allreduce = lambda comm, buf, count, dtype, stream: rig.lib.calls.append(
        ("allreduce", count, dtype)) or 0
    return st


@pytest.mark.parametrize("ws,force", [(1, True), (2, False)])
def test_native_call_sequence_with_collectives(rig, ws, force):
    st = rig.make()
    st.error_dtype = torch.float32
    st.force_exchange = force
    _with_comms(rig, st, ws)
    for err_in in (0, 1, 1):
        calls = rig.call(st)
        plan = rig.plans[(0, st._plan_ratio())]
        assert calls == [("encode_mixed", err_in), ("allreduce", plan.info.sketch_len, N.BF16), ("select", ws),
                         ("pack_mixed", err_in), ("allreduce", plan.info.packed_len, N.BF16), ("decode", N.EF14)]
    # the plan's buffers are registered once per plan, not once per call
    sk, pk = st._test_comms
    assert len(sk.registered) == 1 and sk.registered[0] is plan.sketch
    assert len(pk.registered) == 1 and pk.registered[0] is plan.packed
    assert plan.comm_registered is pk and st.mixed_calls == 3


def test_no_collectives_without_communicators(rig):
    st = rig.make()
    st.error_dtype = torch.float32
    _with_comms(rig, st, 1)  # world size 1, no force_exchange, no emulated wire
    assert rig.call(st) == [("encode_mixed", 0), ("select", 1), ("pack_mixed", 0), ("decode", N.EF14)]
    assert not st._test_comms[0].registered and not st._test_comms[1].registered


def test_pending_deferred_steps_are_finished_first(rig):
    st = rig.make()
    st.error_dtype = torch.float32
    st.defer_decode = True
    rig.lib.arctopk_exchange_finish = lambda *a: rig.lib.calls.append(("exchange_finish",)) or 0
    # a default-path call of another bucket (fp32: the option does not apply) that defers its decode
    G = torch.ones(bucket_numel(SHAPES), dtype=torch.float32)
    fut = H.group_topk_hook(st, SyntheticBucket(G, SHAPES, index=1, is_last=False))
    assert not fut.done() and len(st._x_pend) == 1
    calls = rig.call(st)
    assert calls == [("exchange_finish",), ("encode_mixed", 0), ("select", 1), ("pack_mixed", 0), ("decode", N.EF14)]
    assert fut.done() and not st._x_pend


def test_bits_at_world_size_two(rig):
    st = rig.make()
    st.error_dtype = torch.float32
    _with_comms(rig, st, 2)
    rig.call(st)
    plan = rig.plans[(0, st._plan_ratio())]
    assert st.comm_bits_this_round == 2 * (2 - 1) * plan.bits_sum == 2000
