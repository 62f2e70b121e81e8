"""``GroupTopKState.ef21_error_dtype`` on CPU, the native library stubbed: the switch and its
validation, which native calls the compressed call of a bf16 EF21 bucket makes with it, what it
leaves alone, checkpoints, and the arithmetic the option exists for (the bf16 global residual
that drops a mean of half an ulp on every call; the restatement's gE == E at world size 1).

(The kernels and the hook on a GPU: tests/test_gpu_mixed_ef21.py.)"""
import types

import pytest
import torch

import mixed_ef21_oracle as M21
from allreducetopk_amd import _native as N
from allreducetopk_amd.bucket import SyntheticBucket, bucket_numel
from allreducetopk_amd.comm_hooks import group_topk_hook_no_reshape as H
from allreducetopk_amd.comm_hooks import group_topk_hook_no_reshape_c4 as H4

SHAPES = [[8, 64], [16]]
BF16 = torch.bfloat16
FP32 = torch.float32
BRANCH = ["encode_mixed21", "select", "pack_mixed21", "decode_mixed21"]


class _Lib:
    """Stands in for libarctopk: records the native calls of a hook call in order."""

    def __init__(self):
        self.calls = []

    def arctopk_exchange_step(self, handle, x, e, g, ef, err_in, *rest):
        self.calls.append("exchange_step")
        return 0

    def arctopk_exchange_finish(self, *a):
        return 0

    def arctopk_encode_mixed(self, *a):
        self.calls.append("encode_mixed")
        return 0

    def arctopk_pack_mixed(self, *a):
        self.calls.append("pack_mixed")
        return 0

    def arctopk_encode_mixed21(self, handle, g, e, v, sk, stream):
        self.calls.append("encode_mixed21")
        return 0

    def arctopk_pack_mixed21(self, handle, g, e, rl, sm, pk, stream):
        self.calls.append("pack_mixed21")
        return 0

    def arctopk_decode_mixed21(self, handle, pk, sm, ws, ge, out, stream):
        self.calls.append("decode_mixed21")
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
        self.lib.calls.append("select")

    def decode(self, ws, ef, gerr, out, stream):
        self.lib.calls.append("decode")


@pytest.fixture()
def rig(monkeypatch):
    lib = _Lib()
    monkeypatch.delenv("ARCTOPK_ERROR_DTYPE", raising=False)
    monkeypatch.delenv("ARCTOPK_EF21_ERROR_DTYPE", raising=False)
    monkeypatch.setattr(H, "_LIB", [lib])
    monkeypatch.setattr(N, "lib", lambda: lib)
    monkeypatch.setattr(H, "_reseed_global", lambda *a, **k: None)
    monkeypatch.setattr(H, "_current_raw_stream", lambda dix: 0)
    monkeypatch.setattr(H, "_claim_projections", lambda *a, **k: False)
    monkeypatch.setattr(H, "_predraw_target", lambda *a, **k: (None, 0))
    monkeypatch.setattr(H.dist, "all_reduce", lambda *a, **k: None)  # (EF21's first call, one rank)
    group = types.SimpleNamespace(size=lambda: 1)
    plans = {}

    def make(cls=H.GroupTopKState, ef="ef21", **kw):
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
    assert rig.make().ef21_error_dtype is None
    monkeypatch.setenv("ARCTOPK_EF21_ERROR_DTYPE", "fp32")
    st = rig.make()
    assert st.ef21_error_dtype is FP32 and st.error_dtype is None  # two options, two variables
    assert rig.make(H4.GroupTopKState).ef21_error_dtype is FP32   # the c4 state inherits it
    for bad in ("bf16", "float32", "1"):
        monkeypatch.setenv("ARCTOPK_EF21_ERROR_DTYPE", bad)
        with pytest.raises(ValueError):
            rig.make()


@pytest.mark.parametrize("ef", ["ef21", "ef14", "noef"])
@pytest.mark.parametrize("bad", [torch.bfloat16, torch.float16, torch.float64, "fp32", True])
def test_other_values_raise(rig, bad, ef):
    st = rig.make(ef=ef)
    st.ef21_error_dtype = bad
    with pytest.raises(ValueError, match="ef21_error_dtype"):
        rig.call(st)
    assert not st.error_dict and not st.global_error_dict and not rig.lib.calls


def test_option_unset_is_the_existing_path(rig):
    st = rig.make()
    assert rig.call(st) == []  # the dense first call
    assert rig.call(st) == ["exchange_step"]
    assert st.error_dict[0].dtype == BF16 and st.global_error_dict[0].dtype == BF16 and st.mixed_calls == 0
    assert not st._mixed_buckets


@pytest.mark.parametrize("error_dtype", [None, FP32])
def test_bf16_ef21_bucket_takes_the_branch(rig, error_dtype):
    """... whatever error_dtype is."""
    st = rig.make()
    st.ef21_error_dtype = FP32
    st.error_dtype = error_dtype
    assert rig.call(st) == []  # first call: torch ops only, both tables created in fp32
    E, gE = st.error_dict[0], st.global_error_dict[0]
    n = bucket_numel(SHAPES)
    assert E.dtype == gE.dtype == FP32 and E.numel() == gE.numel() == n
    assert torch.equal(E, torch.ones(n)) and torch.equal(gE, torch.ones(n))  # E_0 = f(G), gE_0 = f(out)
    assert E.data_ptr() != gE.data_ptr()
    for _ in range(3):
        assert rig.call(st) == BRANCH
    assert st.error_dict[0] is E and st.global_error_dict[0] is gE
    assert st.mixed_calls == 3 and st._mixed_buckets == {0} and not st._x_pend
    assert st.iter == 4 and st.comm_bits_this_round == n * 16  # the first call's; 2 (ws - 1) bits_sum = 0 after
    st4 = rig.make(H4.GroupTopKState)  # the c4 hook inherits the branch
    st4.ef21_error_dtype = FP32
    assert rig.call(st4, hook=H4.group_topk_hook) == []
    assert rig.call(st4, hook=H4.group_topk_hook) == BRANCH
    assert st4.error_dict[0].dtype == st4.global_error_dict[0].dtype == FP32


def test_fp32_buckets_noef_and_ef14_ignore_it(rig):
    st = rig.make()
    st.ef21_error_dtype = FP32
    assert rig.call(st, dtype=FP32) == [] and rig.call(st, dtype=FP32) == ["exchange_step"]
    assert st.mixed_calls == 0 and not st._mixed_buckets
    st = rig.make(ef="noef")
    st.ef21_error_dtype = FP32
    assert rig.call(st) == ["exchange_step"] and not st.error_dict
    st = rig.make(ef="ef14")
    st.ef21_error_dtype = FP32
    assert rig.call(st) == ["exchange_step"] and st.error_dict[0].dtype == BF16 and st.mixed_calls == 0
    st = rig.make(ef="ef14")  # EF14's own option is untouched by this one
    st.ef21_error_dtype = FP32
    st.error_dtype = FP32
    assert rig.call(st) == ["encode_mixed", "select", "pack_mixed", "decode"]


def test_error_dtype_alone_still_refuses_ef21(rig):
    st = rig.make()
    st.error_dtype = FP32
    with pytest.raises(ValueError, match="ef14") as ei:
        rig.call(st)
    assert "ef21_error_dtype" in str(ei.value)
    assert not st.error_dict and not st.global_error_dict and not rig.lib.calls


def test_switching_mid_run_is_an_error_not_a_reinterpretation(rig):
    st = rig.make()
    rig.call(st), rig.call(st)  # bf16 residuals exist
    st.ef21_error_dtype = FP32
    with pytest.raises(RuntimeError, match="ef21_error_dtype"):
        rig.call(st)
    st = rig.make()
    st.ef21_error_dtype = FP32
    rig.call(st), rig.call(st)
    st.ef21_error_dtype = None
    with pytest.raises(RuntimeError, match="float32"):
        rig.call(st)
    # one table of the wrong dtype is enough
    st = rig.make()
    st.ef21_error_dtype = FP32
    rig.call(st)
    st.global_error_dict[0] = st.global_error_dict[0].to(BF16)
    with pytest.raises(RuntimeError, match="global_error_dict"):
        rig.call(st)


def test_state_dict_round_trip_and_conversion(rig, tmp_path):
    st = rig.make()
    st.ef21_error_dtype = FP32
    rig.call(st), rig.call(st)
    n = st.error_dict[0].numel()
    st.error_dict[0].copy_(torch.randn(n))
    st.global_error_dict[0].copy_(torch.randn(n))
    torch.save(st.state_dict(), tmp_path / "ck.pt")
    sd = torch.load(tmp_path / "ck.pt", weights_only=True)
    assert sd["ef21_error_dtype"] == "fp32" and sd["error_dtype"] is None and sd["mixed_buckets"] == [0]
    st2 = rig.make()
    st2.ef21_error_dtype = FP32
    st2.load_state_dict(sd)
    for name in ("error_dict", "global_error_dict"):
        t = getattr(st2, name)[0]
        assert t.dtype == FP32 and torch.equal(t, getattr(st, name)[0])
    assert rig.call(st2) == BRANCH
    # fp32 residuals of bf16 buckets into a state without the option: refused, nothing loaded --
    # also when only EF14's option is set
    for ed in (None, FP32):
        st3 = rig.make()
        st3.error_dtype = ed
        with pytest.raises(ValueError, match="ef21_error_dtype"):
            st3.load_state_dict(sd)
        assert not st3.error_dict and not st3.global_error_dict and st3.iter == 0
    # bf16 residuals into a state with the option: converted exactly, both tables
    old = rig.make()
    rig.call(old), rig.call(old)
    old.error_dict[0].copy_(torch.randn(n))
    old.global_error_dict[0].copy_(torch.randn(n))
    sd_old = old.state_dict()
    assert sd_old["ef21_error_dtype"] is None and sd_old["error_dtype"] is None and sd_old["mixed_buckets"] == []
    sd_old.pop("ef21_error_dtype")  # a checkpoint from before the option: a missing key is None
    st4 = rig.make()
    st4.ef21_error_dtype = FP32
    st4.load_state_dict(sd_old)
    for name in ("error_dict", "global_error_dict"):
        t = getattr(st4, name)[0]
        assert t.dtype == FP32 and torch.equal(t.to(BF16), getattr(old, name)[0])
        assert torch.equal(t, getattr(old, name)[0].float())
    assert rig.call(st4) == BRANCH
    assert st4.state_dict()["mixed_buckets"] == [0]
    # ... and into a state without it: as ever
    st5 = rig.make()
    st5.load_state_dict(sd_old)
    assert st5.error_dict[0].dtype == BF16 and rig.call(st5) == ["exchange_step"]


def test_drift_arithmetic():
    """Two ranks, a row at 1024 (bf16 ulp 8): rank 0's row grows by 8 per call, rank 1's stays.  The
    mean moves by 4, half an ulp of gE: bf16 gE := b(gE + mean) is a tie that rounds to even, back to
    1024, on every call; the fp32 gE adds it."""
    g16 = torch.tensor(1024.0, dtype=BF16)
    g32 = torch.tensor(1024.0)
    E0, E1 = torch.tensor(1024.0), torch.tensor(1024.0)
    for t in range(1, 17):
        G0, G1 = torch.tensor(1024.0 + 8 * t, dtype=BF16), torch.tensor(1024.0, dtype=BF16)
        assert G0.item() == 1024.0 + 8 * t  # representable
        p0, p1 = M21.b(M21.f(G0) - E0), M21.b(M21.f(G1) - E1)
        E0, E1 = E0 + M21.f(p0), E1 + M21.f(p1)
        P = p0 + p1                      # the wire's bf16 sum
        g32 = g32 + M21.f(P) / 2.0       # fp32 gE
        g16 = g16 + (P / 2)              # today's: the bf16 mean, then one bf16 add
    assert (E0.item(), E1.item()) == (1152.0, 1024.0)
    assert (E0.item() + E1.item()) / 2 == 1088.0  # the truth: the mean of the ranks' E
    assert g32.item() == 1088.0 and M21.b(g32).item() == 1088.0
    assert g16.item() == 1024.0
    assert (torch.tensor(1024.0, dtype=BF16) + torch.tensor(4.0, dtype=BF16)).item() == 1024.0  # the tie itself


@pytest.mark.parametrize("dense_1d", [False, True])
def test_oracle_invariant_at_world_size_one(dense_1d):
    """gE == E bit for bit after every call at world size 1, and out == b(gE), whatever the rows."""
    shapes = [(16, 64), (5,), (9, 100), (8, 4, 3, 3), (7,)]
    gen = torch.Generator().manual_seed(3)
    n = bucket_numel(shapes)
    segs = M21.segments(shapes, 0.25, dense_1d)
    G = torch.randn(n, generator=gen).to(BF16)
    out, Es, gE = M21.first_call([G])
    assert torch.equal(out, G) and torch.equal(Es[0], gE)
    moved = torch.zeros(n, dtype=torch.bool)
    for it in range(3):
        G = (torch.randn(n, generator=gen) * 10.0 ** (it - 1)).to(BF16)
        rows = [torch.randperm(s.n, generator=gen)[:s.k_rows].sort().values for s in segs]
        res = M21.simulate_step([G], Es, gE, shapes, 0.25, 4, 11 + it, rows, dense_1d=dense_1d)
        assert torch.equal(res["gE_new"], res["E_new"][0]), f"call {it}"
        assert torch.equal(res["out"], M21.b(res["gE_new"]))
        same = res["E_new"][0] == Es[0]
        sent = torch.zeros(n, dtype=torch.bool)
        for s, idx in zip(segs, res["rows"]):
            sent[s.offset:s.offset + s.numel].view(s.n, s.m)[idx] = True
        assert same[~sent].all(), "unselected rows are untouched"
        # a sent element lands within one bf16 rounding of D from G: the remainder stays in G - E
        rem = (M21.f(G) - res["E_new"][0])[sent].abs()
        assert (rem <= res["D"][0][sent].abs() * 2.0 ** -8).all()
        moved |= sent
        Es, gE = res["E_new"], res["gE_new"]
    assert moved.any() and not moved.all()


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


def _branch_with_collectives(plan):
    return ["encode_mixed21", ("allreduce", plan.info.sketch_len, N.BF16), "select", "pack_mixed21",
            ("allreduce", plan.info.packed_len, N.BF16), "decode_mixed21"]


@pytest.mark.parametrize("ws,force", [(1, True), (2, False)])
def test_native_call_sequence_with_collectives(rig, ws, force):
    st = rig.make()
    st.ef21_error_dtype = FP32
    st.force_exchange = force
    _with_comms(rig, st, ws)
    assert rig.call(st) == []  # the dense first call (torch's process group)
    for _ in range(3):
        calls = rig.call(st)
        plan = rig.plans[(0, st._plan_ratio())]
        assert calls == _branch_with_collectives(plan)
    # the plan's buffers are registered once per plan, not once per call
    sk, pk = st._test_comms
    assert len(sk.registered) == 1 and sk.registered[0] is plan.sketch
    assert len(pk.registered) == 1 and pk.registered[0] is plan.packed
    assert plan.comm_registered is pk and st.mixed_calls == 3


def test_no_collectives_without_communicators(rig):
    st = rig.make()
    st.ef21_error_dtype = FP32
    _with_comms(rig, st, 1)  # world size 1, no force_exchange, no emulated wire
    assert rig.call(st) == [] and rig.call(st) == BRANCH
    assert not st._test_comms[0].registered and not st._test_comms[1].registered


def test_pending_deferred_steps_are_finished_first(rig):
    st = rig.make()
    st.ef21_error_dtype = FP32
    st.defer_decode = True
    rig.lib.arctopk_exchange_finish = lambda *a: rig.lib.calls.append("exchange_finish") or 0
    assert rig.call(st) == []  # bucket 0's dense first call
    # default-path calls of another bucket (fp32: the option does not apply); the second defers its decode
    G = torch.ones(bucket_numel(SHAPES), dtype=FP32)
    assert H.group_topk_hook(st, SyntheticBucket(G, SHAPES, index=1, is_last=False)).done()
    fut = H.group_topk_hook(st, SyntheticBucket(G, SHAPES, index=1, is_last=False))
    assert not fut.done() and len(st._x_pend) == 1
    assert rig.call(st) == ["exchange_finish"] + BRANCH
    assert fut.done() and not st._x_pend


def test_bits_at_world_size_two(rig):
    st = rig.make()
    st.ef21_error_dtype = FP32
    _with_comms(rig, st, 2)
    rig.call(st)
    first = st.comm_bits_this_round
    assert first == bucket_numel(SHAPES) * 16  # the dense first call's
    rig.call(st)
    plan = rig.plans[(0, st._plan_ratio())]
    assert st.comm_bits_this_round - first == 2 * (2 - 1) * plan.bits_sum == 2000
