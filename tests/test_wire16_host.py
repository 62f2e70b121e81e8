"""``GroupTopKState.wire_dtype`` on CPU, the native library stubbed: the restatement's identities
(wire16_oracle), the switch and its validation, which native calls the compressed call of an fp32
bucket makes with it, the bit accounting, checkpoints, and the entry points' host-side refusals.

(The kernels and the hook on a GPU: tests/test_gpu_wire16.py.)"""
import ctypes
import os
import types

import pytest
import torch

import wire16_oracle as W
from allreducetopk_amd import _native as N
from allreducetopk_amd.bucket import SyntheticBucket, bucket_numel
from allreducetopk_amd.build import LIB, build
from allreducetopk_amd.comm_hooks import group_topk_hook_no_reshape as H
from allreducetopk_amd.comm_hooks import group_topk_hook_no_reshape_c4 as H4
from oracle import arctopk as A

SHAPES = [[8, 64], [16]]
MIX = [[12, 20], [9], [6, 4, 3, 3], [33]]  # SKETCH, 1-D, ND, 1-D (RAW, or DENSE under the c4 rules)
BF16 = torch.bfloat16


# ---- 1. the restatement ----------------------------------------------------------------------
def _cpu_rows(X, segs, r, seed):
    """Rows by the reference's own select on a CPU sketch of X (any rows would do)."""
    g = torch.Generator().manual_seed(seed)
    Ps = [X[s.offset:s.offset + s.numel].clone() if s.kind == W.RAW
          else None if s.kind == W.DENSE
          else X[s.offset:s.offset + s.numel].view(s.n, s.m) @ torch.randn(s.m, r, generator=g) for s in segs]
    rows = []
    for P, s in zip(Ps, segs):
        rows.append(torch.arange(s.n) if P is None else A.select([P], 1, [s])[1][0].sort().values)
    return rows


@pytest.mark.parametrize("dense", [False, True])
def test_pack_remainder_is_exact(dense):
    """E_new = X - f(b(X)) (EF14) in one fp32 subtract loses nothing: it equals the float64
    difference, over three calls, subnormals and large values included."""
    segs = W.segments(MIX, 0.25, dense)
    assert {s.kind for s in segs} == ({W.SKETCH, W.DENSE} if dense else {W.SKETCH, W.RAW})
    n = bucket_numel(MIX)
    E = None
    for it in range(3):
        G = torch.randn(n, generator=torch.Generator().manual_seed(it)) * 10.0 ** (3 * it - 3)
        G[::7] *= 1e-38  # subnormal fp32 values
        X = W.pre_apply(G, E, "ef14")
        rows = W.full_rows(_cpu_rows(X, segs, 4, it), segs)
        vals, En = W.pack(G, E, "ef14", rows, segs)
        sel = A.decode(torch.ones(vals.numel()), 1, rows, segs, n, torch.float32) != 0
        sent = A.decode(vals.float(), 1, rows, segs, n, torch.float32)
        assert torch.equal(En.double(), torch.where(sel, X.double() - sent.double(), X.double()))
        assert sel.any() and not sel.all()
        E = En


@pytest.mark.parametrize("dense", [False, True])
def test_identities_at_world_size_one(dense):
    n = bucket_numel(MIX)
    o14 = W.Wire16Oracle(1, MIX, 0.25, "ef14", c4=dense, gradual=False)
    o21 = W.Wire16Oracle(1, MIX, 0.25, "ef21", c4=dense, gradual=False)
    segs = W.segments(MIX, 0.25, dense)
    E_old = torch.zeros(n)
    for it in range(4):
        G = torch.randn(n, generator=torch.Generator().manual_seed(70 + it)) * 10.0 ** (it - 2)
        rows = _cpu_rows(G + E_old, segs, 4, it)
        out = o14.call([G], rows)["out"]
        assert torch.equal(out + o14.Es[0], G + E_old), f"EF14 conservation, call {it}"
        E_old = o14.Es[0]
        res = o21.call([G], rows)
        assert torch.equal(o21.gE, o21.Es[0]) and torch.equal(res["out"], o21.gE), f"EF21 gE == E, call {it}"
    assert o14.bits == 0 and o21.bits == n * 32


def test_two_rank_sum_is_one_rounding():
    g = torch.Generator().manual_seed(3)
    a, b_ = torch.randn(4096, generator=g).to(BF16), (torch.randn(4096, generator=g) * 3).to(BF16)
    assert torch.equal(W.wire_sum([a, b_]), W.b(W.f(a) + W.f(b_)))


# ---- 2. the option ---------------------------------------------------------------------------
class _Lib:
    """Stands in for libarctopk: records the native calls of a hook call in order."""

    def __init__(self):
        self.calls = []

    def arctopk_exchange_step(self, handle, x, e, g, ef, err_in, *rest):
        self.calls.append(("exchange_step", err_in))
        return 0

    def arctopk_exchange_finish(self, *a):
        return 0

    def arctopk_pack_wire16(self, handle, g, e, ef, err_in, rl, sm, pk, stream):
        self.calls.append(("pack_wire16", ef, err_in))
        return 0

    def arctopk_decode_wire16(self, handle, pk, sm, ws, ef, gerr, out, stream):
        self.calls.append(("decode_wire16", ef, ws))
        return 0

    def arctopk_comm_allreduce(self, comm, buf, count, dtype, stream):
        self.calls.append(("allreduce", count, dtype))
        return 0


class _Plan:
    """What the hook touches of a BucketPlan."""

    def __init__(self, lib, dtype, shapes=SHAPES, ratio=0.2):
        self.lib = lib
        self.handle = object()
        segs = W.segments(shapes, ratio)
        self.segments = [types.SimpleNamespace(kind=s.kind, n=s.n, m=s.m, k_rows=s.k_rows) for s in segs]
        self.r = 4
        self.slotmap = torch.zeros(24, dtype=torch.int32)
        self.rowlist = torch.zeros(24, dtype=torch.int32)
        self.sketch = torch.zeros(64, dtype=dtype)
        self.packed = torch.zeros(80, dtype=dtype)
        self.V_ring = [torch.zeros(256, dtype=dtype)]
        self.info = types.SimpleNamespace(sketch_len=W.sketch_elems(segs, 4), packed_len=80, v_len=256,
                                          values_len=sum(s.k for s in segs))
        self.bits_sum = 1000
        self.philox_advance = 0
        self.comm_registered = None
        self.packed16 = None
        self.packed16_registered = None

    def encode(self, grad, err, ef, err_in, V, stream):
        self.lib.calls.append(("encode", ef, int(err_in)))

    def select(self, ws, stream, *a):
        self.lib.calls.append(("select", ws))


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


@pytest.fixture()
def rig(monkeypatch):
    lib = _Lib()
    for v in ("ARCTOPK_WIRE_DTYPE", "ARCTOPK_ERROR_DTYPE", "ARCTOPK_EF21_ERROR_DTYPE"):
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setattr(H, "_LIB", [lib])
    monkeypatch.setattr(N, "lib", lambda: lib)
    monkeypatch.setattr(H, "_reseed_global", lambda *a, **k: None)
    monkeypatch.setattr(H, "_current_raw_stream", lambda dix: 0)
    monkeypatch.setattr(H, "_claim_projections", lambda *a, **k: False)
    monkeypatch.setattr(H, "_predraw_target", lambda *a, **k: (None, 0))
    plans = {}

    def make(cls=H.GroupTopKState, ef="ef14", ws=1, **kw):
        group = types.SimpleNamespace(size=lambda: ws)
        st = cls(group, r=4, compress_ratio=0.2, start_compress_iter=0, use_error_feedback=ef, **kw)
        st.select_streams = "off"
        st.defer_decode = False
        st.trail_bytes = 0
        st._plan_for = lambda bucket, buf=None: plans.setdefault(
            (id(st), bucket.index(), buf.dtype, st._plan_ratio()), _Plan(lib, buf.dtype))
        st._test_comms = (_Comm(), _Comm())
        st._exchange_comms = lambda group, dev: st._test_comms
        return st

    def call(st, dtype=torch.float32, b=0, hook=H.group_topk_hook):
        del lib.calls[:]
        G = torch.ones(bucket_numel(SHAPES), dtype=dtype)
        fut = hook(st, SyntheticBucket(G, SHAPES, index=b))
        assert fut.done()
        return list(lib.calls)

    return types.SimpleNamespace(lib=lib, make=make, call=call, plans=plans)


def test_default_and_environment(rig, monkeypatch):
    st = rig.make()
    assert st.wire_dtype is None and st.wire16_calls == 0
    assert rig.call(st) == [("exchange_step", N.ERR_IN_NONE)] and st.wire16_calls == 0  # today's path
    monkeypatch.setenv("ARCTOPK_WIRE_DTYPE", "bf16")
    assert rig.make().wire_dtype is torch.bfloat16
    assert rig.make(H4.GroupTopKState).wire_dtype is torch.bfloat16  # the c4 state inherits it
    for bad in ("fp16", "bfloat16", "1"):
        monkeypatch.setenv("ARCTOPK_WIRE_DTYPE", bad)
        with pytest.raises(ValueError):
            rig.make()


@pytest.mark.parametrize("bad", [torch.float16, torch.float32, "bf16", True])
def test_other_values_raise_at_the_first_compressed_call(rig, bad):
    st = rig.make()
    st.wire_dtype = bad
    with pytest.raises(ValueError, match="wire_dtype"):
        rig.call(st)
    assert not st.error_dict and not rig.lib.calls


@pytest.mark.parametrize("ef,code", [("noef", N.EF_NONE), ("ef14", N.EF14)])
def test_fp32_bucket_takes_the_branch(rig, ef, code):
    st = rig.make(ef=ef)
    st.wire_dtype = torch.bfloat16
    assert rig.call(st) == [("encode", code, 0 if ef == "ef14" else 1), ("select", 1), ("pack_wire16", code, 0 if ef == "ef14" else 1),
                            ("decode_wire16", code, 1)]
    plan = next(iter(rig.plans.values()))
    assert plan.packed16.dtype == BF16 and plan.packed16.numel() == 80 and not plan.packed16.any()
    p16 = plan.packed16
    # the residual is read from the second call on; zero rows (err_in = 2) are never claimed
    for _ in range(2):
        assert rig.call(st) == [("encode", code, 1), ("select", 1), ("pack_wire16", code, 1), ("decode_wire16", code, 1)]
    assert plan.packed16 is p16 and st.wire16_calls == 3 and not st._zr and not st._x_pend
    assert st.comm_bits_this_round == 0 and st.iter == 3
    if ef == "ef14":
        assert st.error_dict[0].dtype == torch.float32
    # the c4 hook inherits the branch
    st4 = rig.make(H4.GroupTopKState, ef=ef)
    st4.wire_dtype = torch.bfloat16
    assert [c[0] for c in rig.call(st4, hook=H4.group_topk_hook)] == ["encode", "select", "pack_wire16", "decode_wire16"]


def test_bf16_bucket_ignores_the_option(rig):
    st = rig.make()
    st.wire_dtype = torch.bfloat16
    assert rig.call(st, dtype=BF16) == [("exchange_step", N.ERR_IN_NONE)]
    assert st.wire16_calls == 0 and st.error_dict[0].dtype == BF16
    st.host_staged = True  # ... and so does its host-staged path's refusal
    assert st._wire16(BF16) is False


def test_host_staged_is_refused(rig):
    st = rig.make()
    st.wire_dtype = torch.bfloat16
    st.host_staged = True
    with pytest.raises(ValueError, match="host_staged"):
        rig.call(st)
    assert not st.error_dict and not rig.lib.calls


def test_state_dict_records_the_option_and_loads_under_either_setting(rig, tmp_path):
    st = rig.make()
    st.wire_dtype = torch.bfloat16
    rig.call(st)
    st.error_dict[0].copy_(torch.randn(st.error_dict[0].numel()))
    torch.save(st.state_dict(), tmp_path / "ck.pt")
    sd = torch.load(tmp_path / "ck.pt", weights_only=True)
    assert sd["wire_dtype"] == "bf16" and sd["mixed_buckets"] == []
    plain = rig.make()
    plain.load_state_dict(sd)  # residuals are plain fp32: loads without the option ...
    assert plain.wire_dtype is None and torch.equal(plain.error_dict[0], st.error_dict[0])
    assert rig.call(plain) == [("exchange_step", N.ERR_IN_READ)]
    sd_plain = plain.state_dict()
    assert sd_plain["wire_dtype"] is None
    st2 = rig.make()
    st2.wire_dtype = torch.bfloat16
    st2.load_state_dict(sd_plain)  # ... and the other way round
    assert rig.call(st2)[0] == ("encode", N.EF14, 1) and st2.wire16_calls == 1


# ---- 3. bit accounting -----------------------------------------------------------------------
@pytest.mark.parametrize("ws", [2, 8])
def test_bit_accounting(rig, ws):
    st = rig.make(ws=ws)
    st.wire_dtype = torch.bfloat16
    calls = rig.call(st)
    segs = W.segments(SHAPES, 0.2)
    sk, k = W.sketch_elems(segs, 4), sum(s.k for s in segs)
    assert st.comm_bits_this_round == 2 * (ws - 1) * (sk * 32 + k * 16) == 2 * (ws - 1) * W.bits_per_call(segs, 4)
    # the sketch goes out in fp32, the packed values in bf16, the latter over the registered bf16 buffer
    assert [c for c in calls if c[0] == "allreduce"] == [("allreduce", sk, N.F32), ("allreduce", 80, N.BF16)]
    plan = next(p for p in rig.plans.values() if p.packed16 is not None)
    assert any(t is plan.packed16 for t in st._test_comms[1].registered)
    # half the default path's bits for the values
    assert W.bits_per_call(segs, 4) == A.bits_per_call(segs, 4, 32) - k * 16


# ---- 4. the C ABI ----------------------------------------------------------------------------
def test_entry_points_refuse_null_arguments_without_a_device():
    if not os.path.exists(LIB):
        build()
    L = ctypes.CDLL(LIB)
    for fn in (L.arctopk_pack_wire16, L.arctopk_decode_wire16):
        fn.restype = ctypes.c_int32
    null = ctypes.c_void_p(None)
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for ef in (N.EF_NONE, N.EF14, N.EF21, 7):
        assert L.arctopk_pack_wire16(null, p, p, ef, 0, p, p, p, null) == N.EINVAL
        assert L.arctopk_pack_wire16(null, null, null, ef, 1, null, null, null, null) == N.EINVAL
        assert L.arctopk_decode_wire16(null, p, p, 1, ef, p, p, null) == N.EINVAL
        assert L.arctopk_decode_wire16(null, null, null, 0, ef, null, null, null) == N.EINVAL
    assert not any(buf)


# ---- 5. pending deferred steps ---------------------------------------------------------------
def test_pending_deferred_steps_are_finished_first(rig):
    st = rig.make()
    st.wire_dtype = torch.bfloat16
    st.defer_decode = True
    rig.lib.arctopk_exchange_finish = lambda *a: rig.lib.calls.append(("exchange_finish",)) or 0
    # a default-path call of another bucket (bf16: the option does not apply) that defers its decode
    G = torch.ones(bucket_numel(SHAPES), dtype=BF16)
    fut = H.group_topk_hook(st, SyntheticBucket(G, SHAPES, index=1, is_last=False))
    assert not fut.done() and len(st._x_pend) == 1
    calls = rig.call(st)
    assert calls == [("exchange_finish",), ("encode", N.EF14, 0), ("select", 1), ("pack_wire16", N.EF14, 0),
                     ("decode_wire16", N.EF14, 1)]
    assert fut.done() and not st._x_pend


def test_bits_at_world_size_two(rig):
    st = rig.make(ws=2)
    st.wire_dtype = torch.bfloat16
    rig.call(st)
    plan = next(p for p in rig.plans.values() if p.packed16 is not None)
    sketch_elems = sum(s.n * plan.r if s.kind == N.SEG_SKETCH else s.n if s.kind == N.SEG_RAW else 0
                       for s in plan.segments)
    assert st.comm_bits_this_round == 2 * (2 - 1) * (sketch_elems * 32 + plan.info.values_len * 16)
    assert st.comm_bits_this_round != 2 * (2 - 1) * plan.bits_sum
