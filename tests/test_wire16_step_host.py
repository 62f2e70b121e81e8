"""``GroupTopKState.wire_exchange`` on CPU, the native library stubbed: the option and its
validation, which native calls a bf16-wire bucket makes with ``wire_exchange="step"`` (the plan
bound to its bf16 buffer, then ONE arctopk_exchange_step, deferred like the default path's), the
scatter of the zero-ahead drain restated in torch ops against wire16_oracle's whole decode, and the
new entry points' declarations against their ctypes bindings.

(The kernels and the hook on a GPU: tests/test_gpu_wire16_step.py.)"""
import os
import re
import types

import pytest
import torch

import wire16_oracle as W
from allreducetopk_amd import _native as N
from allreducetopk_amd.bucket import SyntheticBucket, bucket_numel
from allreducetopk_amd.comm_hooks import group_topk_hook_no_reshape as H
from allreducetopk_amd.comm_hooks import group_topk_hook_no_reshape_c4 as H4

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [[8, 64], [16]]
BF16 = torch.bfloat16
MIXA = [[16, 64], [5], [64, 128], [100, 72], [9, 100], [8, 4, 3, 3], [16, 8, 1, 1], [8, 40], [4, 5461], [7]]
ALIGNB = [[4, 4], [32, 2048], [6, 24], [10, 24], [16, 64]]
LAYOUTS = {"mixa": (MIXA, False), "alignb": (ALIGNB, False), "mixa_dense": (MIXA, True)}


class _Lib:
    """Stands in for libarctopk: records the native calls of a hook call in order."""

    def __init__(self):
        self.calls = []

    def arctopk_plan_bind_wire16(self, handle, packed):
        self.calls.append(("bind_wire16", packed is not None))
        return 0

    def arctopk_exchange_step(self, handle, x, e, g, ef, err_in, draw, seed, nxt, nseed, sk, pk, stream, ars, defer,
                              ride, ride_marks, fin, fin_marks, nf, V, marks, sel_stream, trail):
        self.calls.append(("exchange_step", err_in, defer, sel_stream, trail))
        return 0

    def arctopk_exchange_finish(self, *a):
        self.calls.append(("exchange_finish",))
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
    """What the hook touches of a BucketPlan (no `groups`: a grouped bucket would raise)."""

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
        self.wire16_bound = False

    def encode(self, grad, err, ef, err_in, V, stream):
        self.lib.calls.append(("encode", ef, int(err_in)))

    def select(self, ws, stream, *a):
        self.lib.calls.append(("select", ws))


class _Comm:
    handle = 1
    kind = "rccl"

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
    for v in ("ARCTOPK_WIRE_DTYPE", "ARCTOPK_WIRE_EXCHANGE", "ARCTOPK_ERROR_DTYPE", "ARCTOPK_EF21_ERROR_DTYPE"):
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
        st._side_stream = lambda table, dev, prio=None: types.SimpleNamespace(cuda_stream=5)
        return st

    def call(st, dtype=torch.float32, b=0, hook=H.group_topk_hook, is_last=True):
        del lib.calls[:]
        G = torch.ones(bucket_numel(SHAPES), dtype=dtype)
        fut = hook(st, SyntheticBucket(G, SHAPES, index=b, is_last=is_last))
        return fut, list(lib.calls)

    return types.SimpleNamespace(lib=lib, make=make, call=call, plans=plans)


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
    assert not st.error_dict and not rig.lib.calls


def test_no_effect_without_the_bf16_wire(rig):
    st = rig.make()
    st.wire_exchange = "step"
    fut, calls = rig.call(st)  # wire_dtype None: today's default step, no binding
    assert fut.done() and calls == [("exchange_step", N.ERR_IN_NONE, 0, None, None)]
    st.wire_dtype = BF16
    fut, calls = rig.call(st, dtype=BF16, b=1)  # a bf16 bucket ignores both options
    assert calls == [("exchange_step", N.ERR_IN_NONE, 0, None, None)]
    assert st.wire16_calls == st.wire16_step_calls == 0 and st.error_dict[1].dtype == BF16


def test_host_staged_takes_precedence(rig):
    st = rig.make()
    st.wire_dtype, st.wire_exchange, st.host_staged = BF16, "step", True
    with pytest.raises(ValueError, match="host_staged"):
        rig.call(st)
    assert not st.error_dict and not rig.lib.calls


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
    assert fut.done() and calls == [("bind_wire16", True), ("exchange_step", first, 0, None, None)]
    plan = next(iter(rig.plans.values()))
    assert plan.wire16_bound and plan.packed16.dtype == BF16 and plan.packed16.numel() == 80 and not plan.packed16.any()
    # bound once; the residual is read from the second call on; zero rows (err_in = 2) are never claimed
    for _ in range(2):
        assert rig.call(st)[1] == [("exchange_step", N.ERR_IN_READ, 0, None, None)]
    assert st.wire16_step_calls == st.wire16_calls == 3 and not st._zr and not st._x_pend
    assert st.comm_bits_this_round == 0 and st.iter == 3
    # the option can change between calls: the default step unbinds the plan, and may claim zero rows again
    st.wire_dtype = None
    assert rig.call(st)[1] == [("bind_wire16", False), ("exchange_step", N.ERR_IN_READ, 0, None, None)]
    assert not plan.wire16_bound and st.wire16_calls == 3
    if ef == "ef14":
        assert rig.call(st)[1] == [("exchange_step", N.ERR_IN_ZERO_ROWS, 0, None, None)]
        st.wire_dtype = BF16  # ... whose record a bf16-wire step drops
        assert rig.call(st)[1] == [("bind_wire16", True), ("exchange_step", N.ERR_IN_READ, 0, None, None)]
        st.wire_dtype = None
        assert rig.call(st)[1] == [("bind_wire16", False), ("exchange_step", N.ERR_IN_READ, 0, None, None)]


def test_step_branch_defers_like_the_default_path(rig):
    st = rig.make()
    st.wire_dtype, st.wire_exchange, st.defer_decode = BF16, "step", True
    f0, c0 = rig.call(st, b=0, is_last=False)
    assert isinstance(f0, H.ExchangeFuture) and not f0.done() and len(st._x_pend) == 1
    assert c0 == [("bind_wire16", True), ("exchange_step", N.ERR_IN_NONE, 1, None, None)]
    f1, c1 = rig.call(st, b=1, is_last=True)  # the backward's last bucket finishes everything pending
    assert c1 == [("bind_wire16", True), ("exchange_step", N.ERR_IN_NONE, 0, None, None)]
    assert f0.done() and f1.done() and not st._x_pend and st.wire16_step_calls == 2
    f2, _ = rig.call(st, b=0, is_last=False)
    assert not f2.done()
    st.flush_exchange()
    assert f2.done() and not st._x_pend and rig.lib.calls[-1] == ("exchange_finish",)
    # the c4 hook inherits the branch
    st4 = rig.make(H4.GroupTopKState)
    st4.wire_dtype, st4.wire_exchange = BF16, "step"
    assert [c[0] for c in rig.call(st4, hook=H4.group_topk_hook)[1]] == ["bind_wire16", "exchange_step"]


def test_step_branch_takes_no_groups_select_stream_or_trail(rig):
    st = rig.make(ws=2)
    st.wire_dtype, st.wire_exchange, st.defer_decode = BF16, "step", True
    st.exchange_groups, st.select_streams, st.trail_bytes = "all", "on", 1 << 30
    fut, calls = rig.call(st, is_last=False)  # (_Plan has no groups(): a grouped bucket would raise)
    assert calls == [("bind_wire16", True), ("exchange_step", N.ERR_IN_NONE, 1, None, None)]
    assert st.trail_calls == 0 and st._trail is None and len(st._x_pend) == 1
    # bits: the sketch in fp32, the selected values in bf16; the bf16 buffer is registered
    segs = W.segments(SHAPES, 0.2)
    assert st.comm_bits_this_round == 2 * (2 - 1) * W.bits_per_call(segs, 4)
    plan = next(p for p in rig.plans.values() if p.packed16 is not None)
    assert any(t is plan.packed16 for t in st._test_comms[1].registered) and plan.packed16_registered is st._test_comms[1]
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
