"""The c4 variant of the ARC-TopK hook without a GPU: the CPU restatement (arc_c4_oracle)
against the reference's own runs (tests/golden/c4arc_*), the native plan geometry with DENSE
1-D tensors, the ratio schedule and cal_k, the registry and the checkpoint."""
import argparse
import ctypes
import json
import os

import pytest
import torch

import arc_c4_oracle as C4
from allreducetopk_amd import _native as N
from allreducetopk_amd.comm_hooks import group_topk_hook_no_reshape as G
from allreducetopk_amd.comm_hooks import group_topk_hook_no_reshape_c4 as G4
from allreducetopk_amd.comm_hooks.utils import add_comm_hook_args, register_comm_hook_for_ddp_model
from golden_io import GOLDEN, Golden, case_names
from test_capi import SHAPE_SETS

CASES = case_names("c4arc_")


def test_fixture_set():
    assert CASES == ["c4arc_g2d_ef21_ws1", "c4arc_g2d_ef21_ws2", "c4arc_gmix_ef14_ws1", "c4arc_gmix_ef14_ws2",
                     "c4arc_gmix_noef_bf16_ws1", "c4arc_gmix_noef_ws1"]
    for name in CASES:
        assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) < (1 << 20)


def _eq(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {a.shape} {a.dtype} vs {b.shape} {b.dtype}"
    assert torch.equal(a, b), f"{what}: max |diff| {(a.double() - b.double()).abs().max().item()}"


@pytest.mark.parametrize("name", CASES)
def test_restatement_replays_reference(name):
    """out, E, gE, bits, iter and the ratio of every call, the seeds, projections, norms and rows of
    every compressed one: bit for bit."""
    g = Golden(name)
    m = g.meta
    ws, dtype = m["ws"], torch.bfloat16 if m.get("dtype") == "bf16" else torch.float32
    o = C4.C4Oracle(ws, m["shapes"], m["ratio"], r=m["r"], start=m["start"], ef=m["ef"], seed=m["seed"],
                    warmup_iters=m["warmup"])
    numel = sum(s.numel for s in C4.segments(m["shapes"], m["ratio"]))
    kinds = []
    for it in range(m["iters"]):
        Gs = [C4.bucket_grad(numel, it, q, dtype) for q in range(ws)]
        for q in range(ws):
            assert C4.digest(Gs[q]) == str(g.np(q, it, "G_sha"))
        res = o.call(Gs)
        kinds.append(res["kind"])
        what = f"{name} it{it} ({res['kind']})"
        _eq(res["out"], g.t(0, it, "out"), what + " out")
        want_ratio = float(g.np(0, it, "ratio"))
        assert (res["ratio"] is None and want_ratio == -1.0) or res["ratio"] == want_ratio, what
        if res["kind"] == "compressed":
            r_ = res["res"]
            assert int(g.np(0, it, "seed")[0]) == res["seed"]
            sk = [j for j, s in enumerate(r_["segs"]) if s.kind == C4.SKETCH]
            assert g.count(0, it, "V") == len(sk) == g.count(0, it, "topk")
            for t, j in enumerate(sk):
                s = r_["segs"][j]
                _eq(r_["V"][j], g.t(0, it, f"V{t}"), what + f" V{t}")
                _eq(r_["norms"][j], g.t(0, it, f"topk{t}_in"), what + f" norms{t}")
                assert int(g.np(0, it, f"topk{t}_k")) == s.k_rows == C4.cal_k(s.shape, res["ratio"]) // s.m
                _eq(r_["rows"][j], g.t(0, it, f"topk{t}_idx"), what + f" rows{t}")
            if dtype == torch.float32:
                assert min([gap for _, gap in r_["gaps"]] or [1.0]) >= 1e-4
        for q in range(ws):
            assert C4.digest(res["out"]) == str(g.np(q, it, "out_sha")), what
            assert int(g.np(q, it, "bits")) == o.bits, what + " bits"
            assert int(g.np(q, it, "iter_after")) == o.iter
            if g.has(q, it, "E_sha"):
                assert C4.digest(o.Es[q]) == str(g.np(q, it, "E_sha")), what + f" r{q} E"
            else:
                assert o.Es[q] is None
            if g.has(q, it, "gE_sha"):
                assert C4.digest(o.gE) == str(g.np(q, it, "gE_sha")), what + " gE"
            if g.has(q, it, "E"):
                _eq(o.Es[q], g.t(q, it, "E"), what + f" r{q} E")
    # the dense warm-up, the ramp with restarted draws and steady calls are all in the run
    assert kinds[0] == "warmup" and kinds.count("compressed") >= 3


def _describe_ex(shapes, r, ratio, flags):
    dims = [int(d) for s in shapes for d in s]
    nd = [len(s) for s in shapes]
    segs = (N.Segment * len(shapes))()
    info = N.PlanInfo()
    st = N.lib().arctopk_plan_describe_ex((ctypes.c_int64 * max(1, len(dims)))(*dims),
                                          (ctypes.c_int32 * len(nd))(*nd), len(nd), r, ratio, flags,
                                          ctypes.cast(segs, ctypes.c_void_p), ctypes.byref(info))
    return st, list(segs), info


def _fields(x):
    return {f: getattr(x, f) for f, _ in x._fields_ if f != "pad"}


@pytest.mark.parametrize("shapes", SHAPE_SETS)
@pytest.mark.parametrize("ratio", [0.2, 0.08, 0.8, 1.0, 0.001])
@pytest.mark.parametrize("r", [4, 2])
def test_plan_geometry_with_dense_1d(shapes, ratio, r):
    for flags in (N.PLAN_DENSE_1D, N.PLAN_DENSE_1D | N.PLAN_RESTART_DRAWS):
        st, segs, info = _describe_ex(shapes, r, ratio, flags)
        assert st == 0
        want_segs, want_info = C4.plan_geometry(shapes, ratio, r)
        assert [_fields(s) for s in segs] == want_segs
        assert _fields(info) == want_info
    for s, shape in zip(segs, shapes):
        assert (s.kind == N.SEG_DENSE) == (len(shape) == 1)
        assert s.k_rows * s.m == C4.cal_k(shape, ratio)
    assert info.sketch_len == sum(s.n * r for s in segs if s.kind == N.SEG_SKETCH)
    assert N.SEG_RAW not in [s.kind for s in segs]


@pytest.mark.parametrize("shapes", SHAPE_SETS)
def test_describe_ex_without_flags_is_describe(shapes):
    from test_capi import _describe
    for ratio, r in ((0.2, 4), (0.08, 3)):
        st0, segs0, info0 = _describe(N.lib(), shapes, r, ratio)
        st1, segs1, info1 = _describe_ex(shapes, r, ratio, 0)
        assert st0 == st1 == 0
        assert [_fields(s) for s in segs0] == [_fields(s) for s in segs1]
        assert _fields(info0) == _fields(info1)
    assert _describe_ex(shapes, 4, 0.2, 4)[0] == N.EINVAL  # unknown flag


def _state(**kw):
    return G4.GroupTopKState(None, **kw)


@pytest.mark.parametrize("warmup", [0, 1, 2])
def test_ratio_schedule_and_cal_k(warmup):
    """start = 1, ratio 0.2: iteration 0 is dense; then 0.8, 0.6, 0.4, 0.2, ... at warmup_iters 2
    (the fixtures' ratios), and the restatement's schedule at 0 and 1."""
    st = _state(compress_ratio=0.2, start_compress_iter=1, warmup_iters=warmup)
    assert (st.base_compress_ratio, st.compress_ratio, st.warmup_iters, st.compression_started,
            st.gradual_compression) == (0.2, 0.2, 1 + warmup, False, True)
    assert st.get_current_compress_ratio() == 0.2  # not started: the base ratio
    st.compression_started = True
    got = []
    for it in range(1, 7):
        st.iter = it
        got.append(st.get_current_compress_ratio())
        assert got[-1] == C4.current_ratio(0.2, it, 1, 1 + warmup)
        assert st._plan_ratio() == got[-1]
        assert st._deterministic_projections() == C4.deterministic(it, 1, 1 + warmup)
        assert st._plan_flags() == N.PLAN_DENSE_1D | (N.PLAN_RESTART_DRAWS if it - 1 < 1 + warmup else 0)
        for shape in ([7], [40, 16], [16, 8, 3, 3], [16, 8, 1, 1]):
            assert G4.cal_k(st, torch.empty(shape)) == C4.cal_k(shape, got[-1])
    if warmup == 2:
        g = Golden("c4arc_gmix_noef_ws1")
        assert got[:5] == [float(g.np(0, it, "ratio")) for it in range(1, 6)]
        assert [round(x, 12) for x in got[:5]] == [0.8, 0.6, 0.4, 0.2, 0.2]
    assert got[-1] == 0.2 and G4.cal_k(st, torch.empty(5)) == 5


@pytest.mark.parametrize("warmup", [0, 1, 2])
def test_ratio_schedule_and_cal_k_against_reference(warmup):
    """The reference state's own ratios and cal_k per iteration (c4arc_ratio_schedule.json), and at
    warmup_iters 1 and 2 the ratios its hook read in the fixture runs."""
    with open(os.path.join(GOLDEN, "c4arc_ratio_schedule.json")) as f:
        ref = json.load(f)
    sch = next(x for x in ref["schedules"] if x["warmup_iters"] == warmup)
    st = _state(compress_ratio=sch["ratio"], start_compress_iter=sch["start"], warmup_iters=warmup)
    assert st.warmup_iters == sch["warmup_field"]
    assert len(sch["calls"]) == 16
    for c in sch["calls"]:
        st.compression_started, st.iter = c["started"], c["iter"]
        assert st.get_current_compress_ratio() == c["ratio"], c
        assert [G4.cal_k(st, torch.empty(s)) for s in ref["shapes"]] == c["cal_k"], c
    for name in {1: ["c4arc_gmix_ef14_ws2", "c4arc_g2d_ef21_ws2"],
                 2: ["c4arc_gmix_noef_ws1", "c4arc_gmix_ef14_ws1", "c4arc_g2d_ef21_ws1"], 0: []}[warmup]:
        g = Golden(name)
        st = _state(compress_ratio=g.meta["ratio"], start_compress_iter=g.meta["start"], warmup_iters=warmup)
        st.compression_started = True
        seen = 0
        for it in range(g.meta["iters"]):
            want = float(g.np(0, it, "ratio"))
            if want >= 0:
                st.iter = it
                assert st.get_current_compress_ratio() == want, (name, it)
                seen += 1
        assert seen >= 3


def test_ratio_schedule_without_warmup_divides_by_nothing():
    st = _state(compress_ratio=0.08, start_compress_iter=0, warmup_iters=0)
    st.compression_started = True
    for it in range(3):
        st.iter = it
        assert st.get_current_compress_ratio() == 0.08 and not st._deterministic_projections()
    st = _state(compress_ratio=0.08, gradual_compression=False)
    st.compression_started, st.iter = True, 3
    assert st.get_current_compress_ratio() == 0.08
    assert st._deterministic_projections()  # the draws restart whatever the ratio does (:300)
    # the reference's defaults
    st = _state()
    assert (st.r, st.compress_ratio, st.start_compress_iter, st.use_error_feedback, st.warmup_iters) == (
        4, 0.08, 2, "noef", 102)


def test_base_hook_state_keeps_its_plan_key():
    st = G.GroupTopKState(None, compress_ratio=0.3)
    assert st._plan_ratio() == 0.3 and st._plan_flags() == 0


class _FakeModel:
    def __init__(self):
        self.hooks = []
        self.lin = torch.nn.Linear(3, 2)

    def register_comm_hook(self, state, hook):
        self.hooks.append((state, hook))

    def named_parameters(self):
        return self.lin.named_parameters()


def test_registry_builds_the_c4_state():
    p = argparse.ArgumentParser()
    add_comm_hook_args(p)
    p.add_argument("--seed", type=int, default=0)
    a = p.parse_args(["--compressor", "group_topk_no_reshape_c4", "--compress_ratio", "0.2",
                      "--use_error_feedback", "ef14", "--seed", "3", "--start_compress_iter", "5", "--r", "2"])
    m = _FakeModel()
    st = register_comm_hook_for_ddp_model(m, None, a)
    assert type(st) is G4.GroupTopKState and m.hooks == [(st, G4.group_topk_hook)]
    assert (st.compress_ratio, st.base_compress_ratio, st.use_error_feedback, st.seed, st.r,
            st.start_compress_iter) == (0.2, 0.2, "ef14", 3, 2, 5)
    assert st.gradual_compression and st.warmup_iters == 105 and not st.compression_started
    assert st._ddp_registered and set(st.param_to_name.values()) == {"weight", "bias"}
    # the base name still builds the base state
    a.compressor = "group_topk_no_reshape"
    st0 = register_comm_hook_for_ddp_model(_FakeModel(), None, a)
    assert type(st0) is G.GroupTopKState


def test_state_dict_round_trips_compression_started():
    st = _state(compress_ratio=0.2, start_compress_iter=1, warmup_iters=2, seed=9)
    st.iter, st.compression_started = 3, True
    torch.randint(0, 1_000_000_000, (2,), generator=st.rng)
    sd = st.state_dict()
    assert sd["compression_started"] is True and sd["iter"] == 3
    st2 = _state(compress_ratio=0.2, start_compress_iter=1, warmup_iters=2, seed=0)
    st2.load_state_dict(sd)
    assert st2.compression_started and st2.iter == 3
    assert st2.get_current_compress_ratio() == st.get_current_compress_ratio() == C4.current_ratio(0.2, 3, 1, 3)
    assert st2._next_seed() == st._next_seed()
    fresh = _state()
    fresh.load_state_dict({k: v for k, v in sd.items() if k != "compression_started"})
    assert fresh.compression_started is False  # an older checkpoint: the first call sets it


def test_ef21_with_1d_tensor_error_fixture():
    with open(os.path.join(GOLDEN, "c4arc_ef21_1d_error.json")) as f:
        e = json.load(f)
    assert e["raises"] == "RuntimeError" and e["call"] == 1 and e["iter_after"] == 1
    assert "refer to a single memory location" in e["message"]
    assert any(len(s) == 1 for s in e["shapes"])


def test_restatement_runs_ef21_with_1d_tensors():
    """The deviation: a 1-D tensor under EF21 behaves as a tensor whose rows are all selected."""
    shapes = [[5], [12, 8], [3]]
    o = C4.C4Oracle(2, shapes, 0.25, start=0, ef="ef21", seed=1, warmup_iters=1)
    Gs0 = [C4.bucket_grad(104, 0, q) for q in range(2)]
    o.call(Gs0)  # EF21 init: E = G, gE = mean
    E0, gE0 = [e.clone() for e in o.Es], o.gE.clone()
    Gs1 = [C4.bucket_grad(104, 1, q) for q in range(2)]
    res = o.call(Gs1)
    for lo, hi in ((0, 5), (101, 104)):  # the 1-D tensors: D = G - E; E += D; out = gE + mean(D)
        D = [Gs1[q][lo:hi] - E0[q][lo:hi] for q in range(2)]
        for q in range(2):
            assert torch.equal(o.Es[q][lo:hi], E0[q][lo:hi] + D[q])
        assert torch.equal(res["out"][lo:hi], gE0[lo:hi] + (D[0] + D[1]) / 2)
    assert torch.equal(o.gE, res["out"])
