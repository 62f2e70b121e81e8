"""The c4 variant of the ARC-TopK hook on an MI355X (run with -m gpu): DENSE 1-D tensors, the
ratio ramp and the restarted projection draws, against the reference's own runs
(tests/golden/c4arc_*) and the CPU restatement (arc_c4_oracle).

Parity bar, as for the base hook: rows equal to the reference's wherever the k-th and (k+1)-th
energies differ by more than the sketch's rounding (the fixtures' thresholds all have a relative
gap >= 1e-4; the GPU's sketch sums differ from CPU sgemm's by ~4e-7), and every output and
residual bit-identical given the rows.
"""
import os
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import arc_c4_oracle as C4
from allreducetopk_amd import _native as N
from allreducetopk_amd.bucket import SyntheticBucket, bucket_numel
from allreducetopk_amd.comm_hooks import group_topk_hook_no_reshape_c4 as G4
from allreducetopk_amd.comm_hooks.group_topk_hook_no_reshape import BucketPlan
from golden_io import Golden
from oracle import arctopk as A
from parity import assert_bitwise, check_rows_tie_aware, ensure_group, rendezvous

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
DEV = "cuda:0"
# [1], [3]: the smallest tensors, and every later offset off 16-B alignment; 4097: one past the
# 4096-element RAW encode tile; 20000: past every single-block select limit (a multi-block select
# item under the base hook)
S10 = [[1], [3], [40, 16], [4097], [16, 8, 1, 1], [5], [96, 40], [20000], [4, 3, 3, 3], [7]]


@pytest.fixture(scope="module", autouse=True)
def group():
    ensure_group("nccl")
    yield


def _gpu_rows(plan):
    rl = plan.rowlist.cpu()
    return [rl[s.sel_off:s.sel_off + s.k_rows].long() for s in plan.segments]


def _state(m, **kw):
    st = G4.GroupTopKState(None, r=m["r"], compress_ratio=m["ratio"], start_compress_iter=m["start"],
                           use_error_feedback=m["ef"], seed=m["seed"], warmup_iters=m["warmup"])
    st.projections = "host"  # the golden vectors come from the reference run on CPU
    for k, v in kw.items():
        setattr(st, k, v)
    return st


def _check_call_against_fixture(g, st, out, rank, it, name, rows_exact=True):
    """One call of a fixture run: rows as sets, out / E / gE bitwise, bits, iter, the ratio."""
    what = f"{name} rank{rank} it{it}"
    if g.has(rank, it, "topk0_idx"):
        plan = st._plans[0][1]
        assert plan.ratio == float(g.np(0, it, "ratio")), what + " ratio"
        rows = _gpu_rows(plan)
        sk = [j for j, s in enumerate(plan.segments) if s.kind == N.SEG_SKETCH]
        assert len(sk) == g.count(rank, it, "topk")
        for t, j in enumerate(sk):
            if rows_exact:
                assert sorted(rows[j].tolist()) == sorted(g.t(rank, it, f"topk{t}_idx").tolist()), \
                    what + f" seg{j} rows"
        for j, s in enumerate(plan.segments):
            if s.kind == N.SEG_DENSE:
                assert torch.equal(rows[j], torch.arange(s.n)), what + f" seg{j}: identity rows"
    else:
        assert float(g.np(0, it, "ratio")) == -1.0 or g.meta["ef"] == "ef21"
    assert C4.digest(out) == str(g.np(rank, it, "out_sha")), what + " out digest"
    assert_bitwise(out, g.t(0, it, "out"), what + " out")
    for key, table in (("E", st.error_dict), ("gE", st.global_error_dict)):
        if g.has(rank, it, key + "_sha"):
            if g.has(rank, it, key):
                assert_bitwise(table[0], g.t(rank, it, key), what + " " + key)
            assert C4.digest(table[0]) == str(g.np(rank, it, key + "_sha")), what + f" {key} digest"
        else:
            assert 0 not in table
    assert st.comm_bits_this_round == int(g.np(rank, it, "bits")), what + " bits"
    assert st.iter == int(g.np(rank, it, "iter_after"))


@pytest.mark.parametrize("force_exchange", [False, True])
@pytest.mark.parametrize("name", ["c4arc_gmix_noef_ws1", "c4arc_gmix_ef14_ws1", "c4arc_g2d_ef21_ws1"])
def test_reference_fixtures_through_hip_hook(name, force_exchange):
    """The dense warm-up, three ramp calls with restarted draws and the steady calls of the
    reference's own run, on the step path and through the exchange step."""
    g = Golden(name)
    m = g.meta
    shapes = [tuple(s) for s in m["shapes"]]
    st = _state(m, force_exchange=force_exchange)
    numel = bucket_numel(shapes)
    flags = []
    for it in range(m["iters"]):
        G = C4.bucket_grad(numel, it, 0)
        out = G4.group_topk_hook(st, SyntheticBucket(G.to(DEV), shapes, index=0, is_last=True)).wait()
        torch.cuda.synchronize()
        _check_call_against_fixture(g, st, out, 0, it, name)
        if g.has(0, it, "topk0_idx"):
            flags.append(st._plans[0][1].flags)
    both = N.PLAN_DENSE_1D | N.PLAN_RESTART_DRAWS
    assert flags[-1] == N.PLAN_DENSE_1D and flags.count(both) >= 2
    assert len(st._plans) == 1  # one live plan per bucket through the ramp


def _ws2_worker(rank, ws, port, name, group_bytes):
    sys.path.insert(0, REPO)
    sys.path.insert(0, HERE)
    torch.set_num_threads(2)
    dist.init_process_group("gloo", init_method=port, rank=rank, world_size=ws)
    g = Golden(name)
    m = g.meta
    shapes = [tuple(s) for s in m["shapes"]]
    st = _state(m)
    if group_bytes:
        st.exchange_groups, st.group_bytes = "all", group_bytes
    numel = bucket_numel(shapes)
    grouped = 0
    for it in range(m["iters"]):
        G = C4.bucket_grad(numel, it, rank)
        out = G4.group_topk_hook(st, SyntheticBucket(G.to(DEV), shapes)).wait()
        torch.cuda.synchronize()
        _check_call_against_fixture(g, st, out, rank, it, name)
        if group_bytes and g.has(rank, it, "topk0_idx"):
            plan = st._plans[0][1]
            units = plan.groups(group_bytes)
            assert units is not None and len(units) >= 3, f"{name}: {units} groups"
            grouped += 1
            if any(len(s) == 1 for s in shapes):  # some group holds DENSE segments only: no sketch
                assert any(u.info.sketch_len == 0 for u in units)
            rl = plan.rowlist.cpu()
            both = [torch.empty_like(rl) for _ in range(ws)]
            dist.all_gather(both, rl)
            assert all(torch.equal(both[0], x) for x in both[1:]), f"{name} it{it}: ranks' rows differ"
    assert not group_bytes or grouped >= 3
    # the plans the ramp replaced are gone, their buffers too: the communicators (callback ones
    # here, which know buffers by address) hold views of the live plan's buffers only
    plan = st._plans[0][1]
    live = {plan.sketch.untyped_storage().data_ptr(), plan.packed.untyped_storage().data_ptr()}
    for c in (st._comms[2], st._comms[3]):
        assert c._views and {v.untyped_storage().data_ptr() for v in c._views.values()} <= live
    dist.destroy_process_group()


@pytest.mark.parametrize("group_bytes", [0, 8192])
@pytest.mark.parametrize("name", ["c4arc_gmix_ef14_ws2", "c4arc_g2d_ef21_ws2"])
def test_reference_ws2_fixtures(name, group_bytes):
    """Two gloo ranks on one GPU, whole buckets and cut into exchange groups of <= 8 KiB."""
    mp.spawn(_ws2_worker, args=(2, rendezvous(), name, group_bytes), nprocs=2, join=True)


def _run_against_restatement(shapes, ef, ratio, gradual, warmup, calls, seed, gseed, **kw):
    """The hook (device projections) against the restatement given the device's rows: outputs and
    residuals bitwise; rows exact where the restatement's threshold gap is >= 1e-4, within a
    2e-4 band below that.  Returns (selects, selects in the second class)."""
    st = G4.GroupTopKState(None, r=4, compress_ratio=ratio, start_compress_iter=0, use_error_feedback=ef,
                           seed=seed, gradual_compression=gradual, warmup_iters=warmup)
    for k, v in kw.items():
        setattr(st, k, v)
    o = C4.C4Oracle(1, shapes, ratio, r=4, start=0, ef=ef, seed=seed, gradual=gradual, warmup_iters=warmup)
    numel = bucket_numel(shapes)
    selects = close = 0
    for it in range(calls):
        G = torch.randn(numel, generator=torch.Generator().manual_seed(gseed + it))
        out = G4.group_topk_hook(st, SyntheticBucket(G.to(DEV), shapes, index=0, is_last=True)).wait()
        torch.cuda.synchronize()
        rows = _gpu_rows(st._plans[0][1]) if 0 in st._plans else None
        res = o.call([G], rows_override=rows, proj_device=DEV)
        what = f"{ef} it{it} ({res['kind']})"
        if res["kind"] == "compressed":
            plan = st._plans[0][1]
            assert plan.ratio == res["ratio"] and bool(plan.flags & N.PLAN_RESTART_DRAWS) == res["restart"]
            gaps = dict(res["res"]["gaps"])
            for j, s in enumerate(plan.segments):
                if s.kind == N.SEG_DENSE:
                    assert torch.equal(rows[j], torch.arange(s.n))
                    continue
                selects += 1
                exact = gaps[j] >= 1e-4
                close += int(not exact)
                flips = check_rows_tie_aware(rows[j], res["res"]["norms"][j], int(s.k_rows),
                                             band=0.0 if exact else 2e-4)
                assert not exact or flips == 0, what + f" seg{j}"
        assert_bitwise(out, res["out"], what + " out")
        if ef != "noef":
            assert_bitwise(st.error_dict[0], o.Es[0], what + " E")
        if ef == "ef21":
            assert_bitwise(st.global_error_dict[0], o.gE, what + " gE")
        assert st.iter == o.iter and st.comm_bits_this_round == o.bits
    return selects, close


@pytest.mark.parametrize("ramp", [False, True])
@pytest.mark.parametrize("ef", ["noef", "ef14", "ef21"])
def test_hook_vs_restatement_given_device_rows(ef, ramp):
    """ramp False: ratio 0.08, gradual_compression off (the first call still restarts its draws:
    warmup_iters 1); ramp True: 0.8 -> 0.08 over warmup_iters 2.  EF21 includes 1-D tensors (the
    deviation from the reference, which raises there)."""
    selects, close = _run_against_restatement(S10, ef, 0.08, ramp, 2 if ramp else 1, 4 + (ef == "ef21"),
                                              seed=77, gseed=300)
    assert selects >= 16 and close * 10 <= selects, f"{close} of {selects} selects within 1e-4 of a tie"


@pytest.mark.parametrize("mode", ["force_exchange", "host_staged"])
def test_other_paths_vs_restatement(mode):
    """The exchange step (the N > 1 code path over one-rank communicators) and the phase entry
    points (arctopk_encode / select / pack / decode, which the host-staged mode calls)."""
    selects, close = _run_against_restatement(S10, "ef14", 0.08, True, 2, 4, seed=78, gseed=400, **{mode: True})
    assert close * 10 <= selects


@pytest.mark.parametrize("force_exchange", [False, True])
@pytest.mark.parametrize("ef", ["noef", "ef14", "ef21"])
def test_bucket_of_1d_tensors_only(ef, force_exchange):
    shapes = [[16], [7]]
    st = G4.GroupTopKState(None, compress_ratio=0.2, start_compress_iter=0, use_error_feedback=ef, seed=5,
                           warmup_iters=1)
    st.force_exchange = force_exchange
    o = C4.C4Oracle(1, shapes, 0.2, start=0, ef=ef, seed=5, warmup_iters=1)
    for it in range(3):
        G = torch.randn(23, generator=torch.Generator().manual_seed(50 + it))
        out = G4.group_topk_hook(st, SyntheticBucket(G.to(DEV), shapes, index=0, is_last=True)).wait()
        torch.cuda.synchronize()
        res = o.call([G])
        assert_bitwise(out, res["out"], f"{ef} it{it} out")
        if ef == "noef":
            assert_bitwise(out, G, "noef: the mean of one rank is the gradient")
        if ef == "ef14":
            assert not st.error_dict[0].any(), "EF14: everything was sent, E stays zero"
        if ef == "ef21":
            assert_bitwise(st.error_dict[0], o.Es[0], f"it{it} E")
            assert_bitwise(st.global_error_dict[0], o.gE, f"it{it} gE")
        if res["kind"] == "compressed":
            plan = st._plans[0][1]
            assert plan.info.sketch_len == 0 and plan.info.v_len == 0
            assert plan.info.values_len == plan.info.sel_rows == plan.info.rows_total == 23
        assert st.comm_bits_this_round == o.bits


def test_plan_facts_with_dense_segments():
    shapes = [[20000], [40, 16], [5], [16, 8, 3, 3], [3]]
    st = G4.GroupTopKState(None, compress_ratio=0.2, start_compress_iter=0, use_error_feedback="ef14", seed=5,
                           warmup_iters=0)
    G = torch.randn(bucket_numel(shapes), generator=torch.Generator().manual_seed(9))
    for _ in range(2):
        G4.group_topk_hook(st, SyntheticBucket(G.to(DEV), shapes, index=0, is_last=True)).wait()
    torch.cuda.synchronize()
    plan = st._plans[0][1]
    assert plan.flags == N.PLAN_DENSE_1D
    segs = plan.segments
    assert [s.kind for s in segs] == [N.SEG_DENSE, N.SEG_SKETCH, N.SEG_DENSE, N.SEG_SKETCH, N.SEG_DENSE]
    assert plan.info.sketch_len == sum(s.n * 4 for s in segs if s.kind == N.SEG_SKETCH) == (40 + 64) * 4
    assert plan.ms == (16, 18)
    assert plan.bits_sum == 32 * (20000 + 5 + 3 + 40 * 4 + 8 * 16 + 64 * 4 + 12 * 18)
    rl, sm = plan.rowlist.cpu(), plan.slotmap.cpu()
    for s in segs:
        if s.kind == N.SEG_DENSE:
            assert s.k_rows == s.n and s.v_off == -1
            assert torch.equal(rl[s.sel_off:s.sel_off + s.n], torch.arange(s.n, dtype=torch.int32))
            assert torch.equal(sm[s.row_off:s.row_off + s.n], torch.arange(s.n, dtype=torch.int32))
    # the public select on other buffers leaves the identity there too
    rl2 = torch.full_like(plan.rowlist, -7)
    sm2 = torch.full_like(plan.slotmap, -7)
    N.check(N.lib().arctopk_select(plan.handle, plan.sketch.data_ptr(), 1, rl2.data_ptr(), sm2.data_ptr(),
                                   torch.cuda.current_stream().cuda_stream), "arctopk_select")
    torch.cuda.synchronize()
    assert torch.equal(rl2.cpu(), rl) and torch.equal(sm2.cpu(), sm)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("r", [2, 4])
def test_restarted_device_draws(dtype, r):
    """arctopk_draw_projections on a RESTART_DRAWS plan: every tensor's V is what a fresh device
    generator seeded with the seed draws (torch.empty(m, r).normal_(generator=g))."""
    ms = [2, 18, 40, 64, 5461]
    shapes = [(3, 2), (5,), (4, 3, 3, 3), (8, 40), (6, 64), (9,), (4, 5461)]
    plan = BucketPlan(shapes, r, 0.5, dtype, DEV, flags=N.PLAN_DENSE_1D | N.PLAN_RESTART_DRAWS)
    assert plan.ms == tuple(ms) and plan.philox_advance == 0
    for seed in (0, 123456789):
        V = plan.V_ring[0]
        V.zero_()
        N.check(N.lib().arctopk_draw_projections(plan.handle, seed, V.data_ptr(),
                                                 torch.cuda.current_stream().cuda_stream), "draw")
        torch.cuda.synchronize()
        for s in plan.segments:
            if s.kind != N.SEG_SKETCH:
                continue
            g = torch.Generator(device=DEV)
            g.manual_seed(seed)
            ref = torch.empty(s.m, r, device=DEV, dtype=dtype).normal_(generator=g)
            assert_bitwise(V[s.v_off:s.v_off + s.m * r].view(s.m, r), ref, f"V of m={s.m} r={r} seed {seed}")
    # the same plan without the flag keeps the advancing stream (the base hook's draws)
    plain = BucketPlan(shapes, r, 0.5, dtype, DEV, flags=N.PLAN_DENSE_1D)
    assert plain.philox_advance > 0


def test_global_generator_after_ramp_and_steady_calls():
    """Device projections: a ramp call leaves the device generator where torch.manual_seed(seed)
    alone does (its draws use generators of their own); a steady call where the base hook's
    draws leave it."""
    shapes = [[64, 256], [128], [32, 16, 3, 3], [200, 96]]
    st = G4.GroupTopKState(None, compress_ratio=0.2, start_compress_iter=0, seed=12, warmup_iters=1)
    rng = torch.Generator().manual_seed(12)
    G = torch.randn(bucket_numel(shapes), generator=torch.Generator().manual_seed(1))
    for it in range(2):
        seed = int(torch.randint(0, 1_000_000_000, (1,), generator=rng).item())
        G4.group_topk_hook(st, SyntheticBucket(G.to(DEV), shapes, index=0, is_last=True)).wait()
        torch.cuda.synchronize()
        after = (torch.cuda.default_generators[0].get_offset(), torch.randn(3, device=DEV).cpu(),
                 torch.randn(3).clone())
        torch.manual_seed(seed)
        if it == 1:  # steady: one global-stream draw per 2-D / ND tensor
            for s in C4.segments(shapes, 0.2):
                if s.kind == C4.SKETCH:
                    torch.empty(s.m, 4, device=DEV).normal_()
        ref = (torch.cuda.default_generators[0].get_offset(), torch.randn(3, device=DEV).cpu(),
               torch.randn(3).clone())
        assert after[0] == ref[0] and (it == 1) == (after[0] > 0), f"call {it}: offset {after[0]} vs {ref[0]}"
        assert torch.equal(after[1], ref[1]) and torch.equal(after[2], ref[2])


def test_bf16_fixture():
    """The bf16 run: the device's rows satisfy the reference's norms under the tie rule within
    one bf16 rounding of the sketch, and outputs are bitwise the restatement's given those rows
    (the restatement replays this fixture bit for bit on the reference's own rows)."""
    name = "c4arc_gmix_noef_bf16_ws1"
    g = Golden(name)
    m = g.meta
    shapes = [tuple(s) for s in m["shapes"]]
    st = _state(m)
    o = C4.C4Oracle(1, shapes, m["ratio"], r=m["r"], start=m["start"], ef=m["ef"], seed=m["seed"],
                    warmup_iters=m["warmup"])
    numel = bucket_numel(shapes)
    same = differ = flips = 0
    for it in range(m["iters"]):
        G = C4.bucket_grad(numel, it, 0, torch.bfloat16)
        out = G4.group_topk_hook(st, SyntheticBucket(G.to(DEV), shapes, index=0, is_last=True)).wait()
        torch.cuda.synchronize()
        assert out.dtype == torch.bfloat16
        rows = _gpu_rows(st._plans[0][1]) if 0 in st._plans else None
        res = o.call([G], rows_override=rows)
        assert_bitwise(out, res["out"], f"{name} it{it} out given the rows")
        if res["kind"] == "compressed":
            assert int(g.np(0, it, "seed")[0]) == res["seed"]
            plan = st._plans[0][1]
            sk = [j for j, s in enumerate(plan.segments) if s.kind == N.SEG_SKETCH]
            ref_out = g.t(0, it, "out")
            agree = {}
            for t, j in enumerate(sk):
                ref_norm = g.t(0, it, f"topk{t}_in").float()
                flips += check_rows_tie_aware(rows[j], ref_norm, int(plan.segments[j].k_rows), band=2.0 ** -7)
                agree[j] = sorted(rows[j].tolist()) == sorted(g.t(0, it, f"topk{t}_idx").tolist())
            # the reference's own output, tensor by tensor (noef: a tensor's output depends on its
            # own rows only): every 1-D tensor, and every tensor whose rows are the reference's
            for j, s in enumerate(plan.segments):
                if agree.get(j, True):
                    lo, hi = int(s.offset), int(s.offset + s.n * s.m)
                    assert_bitwise(out[lo:hi], ref_out[lo:hi], f"{name} it{it} seg{j} out vs the reference")
            same += sum(agree.values())
            differ += len(agree) - sum(agree.values())
        else:
            assert_bitwise(out, g.t(0, it, "out"), f"{name} it{it} out")
        assert st.comm_bits_this_round == int(g.np(0, it, "bits")) and st.iter == int(g.np(0, it, "iter_after"))
    # the comparison against the reference's own outputs ran for 2-D / ND tensors too (bf16 norms
    # tie often at the k-th value and the reference's tie order is its own, so not for every one)
    print(f"{name}: {same} selects with the reference's rows, {differ} without, {flips} rows off the exact tie rule")
    assert same >= 1, "no tensor got the reference's rows: its outputs were compared for 1-D tensors only"


def test_resume_mid_ramp_is_bit_identical(tmp_path):
    """Checkpoint after the second ramp call, load into a fresh state: the remaining calls (the
    third ramp call at its own ratio, with restarted draws, then steady ones) are bit-identical."""
    shapes = [tuple(s) for s in S10]
    numel = bucket_numel(shapes)

    def fresh():
        return G4.GroupTopKState(None, compress_ratio=0.2, start_compress_iter=1, use_error_feedback="ef21",
                                 seed=31, warmup_iters=3)

    def call(st, it):
        flags = st._plan_flags()  # (of this call, once compression has started)
        G = torch.randn(numel, generator=torch.Generator().manual_seed(700 + it))
        out = G4.group_topk_hook(st, SyntheticBucket(G.to(DEV), shapes, index=0, is_last=True)).wait()
        torch.cuda.synchronize()
        return out.cpu().clone(), st.error_dict[0].cpu().clone() if 0 in st.error_dict else None, \
            st.global_error_dict[0].cpu().clone() if 0 in st.global_error_dict else None, \
            st.get_current_compress_ratio(), flags

    a = fresh()
    want = [call(a, it) for it in range(7)]  # dense, EF21 init, ramp, ramp | ramp, steady, steady
    b = fresh()
    for it in range(4):
        call(b, it)
    assert b.compression_started and b._deterministic_projections()
    torch.save(b.state_dict(), tmp_path / "ck.pt")
    c = fresh()
    c.load_state_dict(torch.load(tmp_path / "ck.pt", weights_only=True), device=DEV)
    assert c.compression_started and c.iter == 4
    for it in range(4, 7):
        got = call(c, it)
        for x, y, what in zip(got[:3], want[it][:3], ("out", "E", "gE")):
            assert_bitwise(x, y, f"resumed call {it} {what}")
        assert got[3:] == want[it][3:]
    assert want[4][4] & N.PLAN_RESTART_DRAWS and not want[6][4] & N.PLAN_RESTART_DRAWS
