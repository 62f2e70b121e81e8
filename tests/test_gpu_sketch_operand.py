"""bf16 operands of the fp32 sketch projection at r = 16 / 32 on an MI355X (run with -m gpu):
arctopk_plan_set_sketch_operands and GroupTopKState.sketch_operand_dtype.
Shapes: test_gpu_sketch_rank_mfma.py's MFMA_MIX (RAW, ND m = 18, row tails, the scalar path at an odd
offset, slab tails, column parts) and MFMA_LARGE (keys mode).  The reference is the product of the
bf16-rounded operands: in int64 where every sum of magnitudes stays below 2^24, else in float64 with
the fp32 dot-product bound m 2^-24 (|b(X)| |b(V)|) + 2^-24 |P|.
"""
import pytest
import torch

from allreducetopk_amd import _native as N
from allreducetopk_amd.bucket import SyntheticBucket, bucket_numel
from allreducetopk_amd.comm_hooks import group_topk_hook_no_reshape as H
from oracle import arctopk as A
from parity import assert_bitwise, check_rows_tie_aware
from sketch_rank import integer_bucket, integer_projection, integer_residual, sequential_energy
from test_gpu_sketch_rank_mfma import DEV, EFS, F32, MFMA_LARGE, MFMA_MIX, _sketches, _stream, group  # noqa: F401

pytestmark = pytest.mark.gpu
RANKS = pytest.mark.parametrize("r", [16, 32])
MODES = pytest.mark.parametrize("mode", list(EFS))


def _plan(shapes, r, on=True):
    plan = H.BucketPlan([tuple(s) for s in shapes], r, 0.2, F32, DEV)
    N.check(N.lib().arctopk_plan_set_sketch_operands(plan.handle, N.BF16 if on else N.F32), "set_sketch_operands")
    return plan


def _encode(plan, G, E, mode, Vs):
    """arctopk_encode of CPU inputs; the residual it leaves (None: noef)."""
    V = torch.cat([v.flatten() for v in Vs if v is not None]).float().to(DEV)
    e_d = E.float().to(DEV) if EFS[mode][0] != "noef" else None
    plan.encode(G.float().to(DEV), e_d, N.EF_CODE[EFS[mode][0]], EFS[mode][1], V, _stream())
    torch.cuda.synchronize()
    return e_d


def _b(x):
    return x.float().bfloat16().double()


@MODES
@RANKS
def test_encode_exact_on_integers(r, mode):
    """Integers of up to 11 significant bits, which bf16 rounds (257 -> 256, 513 -> 512, 1023 -> 1024):
    the sketch is the int64 product of the rounded X and V, E what the fp32 operands leave."""
    n_el = bucket_numel(MFMA_MIX)
    Gi = torch.tensor([-3, 257, -513, 1023, 2, -1, 0])[integer_bucket(n_el) + 3]
    Ei = integer_residual(n_el) * 129
    Xi = Gi + Ei if mode == "ef14" else Gi - Ei if mode == "ef21" else Gi
    plan = _plan(MFMA_MIX, r)
    assert plan.encode_tiles()["n_split"] >= 1 and plan.encode_tiles()["raw"] >= 1
    Vi = [integer_projection(int(s.m), r) if s.kind == N.SEG_SKETCH else None for s in plan.segments]
    e_on = _encode(plan, Gi, Ei, mode, Vi)
    for s, v, got in zip(plan.segments, Vi, _sketches(plan, r)):
        x = Xi[s.offset:s.offset + s.n * s.m]
        if v is not None:
            x = _b(x).long().view(s.n, s.m)
            assert int((x.abs() @ v.abs()).max()) < 2 ** 24 and (x != Xi[s.offset:s.offset + s.n * s.m].view(s.n, s.m)).any()
            x = (x @ v).flatten()
        assert_bitwise(got, x.float(), f"{mode}: sketch of [{s.n}, {s.m}] at offset {s.offset}")
    if e_on is not None:
        assert_bitwise(e_on, _encode(_plan(MFMA_MIX, r, on=False), Gi, Ei, mode, Vi), f"{mode}: E against the fp32 operands'")
        assert_bitwise(e_on, (Ei if mode == "ef21" else Xi).float(), f"{mode}: the residual after the encode")


def _random(shapes, r, seed):
    gen = torch.Generator().manual_seed(seed)
    n_el = bucket_numel(shapes)
    G, E = torch.randn(n_el, generator=gen), torch.randn(n_el, generator=gen) * 0.5
    plan = _plan(shapes, r)
    return G, E, plan, [torch.randn(int(s.m), r, generator=gen) if s.kind == N.SEG_SKETCH else None for s in plan.segments]


@MODES
@RANKS
def test_encode_random_within_the_bound(r, mode):
    G, E, plan, Vs = _random(MFMA_MIX, r, 1700 + r)
    X = G + E if mode == "ef14" else G - E if mode == "ef21" else G
    _encode(plan, G, E, mode, Vs)
    for s, v, got in zip(plan.segments, Vs, _sketches(plan, r)):
        if v is None:
            continue
        x, v = _b(X[s.offset:s.offset + s.n * s.m].view(s.n, s.m)), _b(v)
        P = x @ v
        excess = ((got.view(s.n, r).double() - P).abs() - s.m * 2.0 ** -24 * (x.abs() @ v.abs()) - 2.0 ** -24 * P.abs()).max()
        assert excess <= 0, f"[{s.n}, {s.m}] at offset {s.offset}: {excess:.3e} beyond the bound"


def test_keys_mode_selects_by_the_rounded_sketch():
    """arctopk_step at world size 1 (keys mode) takes the rows of the sequential energies of the sketch
    that arctopk_encode writes for the same inputs."""
    G, E, plan, Vs = _random(MFMA_LARGE, 32, 1800)
    _encode(plan, G, E, "noef", Vs)
    sk = _sketches(plan, 32)
    plan.V_ring[0].copy_(torch.cat([v.flatten() for v in Vs if v is not None]))
    g_d = G.to(DEV)
    N.check(N.lib().arctopk_step(plan.handle, g_d.data_ptr(), None, None, N.EF_NONE, 1, 0, 0, None, 0,
                                 _stream(), None), "arctopk_step")
    torch.cuda.synchronize()
    assert plan.encode_tiles()["keyed"] == 2
    for s, got in zip(plan.segments, sk):
        energy = sequential_energy(got.view(s.n, 32)) if s.kind == N.SEG_SKETCH else got ** 2
        rows = plan.rowlist[s.sel_off:s.sel_off + s.k_rows].cpu().long()
        assert check_rows_tie_aware(rows, energy, int(s.k_rows)) == 0


@pytest.mark.parametrize("r,gseeds", [(16, [362, 300]), (32, [346, 340])])
def test_hook_selects_by_the_rounded_sketch(r, gseeds):
    """Two EF14 backwards with sketch_operand_dtype: bucket and residual bit for bit those of the oracle
    given the top-k rows of the float64 energies of the rounded-operand sketch.  Gradient seeds chosen on
    the CPU so that the k-th and (k+1)-th energy of every tensor lie further apart (1.7 x at least) than
    the encode's bound and the fp32 energy sum can move them: asserted below."""
    st = H.GroupTopKState(None, r=r, compress_ratio=0.2, start_compress_iter=0, use_error_feedback="ef14", seed=77)
    st.projections, st.sketch_operand_dtype = "host", torch.bfloat16
    ost, E = A.OracleState(r=r, compress_ratio=0.2, start_compress_iter=0, use_error_feedback="ef14", seed=77), None
    for it in range(2):
        G = torch.randn(bucket_numel(MFMA_MIX), generator=torch.Generator().manual_seed(gseeds[it]))
        seed, X, rows = ost.next_seed(), G if E is None else G + E, []
        ref = A.simulate_step([G], [E], None, MFMA_MIX, 0.2, r, "ef14", seed)
        for o, v in zip(ref["segs"], ref["V"]):
            x = X[o.offset:o.offset + o.n * o.m]
            if v is None:
                en, tol = x.double() ** 2, 0.0
            else:
                x, v = _b(x.view(o.n, o.m)), _b(v)
                P = x @ v
                b = o.m * 2.0 ** -24 * (x.abs() @ v.abs()) + 2.0 ** -24 * P.abs()
                en = (P ** 2).sum(1)
                tol = (2 * P.abs() * b + b ** 2).sum(1) + (r + 1) * 2.0 ** -23 * en
            top = torch.topk(en, o.k_rows + 1 if o.k_rows < o.n else o.k_rows)
            assert o.k_rows == o.n or top.values[-2] - top.values[-1] > (tol if v is None else tol[top.indices[-2:]].sum())
            rows.append(top.indices[:o.k_rows])
        res = A.simulate_step([G], [E], None, MFMA_MIX, 0.2, r, "ef14", seed, rows_override=rows)
        out = H.group_topk_hook(st, SyntheticBucket(G.to(DEV), MFMA_MIX, index=0, is_last=True)).wait()
        torch.cuda.synchronize()
        assert_bitwise(out, res["out"], f"it{it} bucket")
        assert_bitwise(st.error_dict[0], res["E_new"][0], f"it{it} E")
        E = st.error_dict[0].cpu().clone()
    assert st.state_dict()["sketch_operand_dtype"] == "bf16"


def test_setter_refusals():
    L, f32 = N.lib(), _plan([[8, 64]], 16)
    for plan, dt in ((f32, 7), (H.BucketPlan([(8, 64)], 4, 0.2, F32, DEV), N.BF16),
                     (H.BucketPlan([(8, 64)], 16, 0.2, torch.bfloat16, DEV), N.BF16)):
        assert L.arctopk_plan_set_sketch_operands(plan.handle, dt) == N.EINVAL
    assert L.arctopk_plan_set_sketch_operands(None, N.BF16) == N.EINVAL
    assert L.arctopk_plan_set_sketch_operands(f32.handle, N.F32) == 0
