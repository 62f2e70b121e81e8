"""Sketch ranks r = 1 .. 8 on an MI355X (run with -m gpu): every encode instantiation, the generic
energy code of the three select flavours, keys mode, the run-time-rank fp32-residual encode, the
refused zero-rows encode and trailing-step carry, and the device projection draw, at ranks other
than the r = 4 the rest of the suite runs (one process, world size 1, ratio 0.2).

Shape sets and integer inputs: tests/sketch_rank.py.  RANK_MIX differs from the set first proposed
by one inserted [5]: without it no tensor reached the 16-byte row path (see that module).

Energies.  The kernels sum a row's squares sequentially in fp32 (bf16: bf16 squares, one rounding of
the sum).  The CPU oracle's torch.sum over dim 1 gives the same bits for r <= 4 in both dtypes and
for fp32 r = 8 (tests/test_sketch_rank_host.py pins that); for fp32 r = 5, 6, 7 and bf16 r = 5 .. 8
it adds in another order (bf16: visible only on the rare row whose two fp32 sums round to different
bf16 values -- [20000, 8] of RANK_LARGE met one, 30.125 against 30.0).  There the bit-exact
expectation is sketch_rank.sequential_energy, the oracle's energies may differ from the device's by
sketch_rank.energy_band (2 (r - 1) 2^-24 relative in fp32, one bf16 step = 2^-7 in bf16), and the
selected rows satisfy the oracle's energies within that band and the sequential ones exactly.

Tolerances: exact equality; that energy band; the suite's 2e-5 (fp32 sketch vs CPU mm), 2^-7 * (|x| @ |v|)
(bf16 sketch) and 2e-4 (rows chosen from the device's own fp32 sketch).  For the bf16 hook runs of
test (d) the row band is 2^-7, the one tests/test_gpu_arctopk.py::test_bf16_golden_on_gpu uses: a
sketch entry summed in another order may round to the neighbouring bf16 value (2^-8 relative), its
square moves by 2^-7; 2e-4 is below one bf16 rounding and cannot be demanded of a bf16 sketch.
"""

import pytest
import torch

import mixed_ef21_oracle as M21
import mixed_ef_oracle as MX
import test_gpu_err_zero_rows as Z
from allreducetopk_amd import _native as N
from allreducetopk_amd.bucket import SyntheticBucket, bucket_numel
from allreducetopk_amd.comm_hooks.group_topk_hook_no_reshape import (BucketPlan, GroupTopKState,
                                                                      group_topk_hook)
from oracle import arctopk as A
from parity import assert_bitwise, assert_close_rel, check_rows_tie_aware, ensure_group
from sketch_rank import (N_SPLIT_F32, ORDER_DEPENDENT, RANK_LARGE, RANK_MIX, energy_band, integer_bucket,
                         integer_projection, integer_residual, sequential_energy)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, BF16 = torch.float32, torch.bfloat16
RANKS = list(range(1, 9))
DTYPES = pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
MIX_T = [tuple(s) for s in RANK_MIX]
LARGE_T = [tuple(s) for s in RANK_LARGE]


@pytest.fixture(scope="module", autouse=True)
def group():
    ensure_group("nccl")
    yield


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _rand(shapes, seed):
    return torch.randn(bucket_numel(shapes), generator=torch.Generator().manual_seed(seed))


def _rows(plan):
    rl = plan.rowlist.cpu()
    return [rl[s.sel_off:s.sel_off + s.k_rows].long() for s in plan.segments]


def _energies(Ps, segs, dtype, r):
    """(the oracle's energies, the energies the kernels must produce bit for bit, the relative band
    between the two): the oracle's own except for fp32 r = 5, 6, 7 (module docstring)."""
    norms, _ = A.select(Ps, 1, segs)
    if (dtype, r) not in ORDER_DEPENDENT:
        return norms, norms, 0.0
    seq = [P ** 2 if s.kind == A.RAW else sequential_energy(P) for P, s in zip(Ps, segs)]
    return norms, seq, energy_band(r, dtype)


def _check_select(plan, Ps, segs, dtype, r, what):
    """Copies the sketch Ps into the plan, runs row_energy and select, and checks energies, rows,
    order and the slot map; returns the rows."""
    ref_sketch = torch.cat([p.flatten() for p in Ps])
    assert ref_sketch.numel() == plan.info.sketch_len
    plan.sketch[:ref_sketch.numel()].copy_(ref_sketch.to(DEV))
    energy = torch.empty(plan.info.rows_total, device=DEV)
    plan.row_energy(1, energy, _stream())
    plan.select(1, _stream())
    torch.cuda.synchronize()
    norms, exact, band = _energies(Ps, segs, dtype, r)
    en = energy.cpu()
    rows = _rows(plan)
    sm = plan.slotmap.cpu()
    for j, (s, nrm, ex, r_) in enumerate(zip(plan.segments, norms, exact, rows)):
        got = en[s.row_off:s.row_off + s.n]
        assert_bitwise(got, ex.float(), f"{what}: energy of segment {j} [{s.n}, {s.m}]")
        if band:
            excess = (got.double() - nrm.double()).abs() - band * nrm.double()
            assert (excess <= 0).all(), f"{what}: segment {j} energy vs torch.sum, excess {excess.max().item():.3e}"
        check_rows_tie_aware(r_, nrm.float(), int(s.k_rows), band=band)
        assert check_rows_tie_aware(r_, ex.float(), int(s.k_rows), band=0.0) == 0, f"{what}: segment {j} rows"
        assert torch.all(r_[1:] > r_[:-1]), f"{what}: segment {j} rows not ascending"
        slots = sm[s.row_off:s.row_off + s.n]
        assert int((slots >= 0).sum()) == s.k_rows
        assert torch.equal(slots[r_], torch.arange(s.k_rows, dtype=torch.int32))
    return rows


# ---- a. which paths, per rank ----------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("r", RANKS)
def test_paths_per_rank(r, dtype):
    """arctopk_diag_encode_tiles: RANK_MIX holds all four encode tile modes at every rank, in both
    dtypes, and as many column-split tensors as (65536 / (4 r)) rounded down to 16-byte units gives;
    [300, 63] alone is a thread-per-row tile up to r = 4 and a (scalar) row tile from r = 5;
    RANK_LARGE has its two keyed tensors ([20000, 8] from a tile, [16000, 72] from row tiles) and
    does not run the short-row kernel."""
    t = BucketPlan(MIX_T, r, 0.2, dtype, DEV).encode_tiles()
    for mode in ("raw", "tile", "row_vec", "row_scalar"):
        assert t[mode] > 0, (mode, t)
    assert t["n_split"] == N_SPLIT_F32[r], t  # (the same tensors split in bf16)
    assert t["keyed"] == 0 and t["enc_short"] == 0
    assert t["mixed_vlds"] == t["mixed_vglobal"] == -1  # no fp32-residual call yet
    solo = BucketPlan([(300, 63)], r, 0.2, dtype, DEV).encode_tiles()
    if r <= 4:
        assert solo["tile"] > 0 and solo["row_vec"] == solo["row_scalar"] == 0 and solo["enc_short"] == 1, solo
    else:
        assert solo["tile"] == 0 and solo["row_vec"] == 0 and solo["row_scalar"] > 0 and solo["enc_short"] == 0, solo
    big = BucketPlan(LARGE_T, r, 0.2, dtype, DEV).encode_tiles()
    assert big["keyed"] == 2 and big["enc_short"] == 0 and big["n_split"] == 0, big
    assert big["tile"] > 0 and big["row_vec"] + big["row_scalar"] > 0 and big["raw"] > 0, big


# ---- b. exact pairing, every rank, every encode path ----------------------------------------
@pytest.mark.parametrize("ef", ["noef", "ef14", "ef21"])
@DTYPES
@pytest.mark.parametrize("r", RANKS)
def test_encode_pairing_exact(r, dtype, ef):
    """Small-integer G, E and V (tests/sketch_rank.py): every sum is an integer below 2^24, exact in
    fp32 in any order, so the sketch is the int64 X.view(n, m) @ V converted to the dtype, bit for
    bit -- a wrong column, projection column or column part is a wrong integer.  EF14 stores
    E := X, EF21 leaves E alone."""
    n_el = bucket_numel(RANK_MIX)
    Gi, Ei = integer_bucket(n_el), integer_residual(n_el)
    Xi = Gi if ef == "noef" else (Gi + Ei if ef == "ef14" else Gi - Ei)
    plan = BucketPlan(MIX_T, r, 0.2, dtype, DEV)
    Vi = [integer_projection(int(s.m), r) if s.kind == N.SEG_SKETCH else None for s in plan.segments]
    V = torch.cat([v.flatten() for v in Vi if v is not None]).to(dtype)
    assert V.numel() == plan.info.v_len
    e_d = Ei.to(dtype).to(DEV) if ef != "noef" else None
    plan.sketch.fill_(-7.0)
    plan.encode(Gi.to(dtype).to(DEV), e_d, N.EF_CODE[ef], True, V.to(DEV), _stream())
    torch.cuda.synchronize()
    sk = plan.sketch_view.cpu()
    for s, v in zip(plan.segments, Vi):
        x = Xi[s.offset:s.offset + s.n * s.m]
        if s.kind == N.SEG_RAW:
            want = x.float().to(dtype)
            got = sk[s.sketch_off:s.sketch_off + s.n]
        else:
            P = x.view(s.n, s.m) @ v
            assert int(P.abs().max()) < 2 ** 24
            want = P.float().to(dtype)
            got = sk[s.sketch_off:s.sketch_off + s.n * r].view(s.n, r)
        assert_bitwise(got, want, f"r {r} {ef}: sketch of [{s.n}, {s.m}] at offset {s.offset}")
    if ef == "ef14":
        assert_bitwise(e_d, Xi.float().to(dtype), "EF14: E := G + E")
    elif ef == "ef21":
        assert_bitwise(e_d, Ei.float().to(dtype), "EF21: E untouched by the encode")


# ---- c. phases with random data ---------------------------------------------------------------
def _phases(r, ef, dtype):
    segs = A.segments(RANK_MIX, 0.2)
    plan = BucketPlan(MIX_T, r, 0.2, dtype, DEV)
    G = _rand(RANK_MIX, 1).to(dtype)
    E = (_rand(RANK_MIX, 2) * 0.5).to(dtype) if ef != "noef" else None
    gE = _rand(RANK_MIX, 3).to(dtype) if ef == "ef21" else None
    Vs = A.draw_projections(987654 + r, segs, r, dtype)
    X, Ps = A.encode(G, E, ef, segs, Vs)
    # --- encode
    Vflat = torch.cat([v.flatten() for v in Vs if v is not None]).to(DEV)
    g_d = G.to(DEV)
    e_d = E.to(DEV) if E is not None else None
    plan.encode(g_d, e_d, N.EF_CODE[ef], True, Vflat, _stream())
    torch.cuda.synchronize()
    sk = plan.sketch_view.cpu()
    for s, o, P, V in zip(plan.segments, segs, Ps, Vs):
        got = sk[s.sketch_off:s.sketch_off + P.numel()].view_as(P)
        if s.kind == N.SEG_RAW:
            assert_bitwise(got, P, f"RAW sketch seg@{s.offset}")
        elif dtype == F32:
            assert_close_rel(got, P, 2e-5, f"sketch seg@{s.offset} m={s.m}")
        else:  # fp32 accumulation, one rounding to bf16; another order: within one rounding of the sum's magnitude
            x = X[o.offset:o.offset + o.numel].view(s.n, s.m).float()
            ref = (x @ V.float()).to(dtype).float()
            scale = (x.abs() @ V.float().abs()).clamp_min(1e-30)
            bad = ((got.float() - ref).abs() > 2.0 ** -7 * scale).sum().item()
            assert bad == 0, f"[{s.n}, {s.m}]: {bad} sketch entries off by more than one rounding"
    if ef == "ef14":
        assert_bitwise(e_d, X, "E := G + E after encode")
    # --- select on the oracle's sketch
    rows = _check_select(plan, Ps, segs, dtype, r, f"r {r} {ef}")
    # --- pack (rows ascending) and residual
    Xo = X.clone()
    vals = A.pack(Xo, rows, segs, ef)
    plan.pack(g_d, e_d, N.EF_CODE[ef], _stream())
    torch.cuda.synchronize()
    assert_bitwise(plan.packed_values(), vals, "packed values")
    if ef == "ef14":
        assert_bitwise(e_d, Xo, "EF14 residual")
    elif ef == "ef21":
        assert_bitwise(e_d, E + Xo, "EF21 residual")
    # --- decode
    out = torch.empty_like(g_d)
    ge_d = gE.to(DEV) if gE is not None else None
    plan.decode(1, N.EF_CODE[ef], ge_d, out, _stream())
    torch.cuda.synchronize()
    ref_out = A.decode(vals, 1, rows, segs, G.numel(), G.dtype)
    if ef == "ef21":
        ref_out = gE + ref_out
        sel_mask = torch.zeros(G.numel(), dtype=torch.bool)
        for s, r_ in zip(segs, rows):
            sel_mask[s.offset:s.offset + s.numel].view(s.n, s.m)[r_] = True
        assert_bitwise(ge_d.cpu()[sel_mask], ref_out[sel_mask], "gE (selected rows)")
        assert_bitwise(ge_d.cpu()[~sel_mask], gE[~sel_mask], "gE (untouched rows)")
    assert_bitwise(out, ref_out, "decoded bucket")


@pytest.mark.parametrize("ef", ["noef", "ef14", "ef21"])
@pytest.mark.parametrize("r", RANKS)
def test_kernel_phases_fp32(r, ef):
    """encode -> select (fed the oracle's sketch) -> pack -> decode on RANK_MIX, phase by phase, as
    tests/test_gpu_arctopk.py::test_kernel_phases_bitexact does at r = 4."""
    _phases(r, ef, F32)


@pytest.mark.parametrize("ef", ["noef", "ef21"])
@pytest.mark.parametrize("r", RANKS)
def test_kernel_phases_bf16(r, ef):
    """The same in bf16: the sketch within 2^-7 * (|x| @ |v|) of the fp32-accumulated product, the
    energies bit for bit (the oracle's up to r = 4, the sequential restatement's from r = 5)."""
    _phases(r, ef, BF16)


# ---- d. multi-block select and keys mode ----------------------------------------------------
@pytest.mark.parametrize("r,ef,dtype", [(r, ef, F32) for r in (1, 3, 5, 8) for ef in ("ef14", "ef21")]
                         + [(3, "noef", BF16), (8, "noef", BF16)],
                         ids=lambda v: {F32: "fp32", BF16: "bf16"}.get(v, str(v)))
def test_hook_large_segments(r, ef, dtype):
    """RANK_LARGE through group_topk_hook for three calls: the multi-block select's key pass, and at
    world size 1 the encode that writes the keys itself (energy_regs<T, R>), from a thread-per-row
    tile ([20000, 8]) and from wave-per-row tiles ([16000, 72]); [20000] is a 1-D multi-block item.
    Outputs and residuals bit for bit given the device's rows; the rows within the band of the
    device's own sketch; the select fed the oracle's sketch exact."""
    st = GroupTopKState(None, r=r, compress_ratio=0.2, start_compress_iter=0, use_error_feedback=ef, seed=4321)
    ost = A.OracleState(r=r, compress_ratio=0.2, start_compress_iter=0, use_error_feedback=ef, seed=4321)
    own_band = 2.0 ** -7 if dtype == BF16 else 2e-4 + (energy_band(r) if (dtype, r) in ORDER_DEPENDENT else 0.0)
    expect_bits = 0  # as oracle_group_topk_hook counts: EF21's dense first call, then 2 (ws - 1) bits_sum = 0
    bits = torch.finfo(dtype).bits
    E = gE = None
    checked = 0
    for it in range(3):
        G = _rand(RANK_LARGE, 200 + it).to(dtype)
        out = group_topk_hook(st, SyntheticBucket(G.to(DEV), RANK_LARGE, index=0, is_last=True)).wait()
        torch.cuda.synchronize()
        assert st.iter == it + 1
        if ef == "ef21" and E is None:  # init call
            E, gE = G.clone(), G.clone()
            assert_bitwise(out, G, "EF21 init out")
            expect_bits += G.numel() * bits
            continue
        seed = ost.next_seed()
        plan = st._plans[0][1]
        assert plan.r == r and plan.info.r == r
        rows = _rows(plan)
        res = A.simulate_step([G], [E], gE, RANK_LARGE, 0.2, r, ef, seed, rows_override=rows, proj_device=DEV)
        for j, (r_, nrm, s) in enumerate(zip(rows, res["norms"], plan.segments)):
            flips = check_rows_tie_aware(r_, nrm.float(), int(s.k_rows), band=own_band)
            print(f"r {r} {ef} call {it} segment {j}: {flips} rows differ from the oracle's exact selection")
            assert torch.all(r_[1:] > r_[:-1])
        assert_bitwise(out, res["out"], f"it{it} output bucket")
        if ef != "noef":
            assert_bitwise(st.error_dict[0], res["E_new"][0], f"it{it} E")
            E = res["E_new"][0]
        if ef == "ef21":
            assert_bitwise(st.global_error_dict[0], res["gE_new"], f"it{it} gE")
            gE = res["gE_new"]
        assert plan.bits_sum == A.bits_per_call(res["segs"], r, bits)
        assert st.comm_bits_this_round == expect_bits
        _check_select(plan, res["P_sum"], res["segs"], dtype, r, f"r {r} {ef} call {it}, oracle's sketch")
        checked += 1
    assert checked == (2 if ef == "ef21" else 3)
    t = st._plans[0][1].encode_tiles()
    assert t["keyed"] == 2 and t["enc_short"] == 0


# ---- e. the N > 1 code path ---------------------------------------------------------------------
def _two_bucket_run(r, layouts, seeds, **attrs):
    """Three backwards of the buckets `layouts` on one EF14 state; per backward the outputs, then
    the residuals and the state."""
    st = GroupTopKState(None, r=r, compress_ratio=0.2, start_compress_iter=0, use_error_feedback="ef14", seed=21)
    st.defer_decode = True  # Futures waited after the backward's last bucket, as DDP does
    for k, v in attrs.items():
        setattr(st, k, v)
    outs, rows = [], []
    for it in range(3):
        futs = [group_topk_hook(st, SyntheticBucket(_rand(sh, seeds + 10 * it + b).to(DEV), sh, index=b,
                                                    is_last=(b == len(layouts) - 1)))
                for b, sh in enumerate(layouts)]
        outs.append([f.wait().clone() for f in futs])
        torch.cuda.synchronize()
        rows.append([_rows(st._plans[b][1]) for b in range(len(layouts))])
    return outs, rows, st


@pytest.mark.parametrize("r", [3, 8])
def test_exchange_path_gives_the_step_paths_bits(r):
    """RANK_MIX as bucket 0 and RANK_LARGE as bucket 1 over three backwards with deferred decodes:
    the exchange step over a one-rank RCCL communicator (the code world sizes above 1 run) gives the
    bits of the world-size-1 step path."""
    layouts = [RANK_MIX, RANK_LARGE]
    step, _, st0 = _two_bucket_run(r, layouts, 700)
    fx, _, st1 = _two_bucket_run(r, layouts, 700, force_exchange=True)
    assert st1._comms is not None and st1._comms[3].kind == "rccl" and st1._comms[3].size == 1
    for it in range(3):
        for b in range(2):
            Z.same_bits(fx[it][b], step[it][b], f"r {r} backward {it} bucket {b} output")
    for b in range(2):
        Z.same_bits(st1.error_dict[b], st0.error_dict[b], f"r {r} bucket {b} E")


# ---- f. the zero-rows encode is refused ---------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("r", [3, 8])
def test_zero_rows_encode_refused_at_other_ranks(r, dtype):
    """The zero-rows kernels exist for r = 4 only: at another rank a call that claims zero rows runs
    as err_in = 1 (reads all of E).  err_zero_rows on and off give the same bits over four
    backwards (the buckets of tests/test_gpu_err_zero_rows.py), and the counter of zero-rows encode
    launches stays 0 with the feature on: refused, not taken."""
    on, off = Z.make_state(True, r=r), Z.make_state(False, r=r)
    for it in range(4):
        Z.compare(on, off, Z.randn_grads(100 + it, dtype), f"r {r} backward {it}")
        assert [Z.zr_count(p) for p in Z.plans(on)] == [0, 0]
        assert [Z.zr_count(p) for p in Z.plans(off)] == [0, 0]
    assert all(p.r == r for p in Z.plans(on))


# ---- g. a trailing step that cannot be carried --------------------------------------------------
SMALL_BUCKET = [[64, 16], [300], [40, 27]]


@pytest.mark.parametrize("r", [3, 4])
def test_trailing_step_at_other_ranks(r):
    """A small bucket of single-block selects followed by RANK_LARGE, select streams off, three
    backwards.  The hook records the small bucket as a trailing step at every rank
    (arctopk_exchange_trail does not look at r: trail_calls is positive at r = 3 as at r = 4); the
    next bucket's native step carries it in its own launches only when r = 4 and otherwise enqueues
    it on its own (trail_run).  Either way the bits are those of a run without trailing steps
    (trail_bytes = 0), and the oracle's given the rows."""
    layouts = [SMALL_BUCKET, RANK_LARGE]
    assert bucket_numel(SMALL_BUCKET) * 4 < 2 << 20
    trail, rows, st_t = _two_bucket_run(r, layouts, 900, select_streams="off")
    plain, rows_p, st_p = _two_bucket_run(r, layouts, 900, select_streams="off", trail_bytes=0)
    print(f"r {r}: trail_calls {st_t.trail_calls} (trailing steps on), {st_p.trail_calls} (off)")
    assert st_t.trail_calls > 0 and st_p.trail_calls == 0
    ost = A.OracleState(r=r, compress_ratio=0.2, start_compress_iter=0, use_error_feedback="ef14", seed=21)
    E = [None, None]
    for it in range(3):
        for b, sh in enumerate(layouts):
            Z.same_bits(trail[it][b], plain[it][b], f"r {r} backward {it} bucket {b} output")
            assert all(torch.equal(x, y) for x, y in zip(rows[it][b], rows_p[it][b]))
            res = A.simulate_step([_rand(sh, 900 + 10 * it + b)], [E[b]], None, sh, 0.2, r, "ef14", ost.next_seed(),
                                  rows_override=rows[it][b], proj_device=DEV)
            for r_, nrm, s in zip(rows[it][b], res["norms"], res["segs"]):
                check_rows_tie_aware(r_, nrm, int(s.k_rows), band=2e-4)
            assert_bitwise(trail[it][b], res["out"], f"r {r} backward {it} bucket {b} vs the oracle")
            E[b] = res["E_new"][0]
    for b in range(2):
        Z.same_bits(st_t.error_dict[b], st_p.error_dict[b], f"r {r} bucket {b} E")
        assert_bitwise(st_t.error_dict[b], E[b], f"r {r} bucket {b} E vs the oracle")


# ---- h. fp32-residual encode at run-time rank ------------------------------------------------
def _mixed_encode(plan, mode, G, Ed, V):
    L = N.lib()
    if mode == "ef14":
        N.check(L.arctopk_encode_mixed(plan.handle, G.data_ptr(), Ed.data_ptr(), 1, V.data_ptr(),
                                       plan.sketch.data_ptr(), _stream()), "arctopk_encode_mixed")
    else:
        N.check(L.arctopk_encode_mixed21(plan.handle, G.data_ptr(), Ed.data_ptr(), V.data_ptr(),
                                         plan.sketch.data_ptr(), _stream()), "arctopk_encode_mixed21")


@pytest.mark.parametrize("mode", ["ef14", "ef21"])
@pytest.mark.parametrize("r", [1, 3, 5, 8])
def test_mixed_encode_pairing_exact(r, mode):
    """arctopk_encode_mixed (X = f(G) + E, E := X) and arctopk_encode_mixed21 (D = f(G) - E, E not
    written) on a bf16 RANK_MIX plan with the integer inputs of (b), E fp32: the sketch is the
    integer product rounded once to bf16, bit for bit.  r = 4 has an instantiation of its own; every
    other rank runs k_mx_encode<0> with the rank as an argument.  V is staged in LDS while
    m * r * 4 <= 65536: at r = 8 five tensors of RANK_MIX are beyond it; [3, 16388] is beyond it at
    every rank (16388 * 4 = 65552), so "no tile reads V from global memory at r = 1" is asserted on
    RANK_MIX without that tensor."""
    n_el = bucket_numel(RANK_MIX)
    Gi, Ei = integer_bucket(n_el), integer_residual(n_el)
    Xi = Gi + Ei if mode == "ef14" else Gi - Ei
    plan = BucketPlan(MIX_T, r, 0.2, BF16, DEV)
    Vi = [integer_projection(int(s.m), r) if s.kind == N.SEG_SKETCH else None for s in plan.segments]
    V = torch.cat([v.flatten() for v in Vi if v is not None]).to(BF16).to(DEV)
    Ed = Ei.float().to(DEV)
    plan.sketch.fill_(-7.0)
    _mixed_encode(plan, mode, Gi.to(BF16).to(DEV), Ed, V)
    torch.cuda.synchronize()
    sk = plan.sketch_view.cpu()
    for s, v in zip(plan.segments, Vi):
        x = Xi[s.offset:s.offset + s.n * s.m]
        if s.kind == N.SEG_RAW:
            want, got = x.float().to(BF16), sk[s.sketch_off:s.sketch_off + s.n]
        else:
            want = (x.view(s.n, s.m) @ v).float().to(BF16)
            got = sk[s.sketch_off:s.sketch_off + s.n * r].view(s.n, r)
        assert_bitwise(got, want, f"r {r} {mode}: sketch of [{s.n}, {s.m}] at offset {s.offset}")
    assert Ed.dtype == F32
    assert_bitwise(Ed, (Xi if mode == "ef14" else Ei).float(), "E := X (EF14) / E untouched (EF21)")
    t = plan.encode_tiles()
    beyond = [s for s in plan.segments if s.kind == N.SEG_SKETCH and s.m * r * 4 > 65536]
    assert len(beyond) == (5 if r == 8 else {1: 1, 3: 2, 5: 3}[r])
    assert t["mixed_vlds"] > 0 and t["mixed_vglobal"] >= len(beyond), t
    if r == 1:
        rest = BucketPlan([s for s in MIX_T if s != (3, 16388)], 1, 0.2, BF16, DEV)
        _mixed_encode(rest, mode, Gi.to(BF16).to(DEV), Ed, V)  # (buffers longer than this plan needs)
        torch.cuda.synchronize()
        t = rest.encode_tiles()
        assert t["mixed_vlds"] > 0 and t["mixed_vglobal"] == 0, t


@pytest.mark.parametrize("mode", ["ef14", "ef21"])
@pytest.mark.parametrize("r", [3, 8])
def test_mixed_hook_vs_restatement(r, mode):
    """The hook with error_dtype / ef21_error_dtype = fp32 on a bf16 RANK_MIX bucket against the
    restatements of tests/mixed_ef_oracle.py and tests/mixed_ef21_oracle.py at rank r, given the
    device's rows: outputs and fp32 residuals bit for bit (the bars of tests/test_gpu_mixed_ef.py
    and tests/test_gpu_mixed_ef21.py)."""
    st = GroupTopKState(None, r=r, compress_ratio=0.2, start_compress_iter=0, use_error_feedback=mode, seed=91)
    if mode == "ef14":
        st.error_dtype = F32
        o = MX.MixedOracle(1, RANK_MIX, 0.2, r=r, seed=91)
    else:
        st.ef21_error_dtype = F32
        o = M21.Mixed21Oracle(1, RANK_MIX, 0.2, r=r, seed=91)
    n = bucket_numel(RANK_MIX)
    compressed = 0
    for it in range(3):
        G = (torch.randn(n, generator=torch.Generator().manual_seed(500 + it)) * 3.0).to(BF16)
        out = group_topk_hook(st, SyntheticBucket(G.to(DEV), RANK_MIX, index=0, is_last=True)).wait()
        torch.cuda.synchronize()
        what = f"r {r} {mode} it{it}"
        if mode == "ef21" and it == 0:
            res = o.call([G])
            assert st.mixed_calls == 0
        else:
            plan = st._plans[0][1]
            assert plan.r == r
            res = o.call([G], _rows(plan), proj_device=DEV)
            compressed += 1
        assert out.dtype == BF16 and st.error_dict[0].dtype == F32
        assert_bitwise(out, res["out"], what + " out")
        assert_bitwise(st.error_dict[0], o.Es[0], what + " E")
        if mode == "ef21":
            assert st.global_error_dict[0].dtype == F32
            assert_bitwise(st.global_error_dict[0], o.gE, what + " gE")
        assert st.comm_bits_this_round == o.bits and st.iter == o.iter == it + 1
    assert st.mixed_calls == compressed == (3 if mode == "ef14" else 2)
    t = st._plans[0][1].encode_tiles()
    assert t["mixed_vlds"] > 0 and t["mixed_vglobal"] > 0, t
