"""Sketch ranks r = 1 .. 8 on the CPU: what the GPU tests of tests/test_gpu_sketch_rank.py rely on.

* which (dtype, r) the oracle's row energies (torch.sum over dim 1) are bit-identical to the
  kernels' sequential sum for, and how far the others are from it;
* the plan geometry per rank against the oracle's segments, and the column-split arithmetic of
  csrc/plan.hip restated;
* the refused ranks;
* a GroupTopKState(r=3) builds its plans and counts its bits with r = 3.
"""
import ctypes
import types

import pytest
import torch

from allreducetopk_amd import _native as N
from allreducetopk_amd.bucket import SyntheticBucket, bucket_numel
from allreducetopk_amd.comm_hooks import group_topk_hook_no_reshape as H
from oracle import arctopk as A
from sketch_rank import (N_SPLIT_F32, ORDER_DEPENDENT, RANK_MIX, energy_band, max_cols, sequential_energy)

RANKS = list(range(1, 9))


# ---- 1. energies ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("r", RANKS)
def test_oracle_energy_vs_sequential_sum(r, dtype):
    """torch's sum over dim 1 is the sequential ((q0 + q1) + q2) + ... for r <= 4 in both dtypes
    (bf16: fp32 accumulation of bf16 squares, one rounding) and for fp32 r = 8.  For fp32 r = 5, 6, 7
    it adds in another order: 34 to 45 % of rows differ in the last bits (largest relative difference
    measured 3.4e-7), by at most 2 (r - 1) 2^-24.  For bf16 r = 5 .. 8 the order differs too and
    shows only where the two fp32 sums round to different bf16 values: 6, 6, 0 and 1 of the
    2,021,007 rows below, one bf16 step apart.  Were a later torch to sum differently, this fails
    before a GPU energy test does."""
    differing, rows, worst = 0, 0, 0.0
    cases = []
    for n in (7, 1000, 20000):  # sketches as the oracle forms them
        segs = A.segments([[n, 40]], 0.2)
        G = torch.randn(n * 40, generator=torch.Generator().manual_seed(n + r)).to(dtype)
        _, Ps = A.encode(G, None, "noef", segs, A.draw_projections(5 + r, segs, r, dtype))
        cases.append((Ps, segs))
    segs = A.segments([[2_000_000, 40]], 0.2)  # ... and many rows, for the rare bf16 boundary
    cases.append(([(torch.randn(2_000_000, r, generator=torch.Generator().manual_seed(r)) * 2).to(dtype)], segs))
    for Ps, segs in cases:
        norms, _ = A.select(Ps, 1, segs)
        ref, seq = norms[0], sequential_energy(Ps[0])
        assert ref.dtype == seq.dtype == dtype and ref.shape == (segs[0].n,)
        if (dtype, r) not in ORDER_DEPENDENT:
            assert torch.equal(ref, seq), f"n {segs[0].n}: {int((ref != seq).sum())} rows differ"
            continue
        rel = (ref.double() - seq.double()).abs() / seq.double().clamp_min(1e-300)
        assert rel.max().item() <= energy_band(r, dtype), f"n {segs[0].n}: {rel.max().item():.3e}"
        worst = max(worst, rel.max().item())
        differing += int((ref != seq).sum())
        rows += segs[0].n
    if (dtype, r) in ORDER_DEPENDENT:
        print(f"{dtype} r {r}: {differing} of {rows} rows differ, largest relative difference {worst:.3e}")
    if dtype == torch.float32 and (dtype, r) in ORDER_DEPENDENT:
        assert differing > 0, "torch.sum has become sequential here: demand its bits in the GPU tests"


# ---- 2. geometry ---------------------------------------------------------------------------
def _describe(shapes, r, ratio=0.2):
    dims = [int(d) for s in shapes for d in s]
    nd = [len(s) for s in shapes]
    segs = (N.Segment * len(shapes))()
    info = N.PlanInfo()
    st = N.lib().arctopk_plan_describe((ctypes.c_int64 * len(dims))(*dims), (ctypes.c_int32 * len(nd))(*nd),
                                       len(nd), r, ratio, ctypes.cast(segs, ctypes.c_void_p), ctypes.byref(info))
    return st, list(segs), info


@pytest.mark.parametrize("r", RANKS)
def test_plan_geometry_per_rank(r):
    st, segs, info = _describe(RANK_MIX, r)
    assert st == 0
    ref = A.segments(RANK_MIX, 0.2)
    sk = vo = 0
    for s, o in zip(segs, ref):
        assert (s.offset, s.n, s.m, s.k_rows) == (o.offset, o.n, o.m, o.k_rows)
        assert s.kind == (N.SEG_SKETCH if o.kind == A.SKETCH else N.SEG_RAW)
        assert s.sketch_off == sk and s.v_off == (vo if o.kind == A.SKETCH else -1)
        sk += o.n * r if o.kind == A.SKETCH else o.n
        vo += o.m * r if o.kind == A.SKETCH else 0
    assert info.r == r and info.nseg == len(RANK_MIX) and info.numel == bucket_numel(RANK_MIX)
    assert info.sketch_len == sum(o.n * r for o in ref if o.kind == A.SKETCH) + sum(
        o.n for o in ref if o.kind == A.RAW)
    assert info.v_len == sum(o.m * r for o in ref if o.kind == A.SKETCH)
    assert info.values_len == sum(o.k for o in ref)


def test_column_split_arithmetic():
    """max_cols = (65536 / (4 r)) rounded down to whole 16-byte units, and what it means for RANK_MIX."""
    assert [max_cols(r, torch.float32) for r in RANKS] == [16384, 8192, 5460, 4096, 3276, 2728, 2340, 2048]
    assert [max_cols(r, torch.bfloat16) for r in RANKS] == [16384, 8192, 5456, 4096, 3272, 2728, 2336, 2048]
    ref = A.segments(RANK_MIX, 0.2)

    def wave_per_row(o, r):  # neither 1-D nor a thread-per-row LDS tile
        return o.kind == A.SKETCH and not (o.m < 64 and (256 * o.m + o.m * r) * 4 <= 65536)

    for dtype in (torch.float32, torch.bfloat16):
        for r in RANKS:
            split = [o for o in ref if wave_per_row(o, r) and o.m > max_cols(r, dtype)]
            assert len(split) == N_SPLIT_F32[r]  # (the same tensors in bf16)

    def parts(m, r):
        return -(-m // max_cols(r, torch.float32))

    assert [parts(5632, r) for r in RANKS] == [1, 1, 2, 2, 2, 3, 3, 3]
    assert [parts(4101, r) for r in RANKS] == [1, 1, 1, 2, 2, 2, 2, 3]
    assert [parts(2056, r) for r in RANKS] == [1] * 7 + [2] and [parts(16388, r) for r in RANKS][0] == 2
    # [300, 63]: an LDS tile up to r = 4 only; [300, 62]: at every rank
    assert [wave_per_row(A.segments([[300, 63]], 0.2)[0], r) for r in RANKS] == [False] * 4 + [True] * 4
    assert not any(wave_per_row(A.segments([[300, 62]], 0.2)[0], r) for r in RANKS)


@pytest.mark.parametrize("r", [0, 9, -1])
def test_other_ranks_are_refused(r):
    assert _describe(RANK_MIX, r)[0] == N.EINVAL
    dims, nd = (ctypes.c_int64 * 2)(8, 64), (ctypes.c_int32 * 1)(2)
    h = ctypes.c_void_p()
    for dt in (N.F32, N.BF16):  # (refused before the device is touched)
        assert N.lib().arctopk_plan_create(dims, nd, 1, r, 0.2, dt, 0, ctypes.byref(h)) == N.EINVAL
        assert h.value is None


def test_encode_tiles_accessor_checks_its_arguments():
    out = (ctypes.c_int64 * 9)()
    assert N.lib().arctopk_diag_encode_tiles(None, out, 9) == N.EINVAL


# ---- 3. the hook state ---------------------------------------------------------------------
SHAPES = [[8, 64], [16], [4, 2, 3, 3]]


def test_state_builds_plans_and_counts_bits_with_its_rank(monkeypatch):
    """GroupTopKState(r=3) on the host path (native calls stubbed, no trailing step): the plan it
    builds gets r = 3, and the bits one call sends are the oracle's for r = 3 (and not for r = 4)."""
    real, bits_of = N.lib(), H.BucketPlan.bits_of
    built = []

    class Lib:
        def arctopk_exchange_step(self, *a):
            return 0

        def arctopk_exchange_finish(self, *a):
            return 0

    class Plan:
        """What the hook touches of a BucketPlan; geometry from arctopk_plan_describe."""

        def __init__(self, shapes, r, ratio, dtype, device, flags=0):
            built.append((shapes, r, ratio))
            self.r, self.ratio, self.flags, self.handle = r, ratio, flags, object()
            dims = [int(d) for s in shapes for d in s]
            nd = [len(s) for s in shapes]
            segs = (N.Segment * len(shapes))()
            self.info = N.PlanInfo()
            assert real.arctopk_plan_describe((ctypes.c_int64 * len(dims))(*dims), (ctypes.c_int32 * len(nd))(*nd),
                                              len(nd), r, ratio, ctypes.cast(segs, ctypes.c_void_p),
                                              ctypes.byref(self.info)) == 0
            self.segments = list(segs)
            self.slotmap = torch.zeros(int(self.info.rows_total), dtype=torch.int32)
            self.rowlist = torch.zeros(int(self.info.sel_rows), dtype=torch.int32)
            self.sketch = torch.zeros(int(self.info.sketch_len), dtype=dtype)
            self.packed = torch.zeros(int(self.info.packed_len), dtype=dtype)
            self.V_ring = [torch.zeros(int(self.info.v_len), dtype=dtype)]
            self.bits_sum = bits_of(self.segments, r, dtype)
            self.philox_advance = 0
            self.comm_registered = None

    lib = Lib()
    monkeypatch.setattr(H, "_LIB", [lib])
    monkeypatch.setattr(N, "lib", lambda: lib)
    monkeypatch.setattr(H, "BucketPlan", Plan)
    monkeypatch.setattr(H, "_check_bucket_layout", lambda buf, grads: None)  # (wants a device tensor)
    monkeypatch.setattr(H, "_reseed_global", lambda *a, **k: None)
    monkeypatch.setattr(H, "_current_raw_stream", lambda dix: 0)
    monkeypatch.setattr(H, "_claim_projections", lambda *a, **k: False)
    monkeypatch.setattr(H, "_predraw_target", lambda *a, **k: (None, 0))
    st = H.GroupTopKState(types.SimpleNamespace(size=lambda: 1), r=3, compress_ratio=0.2, start_compress_iter=0,
                          use_error_feedback="ef14")
    st.select_streams, st.defer_decode, st.trail_bytes = "off", False, 0
    for _ in range(2):
        fut = H.group_topk_hook(st, SyntheticBucket(torch.ones(bucket_numel(SHAPES)), SHAPES, index=0))
        assert fut.done()
    assert st.r == 3 and len(built) == 1
    assert built[0] == ([tuple(s) for s in SHAPES], 3, 0.2)
    plan = st._plans[0][1]
    segs = A.segments(SHAPES, 0.2)
    assert plan.info.r == 3 and plan.info.sketch_len == 8 * 3 + 16 + 4 * 3 and plan.info.v_len == (64 + 18) * 3
    assert plan.bits_sum == A.bits_per_call(segs, 3, 32) != A.bits_per_call(segs, 4, 32)
    assert st.comm_bits_this_round == 0 and st.iter == 2  # world size 1: 2 (ws - 1) bits_sum
