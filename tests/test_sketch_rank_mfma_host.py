"""Sketch ranks 16 and 32 on the CPU: the ranks a plan accepts, the geometry at the new ones, and the
refusal of the fp32-residual options there."""
import ctypes

import pytest
import torch

from allreducetopk_amd import _native as N
from allreducetopk_amd.comm_hooks.group_topk_hook_no_reshape import GroupTopKState
from oracle import arctopk as A
from test_sketch_rank_host import _describe

MFMA_MIX = [[10], [40, 16], [4, 3, 3, 3], [300, 63], [33, 130], [5], [130, 2048], [6, 2049], [3, 16388]]


@pytest.mark.parametrize("r", [9, 12, 15, 17, 24, 31, 33, 64])
def test_ranks_between_and_beyond_are_refused(r):
    assert _describe(MFMA_MIX, r)[0] == N.EINVAL
    dims, nd, h = (ctypes.c_int64 * 2)(8, 64), (ctypes.c_int32 * 1)(2), ctypes.c_void_p()
    for dt in (N.F32, N.BF16):  # (refused before the device is touched)
        assert N.lib().arctopk_plan_create(dims, nd, 1, r, 0.2, dt, 0, ctypes.byref(h)) == N.EINVAL
        assert h.value is None


@pytest.mark.parametrize("r", [16, 32])
def test_plan_geometry(r):
    st, segs, info = _describe(MFMA_MIX, r)
    ref = A.segments(MFMA_MIX, 0.2)
    assert st == 0 and info.r == r
    assert [(s.offset, s.n, s.m, s.k_rows) for s in segs] == [(o.offset, o.n, o.m, o.k_rows) for o in ref]
    assert info.sketch_len == sum(o.n * r if o.kind == A.SKETCH else o.n for o in ref)
    assert info.v_len == sum(o.m * r for o in ref if o.kind == A.SKETCH)


@pytest.mark.parametrize("option,ef", [("error_dtype", "ef14"), ("ef21_error_dtype", "ef21")])
def test_fp32_residual_options_are_refused(option, ef):
    st = GroupTopKState(None, r=16, compress_ratio=0.2, start_compress_iter=0, use_error_feedback=ef, seed=1)
    setattr(st, option, torch.float32)
    decide = st._mixed_residual if ef == "ef14" else st._mixed21_residual
    with pytest.raises(ValueError, match="error_dtype.*ef21_error_dtype"):
        decide(torch.bfloat16, N.EF_CODE[ef])
