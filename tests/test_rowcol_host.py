"""Row- / column-wise selection without a GPU: the CPU restatement against the reference's own
selections, the k rules, and the argument checks of the native entries."""
import numpy as np
import pytest
import torch

import rowcol_oracle as RC
from allreducetopk_amd import _native as N
from allreducetopk_amd.comm_hooks import sparse_hook, sparse_hook_c4

RATIOS = [0.2, 0.01]


@pytest.fixture(scope="module")
def gold():
    return RC.golden_load()


@pytest.mark.parametrize("mode", ["row", "column"])
@pytest.mark.parametrize("ratio", RATIOS)
def test_helper_reproduces_reference_segments(gold, mode, ratio):
    want = RC.golden_positions(gold, mode, ratio)
    for i, shape in enumerate(gold["shapes"][mode]):
        x = RC.golden_input(gold, i, shape)
        _, _, _, _, k, _ = RC.geometry(shape, ratio, mode)
        got = RC.topk_positions(RC.segments(x, shape, mode), k)
        assert torch.equal(got, want[i]), f"{mode} {ratio} {shape}"
        # and through the layout and back
        idx = RC.layout(got, *RC.geometry(shape, ratio, mode)[:2], mode)
        assert torch.equal(RC.payload_positions(idx, shape, ratio, mode), want[i])


@pytest.mark.parametrize("mod", [sparse_hook, sparse_hook_c4])
@pytest.mark.parametrize("ratio", RATIOS)
def test_cal_k_by_row_and_column(gold, mod, ratio):
    for mode, fn in (("row", mod.cal_k_by_row), ("column", mod.cal_k_by_column)):
        ks = gold["z"][f"{mode}_r{ratio}_k"]
        for shape, k in zip(gold["shapes"][mode], ks):
            assert fn(torch.empty(shape), ratio) == int(k), f"{mode} {shape}"
            assert RC.geometry(shape, ratio, mode)[5] == int(k)


def test_unknown_sparse_type_still_raises():
    st = sparse_hook.SparseState(None, sparse_type="diagonal")
    with pytest.raises(ValueError):
        sparse_hook._check_compressible(st, torch.zeros(4))
    for ok in ("tensor", "row", "column"):  # accepted: the next check (a GPU bucket) is what fails
        st = sparse_hook.SparseState(None, sparse_type=ok)
        with pytest.raises(RuntimeError):
            sparse_hook._check_compressible(st, torch.zeros(4))


def _select(rows, cols, kseg, by_column=0, dtype=0, idx=1, hashed=1):
    a = N.i64_array
    return N.lib().arctopk_seg_select(None, 1, None, a([rows]), a([cols]), a([kseg]), a([0]), by_column, hashed,
                                      7, idx, None, 1, dtype, 0, None)


def test_seg_entries_reject_bad_arguments_without_a_gpu():
    """Validation comes before anything is enqueued (idx / workspace are never dereferenced)."""
    L = N.lib()
    a = N.i64_array
    assert L.arctopk_seg_workspace_bytes(1, a([4]), a([9]), a([3]), 0) > 0
    assert L.arctopk_seg_workspace_bytes(2, a([2, 300]), a([13000, 1025]), a([130, 10]), 0) > 100_000
    for by_column in (0, 1):
        seg_len = 4 if by_column else 9
        for kseg in (0, seg_len + 1):  # k_seg outside [1, segment length]
            assert L.arctopk_seg_workspace_bytes(1, a([4]), a([9]), a([kseg]), by_column) == -N.EINVAL
            assert _select(4, 9, kseg, by_column) == N.EINVAL
        assert L.arctopk_seg_workspace_bytes(1, a([4]), a([9]), a([seg_len]), by_column) > 0
    assert L.arctopk_seg_workspace_bytes(1, a([1 << 16]), a([1 << 15]), a([1]), 0) == -N.EINVAL  # 2^31 elements
    assert _select(1 << 16, 1 << 15, 1) == N.EINVAL
    assert L.arctopk_seg_workspace_bytes(1, a([0]), a([5]), a([1]), 0) == -N.EINVAL
    assert L.arctopk_seg_workspace_bytes(0, None, None, None, 0) == -N.EINVAL
    assert _select(4, 9, 3, dtype=7) == N.EINVAL      # bad dtype
    assert _select(4, 9, 3, idx=None) == N.EINVAL     # null idx
    assert _select(4, 9, 3, hashed=0) == N.EINVAL     # TopK needs x


def test_hseed_of_segment_zero_is_the_tensor_seed():
    from oracle import sparse as S
    for seed, t in ((0, 0), (123456789, 3), (999_999_999, 47)):
        assert RC.hseed(seed, t, 0) == S.randk_hash_seed(seed, t)
        assert RC.hseed(seed, t, 1) != RC.hseed(seed, t, 0)
    got = RC.hash_positions(1, 500, 100, 42, 2)[0]
    assert torch.equal(got.to(torch.int32), S.randk_hash_indices(500, 100, 42, 2))
