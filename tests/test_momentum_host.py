"""Momentum fold, host side (no GPU): arctopk_momentum_fold's argument checks, which run
before any device call, and HookState.accumulate_momentum_on_bucket's torch path -- a CPU
bucket gives exactly the two torch ops of the reference (comm_hooks/utils.py:54-65) -- its
KeyError, and the key the per-bucket cache of the native path is compared by."""
import ctypes
import os

import pytest
import torch

from allreducetopk_amd import _native as N
from allreducetopk_amd.bucket import SyntheticBucket
from allreducetopk_amd.build import LIB, build
from allreducetopk_amd.comm_hooks.utils import HookState


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        build()
    return N.lib()


FAKE = 0x10000  # never dereferenced: every call below is refused (or has nothing to do) on the host


def _fold(lib, bucket=FAKE, nt=1, offsets=(0,), numels=(8,), moments=(FAKE,), dtype=N.F32, mom=N.F32):
    offs = N.i64_array(offsets) if offsets is not None else None
    nums = N.i64_array(numels) if numels is not None else None
    moms = (ctypes.c_void_p * max(1, len(moments)))(*moments) if moments is not None else None
    return lib.arctopk_momentum_fold(bucket, nt, offs, nums, moms, 0.1, 0.9, dtype, mom, None)


def test_null_arguments_are_einval(lib):
    assert _fold(lib, bucket=None) == N.EINVAL
    assert _fold(lib, offsets=None) == N.EINVAL
    assert _fold(lib, numels=None) == N.EINVAL
    assert _fold(lib, moments=None) == N.EINVAL


def test_bad_counts_and_ranges_are_einval(lib):
    assert _fold(lib, nt=-1) == N.EINVAL
    assert _fold(lib, offsets=(-1,)) == N.EINVAL
    assert _fold(lib, numels=(-1,)) == N.EINVAL
    assert _fold(lib, nt=2, offsets=(0, 8), numels=(8, 4), moments=(FAKE, None)) == N.EINVAL


def test_misaligned_moment_is_einval(lib):
    assert _fold(lib, moments=(FAKE + 2,)) == N.EINVAL              # fp32 moment at 2 mod 4
    assert _fold(lib, moments=(FAKE + 1,), dtype=N.BF16, mom=N.BF16) == N.EINVAL
    assert _fold(lib, moments=(FAKE + 2,), dtype=N.BF16, mom=N.F32) == N.EINVAL


def test_unsupported_dtype_pairs_are_edtype(lib):
    assert _fold(lib, dtype=N.F32, mom=N.BF16) == N.EDTYPE
    assert _fold(lib, dtype=2, mom=N.F32) == N.EDTYPE
    assert _fold(lib, dtype=N.BF16, mom=7) == N.EDTYPE
    assert _fold(lib, dtype=-1, mom=-1) == N.EDTYPE


def test_nothing_to_do_returns_zero(lib):
    assert _fold(lib, nt=0, offsets=(0,), numels=(0,), moments=(None,)) == 0
    # tensors of numel 0 are skipped, null moment and all
    assert _fold(lib, nt=2, offsets=(0, 0), numels=(0, 0), moments=(None, None)) == 0
    for dtype, mom in ((N.F32, N.F32), (N.BF16, N.BF16), (N.BF16, N.F32)):
        assert _fold(lib, nt=0, dtype=dtype, mom=mom) == 0


SHAPES = [(5, 3), (7,), (2, 2, 2), (1,)]


def _state_and_bucket(dtype=torch.float32, beta=0.9, seed=0):
    g = torch.Generator().manual_seed(seed)
    n = sum(torch.Size(s).numel() for s in SHAPES)
    params = [torch.nn.Parameter(torch.zeros(s)) for s in SHAPES]
    bucket = SyntheticBucket(torch.randn(n, generator=g).to(dtype), SHAPES, parameters=params)
    st = HookState(None)
    st.init_momentum_field({p: {"exp_avg": torch.randn(s, generator=g).to(dtype)}
                            for p, s in zip(params, SHAPES)}, beta)
    return st, bucket, params


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float64])
@pytest.mark.parametrize("beta", [0.9, 0.999, 0.0])
def test_cpu_bucket_is_the_two_torch_ops(dtype, beta):
    st, bucket, params = _state_and_bucket(dtype, beta)
    want = [g.clone().mul_(1 - beta).add_(st.param_state[p]["exp_avg"], alpha=beta)
            for p, g in zip(params, bucket.gradients())]
    moments = [st.param_state[p]["exp_avg"].clone() for p in params]
    st.accumulate_momentum_on_bucket(bucket)
    assert st.momentum_native_calls == 0
    ibits = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float64: torch.int64}[dtype]
    for w, g in zip(want, bucket.gradients()):
        assert torch.equal(w.view(ibits), g.view(ibits))
    for m, p in zip(moments, params):
        assert torch.equal(m, st.param_state[p]["exp_avg"])


def test_missing_exp_avg_raises_keyerror():
    st, bucket, params = _state_and_bucket()
    del st.param_state[params[2]]["exp_avg"]
    with pytest.raises(KeyError, match="exp_avg"):
        st.accumulate_momentum_on_bucket(bucket)
    del st.param_state[params[1]]
    with pytest.raises(KeyError):
        st.accumulate_momentum_on_bucket(bucket)


def test_errors_before_the_fold_are_unchanged():
    st = HookState(None)
    bucket = SyntheticBucket(torch.ones(4), [(4,)])
    with pytest.raises(RuntimeError, match="not enabled"):
        st.accumulate_momentum_on_bucket(bucket)
    st.compress_momentum = True
    with pytest.raises(RuntimeError, match="not initialized"):
        st.accumulate_momentum_on_bucket(bucket)


def test_env_switch_is_read_per_call(monkeypatch):
    st, bucket, params = _state_and_bucket()
    grads = bucket.gradients()
    moments = [st.param_state[p]["exp_avg"] for p in params]
    monkeypatch.setenv("ARCTOPK_MOMENTUM_NATIVE", "0")
    assert st._accumulate_momentum_native(bucket, grads, moments) is False
    monkeypatch.delenv("ARCTOPK_MOMENTUM_NATIVE")
    assert st._accumulate_momentum_native(bucket, grads, moments) is False  # a CPU bucket
    assert st.momentum_native_calls == 0


class _FakeDeviceBuffer:
    """A CPU tensor that says it is on the GPU: the cache key is pure host bookkeeping."""

    def __init__(self, t):
        self._t = t

    is_cuda = True

    def __getattr__(self, name):
        return getattr(self._t, name)


def test_cache_key_follows_the_moments():
    st, bucket, params = _state_and_bucket()
    bucket._buffer = _FakeDeviceBuffer(bucket.buffer())
    grads = bucket.gradients()

    def key():
        return st._momentum_fold_key(bucket, grads, [st.param_state[p]["exp_avg"] for p in params])
    k0 = key()
    assert k0 is not None and k0 == key()
    assert k0[:2] == (torch.float32, torch.float32)
    assert k0[2] == (0, 15, 22, 30) and k0[3] == (15, 7, 8, 1)
    # what optimizer.load_state_dict does: new moment tensors
    old = st.param_state[params[1]]["exp_avg"]
    st.param_state[params[1]]["exp_avg"] = old.clone()
    k1 = key()
    assert k1 is not None and k1 != k0 and k1[4][1] != k0[4][1]
    assert k1[:4] == k0[:4] and k1[4][0] == k0[4][0]
    # what the torch loop handles and the native fold does not: no key
    st.param_state[params[1]]["exp_avg"] = torch.zeros(1)             # broadcastable, other shape
    assert key() is None
    st.param_state[params[1]]["exp_avg"] = old.to(torch.float64)      # unsupported pair
    assert key() is None
    st.param_state[params[1]]["exp_avg"] = torch.zeros(7, 2)[:, 0]    # not contiguous
    assert key() is None
    st.param_state[params[1]]["exp_avg"] = old
    assert key() == k0
    grads[0] = grads[0].clone()                                        # not a view of the buffer
    assert key() is None
