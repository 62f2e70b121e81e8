"""fp32 residuals under a bf16 bucket for the TopK / RandK hooks (``SparseState.error_dtype``,
DESIGN.md section 4g): what can be checked without a GPU -- the arithmetic the option exists for,
the restatement's two consequences, the option's validation and the checkpoint rules."""
import pytest
import torch

import sparse_mixed_oracle as SM
from allreducetopk_amd import _native as N
from allreducetopk_amd.bucket import SyntheticBucket, bucket_numel
from allreducetopk_amd.comm_hooks import sparse_hook as SH
from allreducetopk_amd.comm_hooks import sparse_hook_c4 as SH4

BF16 = torch.bfloat16
MIX = [[5], [16, 64], [7], [100, 72], [3, 4099], [8, 4, 3, 3], [1], [130, 100]]


@pytest.fixture(autouse=True)
def _no_env(monkeypatch):
    monkeypatch.delenv("ARCTOPK_SPARSE_ERROR_DTYPE", raising=False)


def _state(cls=SH.SparseState, ef="ef14", **kw):
    return cls(None, compress_ratio=0.25, start_compress_iter=0, sparse_type="tensor", use_error_feedback=ef, **kw)


# ---- the arithmetic ----------------------------------------------------------------------
def test_stall_arithmetic():
    """An unselected element that receives 2^-3 every step: the bf16 residual stops at 2^8 * 2^-3
    (the next sum is a tie that rounds to even, back to 32), the fp32 fold carries all of it."""
    g = torch.tensor([2.0 ** -3], dtype=BF16)
    e16 = torch.zeros(1, dtype=BF16)
    e32 = None
    for _ in range(300):
        e16 = g + e16
        e32 = SM.fold14(g, e32)
    assert e16.item() == 32.0
    assert e32.item() == 37.5
    # a contribution below 2^-9 of a bf16 residual element is dropped whole
    assert (torch.tensor(1.0, dtype=BF16) + torch.tensor(2.0 ** -10, dtype=BF16)).item() == 1.0


def test_pack_remainder_is_exact():
    """X - f(b(X)) is representable in fp32: f(b(X)) + E_new == X on every selected element."""
    g = torch.Generator().manual_seed(3)
    X = torch.randn(1 << 16, generator=g) * torch.exp2(torch.randint(-30, 30, (1 << 16,), generator=g).float())
    vals, E = SM.pack14(X, [[X.numel()]], [torch.arange(X.numel(), dtype=torch.int32)])
    assert torch.equal((SM.f(vals).double() + E.double()), X.double())


def test_fma32_is_one_rounding():
    g = torch.Generator().manual_seed(4)
    m, e = torch.randn(4096, generator=g), torch.randn(4096, generator=g)
    assert torch.equal(SM.fma32(1.0, m, e), m + e)
    # 0.7f * m + e, exactly, rounded once (fractions)
    from fractions import Fraction
    import numpy as np
    d = float(np.float32(0.7))
    got = SM.fma32(0.7, m[:256], e[:256])
    for i in range(256):
        exact = Fraction(d) * Fraction(float(m[i])) + Fraction(float(e[i]))
        lo = float(np.nextafter(np.float32(got[i].item()), np.float32(-np.inf)))
        hi = float(np.nextafter(np.float32(got[i].item()), np.float32(np.inf)))
        r = Fraction(float(got[i]))
        assert abs(exact - r) <= abs(exact - Fraction(lo)) and abs(exact - r) <= abs(exact - Fraction(hi))
    # (1 + x)(1 - x + x^2) = 1 + x^3, x = 2^-12: the exact sum 2^20 + 2^-4 + 2^-40 loses its last term
    # to the 53-bit rounding and lands on an fp32 tie, which would round to even (down); one rounding
    # goes up
    m1 = torch.tensor([2.0 ** -4 * (1 - 2.0 ** -12 + 2.0 ** -24)])
    assert m1.double().item() == 2.0 ** -4 * (1 - 2.0 ** -12 + 2.0 ** -24)
    assert SM.fma32(1 + 2.0 ** -12, m1, torch.tensor([2.0 ** 20])).item() == 2.0 ** 20 + 2.0 ** -3


# ---- the restatement's consequences ------------------------------------------------------
@pytest.mark.parametrize("random,source", [(False, "host"), (True, "host"), (True, "hash")])
def test_ef14_conservation(random, source):
    """World size 1: f(out) + E_new == f(G) + E_old on every element, as fp32 numbers."""
    o = SM.SparseMixedOracle(1, MIX, 0.25, "ef14", random=random, index_source=source, seed=11)
    n = bucket_numel(MIX)
    for it in range(5):
        G = (torch.randn(n, generator=torch.Generator().manual_seed(100 + it)) * 10.0 ** (it - 2)).to(BF16)
        res = o.call([G])
        E_old = res["E_old"][0] if res["E_old"] is not None else torch.zeros(n)
        assert o.Es[0].dtype == torch.float32 and res["out"].dtype == BF16
        assert torch.equal(res["out"].float() + o.Es[0], G.float() + E_old), f"call {it}"


@pytest.mark.parametrize("random,source", [(False, "host"), (True, "host"), (True, "hash")])
def test_ef21_global_equals_local(random, source):
    """World size 1, decay 1: gE == E bit for bit after every call, and out == b(gE)."""
    o = SM.SparseMixedOracle(1, MIX, 0.25, "ef21", random=random, index_source=source, seed=12)
    n = bucket_numel(MIX)
    for it in range(6):  # the dense first call, then five compressed ones
        G = torch.randn(n, generator=torch.Generator().manual_seed(200 + it)).to(BF16)
        res = o.call([G])
        assert res["dense"] == (it == 0)
        assert torch.equal(o.gE.view(torch.int32), o.Es[0].view(torch.int32)), f"call {it}"
        assert torch.equal(res["out"], SM.b(o.gE))


def test_topk_ties_lowest_index_first():
    x = torch.tensor([1.0, -2.0, 2.0, 0.5, 2.0, -1.0, 1.0])
    assert SM.topk_indices(x, 2).tolist() == [1, 2]
    assert SM.topk_indices(x, 4).tolist() == [0, 1, 2, 4]


# ---- the option --------------------------------------------------------------------------
@pytest.mark.parametrize("cls", [SH.SparseState, SH4.SparseState])
def test_default_and_environment(cls, monkeypatch):
    st = _state(cls)
    assert st.error_dtype is None and st.mixed_calls == 0
    monkeypatch.setenv("ARCTOPK_SPARSE_ERROR_DTYPE", "fp32")
    assert _state(cls).error_dtype is torch.float32
    for bad in ("bf16", "float32", "1"):
        monkeypatch.setenv("ARCTOPK_SPARSE_ERROR_DTYPE", bad)
        with pytest.raises(ValueError, match="ARCTOPK_SPARSE_ERROR_DTYPE"):
            _state(cls)
    monkeypatch.setenv("ARCTOPK_SPARSE_ERROR_DTYPE", "")
    assert _state(cls).error_dtype is None


@pytest.mark.parametrize("bad", [torch.bfloat16, torch.float16, torch.float64, "fp32", True])
def test_other_values_raise(bad):
    st = _state()
    st.error_dtype = bad
    with pytest.raises(ValueError, match="error_dtype"):
        st._mixed_residual(BF16, N.EF14)


def test_where_the_option_applies():
    st = _state()
    assert not st._mixed_residual(BF16, N.EF14)  # unset
    st.error_dtype = torch.float32
    assert st._mixed_residual(BF16, N.EF14) and st._mixed_residual(BF16, N.EF21)
    assert not st._mixed_residual(torch.float32, N.EF14) and not st._mixed_residual(torch.float32, N.EF21)
    assert not st._mixed_residual(BF16, N.EF_NONE)


@pytest.mark.parametrize("cls,hook", [(SH.SparseState, SH.sparse_hook_sync), (SH4.SparseState, SH4.sparse_hook_sync)])
def test_large_batch_init_is_refused(cls, hook):
    st = _state(cls, ef="ef21")
    st.large_batch_init = True
    st.error_dtype = torch.float32
    with pytest.raises(ValueError, match="large_batch_init"):
        hook(st, SyntheticBucket.zeros([[4, 8]], dtype=BF16))
    assert not st.error_dict and st.iter == 0


# ---- checkpoints -------------------------------------------------------------------------
def _with_residuals(st, dtype, ef):
    g = torch.Generator().manual_seed(7)
    st.error_dict[0] = torch.randn(40, generator=g).to(dtype)
    if ef == "ef21":
        st.global_error_dict[0] = torch.randn(40, generator=g).to(dtype)
    if dtype == torch.float32:
        st._mixed_buckets.add(0)
    return st


@pytest.mark.parametrize("cls", [SH.SparseState, SH4.SparseState])
@pytest.mark.parametrize("ef", ["ef14", "ef21"])
def test_checkpoint_rules(cls, ef, tmp_path):
    st = _state(cls, ef=ef, random=True, random_seed=3)
    st.error_dtype = torch.float32
    _with_residuals(st, torch.float32, ef)
    torch.save(st.state_dict(), tmp_path / "ck.pt")
    sd = torch.load(tmp_path / "ck.pt", weights_only=True)
    assert sd["error_dtype"] == "fp32" and sd["mixed_buckets"] == [0]
    # into a state with the option: fp32 tensors, bit for bit
    st2 = _state(cls, ef=ef, random=True, random_seed=99)
    st2.error_dtype = torch.float32
    st2.load_state_dict(sd)
    for name in ("error_dict", "global_error_dict")[:2 if ef == "ef21" else 1]:
        a, b_ = getattr(st2, name)[0], getattr(st, name)[0]
        assert a.dtype == torch.float32 and torch.equal(a, b_) and a.data_ptr() != b_.data_ptr()
    assert st2._mixed_buckets == {0} and torch.equal(st2.rng.get_state(), st.rng.get_state())
    # into a state without it: refused, nothing loaded
    st3 = _state(cls, ef=ef)
    with pytest.raises(ValueError, match="error_dtype"):
        st3.load_state_dict(sd)
    assert not st3.error_dict and not st3.global_error_dict
    # bf16 residuals into a state with the option: widened, exactly
    old = _with_residuals(_state(cls, ef=ef), BF16, ef)
    sd_old = old.state_dict()
    assert sd_old["error_dtype"] is None and sd_old["mixed_buckets"] == []
    st4 = _state(cls, ef=ef)
    st4.error_dtype = torch.float32
    st4.load_state_dict(sd_old)
    assert st4.error_dict[0].dtype == torch.float32 and torch.equal(st4.error_dict[0].to(BF16), old.error_dict[0])
    if ef == "ef21":
        assert st4.global_error_dict[0].dtype == torch.float32
        assert torch.equal(st4.global_error_dict[0].to(BF16), old.global_error_dict[0])
    assert st4.state_dict()["mixed_buckets"] == [0]
    # ... and into one without it: bf16 as ever
    st5 = _state(cls, ef=ef)
    st5.load_state_dict(sd_old)
    assert st5.error_dict[0].dtype == BF16 and st5._mixed_buckets == set()
