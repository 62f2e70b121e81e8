"""``SparseState.wire_dtype`` on the CPU: the restatement's identities (sparse_wire16_oracle), the bit
formulas, the option's parsing and the two C entries' refusals, which precede any device call.

(The kernels and the hooks on a GPU: tests/test_gpu_sparse_wire16.py.)"""
import ctypes
import os

import pytest
import torch

import sparse_mixed_oracle as SM
import sparse_wire16_oracle as W
from allreducetopk_amd import _native as N
from allreducetopk_amd.bucket import bucket_numel
from allreducetopk_amd.build import LIB, build
from allreducetopk_amd.comm_hooks import sparse_hook as SH
from allreducetopk_amd.comm_hooks import sparse_hook_c4 as SH4

MIX = [[5], [16, 64], [7], [100, 72], [3, 4099], [8, 4, 3, 3], [1], [130, 100]]
BF16 = torch.bfloat16


def _grad(n, seed, scale=1.0):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed)) * scale


# ---- 1. the restatement ------------------------------------------------------------------
@pytest.mark.parametrize("random,source", [(False, "host"), (True, "hash")])
def test_ef14_conserves_and_sends_bf16(random, source):
    """World size 1: out + E_new == fl(G + E_old) on every element, in fp32 and exactly so in
    float64 (the remainder is exact), and every out is bf16-representable."""
    o = W.SparseWire16Oracle(1, MIX, 0.25, "ef14", random=random, index_source=source, seed=3)
    n = bucket_numel(MIX)
    E_old = torch.zeros(n)
    for it in range(5):
        G = _grad(n, it, 10.0 ** (it - 2))
        out = o.call([G])["out"]
        X = G + E_old
        assert torch.equal(out + o.Es[0], X), f"call {it}"
        assert torch.equal(out.double() + o.Es[0].double(), X.double()), f"call {it}: an inexact remainder"
        assert torch.equal(out.to(BF16).float(), out), f"call {it}"
        assert (out != 0).any() and (o.Es[0] != X).any()  # something was sent, and something rounded
        E_old = o.Es[0].clone()


def test_noef_out_is_bf16_representable():
    o = W.SparseWire16Oracle(1, MIX, 0.25, "noef")
    G = _grad(bucket_numel(MIX), 7)
    res = o.call([G])
    out = res["out"]
    pos = SM._flat(MIX, res["indices"][0])
    assert torch.equal(out.to(BF16).float(), out) and o.Es is None and o.gE is None
    assert torch.equal(out[pos], G[pos].to(BF16).float()) and int((out != 0).sum()) <= pos.numel()


@pytest.mark.parametrize("random,source", [(False, "host"), (True, "hash")])
def test_ef21_global_residual_is_the_local_one(random, source):
    """World size 1, decay 1: gE == E after every call (the dense one and five compressed ones)."""
    o = W.SparseWire16Oracle(1, MIX, 0.25, "ef21", random=random, index_source=source, seed=3)
    n = bucket_numel(MIX)
    for it in range(6):
        res = o.call([_grad(n, 20 + it, 10.0 ** (it - 2))])
        assert res["dense"] == (it == 0)
        assert torch.equal(o.gE.view(torch.int32), o.Es[0].view(torch.int32)), f"call {it}"
        assert torch.equal(res["out"], o.gE)
    assert o.wire16_calls == 5


def test_pack_stores_the_remainder_whatever_E_holds_at_the_selection():
    n = bucket_numel(MIX)
    X = _grad(n, 40)
    idxs = SM.select(X, MIX, 0.25, "tensor", False, "host", None)
    pos = SM._flat(MIX, idxs)
    zeroed = X.clone()
    zeroed[pos] = 0.0
    a = W.pack(X[pos], X, MIX, idxs, "ef14")
    b = W.pack(X[pos], zeroed, MIX, idxs, "ef14")
    assert torch.equal(a[0].view(torch.int16), b[0].view(torch.int16)) and torch.equal(a[1], b[1])


def test_rank_order_of_the_sums_matters():
    """Magnitudes 2^12, 1 and 2^-12 at one element: the restatement adds in rank order from 0."""
    idx = [[torch.tensor([0], dtype=torch.int32)]] * 3
    vals = [torch.tensor([v]).to(BF16) for v in (4096.0, 2.0 ** -12, -4096.0)]
    assert W.sums(vals, idx, [[2]], 2)[0] == 0.0  # 4096 + 2^-12 rounds to 4096 in fp32
    assert W.sums(vals, idx, [[2]], 2, order=(0, 2, 1))[0] == 2.0 ** -12
    neg = W.decode([torch.tensor([-0.0]).to(BF16)], [[torch.tensor([1], dtype=torch.int32)]], [[2]], 3, 2)[0]
    assert neg.view(torch.int32).tolist() == [0, 0]  # 0.0f + -0 is +0


# ---- 2. bits -----------------------------------------------------------------------------
@pytest.mark.parametrize("ws", [1, 2, 4])
@pytest.mark.parametrize("random", [False, True])
def test_bit_formulas(random, ws):
    shapes = [[16, 64], [7], [33]]
    o = W.SparseWire16Oracle(ws, shapes, 0.25, "ef14", random=random, index_source="hash", seed=1)
    n = bucket_numel(shapes)
    sum_k = sum(SM.layout_ks(shapes, 0.25, "tensor"))
    assert sum_k == 256 + 1 + 8
    for it in range(2):
        o.call([_grad(n, 50 + 10 * it + q) for q in range(ws)])
    per_call = 2 * (ws - 1) * sum_k * 16 if random else (ws - 1) * ws * sum_k * (16 + 32)
    assert o.bits == 2 * per_call == 2 * W.comm_bits(sum_k, ws, random)
    # against the fp32 wire: RandK half, TopK three quarters
    fp32 = 2 * (ws - 1) * sum_k * 32 if random else (ws - 1) * ws * sum_k * (32 + 32)
    assert per_call * (2 if random else 4) == fp32 * (1 if random else 3)


# ---- 3. the option -----------------------------------------------------------------------
@pytest.mark.parametrize("cls", [SH.SparseState, SH4.SparseState])
def test_option_parsing(cls, monkeypatch):
    monkeypatch.delenv("ARCTOPK_SPARSE_WIRE_DTYPE", raising=False)
    st = cls(None)
    assert st.wire_dtype is None and st.wire16_calls == 0 and st.state_dict()["wire_dtype"] is None
    assert not st._wire16(torch.float32) and not st._wire16(BF16)
    st.wire_dtype = BF16
    assert st._wire16(torch.float32) and not st._wire16(BF16)  # a bf16 bucket's wire is bf16 already
    assert st.state_dict()["wire_dtype"] == "bf16"
    fresh = cls(None)
    fresh.load_state_dict(st.state_dict())  # recorded for information: loading sets nothing
    assert fresh.wire_dtype is None
    for bad in (torch.float16, torch.float32, "bf16"):
        st.wire_dtype = bad
        with pytest.raises(ValueError, match="wire_dtype"):
            st._wire16(torch.float32)
    monkeypatch.setenv("ARCTOPK_SPARSE_WIRE_DTYPE", "bf16")
    assert cls(None).wire_dtype is BF16
    monkeypatch.setenv("ARCTOPK_SPARSE_WIRE_DTYPE", "")
    assert cls(None).wire_dtype is None
    for bad in ("fp16", "BF16", "1"):
        monkeypatch.setenv("ARCTOPK_SPARSE_WIRE_DTYPE", bad)
        with pytest.raises(ValueError, match="ARCTOPK_SPARSE_WIRE_DTYPE"):
            cls(None)


# ---- 4. the C ABI ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def entries():
    if not os.path.exists(LIB):
        build()
    L = ctypes.CDLL(LIB)
    fns = []
    for name in ("arctopk_sparse_pack_wire16", "arctopk_sparse_decode_wire16"):
        fn = getattr(L, name)
        fn.restype, fn.argtypes = N._SIGS[name]
        fns.append(fn)
    return fns


def _host_buffers():
    """16-B aligned host arrays standing in for device buffers: no refused call reaches a device."""
    raw = (ctypes.c_char * (4096 + 16))()
    base = (ctypes.addressof(raw) + 15) & ~15
    return raw, base


def test_pack_refusals_precede_any_device_call(entries):
    pack, _ = entries
    raw, p = _host_buffers()
    a = N.i64_array
    good = dict(values=p, E=p + 1024, numel=16, nt=2, offsets=a([0, 8]), ks=a([3, 3]), k_off=a([0, 3]), idx=p + 2048,
                vals16=p + 3072, ef=N.EF14, decay=1.0, stream=None)

    def call(**kw):
        return pack(*{**good, **kw}.values())

    for name in ("values", "offsets", "ks", "k_off", "idx", "vals16", "E"):  # a null pointer
        assert call(**{name: None}) == N.EINVAL, name
    assert call(E=None, ef=N.EF21) == N.EINVAL
    assert call(nt=0) == N.EINVAL and call(nt=-1) == N.EINVAL
    assert call(numel=0) == N.EINVAL
    assert call(ks=a([3, 9])) == N.EINVAL  # k > extent
    assert call(ks=a([0, 3])) == N.EINVAL
    assert call(numel=12, offsets=a([0, 12])) == N.EINVAL  # an empty tensor
    assert call(offsets=a([8, 0])) == N.EINVAL  # not in order
    assert call(vals16=p + 3073) == N.EINVAL  # misaligned
    assert call(E=p + 1026) == N.EINVAL
    assert call(values=p + 2) == N.EINVAL
    assert call(ef=7) == N.EINVAL
    # a bad tensor in the second batch of 64 is found before the first batch is launched
    nt = 70
    ks = [1] * nt
    ks[69] = 9
    assert call(numel=2 * nt, nt=nt, offsets=a(range(0, 2 * nt, 2)), ks=a(ks), k_off=a(range(nt))) == N.EINVAL
    assert not any(raw.raw)


def test_decode_refusals_precede_any_device_call(entries):
    _, decode = entries
    raw, p = _host_buffers()
    a = N.i64_array
    good = dict(out=p, numel=16, nt=2, offsets=a([0, 8]), ks=a([3, 3]), k_off=a([0, 3]), packed_len=6, idx=p + 1024,
                vals16=p + 2048, nranks=1, world_size=1, accumulate=1, gE=p + 3072, decay=1.0, stream=None)

    def call(**kw):
        return decode(*{**good, **kw}.values())

    for name in ("out", "offsets", "ks", "k_off", "idx", "vals16"):  # a null pointer (gE may be one)
        assert call(**{name: None}) == N.EINVAL, name
    assert call(nt=0) == N.EINVAL and call(nt=-1) == N.EINVAL
    assert call(nranks=0) == N.EINVAL and call(world_size=0) == N.EINVAL
    for acc in (0, 1, 2, 3):
        assert call(accumulate=acc, ks=a([3, 9])) == N.EINVAL  # k > extent, on either route
    assert call(packed_len=5) == N.EINVAL
    assert call(vals16=p + 2049) == N.EINVAL  # misaligned
    assert call(gE=p + 3074) == N.EINVAL and call(out=p + 2) == N.EINVAL
    assert call(accumulate=-1) == N.EINVAL and call(accumulate=4) == N.EINVAL
    nt = 70
    ks = [1] * nt
    ks[69] = 9
    assert call(numel=2 * nt, nt=nt, offsets=a(range(0, 2 * nt, 2)), ks=a(ks), k_off=a(range(nt)),
                packed_len=nt + 8) == N.EINVAL
    assert not any(raw.raw)
