"""TopK's indices as a per-tensor bitmap (``SparseState.index_wire = "bitmap"`` / ``"auto"``, DESIGN.md
section 4j) on the GPU, bit for bit: pack and unpack against the NumPy restatement of the format, the
decode against oracle/sparse.py (fp32 values) and tests/sparse_wire16_oracle.py (bf16 values) fed the
original indices, and the hooks against ``index_wire=None`` states fed the same gradients."""
import functools
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import sparse_bitmap_format as F
from allreducetopk_amd import _native as N
from allreducetopk_amd.bucket import bucket_numel
from parity import rendezvous
from test_gpu_sparse_idx16 import (BF16, CONFIGS, F32, HERE, MIX, MIX_2D, REPO, SM, S, _args, _bad_wire_args, _call, _grad,
                                   _guarded, _intact, _restatement, _same_bits, _state, _stream, _want,
                                   group)  # noqa: F401  (the module's process group fixture)

pytestmark = pytest.mark.gpu
C = 4096


@functools.lru_cache(None)
def _case(name):
    """(shapes, ks, per-tensor ascending int32 indices)."""
    hand = {"hand": ([[3 * C + 5]], [C - 1, C, 3 * C + 4]),  # a chunk edge, an empty chunk, one entry at each end
            "late": ([[2 * C + 10], [C + 1]], [C + 7, 2 * C + 3], [C])}  # no tensor's first index is in chunk 0
    if name in hand:
        shapes, *idxs = hand[name]
        return shapes, [len(i) for i in idxs], [torch.tensor(i, dtype=torch.int32) for i in idxs]
    shapes, ratio = {"edge": ([[31], [32], [33], [C - 1], [C], [C + 1], [2 * C + 1]], 0.25), "full": ([[C + 1]], 1.0),
                     "mix": (MIX, 0.25), "many": ([[33]] * 70, 0.25), "one": ([[1]], 0.25),
                     # ARCTOPK_SPARSE_MAX_BATCH + 1 tensors, so two launches per entry; a tensor that crosses an
                     # idx16 block in the first batch, one that crosses a chunk alone in the second
                     "batches": ([[33]] * 63 + [[65537], [C + 1]], 0.25)}[name]
    X = _grad(bucket_numel(shapes), 5)
    return shapes, SM.layout_ks(shapes, ratio, "tensor"), SM.select(X, shapes, ratio, "tensor", False, "host", None)


def _encode(shapes, ks, idxs):
    return torch.from_numpy(F.encode([S.numel_of(s) for s in shapes], ks, torch.cat(idxs).numpy()).copy())


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("name", ["edge", "full", "hand", "late", "mix", "many", "one", "batches"])
def test_pack_then_unpack(name, shift):
    shapes, ks, idxs = _case(name)
    _, lay = _args(shapes, ks)
    idx, want = torch.cat(idxs), _encode(shapes, ks, idxs)
    ibuf, idx_d = _guarded(idx, shift)
    stride = want.numel() + 16  # two payloads, a gap between them
    wbuf, wire_d = _guarded(torch.full((2 * stride,), 0x5A, dtype=torch.uint8), shift)
    for r in range(2):
        N.check(N.lib().arctopk_sparse_bitmap_pack(*lay, idx_d.data_ptr(), wire_d.data_ptr() + r * stride, _stream()),
                "arctopk_sparse_bitmap_pack")
    obuf, out_d = _guarded(torch.full((2 * sum(ks),), -7, dtype=torch.int32), shift)

    def unpack(lay=lay, packed_len=sum(ks), wire=wire_d.data_ptr(), stride=stride, nranks=2):
        return N.lib().arctopk_sparse_bitmap_unpack(*lay, packed_len, wire, stride, nranks, out_d.data_ptr(), _stream())
    for bad in _bad_wire_args(sum(ks), wire_d.data_ptr(), want.numel()):
        assert unpack(**bad) == N.EINVAL, bad
    torch.cuda.synchronize()
    assert bool((out_d == -7).all())  # a refusal launches nothing
    N.check(unpack(), "arctopk_sparse_bitmap_unpack")
    torch.cuda.synchronize()
    got = wire_d.cpu().view(2, stride)
    assert torch.equal(got[:, :want.numel()], want.expand(2, -1)) and bool((got[:, want.numel():] == 0x5A).all())
    assert torch.equal(out_d.cpu(), idx.repeat(2)) and torch.equal(idx_d.cpu(), idx)
    out_d.fill_(-7)
    N.check(unpack(lay=_args(shapes, ks, first=8)[1]), "arctopk_sparse_bitmap_unpack")  # only a decode needs offsets[0] == 0
    torch.cuda.synchronize()
    assert torch.equal(out_d.cpu(), idx.repeat(2))
    assert _intact(ibuf, idx_d) and _intact(wbuf, wire_d) and _intact(obuf, out_d)


def _draws(name, nranks):
    """Per rank one ascending draw per tensor (rank 0: the case's) and values of magnitudes 2^12, 1, 2^-12."""
    shapes, ks, idxs = _case(name)
    g = torch.Generator().manual_seed(11)
    all_idx, all_vals = [idxs], []
    for q in range(nranks):
        if q:
            all_idx.append([torch.randperm(S.numel_of(s), generator=g)[:k].sort().values.to(torch.int32)
                            for s, k in zip(shapes, ks)])
        v = torch.randn(sum(ks), generator=g) * 2.0 ** (12 - 12 * q)
        v[::9] = -0.0
        all_vals.append(v)
    return shapes, ks, all_idx, all_vals


def _decode(shapes, ks, wires, vals, nranks, gE0, decay, shift=0, gap=0):
    """One arctopk_sparse_decode_bitmap between guards, the payloads `gap` bytes apart, behind the calls it has to
    refuse (which launch nothing): (out, gE) on the CPU."""
    numels, lay = _args(shapes, ks)
    obuf, out_d = _guarded(torch.full((sum(numels),), 5.0), shift)
    gbuf, gE_d = _guarded(gE0, shift) if gE0 is not None else (None, None)
    wbuf, wire_d = _guarded(torch.cat([torch.cat([w, torch.full((gap,), 0x5A, dtype=torch.uint8)]) for w in wires]))
    vbuf, vals_d = _guarded(torch.cat(vals))

    def decode(lay=lay, packed_len=sum(ks), wire=wire_d.data_ptr(), stride=wires[0].numel() + gap, nranks=nranks):
        return N.lib().arctopk_sparse_decode_bitmap(out_d.data_ptr(), *lay, packed_len, wire, stride, vals_d.data_ptr(),
                                                    N.DTYPE_CODE[vals[0].dtype], nranks, len(wires), N.ptr(gE_d), decay,
                                                    _stream())
    refused = _bad_wire_args(sum(ks), wire_d.data_ptr(), wires[0].numel()) + [dict(lay=_args(shapes, ks, first=8)[1])]
    for bad in refused:
        assert decode(**bad) == N.EINVAL, bad
    torch.cuda.synchronize()
    assert bool((out_d == 5.0).all()) and (gE_d is None or torch.equal(gE_d.cpu(), gE0))
    N.check(decode(), "arctopk_sparse_decode_bitmap")
    torch.cuda.synchronize()
    assert _intact(obuf, out_d) and _intact(wbuf, wire_d) and _intact(vbuf, vals_d)
    assert gE_d is None or _intact(gbuf, gE_d)
    return out_d.cpu(), None if gE_d is None else gE_d.cpu()


@pytest.mark.parametrize("decay", [None, 0.7])
@pytest.mark.parametrize("vdtype", [F32, BF16])
@pytest.mark.parametrize("nr", [1, 2, 3])
@pytest.mark.parametrize("name", ["edge", "hand", "mix", "batches"])
def test_decode_phase(name, nr, vdtype, decay):
    shapes, ks, all_idx, all_vals = _draws(name, nr)
    all_vals = [v.to(vdtype) for v in all_vals]
    wires = [_encode(shapes, ks, ix) for ix in all_idx]
    gE0 = None
    if decay is not None:
        gE0 = _grad(bucket_numel(shapes), 9, 0.37)
        gE0[::5] = -0.0
    out, gE = _decode(shapes, ks, wires, all_vals, nr, gE0, decay or 1.0, shift=int(name == "mix"),
                      gap=16 * (name == "batches"))
    want_out, want_gE = _want(shapes, ks, all_idx, all_vals, nr, gE0, decay or 1.0)
    _same_bits(out, want_out, f"{name}/{nr}/{vdtype} out")
    if gE0 is not None:
        _same_bits(gE, want_gE, f"{name}/{nr}/{vdtype} gE")


@pytest.mark.parametrize("vdtype", [F32, BF16])
def test_a_remote_payload_that_holds_anything(vdtype):
    """Rank 1's words are all ones, bits beyond n included; its table has a negative entry, one above ks
    and a descending pair; its values are zeros.  So rank 0's contributions must come out as without it,
    and neither the decode nor the unpack writes outside its buffers."""
    shapes, ks, (idxs,), (v0,) = _draws("hand", 1)
    _, lay = _args(shapes, ks)
    good = _encode(shapes, ks, idxs)
    bad = torch.full_like(good, 0xFF)
    bad[-16:] = torch.from_numpy(np.array([-5, 1000, 2, 1], dtype="<i4").view(np.uint8).copy())
    vals = [v0.to(vdtype), torch.zeros(3, dtype=vdtype)]
    out, _ = _decode(shapes, ks, [good, bad], vals, 2, None, 1.0)
    _same_bits(out, _want(shapes, ks, [idxs], vals[:1], 2, None, 1.0)[0], "out")
    wbuf, wire_d = _guarded(torch.cat([good, bad]))
    obuf, out_d = _guarded(torch.full((6,), -7, dtype=torch.int32))
    N.check(N.lib().arctopk_sparse_bitmap_unpack(*lay, 3, wire_d.data_ptr(), good.numel(), 2, out_d.data_ptr(), _stream()),
            "arctopk_sparse_bitmap_unpack")
    torch.cuda.synchronize()
    assert torch.equal(out_d.cpu()[:3], idxs[0]) and _intact(obuf, out_d) and _intact(wbuf, wire_d)


def _vs_plain(st, plain, shapes, calls, dtype=F32, seed=400):
    n = bucket_numel(shapes)
    for it in range(calls):
        G = _grad(n, seed + it, 10.0 ** (it % 3 - 1)).to(dtype)
        _same_bits(_call(st, G, shapes), _call(plain, G, shapes), f"call {it} out")
        for got, ref in ((st.error_dict.get(0), plain.error_dict.get(0)),
                         (st.global_error_dict.get(0), plain.global_error_dict.get(0))):
            if got is not None:
                _same_bits(got, ref, f"call {it} residual")
        if hasattr(plain, "last_indices"):  # a compressed call: the selection stays the int32 one
            assert st.last_indices.dtype == torch.int32 and torch.equal(st.last_indices, plain.last_indices)
        assert st.comm_bits_this_round == 0
    return G


@pytest.mark.parametrize("index_wire", ["bitmap", "auto"])
@pytest.mark.parametrize("config", ["fp32", "fp32_wire16", "bf16"])
@pytest.mark.parametrize("ef", ["ef14", "ef21"])
def test_hook_vs_plain(ef, config, index_wire):
    dtype, options = CONFIGS[config]
    st, plain = _state(ef, index_wire=index_wire, **options), _state(ef, index_wire=None, **options)
    _vs_plain(st, plain, MIX, 4 if ef == "ef21" else 3, dtype)  # EF21: the dense first call, then three compressed
    assert st.bitmap_calls == 3 and st.idx16_calls == 0 and st.state_dict()["index_wire"] == index_wire


def test_c4_auto_crosses_over():
    """The ramp runs from 0.8 (bitmap) down to 0.02 (idx16)."""
    st, plain = _state("ef14", c4=True, index_wire="auto"), _state("ef14", c4=True, index_wire=None)
    for s in (st, plain):
        s.compress_ratio = s.base_compress_ratio = 0.02
    _vs_plain(st, plain, MIX, 6)
    assert st.bitmap_calls + st.idx16_calls == 6 and st.bitmap_calls > 0 and st.idx16_calls > 0


def test_row_column_large_batch_and_randk():
    kw = dict(index_wire="bitmap")
    row, randk = _state("ef14", sparse_type="row", **kw), _state("ef14", random=True, **kw)
    G = _vs_plain(row, _state("ef14", sparse_type="row", index_wire=None), MIX_2D, 2, seed=500)
    _vs_plain(randk, _state("ef14", random=True, index_wire=None), MIX_2D, 2, seed=500)
    assert (row.bitmap_calls, randk.bitmap_calls, row.idx16_calls) == (2, 0, 0)
    with pytest.raises(ValueError, match="column"):
        _call(_state("ef14", sparse_type="column", **kw), G, MIX_2D)
    st = _state("ef21", **kw)
    st.large_batch_init = True
    with pytest.raises(ValueError, match="large_batch_init"):
        _call(st, G, MIX_2D)


def _two_rank_worker(rank, ws, port):
    sys.path[:0] = [HERE, REPO]
    torch.set_num_threads(2)
    dist.init_process_group("gloo", init_method=port, rank=rank, world_size=ws)
    st = _state("ef14", index_wire="bitmap", wire_dtype=BF16)
    restated = _restatement("fp32_wire16", "ef14", False, ws)
    n = bucket_numel(MIX)
    sum_k = sum(SM.layout_ks(MIX, 0.25, "tensor"))
    for it in range(2):
        Gl = _grad(n, 1000 * it + rank)
        parts = [torch.empty(n) for _ in range(ws)]
        dist.all_gather(parts, Gl)
        out = _call(st, Gl, MIX)
        want_out, want_E, _ = restated(parts)
        _same_bits(out, want_out, f"call {it} rank {rank} out")
        _same_bits(st.error_dict[0], want_E[rank], f"call {it} rank {rank} E")
        assert st.comm_bits_this_round == (it + 1) * 2 * (sum_k * 16 + F.info_bits([S.numel_of(s) for s in MIX]))
    assert st.bitmap_calls == 2 and st.idx16_calls == 0
    dist.destroy_process_group()


def test_two_ranks_one_gpu():
    mp.spawn(_two_rank_worker, args=(2, rendezvous()), nprocs=2, join=True)
