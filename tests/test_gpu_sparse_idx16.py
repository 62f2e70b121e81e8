"""TopK's indices as 16-bit block offsets (``SparseState.index_wire = "idx16"``)
on the GPU: pack and unpack against the NumPy restatement of the format, the decode bit for bit
against oracle/sparse.py (fp32 values) and tests/sparse_wire16_oracle.py (bf16 values) fed the
original indices, and the hooks against the restatements of their configuration."""
import functools
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import sparse_idx16_format as F
import sparse_mixed_oracle as SM
import sparse_wire16_oracle as W
from allreducetopk_amd import _native as N
from allreducetopk_amd.bucket import SyntheticBucket, bucket_numel
from allreducetopk_amd.comm_hooks import sparse_hook as SH
from allreducetopk_amd.comm_hooks import sparse_hook_c4 as SH4
from oracle import sparse as S
from parity import ensure_group, rendezvous
from test_gpu_sparse_wire16 import HERE, MIX, MIX_2D, REPO, _grad, _same_bits, _stream

pytestmark = pytest.mark.gpu

DEV, BF16, F32, B = "cuda:0", torch.bfloat16, torch.float32, 65536
GUARD = 64


@pytest.fixture(scope="module", autouse=True)
def group():
    ensure_group("nccl")


@functools.lru_cache(None)
def _case(name):
    """(shapes, ks, per-tensor ascending int32 indices)."""
    hand = {"hand": ([[3 * B + 5]], [B - 1, B, 3 * B + 4]),  # a block edge, two empty blocks, one entry at each end
            "late": ([[2 * B + 10], [B + 1]], [B + 7, 2 * B + 3], [B])}  # no tensor's first index is in block 0
    if name in hand:
        shapes, *idxs = hand[name]
        return shapes, [len(i) for i in idxs], [torch.tensor(i, dtype=torch.int32) for i in idxs]
    shapes, ratio = {"edge": ([[B - 1], [B], [B + 1], [2 * B + 1]], 0.25), "full": ([[B + 1]], 1.0), "mix": (MIX, 0.25),
                     "many": ([[33]] * 70, 0.25), "one": ([[1]], 0.25),
                     # ARCTOPK_SPARSE_MAX_BATCH + 1 tensors, so two launches per entry; a tensor that crosses a block
                     # in the first batch, one that crosses a bitmap chunk alone in the second
                     "batches": ([[33]] * 63 + [[B + 1], [4097]], 0.25)}[name]
    X = _grad(bucket_numel(shapes), 5)
    return shapes, SM.layout_ks(shapes, ratio, "tensor"), SM.select(X, shapes, ratio, "tensor", False, "host", None)


def _guarded(t, shift=0):
    """t (CPU) on the device between sentinels, `shift` 4-byte steps off 16-B alignment: (buffer, view)."""
    shift *= 4 // t.element_size()
    buf = torch.full((t.numel() + 2 * GUARD,), 0xA5 if t.dtype == torch.uint8 else 1536, device=DEV, dtype=t.dtype)
    view = buf[GUARD + shift:GUARD + shift + t.numel()]
    view.copy_(t)
    return buf, view


def _intact(buf, view):
    lo = (view.data_ptr() - buf.data_ptr()) // buf.element_size()
    return bool((buf[:lo] == buf[0]).all() and (buf[lo + view.numel():] == buf[0]).all())


def _args(shapes, ks, first=0):
    """(numels, the entries' layout arguments); the tensors tile [first, first + sum(numels))."""
    numels = [S.numel_of(s) for s in shapes]
    offs, koff = ([base + sum(v[:i]) for i in range(len(v))] for base, v in ((first, numels), (0, ks)))
    return numels, (first + sum(numels), len(shapes), N.i64_array(offs), N.i64_array(ks), N.i64_array(koff))


def _bad_wire_args(sum_k, wire, nbytes):
    """What both readers refuse of the gathered payloads (`nbytes` each, a multiple of 16), one argument at a
    time: a misaligned wire, a stride that is no multiple of 4, a stride below the payload, no rank, more
    ranks than a grid's z takes, another packed_len."""
    return [dict(wire=wire + 2), dict(stride=nbytes + 2), dict(stride=nbytes - 4), dict(nranks=0), dict(nranks=65536),
            dict(packed_len=sum_k + 1)]


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("name", ["edge", "full", "hand", "late", "mix", "many", "one", "batches"])
def test_pack_then_unpack(name, shift):
    shapes, ks, idxs = _case(name)
    numels, lay = _args(shapes, ks)
    idx = torch.cat(idxs)
    want = torch.from_numpy(F.encode(numels, ks, idx.numpy()).copy())
    ibuf, idx_d = _guarded(idx, shift)
    stride = want.numel() + 16  # two payloads, a gap between them
    wbuf, wire_d = _guarded(torch.full((2 * stride,), 0x5A, dtype=torch.uint8), shift)
    for r in range(2):
        N.check(N.lib().arctopk_sparse_idx16_pack(*lay, idx_d.data_ptr(), wire_d.data_ptr() + r * stride, _stream()),
                "arctopk_sparse_idx16_pack")
    obuf, out_d = _guarded(torch.full((2 * sum(ks),), -7, dtype=torch.int32), shift)

    def unpack(lay=lay, packed_len=sum(ks), wire=wire_d.data_ptr(), stride=stride, nranks=2):
        return N.lib().arctopk_sparse_idx16_unpack(*lay, packed_len, wire, stride, nranks, out_d.data_ptr(), _stream())
    for bad in _bad_wire_args(sum(ks), wire_d.data_ptr(), want.numel()):
        assert unpack(**bad) == N.EINVAL, bad
    torch.cuda.synchronize()
    assert bool((out_d == -7).all())  # a refusal launches nothing
    N.check(unpack(), "arctopk_sparse_idx16_unpack")
    torch.cuda.synchronize()
    got = wire_d.cpu().view(2, stride)
    assert torch.equal(got[:, :want.numel()], want.expand(2, -1)) and bool((got[:, want.numel():] == 0x5A).all())
    assert torch.equal(out_d.cpu(), idx.repeat(2)) and torch.equal(idx_d.cpu(), idx)
    out_d.fill_(-7)
    N.check(unpack(lay=_args(shapes, ks, first=8)[1]), "arctopk_sparse_idx16_unpack")  # only a decode needs offsets[0] == 0
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
    """One arctopk_sparse_decode_idx16 between guards, the payloads `gap` bytes apart, behind the calls it has to
    refuse (which launch nothing): (out, gE) on the CPU."""
    numels, lay = _args(shapes, ks)
    n = sum(numels)
    obuf, out_d = _guarded(torch.full((n,), 5.0), shift)
    gbuf, gE_d = _guarded(gE0, shift) if gE0 is not None else (None, None)
    wbuf, wire_d = _guarded(torch.cat([torch.cat([w, torch.full((gap,), 0x5A, dtype=torch.uint8)]) for w in wires]))
    vbuf, vals_d = _guarded(torch.cat(vals))

    def decode(lay=lay, packed_len=sum(ks), wire=wire_d.data_ptr(), stride=wires[0].numel() + gap, nranks=nranks):
        return N.lib().arctopk_sparse_decode_idx16(out_d.data_ptr(), *lay, packed_len, wire, stride, vals_d.data_ptr(),
                                                   N.DTYPE_CODE[vals[0].dtype], nranks, len(wires), N.ptr(gE_d), decay,
                                                   _stream())
    refused = _bad_wire_args(sum(ks), wire_d.data_ptr(), wires[0].numel()) + [dict(lay=_args(shapes, ks, first=8)[1])]
    for bad in refused:
        assert decode(**bad) == N.EINVAL, bad
    torch.cuda.synchronize()
    assert bool((out_d == 5.0).all()) and (gE_d is None or torch.equal(gE_d.cpu(), gE0))
    N.check(decode(), "arctopk_sparse_decode_idx16")
    torch.cuda.synchronize()
    assert _intact(obuf, out_d) and _intact(wbuf, wire_d) and _intact(vbuf, vals_d)
    assert gE_d is None or _intact(gbuf, gE_d)
    return out_d.cpu(), None if gE_d is None else gE_d.cpu()


def _want(shapes, ks, all_idx, all_vals, ws, gE0, decay):
    n = bucket_numel(shapes)
    if all_vals[0].dtype == BF16:
        return W.decode(all_vals, all_idx, shapes, ws, n, gE0, decay)
    out = S.decode_topk(all_vals, [torch.cat(ix) for ix in all_idx], shapes, ks, ws, n)
    return (out, None) if gE0 is None else (SM.fma32(decay, out, gE0),) * 2


@pytest.mark.parametrize("decay", [None, 0.7])
@pytest.mark.parametrize("vdtype", [F32, BF16])
@pytest.mark.parametrize("nr", [1, 2, 3])
@pytest.mark.parametrize("name", ["edge", "hand", "mix", "batches"])
def test_decode_phase(name, nr, vdtype, decay):
    shapes, ks, all_idx, all_vals = _draws(name, nr)
    numels = [S.numel_of(s) for s in shapes]
    all_vals = [v.to(vdtype) for v in all_vals]
    wires = [torch.from_numpy(F.encode(numels, ks, torch.cat(ix).numpy()).copy()) for ix in all_idx]
    gE0 = None
    if decay is not None:
        gE0 = _grad(sum(numels), 9, 0.37)
        gE0[::5] = -0.0
    out, gE = _decode(shapes, ks, wires, all_vals, nr, gE0, decay or 1.0, shift=int(name == "mix"),
                      gap=16 * (name == "batches"))
    want_out, want_gE = _want(shapes, ks, all_idx, all_vals, nr, gE0, decay or 1.0)
    _same_bits(out, want_out, f"{name}/{nr}/{vdtype} out")
    if gE0 is not None:
        _same_bits(gE, want_gE, f"{name}/{nr}/{vdtype} gE")


@pytest.mark.parametrize("vdtype", [F32, BF16])
def test_a_remote_payload_that_holds_anything(vdtype):
    """Rank 1's table has an entry above ks and a descending pair, its lo16 descends too; its values are
    zeros, so rank 0's contributions must come out as without it, and nothing is written outside."""
    shapes, ks, (idxs,), (v0,) = _draws("hand", 1)
    numels, lay = _args(shapes, ks)
    good = F.encode(numels, ks, idxs[0].numpy())
    bad = good.copy()
    bad[:6] = np.array([9, 3, 65535], dtype="<u2").view(np.uint8)
    bad[16:32] = np.array([2, 1000, -5, 1], dtype="<i4").view(np.uint8)
    wires = [torch.from_numpy(w.copy()) for w in (good, bad)]
    vals = [v0.to(vdtype), torch.zeros(3, dtype=vdtype)]
    out, _ = _decode(shapes, ks, wires, vals, 2, None, 1.0)
    _same_bits(out, _want(shapes, ks, [idxs], vals[:1], 2, None, 1.0)[0], "out")
    wbuf, wire_d = _guarded(torch.cat(wires))
    obuf, out_d = _guarded(torch.full((6,), -7, dtype=torch.int32))
    N.check(N.lib().arctopk_sparse_idx16_unpack(*lay, 3, wire_d.data_ptr(), good.size, 2, out_d.data_ptr(), _stream()),
            "arctopk_sparse_idx16_unpack")
    torch.cuda.synchronize()
    assert torch.equal(out_d.cpu()[:3], idxs[0]) and _intact(obuf, out_d) and _intact(wbuf, wire_d)


@functools.lru_cache(None)
def _edge_payloads(nranks):
    """Four tensors at which chunk (4096) and block (65,536) edges exist, k about a quarter of each;
    every rank's ascending indices hold element 0, the last element and the elements either side of
    each edge, the rest drawn per rank: (shapes, ks, per rank the indices, per rank bf16 values)."""
    shapes, ks = [[5], [4095], [4097], [65537]], [2, 1024, 1024, 16384]
    g = torch.Generator().manual_seed(23)
    all_idx, all_vals = [], []
    for q in range(nranks):
        idxs = []
        for (n,), k in zip(shapes, ks):
            forced = torch.tensor([e for e in (0, 4095, 4096, 65535, 65536, n - 1) if e < n]).unique()
            free = torch.ones(n, dtype=torch.bool)
            free[forced] = False
            rest = free.nonzero().flatten()
            rest = rest[torch.randperm(rest.numel(), generator=g)[:k - forced.numel()]]
            idxs.append(torch.cat([forced, rest]).sort().values.to(torch.int32))
        v = torch.randn(sum(ks), generator=g) * 2.0 ** (8 - 8 * q)
        v[::9] = -0.0
        all_idx.append(idxs)
        all_vals.append(v.to(BF16))
    return shapes, ks, all_idx, all_vals


@pytest.mark.parametrize("nr", [1, 3])
@pytest.mark.parametrize("ge", ["none", "aligned", "shifted"])
@pytest.mark.parametrize("shift", [0, 1])
def test_the_two_chunk_decodes_agree(shift, ge, nr):
    """arctopk_sparse_decode_idx16 (bf16 values) and arctopk_sparse_decode_wire16 (accumulate 1) are the
    same chunk decode over two index formats: on the same selection `out` and `gE` agree bit for
    bit, with the bucket 16-B aligned or one element off and gE absent, aligned with `out`, or one
    element off it (every element then goes the scalar way)."""
    shapes, ks, all_idx, all_vals = _edge_payloads(nr)
    numels, lay = _args(shapes, ks)
    n, sum_k, stream = sum(numels), sum(ks), _stream()
    wires = [torch.from_numpy(F.encode(numels, ks, torch.cat(ix).numpy()).copy()) for ix in all_idx]
    wbuf, wire_d = _guarded(torch.cat(wires))
    ibuf, idx_d = _guarded(torch.cat([torch.cat(ix) for ix in all_idx]))
    vbuf, vals_d = _guarded(torch.cat(all_vals))
    gE0 = _grad(n, 9, 0.37)
    gE0[::5] = -0.0
    got = []
    for fmt in ("idx16", "int32"):
        obuf, out_d = _guarded(torch.full((n,), 5.0), shift)
        gbuf, gE_d = (None, None) if ge == "none" else _guarded(gE0, shift + (ge == "shifted"))
        if fmt == "idx16":
            rc = N.lib().arctopk_sparse_decode_idx16(out_d.data_ptr(), *lay, sum_k, wire_d.data_ptr(), wires[0].numel(),
                                                     vals_d.data_ptr(), N.BF16, nr, nr, N.ptr(gE_d), 0.7, stream)
        else:
            rc = N.lib().arctopk_sparse_decode_wire16(out_d.data_ptr(), *lay, sum_k, idx_d.data_ptr(), vals_d.data_ptr(),
                                                      nr, nr, 1, N.ptr(gE_d), 0.7, stream)
        N.check(rc, fmt)
        torch.cuda.synchronize()
        assert _intact(obuf, out_d) and (gE_d is None or _intact(gbuf, gE_d)), fmt
        got.append((out_d.cpu(), None if gE_d is None else gE_d.cpu()))
    assert _intact(wbuf, wire_d) and _intact(ibuf, idx_d) and _intact(vbuf, vals_d)
    _same_bits(got[0][0], got[1][0], "out")
    assert not torch.equal(got[0][0], torch.full((n,), 5.0))
    if ge != "none":
        _same_bits(got[0][1], got[1][1], "gE")
        _same_bits(got[0][1], got[0][0], "gE against out")


# ---- the hooks ---------------------------------------------------------------------------
CONFIGS = {"fp32": (F32, {}), "fp32_wire16": (F32, dict(wire_dtype=BF16)), "bf16": (BF16, {}),
           "bf16_err32": (BF16, dict(error_dtype=F32))}


def _state(ef, c4=False, index_wire="idx16", random=False, sparse_type="tensor", **options):
    kw = dict(compress_ratio=0.25, start_compress_iter=0, sparse_type=sparse_type, random=random,
              use_error_feedback=ef, random_seed=21, index_source="hash" if random else "host")
    st = SH4.SparseState(None, warmup_iters=4, **kw) if c4 else SH.SparseState(None, **kw)
    st.index_wire = index_wire
    for k, v in options.items():
        setattr(st, k, v)
    return st


def _call(st, G, shapes):
    hook = SH4.sparse_hook_sync if isinstance(st, SH4.SparseState) else SH.sparse_hook_sync
    out = hook(st, SyntheticBucket(G.to(DEV), shapes, index=0, is_last=True)).wait()
    torch.cuda.synchronize()
    return out


def _restatement(config, ef, c4, ws=1):
    """Gs -> (out, E per rank, gE) of one hook call in this configuration on the CPU."""
    kw = dict(c4=c4, warmup_iters=4)
    if config in ("fp32_wire16", "bf16_err32"):
        o = (W.SparseWire16Oracle if config == "fp32_wire16" else SM.SparseMixedOracle)(ws, MIX, 0.25, ef, **kw)
        return lambda Gs: (o.call(Gs)["out"], o.Es, o.gE)
    state = dict(Es=[None], gE=None, it=0)  # the bucket's own dtype throughout: oracle/sparse.py

    def call(Gs):
        ratio = S.gradual_ratio(0.25, state["it"], 0, 4) if c4 else 0.25
        state["it"] += 1
        if ef == "ef21" and state["gE"] is None:  # the dense first call
            state.update(Es=[Gs[0].clone()], gE=Gs[0].clone())
            return Gs[0], state["Es"], state["gE"]
        X = S.encode(Gs[0], state["Es"][0], ef)
        res = S.simulate_step(Gs, state["Es"], state["gE"], MIX, ratio, ef, False, None,
                              indices_override=[SM.select(X.float(), MIX, ratio, "tensor", False, "host", None)],
                              error_decay=1.0)
        state.update(Es=res["E_new"], gE=res["gE_new"])
        return res["out"], state["Es"], state["gE"]
    return call


@pytest.mark.parametrize("c4", [False, True])
@pytest.mark.parametrize("ef,config", [(ef, c) for ef in ("ef14", "ef21") for c in CONFIGS
                                       if (ef, c) != ("ef14", "bf16_err32")])
def test_hook_vs_restatement(ef, config, c4):
    dtype, options = CONFIGS[config]
    st, plain = _state(ef, c4, **options), _state(ef, c4, index_wire=None, **options)
    restated = _restatement(config, ef, c4)
    n = bucket_numel(MIX)
    for it in range(4 if ef == "ef21" else 3):  # EF21: the dense first call, then three compressed ones
        G = _grad(n, 400 + it, 10.0 ** (it - 1)).to(dtype)
        out, same = _call(st, G, MIX), _call(plain, G, MIX)
        want_out, want_E, want_gE = restated([G])
        what = f"{ef}/{config}/c4={c4} call {it}"
        for got, ref, want in ((out, same, want_out), (st.error_dict[0], plain.error_dict[0], want_E[0]),
                               (st.global_error_dict.get(0), plain.global_error_dict.get(0), want_gE)):
            if got is not None:
                _same_bits(got, want, what)
                _same_bits(got, ref, what + " against index_wire=None")
        if ef == "ef14" or it:  # a compressed call: the selection stays the int32 one
            assert st.last_indices.dtype == torch.int32 and torch.equal(st.last_indices, plain.last_indices), what
        assert st.comm_bits_this_round == 0
    assert st.idx16_calls == 3 and plain.idx16_calls == 0 and st.state_dict()["index_wire"] == "idx16"


def test_row_column_large_batch_and_randk():
    n = bucket_numel(MIX_2D)
    row, plain = _state("ef14", sparse_type="row"), _state("ef14", sparse_type="row", index_wire=None)
    randk, randk_plain = _state("ef14", random=True), _state("ef14", random=True, index_wire=None)
    for it in range(2):
        G = _grad(n, 500 + it)
        _same_bits(_call(row, G, MIX_2D), _call(plain, G, MIX_2D), "row out")
        _same_bits(row.error_dict[0], plain.error_dict[0], "row E")
        _same_bits(_call(randk, G, MIX_2D), _call(randk_plain, G, MIX_2D), "randk out")
    assert row.idx16_calls == 2 and randk.idx16_calls == 0
    with pytest.raises(ValueError, match="column"):
        _call(_state("ef14", sparse_type="column"), G, MIX_2D)
    st = _state("ef21")
    st.large_batch_init = True
    with pytest.raises(ValueError, match="large_batch_init"):
        _call(st, G, MIX_2D)


def _two_rank_worker(rank, ws, port):
    sys.path[:0] = [HERE, REPO]
    torch.set_num_threads(2)
    dist.init_process_group("gloo", init_method=port, rank=rank, world_size=ws)
    st = _state("ef14", wire_dtype=BF16)
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
        assert st.comm_bits_this_round == (it + 1) * 2 * (sum_k * 32 + 32 * F.blocks([S.numel_of(s) for s in MIX]))
    assert st.idx16_calls == 2
    dist.destroy_process_group()


def test_two_ranks_one_gpu():
    mp.spawn(_two_rank_worker, args=(2, rendezvous()), nprocs=2, join=True)
