"""bf16 values on the wire of an fp32 bucket for the TopK / RandK hooks (``SparseState.wire_dtype``,
DESIGN.md section 4h) on the GPU: the two wire entries of csrc/sparse_mixed.hip phase by phase (both
decode routes), the hooks at world size 1 and on two ranks, refusals and checkpoints -- everything
bit for bit against the restatement in tests/sparse_wire16_oracle.py."""
import os
import sys
import time

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import sparse_mixed_oracle as SM
import sparse_wire16_oracle as W
from allreducetopk_amd import _native as N
from allreducetopk_amd.bucket import SyntheticBucket, bucket_numel
from allreducetopk_amd.comm_hooks import sparse_hook as SH
from allreducetopk_amd.comm_hooks import sparse_hook_c4 as SH4
from oracle import sparse as S
from parity import assert_bitwise, ensure_group, rendezvous

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
DEV = "cuda:0"
BF16 = torch.bfloat16
F32 = torch.float32
# [5]: every later offset odd; [1]: k = n = 1; [3, 4099] and [130, 100]: 12,297 and 13,000 keys, just
# past the 12,288-key single-block select (and four chunks of the merged decode each)
MIX = [[5], [16, 64], [7], [100, 72], [3, 4099], [8, 4, 3, 3], [1], [130, 100]]
MIX_2D = [s for s in MIX if s != [1]]
EDGES = [[4095], [4096], [4097], [8193]]  # around the merged decode's 4096-element chunk
MANY = [[33]] * 70                         # past ARCTOPK_SPARSE_MAX_BATCH = 64 and the select's 48 items
TAIL = [[16, 64], [3]]                     # total % 8 == 3
SETS = {"mix": MIX, "edges": EDGES, "many": MANY, "tail": TAIL, "mix2d": MIX_2D}
GUARD = 64
SENTINEL = 1536.0  # exact in bf16, fp32 and int32


@pytest.fixture(scope="module", autouse=True)
def group():
    ensure_group("nccl")
    yield


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _guarded(t: torch.Tensor, shift: int = 0):
    """t (CPU) on the device inside a buffer of sentinels: (whole buffer, view).  shift = 0: the
    view is 16-B aligned; 1: aligned to its element only."""
    buf = torch.full((t.numel() + 2 * GUARD,), SENTINEL, device=DEV, dtype=t.dtype)
    view = buf[GUARD + shift:GUARD + shift + t.numel()]
    view.copy_(t)
    assert (view.data_ptr() % 16 == 0) == (shift == 0)
    return buf, view


def _intact(buf, view):
    lo = (view.data_ptr() - buf.data_ptr()) // buf.element_size()
    return bool((buf[:lo] == SENTINEL).all() and (buf[lo + view.numel():] == SENTINEL).all())


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.detach().cpu().contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


def _same_bits(got, want, what):
    assert_bitwise(_bits(got), _bits(want), what + " bits")


def _layout(shapes, ks):
    numels = [S.numel_of(s) for s in shapes]
    offs = [sum(numels[:i]) for i in range(len(numels))]
    koff = [sum(ks[:i]) for i in range(len(ks))]
    return numels, offs, koff


# ---- 1. pack -----------------------------------------------------------------------------
PACK_MODES = ["noef", "ef14_zeroed", "ef14_x", "ef21_d1", "ef21_d0.7"]


def _pack(v_d, E_d, n, shapes, idx_d, ks, ef, decay, vals_d):
    _, offs, koff = _layout(shapes, ks)
    N.check(N.lib().arctopk_sparse_pack_wire16(v_d.data_ptr(), N.ptr(E_d), n, len(shapes), N.i64_array(offs),
                                               N.i64_array(ks), N.i64_array(koff), idx_d.data_ptr(),
                                               vals_d.data_ptr(), ef, decay, _stream()), "arctopk_sparse_pack_wire16")
    torch.cuda.synchronize()


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("mode", PACK_MODES)
@pytest.mark.parametrize("name,ratio", [("mix", 0.25), ("tail", 0.25), ("many", 0.25), ("tail", 1.0)])
def test_pack_phase(name, ratio, mode, shift):
    shapes = SETS[name]
    n = bucket_numel(shapes)
    g = torch.Generator().manual_seed(2)
    X = torch.randn(n, generator=g) * 3.0
    E0 = torch.randn(n, generator=g) * 0.37
    ks = SM.layout_ks(shapes, ratio, "tensor")
    idxs = SM.select(X, shapes, ratio, "tensor", False, "host", None)
    pos = SM._flat(shapes, idxs)
    v = X[pos].clone()
    ef = {"noef": "noef", "ef14": "ef14", "ef21": "ef21"}[mode.split("_")[0]]
    decay = float(mode.split("_d")[1]) if ef == "ef21" else 1.0
    if mode == "ef14_zeroed":  # the select's last pass has zeroed E at the selection
        E_in = X.clone()
        E_in[pos] = 0.0
    elif mode == "ef14_x":  # a draw followed by the gather: X is still there
        E_in = X.clone()
    else:
        E_in = None if ef == "noef" else E0
    want_v, want_E = W.pack(v, E_in, shapes, idxs, ef, decay)
    vbuf, v_d = _guarded(v, shift)
    ibuf, idx_d = _guarded(torch.cat(idxs), shift)
    obuf, vals_d = _guarded(torch.full((sum(ks),), 3.0, dtype=BF16), shift)
    ebuf, E_d = _guarded(E_in, shift) if E_in is not None else (None, None)
    _pack(v_d, E_d, n, shapes, idx_d, ks, N.EF_CODE[ef], decay, vals_d)
    _same_bits(vals_d, want_v, "vals16")
    _same_bits(v_d, v, "values untouched")
    assert _intact(vbuf, v_d) and _intact(ibuf, idx_d) and _intact(obuf, vals_d)
    if ef != "noef":
        _same_bits(E_d, want_E, "E")
        assert _intact(ebuf, E_d)
    if ef == "ef14":  # both inputs give X with the remainder at the selection: nothing of X is lost
        sent = torch.zeros(n, dtype=torch.float64)
        sent[pos] = vals_d.cpu().double()
        assert torch.equal(sent + E_d.cpu().double(), X.double())


def test_pack_skips_an_index_outside_its_tensor():
    """An index outside tensor 1 -- negative, its numel, or far past it -- writes a zero value and
    nothing else, and tensor 0's entries are what they are without it."""
    shapes = [[8], [8]]
    X = torch.arange(1.0, 17.0) * 1.001
    idxs = [torch.tensor([2, 5, 7], dtype=torch.int32), torch.tensor([0, 8, -1, 2 ** 31 - 1], dtype=torch.int32)]
    v = torch.tensor([X[2], X[5], X[7], X[8], 55.5, 66.5, 77.5])
    for ef, E_in in (("ef14", X), ("ef21", X * 0.5), ("noef", None)):
        want_v, want_E = W.pack(v, E_in, shapes, idxs, ef, 0.7)
        assert want_v[4:].float().tolist() == [0.0, 0.0, 0.0]
        vbuf, v_d = _guarded(v)
        obuf, vals_d = _guarded(torch.full((7,), 3.0, dtype=BF16))
        ebuf, E_d = _guarded(E_in) if E_in is not None else (None, None)
        _pack(v_d, E_d, 16, shapes, torch.cat(idxs).to(DEV), [3, 4], N.EF_CODE[ef], 0.7, vals_d)
        _same_bits(vals_d, want_v, ef + " vals16")
        assert _intact(obuf, vals_d)
        if E_in is not None:
            _same_bits(E_d, want_E, ef + " E")
            assert torch.equal(E_d.cpu()[9:], E_in[9:]) and _intact(ebuf, E_d)


# ---- 2. decode ---------------------------------------------------------------------------
def _payloads(shapes, ratio, nranks, seed, how="random"):
    """Per rank (per-tensor ascending int32 indices, bf16 values); the ranks' magnitudes are 2^12, 1
    and 2^-12, so the fp32 sum of an element several ranks selected depends on the order."""
    g = torch.Generator().manual_seed(seed)
    numels = [S.numel_of(s) for s in shapes]
    ks = SM.layout_ks(shapes, ratio, "tensor")
    all_idx, all_vals = [], []
    perms = [torch.randperm(m, generator=g) for m in numels]
    for q in range(nranks):
        if how == "identical":
            ix = [p[:k] for p, k in zip(perms, ks)]
        elif how == "disjoint":  # (a tensor of fewer than nranks * k elements: the same ones)
            ix = [p[q * k:(q + 1) * k] if nranks * k <= p.numel() else p[:k] for p, k in zip(perms, ks)]
        else:
            ix = [torch.randperm(m, generator=g)[:k] for m, k in zip(numels, ks)]
        all_idx.append([i.sort().values.to(torch.int32) for i in ix])
        vals = (torch.randn(sum(ks), generator=g) * 2.0 ** (12 - 12 * q)).to(BF16)
        vals[::9] = -0.0  # a -0 alone at an element comes out as +0
        all_vals.append(vals)
    return ks, all_idx, all_vals


def _decode(shapes, ks, all_idx, all_vals, nranks, ws, accumulate, gE0, decay, shift=0):
    """One arctopk_sparse_decode_wire16 between guards: (out, gE) on the CPU."""
    n = bucket_numel(shapes)
    _, offs, koff = _layout(shapes, ks)
    obuf, out_d = _guarded(torch.full((n,), 5.0), shift)
    gbuf, gE_d = _guarded(gE0, shift) if gE0 is not None else (None, None)
    ibuf, idx_d = _guarded(torch.cat([torch.cat(ix) for ix in all_idx[:nranks]]))
    vbuf, vals_d = _guarded(torch.cat(all_vals[:nranks]))
    N.check(N.lib().arctopk_sparse_decode_wire16(out_d.data_ptr(), n, len(shapes), N.i64_array(offs), N.i64_array(ks),
                                                 N.i64_array(koff), sum(ks), idx_d.data_ptr(), vals_d.data_ptr(),
                                                 nranks, ws, accumulate, N.ptr(gE_d), decay, _stream()),
            "arctopk_sparse_decode_wire16")
    torch.cuda.synchronize()
    assert _intact(obuf, out_d) and _intact(ibuf, idx_d) and _intact(vbuf, vals_d)
    assert gE_d is None or _intact(gbuf, gE_d)
    return out_d.cpu(), None if gE_d is None else gE_d.cpu()


def _check_decode(shapes, ks, all_idx, all_vals, nr, gemode, shift, what):
    """TopK payloads through accumulate 1 (merged) and 3 (scattered), the first payload as RandK's
    all-reduced one through 2 (merged) and 0 (scattered), at world size nr, each against the
    restatement -- so the two routes agree with each other as well."""
    n = bucket_numel(shapes)
    gE0 = decay = None
    if gemode is not None:
        decay = gemode
        gE0 = torch.randn(n, generator=torch.Generator().manual_seed(9)) * 0.37
        gE0[::5] = -0.0  # a stored -0.0 becomes +0.0 where nothing is added, as fma(d, 0, gE) gives
    for acc in (1, 3, 2, 0):
        pr = nr if acc in (1, 3) else 1
        want_out, want_gE = W.decode(all_vals[:pr], all_idx[:pr], shapes, nr, n, gE0, decay or 1.0)
        out, gE = _decode(shapes, ks, all_idx, all_vals, pr, nr, acc, gE0, decay or 1.0, shift)
        _same_bits(out, want_out, f"{what} accumulate {acc} out")
        if gE0 is not None:
            _same_bits(gE, want_gE, f"{what} accumulate {acc} gE")


@pytest.mark.parametrize("gemode", [None, 1.0, 0.7])
@pytest.mark.parametrize("nr", [1, 2, 3])
@pytest.mark.parametrize("name,ratio", [("mix", 0.25), ("edges", 1.0), ("edges", 0.01), ("many", 0.25), ("tail", 0.25)])
def test_decode_phase(name, ratio, nr, gemode):
    shapes = SETS[name]
    ks, all_idx, all_vals = _payloads(shapes, ratio, nr, 3)
    if ratio == 1.0:  # every index is selected: 4095, 4096 and each tensor's last element too
        assert all(ix.tolist() == list(range(S.numel_of(s))) for ix, s in zip(all_idx[0], shapes))
    # element-aligned buffers where the total is odd enough to matter, 16-B aligned ones otherwise
    _check_decode(shapes, ks, all_idx, all_vals, nr, gemode, 1 if name in ("tail", "mix") else 0, f"{name}/{ratio}")


@pytest.mark.parametrize("gemode", [None, 0.7])
@pytest.mark.parametrize("how", ["identical", "disjoint"])
def test_decode_three_ranks_sum_in_rank_order(how, gemode):
    """Three ranks selecting the same elements (magnitudes 2^12, 1, 2^-12: another order of the fp32
    adds gives other bits) and three selecting disjoint ones."""
    ks, all_idx, all_vals = _payloads(MIX, 0.25, 3, 4, how)
    n = bucket_numel(MIX)
    in_order = W.sums(all_vals, all_idx, MIX, n)
    if how == "identical":
        assert all(torch.equal(torch.cat(all_idx[0]), torch.cat(ix)) for ix in all_idx[1:])
        assert not torch.equal(in_order, W.sums(all_vals, all_idx, MIX, n, order=(2, 1, 0))), "order-insensitive input"
    else:
        elements = torch.cat([SM._flat(MIX, ix) for ix in all_idx]).unique().numel()
        assert elements == sum(3 * k if 3 * k <= S.numel_of(s) else k for k, s in zip(ks, MIX))
    _check_decode(MIX, ks, all_idx, all_vals, 3, gemode, 0, how)


def test_decode_skips_an_index_outside_its_tensor():
    shapes = [[8], [8]]
    ks = [3, 4]
    idx = [[torch.tensor([-1, 2, 5], dtype=torch.int32), torch.tensor([0, 3, 8, 2 ** 31 - 1], dtype=torch.int32)]]
    vals = [torch.arange(1.0, 8.0).to(BF16)]
    want = torch.zeros(16)
    want[2], want[5], want[8], want[11] = 2.0, 3.0, 4.0, 5.0
    assert torch.equal(W.decode(vals, idx, shapes, 1, 16)[0], want)
    for acc in (0, 1, 2, 3):
        out, _ = _decode(shapes, ks, idx, vals, 1, 1, acc, None, 1.0)
        _same_bits(out, want, f"accumulate {acc}")


# ---- the hooks ---------------------------------------------------------------------------
def _state(kind, ef, source="host", sparse_type="tensor", c4=False, seed=21, option=True, ratio=0.25):
    kw = dict(compress_ratio=ratio, start_compress_iter=0, sparse_type=sparse_type, random=kind == "randk",
              use_error_feedback=ef, random_seed=seed, index_source=source)
    st = SH4.SparseState(None, warmup_iters=4, **kw) if c4 else SH.SparseState(None, **kw)
    if option:
        st.wire_dtype = BF16
    return st


def _hook(st):
    return SH4.sparse_hook_sync if isinstance(st, SH4.SparseState) else SH.sparse_hook_sync


def _call(st, G, shapes):
    out = _hook(st)(st, SyntheticBucket(G.to(DEV), shapes, index=0, is_last=True)).wait()
    torch.cuda.synchronize()
    return out


def _grad(n, seed, scale=1.0):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed)) * scale


# ---- 3. hooks at world size 1 ------------------------------------------------------------
HOOK_CASES = [(kind, source, ef, "mix", "tensor", c4)
              for c4 in (False, True) for ef in ("noef", "ef14", "ef21")
              for kind, source in (("topk", "host"), ("randk", "hash"), ("randk", "host"))]
HOOK_CASES += [(kind, source, ef, "mix2d", st, False)
               for st in ("row", "column") for ef in ("noef", "ef14", "ef21")
               for kind, source in (("topk", "host"), ("randk", "hash"), ("randk", "host"))]


@pytest.mark.parametrize("kind,source,ef,name,sparse_type,c4", HOOK_CASES)
def test_hook_vs_restatement(kind, source, ef, name, sparse_type, c4):
    shapes = SETS[name]
    st = _state(kind, ef, source, sparse_type, c4)
    plain = _state(kind, ef, source, sparse_type, c4, option=False)
    o = W.SparseWire16Oracle(1, shapes, 0.25, ef, random=kind == "randk", index_source=source,
                             sparse_type=sparse_type, seed=21, c4=c4, warmup_iters=4)
    n = bucket_numel(shapes)
    compressed = 0
    for it in range(4 if ef == "ef21" else 3):  # EF21: the dense first call, then three compressed ones
        G = _grad(n, 400 + it, 10.0 ** (it - 1))
        out = _call(st, G, shapes)
        res = o.call([G])
        what = f"{kind}/{source}/{ef}/{name}/{sparse_type}/c4={c4} call {it}"
        assert out.dtype == F32, what
        _same_bits(out, res["out"], what + " out")
        if ef != "noef":
            assert st.error_dict[0].dtype == F32
            _same_bits(st.error_dict[0], o.Es[0], what + " E")
        if ef == "ef21":
            _same_bits(st.global_error_dict[0], o.gE, what + " gE")
        assert st.comm_bits_this_round == o.bits == 0 and st.iter == o.iter, what
        assert st.wire16_calls == o.wire16_calls, what
        _call(plain, G, shapes)
        if not res["dense"]:
            assert torch.equal(st.last_indices.cpu(), torch.cat(res["indices"][0])), what + " indices"
            assert list(st.last_k) == res["ks"], what
            if compressed == 0:  # same inputs and residual: the default path selects the same indices
                assert torch.equal(plain.last_indices, st.last_indices), what + " default-path indices"
            compressed += 1
    assert st.wire16_calls == 3 and plain.wire16_calls == 0
    assert st.state_dict()["wire_dtype"] == "bf16" and plain.state_dict()["wire_dtype"] is None


# ---- 4. invariants through the hook ------------------------------------------------------
@pytest.mark.parametrize("kind,source", [("topk", "host"), ("randk", "hash")])
def test_ef14_conserves_through_the_hook(kind, source):
    """World size 1: out + E_new == fl(G + E_old) on every element, and out is bf16-representable."""
    st = _state(kind, "ef14", source)
    n = bucket_numel(MIX)
    for it in range(5):
        G = _grad(n, 700 + it, 10.0 ** (it - 2))
        E_old = st.error_dict[0].cpu().clone() if 0 in st.error_dict else torch.zeros(n)
        out = _call(st, G, MIX).cpu()
        assert torch.equal(out + st.error_dict[0].cpu(), G + E_old), f"call {it}"
        assert torch.equal(out.to(BF16).float(), out), f"call {it}: out is not bf16-representable"
    assert st.wire16_calls == 5


@pytest.mark.parametrize("kind,source", [("topk", "host"), ("randk", "hash")])
def test_ef21_global_residual_is_the_local_one(kind, source):
    """World size 1, decay 1: gE == E after every call."""
    st = _state(kind, "ef21", source)
    n = bucket_numel(MIX)
    for it in range(6):  # the dense call and five compressed ones
        out = _call(st, _grad(n, 800 + it, 10.0 ** (it - 2)), MIX)
        _same_bits(st.global_error_dict[0], st.error_dict[0], f"call {it} gE == E")
        _same_bits(out, st.global_error_dict[0], f"call {it} out == gE")
    assert st.wire16_calls == 5


# ---- 5. two ranks ------------------------------------------------------------------------
def _two_rank_worker(rank, ws, port, kind, source, ef, decay):
    sys.path.insert(0, REPO)
    sys.path.insert(0, HERE)
    torch.set_num_threads(2)
    dist.init_process_group("gloo", init_method=port, rank=rank, world_size=ws)
    st = _state(kind, ef, source, seed=77)
    st.error_decay = decay
    o = W.SparseWire16Oracle(ws, MIX, 0.25, ef, random=kind == "randk", index_source=source, seed=77, decay=decay)
    n = bucket_numel(MIX)
    for it in range(3 if ef == "ef21" else 2):  # EF21: the dense first call, then two compressed ones
        Gl = _grad(n, 1000 * it + rank)
        parts = [torch.empty(n) for _ in range(ws)]
        dist.all_gather(parts, Gl)
        out = _call(st, Gl, MIX)
        res = o.call(parts)
        what = f"{kind}/{ef} call {it} rank {rank}"
        _same_bits(out, res["out"], what + " out")
        outs = [torch.empty(n) for _ in range(ws)]
        dist.all_gather(outs, out.cpu())
        _same_bits(outs[0], outs[1], what + " both ranks' out")
        _same_bits(st.error_dict[0], o.Es[rank], what + " E")
        if ef == "ef21":
            _same_bits(st.global_error_dict[0], o.gE, what + " gE")
        if not res["dense"]:
            assert torch.equal(st.last_indices.cpu(), torch.cat(res["indices"][rank])), what + " indices"
        assert st.comm_bits_this_round == o.bits, what
    sum_k = sum(SM.layout_ks(MIX, 0.25, "tensor"))
    assert st.wire16_calls == 2 and o.bits == 2 * (2 * sum_k * 16 if kind == "randk" else 2 * sum_k * 48)
    dist.destroy_process_group()


@pytest.mark.parametrize("kind,source,ef,decay", [("topk", "host", "ef14", 1.0), ("topk", "host", "ef21", 0.7),
                                                  ("randk", "hash", "ef14", 1.0)])
def test_two_ranks_one_gpu(kind, source, ef, decay):
    ctx = mp.spawn(_two_rank_worker, args=(2, rendezvous(), kind, source, ef, decay), nprocs=2, join=False)
    deadline = time.monotonic() + 120.0
    try:  # join() returns once a rank has exited (raising its error) or the time is up
        while not ctx.join(timeout=max(0.1, deadline - time.monotonic())):
            assert time.monotonic() < deadline, "the two ranks did not finish in 120 s"
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.kill()


# ---- 6. refusals and ignores -------------------------------------------------------------
@pytest.mark.parametrize("kind,ef", [("topk", "ef14"), ("randk", "ef21")])
def test_bf16_bucket_ignores_the_option(kind, ef):
    n = bucket_numel(MIX)
    a, b = _state(kind, ef), _state(kind, ef, option=False)
    for it in range(3):
        G = _grad(n, 900 + it).to(BF16)
        _same_bits(_call(a, G, MIX), _call(b, G, MIX), f"call {it} out")
        _same_bits(a.error_dict[0], b.error_dict[0], f"call {it} E")
    assert a.wire16_calls == 0 and a.error_dict[0].dtype == BF16


def test_refusals():
    G = _grad(bucket_numel(TAIL), 1)
    st = _state("topk", "ef21")
    st.large_batch_init = True
    with pytest.raises(ValueError, match="large_batch_init"):
        _call(st, G, TAIL)
    st = _state("topk", "ef14")
    st.wire_dtype = torch.float16  # any other value: ValueError at the first compressed call
    with pytest.raises(ValueError, match="wire_dtype"):
        _call(st, G, TAIL)
    assert not st.error_dict and st.wire16_calls == 0
    # dense warm-up calls ignore the option
    st = _state("topk", "ef14")
    st.start_compress_iter = 1
    _same_bits(_call(st, G, TAIL), G, "dense warm-up out")
    assert st.wire16_calls == 0
    _call(st, G, TAIL)
    assert st.wire16_calls == 1


# ---- 7. checkpoints ----------------------------------------------------------------------
@pytest.mark.parametrize("kind,source,ef", [("topk", "host", "ef14"), ("randk", "hash", "ef21")])
def test_resume_from_checkpoint_is_bit_identical(kind, source, ef, tmp_path):
    n = bucket_numel(MIX)
    first = 1 if ef == "ef21" else 0  # EF21's dense call comes before the three compressed ones
    Gs = [_grad(n, 600 + it) for it in range(first + 3)]
    a = _state(kind, ef, source, seed=5)
    outs = []
    for it, G in enumerate(Gs):
        if it == first + 2:
            torch.save(a.state_dict(), tmp_path / "ck.pt")
        outs.append(_call(a, G, MIX).cpu())
    sd = torch.load(tmp_path / "ck.pt", weights_only=True)
    assert sd["wire_dtype"] == "bf16" and sd["error_dict"][0].dtype == F32
    b = _state(kind, ef, source, seed=999)
    b.load_state_dict(sd, device=DEV)
    _same_bits(_call(b, Gs[-1], MIX), outs[-1], "resumed call out")
    _same_bits(b.error_dict[0], a.error_dict[0], "E")
    if ef == "ef21":
        _same_bits(b.global_error_dict[0], a.global_error_dict[0], "gE")
    assert a.wire16_calls == 3 and b.wire16_calls == 1
