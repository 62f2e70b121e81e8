"""fp32 residuals under a bf16 bucket for the TopK / RandK hooks (``SparseState.error_dtype``,
DESIGN.md section 4g) on the GPU: the three kernels of csrc/sparse_mixed.hip phase by phase, the
hooks at world size 1 and on two ranks, the stall the option removes and checkpoints -- everything
bit for bit against the restatement in tests/sparse_mixed_oracle.py."""
import os
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import sparse_mixed_oracle as SM
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
# [5]: every later offset odd, so per-tensor gathers are misaligned; [1]: k = n = 1; [3, 4099] and
# [130, 100]: 12,297 and 13,000 keys, just past the 12,288-key single-block select
MIX = [[5], [16, 64], [7], [100, 72], [3, 4099], [8, 4, 3, 3], [1], [130, 100]]
MIX_2D = [s for s in MIX if s != [1]]
ALIGNED = [[32, 2048], [16, 64], [8, 24]]  # offsets and total multiples of 8
TAIL = [[16, 64], [3]]                     # total % 8 == 3
MANY = [[33]] * 70                         # past ARCTOPK_SPARSE_MAX_BATCH = 64 and the select's 48 items
SETS = {"mix": MIX, "aligned": ALIGNED, "tail": TAIL, "many": MANY, "mix2d": MIX_2D}
GUARD = 64
SENTINEL = 1536.0  # exact in bf16 and fp32


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


def _inputs(shapes, seed):
    g = torch.Generator().manual_seed(seed)
    n = bucket_numel(shapes)
    G = (torch.randn(n, generator=g) * 3.0).to(BF16)
    E0 = torch.randn(n, generator=g) * 0.37  # fp32: low bits set
    return G, E0, g


def _layout(shapes, ks):
    numels = [S.numel_of(s) for s in shapes]
    offs = [sum(numels[:i]) for i in range(len(numels))]
    koff = [sum(ks[:i]) for i in range(len(ks))]
    return numels, offs, koff


# ---- 1. phases ---------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("mode", ["ef14_first", "ef14", "ef21"])
@pytest.mark.parametrize("name", ["mix", "aligned", "tail"])
def test_fold_phase(name, mode, shift):
    G, E0, _ = _inputs(SETS[name], 1)
    n = G.numel()
    gbuf, Gd = _guarded(G, shift)
    ebuf, Ed = _guarded(E0, shift)
    dbuf, Dd = _guarded(torch.full((n,), 7.0), shift)
    ef = N.EF21 if mode == "ef21" else N.EF14
    N.check(N.lib().arctopk_sparse_fold_mixed(Gd.data_ptr(), Ed.data_ptr(), Dd.data_ptr() if ef == N.EF21 else None,
                                              n, ef, int(mode != "ef14_first"), _stream()),
            "arctopk_sparse_fold_mixed")
    torch.cuda.synchronize()
    assert_bitwise(Gd, G, "G untouched")
    if mode == "ef21":
        assert_bitwise(Dd, SM.fold21(G, E0), "D")
        assert_bitwise(Ed, E0, "E untouched")
    else:
        assert_bitwise(Ed, SM.fold14(G, None if mode == "ef14_first" else E0), "E")
        assert_bitwise(Dd, torch.full((n,), 7.0), "D untouched")
    assert _intact(gbuf, Gd) and _intact(ebuf, Ed) and _intact(dbuf, Dd)


def _pack(src_d, E_d, n, shapes, idxs, ks, ef, decay, vals_d):
    _, offs, koff = _layout(shapes, ks)
    idx_d = torch.cat(idxs).to(DEV)
    N.check(N.lib().arctopk_sparse_pack_mixed(src_d.data_ptr(), E_d.data_ptr(), n, len(shapes), N.i64_array(offs),
                                              N.i64_array(ks), N.i64_array(koff), idx_d.data_ptr(),
                                              vals_d.data_ptr(), ef, decay, _stream()), "arctopk_sparse_pack_mixed")
    torch.cuda.synchronize()


@pytest.mark.parametrize("case", ["ef14", "ef21_d1", "ef21_d0.7"])
@pytest.mark.parametrize("name,ratio", [("mix", 0.25), ("aligned", 0.25), ("tail", 0.25), ("tail", 1.0), ("many", 0.25)])
def test_pack_phase(name, ratio, case):
    shapes = SETS[name]
    G, E0, _ = _inputs(shapes, 2)
    n = G.numel()
    ks = SM.layout_ks(shapes, ratio, "tensor")
    if case == "ef14":
        src = SM.fold14(G, E0)
        idxs = SM.select(src, shapes, ratio, "tensor", False, "host", None)
        want_v, want_E = SM.pack14(src, shapes, idxs)
        ebuf, Ed = _guarded(src)
        src_d, ef, decay = Ed, N.EF14, 1.0
    else:
        decay = float(case.split("_d")[1])
        src = SM.fold21(G, E0)
        idxs = SM.select(src, shapes, ratio, "tensor", False, "host", None)
        want_v, want_E = SM.pack21(src, E0, shapes, idxs, decay)
        ebuf, Ed = _guarded(E0)
        sbuf, src_d = _guarded(src)
        ef = N.EF21
    vbuf, vals_d = _guarded(torch.full((sum(ks),), 3.0, dtype=BF16))
    _pack(src_d, Ed, n, shapes, idxs, ks, ef, decay, vals_d)
    assert_bitwise(vals_d, want_v, "values")
    assert_bitwise(Ed, want_E, "E")
    assert _intact(ebuf, Ed) and _intact(vbuf, vals_d)
    if ef == N.EF21:
        assert_bitwise(src_d, src, "D untouched")
        assert _intact(sbuf, src_d)
    if ratio == 1.0 and case == "ef14":  # k = n: every E is a remainder, f(vals) + E == X exactly
        assert torch.equal(vals_d.cpu().double() + Ed.cpu().double(), src.double())


def test_pack_checks_every_index_against_its_tensor():
    """An index outside its tensor -- negative, its numel, or one that would land in the next
    tensor -- writes a zero value and nothing else; a layout that does not fit is refused."""
    shapes = [[8], [8]]
    X = torch.arange(1.0, 17.0) * 1.001
    ebuf, Ed = _guarded(X)
    vbuf, vals_d = _guarded(torch.full((6,), 3.0, dtype=BF16))
    idxs = [torch.tensor([2, 8, -1], dtype=torch.int32), torch.tensor([0, 9, 2 ** 31 - 1], dtype=torch.int32)]
    _pack(Ed, Ed, 16, shapes, idxs, [3, 3], N.EF14, 1.0, vals_d)
    want_v, want_E = SM.pack14(X, shapes, [torch.tensor([2], dtype=torch.int32), torch.tensor([0], dtype=torch.int32)])
    want = torch.zeros(6, dtype=BF16)
    want[0], want[3] = want_v[0], want_v[1]
    assert_bitwise(vals_d, want, "values")
    assert_bitwise(Ed, want_E, "E")
    assert _intact(ebuf, Ed) and _intact(vbuf, vals_d)
    # refused with nothing enqueued: a k past its tensor, an empty tensor, EF14 with src != E
    L, a = N.lib(), N.i64_array
    idx_d = torch.zeros(6, dtype=torch.int32, device=DEV)
    tail = (idx_d.data_ptr(), vals_d.data_ptr(), N.EF14, 1.0, _stream())
    e = Ed.data_ptr()
    assert L.arctopk_sparse_pack_mixed(e, e, 16, 2, a([0, 8]), a([3, 9]), a([0, 3]), *tail) == N.EINVAL
    assert L.arctopk_sparse_pack_mixed(e, e, 12, 2, a([0, 12]), a([3, 3]), a([0, 3]), *tail) == N.EINVAL
    assert L.arctopk_sparse_pack_mixed(e, vals_d.data_ptr(), 16, 2, a([0, 8]), a([3, 3]), a([0, 3]), *tail) == N.EINVAL
    torch.cuda.synchronize()
    assert_bitwise(Ed, want_E, "E after the refused calls")


@pytest.mark.parametrize("nranks,ws,decay", [(1, 1, 1.0), (1, 2, 1.0), (1, 3, 0.7), (2, 2, 0.7), (2, 3, 1.0)])
@pytest.mark.parametrize("name", ["mix", "aligned", "tail", "many"])
def test_decode_mixed21_phase(name, nranks, ws, decay):
    shapes = SETS[name]
    _, gE0, g = _inputs(shapes, 3)
    n = gE0.numel()
    gE0[::5] = -0.0  # a stored -0.0 becomes +0.0 where nothing is added, as gE + 0.0
    ks = SM.layout_ks(shapes, 0.25, "tensor")
    numels, offs, koff = _layout(shapes, ks)
    all_idx = [[torch.randperm(m, generator=g)[:k].to(torch.int32) for m, k in zip(numels, ks)] for _ in range(nranks)]
    all_vals = [(torch.randn(sum(ks), generator=g) * 2.0).to(BF16) for _ in range(nranks)]
    want_out, want_gE = SM.decode21(all_vals, all_idx, shapes, ws, gE0, decay)
    obuf, out_d = _guarded(torch.full((n,), 5.0, dtype=BF16))
    gbuf, gE_d = _guarded(gE0)
    sbuf, scr_d = _guarded(torch.full((n,), 9.0))
    idx_d = torch.cat([torch.cat(ix) for ix in all_idx]).to(DEV)
    vals_d = torch.cat(all_vals).to(DEV)
    N.check(N.lib().arctopk_sparse_decode_mixed21(out_d.data_ptr(), gE_d.data_ptr(), scr_d.data_ptr(), n, len(shapes),
                                                  N.i64_array(offs), N.i64_array(ks), N.i64_array(koff), sum(ks),
                                                  idx_d.data_ptr(), vals_d.data_ptr(), nranks, ws, decay, _stream()),
            "arctopk_sparse_decode_mixed21")
    torch.cuda.synchronize()
    assert_bitwise(gE_d.view(torch.int32), want_gE.view(torch.int32), "gE bits")
    assert_bitwise(out_d, want_out, "out")
    assert _intact(obuf, out_d) and _intact(gbuf, gE_d) and _intact(sbuf, scr_d)


def test_decode_mixed21_skips_an_index_outside_its_tensor():
    """-1, a tensor's numel and INT32_MAX among valid indices, in both ranks' payloads: those entries
    add nothing, every other element is what the valid entries alone give, the guards stay intact."""
    shapes, ks = [[8], [8]], [3, 4]
    i32 = torch.int32
    idx = [[torch.tensor([-1, 2, 5], dtype=i32), torch.tensor([0, 3, 8, 2 ** 31 - 1], dtype=i32)],
           [torch.tensor([7, -1, 8], dtype=i32), torch.tensor([8, 1, 3, -5], dtype=i32)]]
    vals = [torch.arange(1.0, 8.0).to(BF16), torch.arange(8.0, 15.0).to(BF16)]
    valid_idx = [[torch.tensor([2, 5], dtype=i32), torch.tensor([0, 3], dtype=i32)],
                 [torch.tensor([7], dtype=i32), torch.tensor([1, 3], dtype=i32)]]
    valid_vals = [torch.tensor([2.0, 3.0, 4.0, 5.0]).to(BF16), torch.tensor([8.0, 12.0, 13.0]).to(BF16)]
    gE0 = torch.arange(16.0) * 0.37 - 1.0
    want_out, want_gE = SM.decode21(valid_vals, valid_idx, shapes, 2, gE0, 0.7)
    assert want_gE[11] != gE0[11] and want_gE[4] == gE0[4] and want_gE[15] == gE0[15]  # 3: both ranks; 4, 15: none
    obuf, out_d = _guarded(torch.full((16,), 5.0, dtype=BF16))
    gbuf, gE_d = _guarded(gE0)
    sbuf, scr_d = _guarded(torch.full((16,), 9.0))
    idx_d = torch.cat([torch.cat(ix) for ix in idx]).to(DEV)
    vals_d = torch.cat(vals).to(DEV)
    N.check(N.lib().arctopk_sparse_decode_mixed21(out_d.data_ptr(), gE_d.data_ptr(), scr_d.data_ptr(), 16, 2,
                                                  N.i64_array([0, 8]), N.i64_array(ks), N.i64_array([0, 3]), 7,
                                                  idx_d.data_ptr(), vals_d.data_ptr(), 2, 2, 0.7, _stream()),
            "arctopk_sparse_decode_mixed21")
    torch.cuda.synchronize()
    assert_bitwise(gE_d.view(torch.int32), want_gE.view(torch.int32), "gE bits")
    assert_bitwise(out_d, want_out, "out")
    assert _intact(obuf, out_d) and _intact(gbuf, gE_d) and _intact(sbuf, scr_d)


# ---- the hooks ---------------------------------------------------------------------------
def _state(kind, ef, source="host", sparse_type="tensor", c4=False, seed=21, option=True, ratio=0.25):
    kw = dict(compress_ratio=ratio, start_compress_iter=0, sparse_type=sparse_type, random=kind == "randk",
              use_error_feedback=ef, random_seed=seed, index_source=source)
    st = SH4.SparseState(None, warmup_iters=4, **kw) if c4 else SH.SparseState(None, **kw)
    if option:
        st.error_dtype = F32
    return st


def _hook(st):
    return SH4.sparse_hook_sync if isinstance(st, SH4.SparseState) else SH.sparse_hook_sync


def _call(st, G, shapes):
    out = _hook(st)(st, SyntheticBucket(G.to(DEV), shapes, index=0, is_last=True)).wait()
    torch.cuda.synchronize()
    return out


# ---- 2. ties -----------------------------------------------------------------------------
def test_topk_ties_resolve_lowest_index_first():
    """G and E small multiples of 0.5, so many |X| are equal (also at the k-th): the device's
    indices are the restatement's (stable descending sort, lowest index first), and bf16 holds
    every X, so no remainder is left at a selected element."""
    st = _state("topk", "ef14")
    o = SM.SparseMixedOracle(1, MIX, 0.25, "ef14")
    n = bucket_numel(MIX)
    for it in range(3):
        G = (torch.randint(-6, 7, (n,), generator=torch.Generator().manual_seed(30 + it)).float() * 0.5).to(BF16)
        out = _call(st, G, MIX)
        res = o.call([G])
        want = torch.cat(res["indices"][0])
        assert torch.equal(st.last_indices.cpu(), want), f"call {it}: indices"
        assert_bitwise(out, res["out"], f"call {it} out")
        assert_bitwise(st.error_dict[0], o.Es[0], f"call {it} E")
        _, offs, _ = _layout(MIX, res["ks"])
        pos = SM._flat(MIX, res["indices"][0])
        assert not st.error_dict[0].cpu()[pos].any(), "a remainder at a selected element"
    x = SM.fold14(G, res["E_old"][0])[offs[4]:offs[4] + 12297].abs()
    kth = torch.topk(x, res["ks"][4]).values.min()
    assert int((x == kth).sum()) > 1, "the input has no tie at the k-th |X|"


# ---- 3. hooks at world size 1 ------------------------------------------------------------
HOOK_CASES = [(kind, source, ef, name, "tensor", False)
              for name in ("mix", "many") for ef in ("ef14", "ef21")
              for kind, source in (("topk", "host"), ("randk", "host"), ("randk", "torch"), ("randk", "hash"))]
HOOK_CASES += [(kind, source, ef, "mix2d", sparse_type, False)
               for kind, source in (("topk", "host"), ("randk", "host"), ("randk", "hash"))
               for ef in ("ef14", "ef21") for sparse_type in ("row", "column")]
HOOK_CASES += [("topk", "host", "ef14", "mix", "tensor", True), ("randk", "hash", "ef21", "mix", "tensor", True),
               ("topk", "host", "ef21", "mix", "tensor", True)]


@pytest.mark.parametrize("kind,source,ef,name,sparse_type,c4", HOOK_CASES)
def test_hook_vs_restatement(kind, source, ef, name, sparse_type, c4):
    shapes = SETS[name]
    st = _state(kind, ef, source, sparse_type, c4)
    o = SM.SparseMixedOracle(1, shapes, 0.25, ef, random=kind == "randk", index_source=source,
                             sparse_type=sparse_type, seed=21, c4=c4, warmup_iters=4, device=DEV)
    n = bucket_numel(shapes)
    seen_ks = []
    for it in range(4 if ef == "ef21" else 3):  # EF21: the dense first call, then three compressed ones
        G = (torch.randn(n, generator=torch.Generator().manual_seed(400 + it)) * 10.0 ** (it - 1)).to(BF16)
        E_old = st.error_dict[0].cpu().clone() if 0 in st.error_dict else torch.zeros(n)
        out = _call(st, G, shapes)
        res = o.call([G])
        what = f"{kind}/{source}/{ef}/{name}/{sparse_type}/c4={c4} call {it}"
        E = st.error_dict[0]
        assert out.dtype == BF16 and E.dtype == F32, what
        assert_bitwise(out, res["out"], what + " out")
        assert_bitwise(E.view(torch.int32), o.Es[0].view(torch.int32), what + " E bits")
        assert st.comm_bits_this_round == o.bits == 0 and st.iter == o.iter, what
        if not res["dense"]:
            assert torch.equal(st.last_indices.cpu(), torch.cat(res["indices"][0])), what + " indices"
            assert list(st.last_k) == res["ks"], what
            seen_ks.append(tuple(res["ks"]))
        if ef == "ef14":  # conservation: nothing of G + E is lost
            assert torch.equal(out.float().cpu() + E.cpu(), G.float() + E_old), what + " conservation"
        else:  # decay 1 at world size 1: the global residual is the local one
            gE = st.global_error_dict[0]
            assert gE.dtype == F32, what
            assert_bitwise(gE.view(torch.int32), o.gE.view(torch.int32), what + " gE bits")
            assert torch.equal(gE.view(torch.int32), E.view(torch.int32)), what + " gE == E"
            assert torch.equal(out, gE.to(BF16)), what + " out == b(gE)"
    assert st.mixed_calls == 3 and len(seen_ks) == 3
    assert len(set(seen_ks)) == (3 if c4 else 1), "the ramp's ks differ on every call"


def test_ef21_decay_through_the_hook():
    st = _state("topk", "ef21")
    st.error_decay = 0.7
    o = SM.SparseMixedOracle(1, MIX, 0.25, "ef21", decay=0.7)
    n = bucket_numel(MIX)
    for it in range(3):
        G = torch.randn(n, generator=torch.Generator().manual_seed(450 + it)).to(BF16)
        out = _call(st, G, MIX)
        res = o.call([G])
        assert_bitwise(out, res["out"], f"call {it} out")
        assert_bitwise(st.error_dict[0].view(torch.int32), o.Es[0].view(torch.int32), f"call {it} E")
        assert_bitwise(st.global_error_dict[0].view(torch.int32), o.gE.view(torch.int32), f"call {it} gE")


# ---- 4. the stall ------------------------------------------------------------------------
@pytest.mark.parametrize("error_dtype,want", [(F32, 37.5), (None, 32.0)])
def test_unselected_elements_stall_in_bf16_and_not_in_fp32(error_dtype, want):
    """[8] at k = 1: element 0 is 1024 and selected every call, the others receive 2^-3 for 300
    calls: 37.5 in an fp32 residual; a bf16 one stops at 2^8 * 2^-3 = 32 (today's behaviour: that
    half passes without the option)."""
    st = _state("topk", "ef14", option=False, ratio=0.125)
    st.error_dtype = error_dtype
    G = torch.full((8,), 0.125)
    G[0] = 1024.0
    Gd = G.to(BF16).to(DEV)
    for _ in range(300):
        out = _hook(st)(st, SyntheticBucket(Gd.clone(), [[8]], index=0, is_last=True)).wait()
        assert st.last_k == [1]
    torch.cuda.synchronize()
    E = st.error_dict[0].float().cpu()
    assert st.last_indices.cpu().tolist() == [0]
    assert out.float().cpu().tolist() == [1024.0] + [0.0] * 7
    assert E[0] == 0 and torch.equal(E[1:], torch.full((7,), want)), E


# ---- 5. two ranks ------------------------------------------------------------------------
def _two_rank_worker(rank, ws, port, kind, ef, decay):
    sys.path.insert(0, REPO)
    sys.path.insert(0, HERE)
    torch.set_num_threads(2)
    dist.init_process_group("gloo", init_method=port, rank=rank, world_size=ws)
    st = _state(kind, ef, "host", seed=77)
    st.error_decay = decay
    o = SM.SparseMixedOracle(ws, MIX, 0.25, ef, random=kind == "randk", index_source="host", seed=77, decay=decay)
    n = bucket_numel(MIX)
    for it in range(4 if ef == "ef21" else 3):
        Gl = torch.randn(n, generator=torch.Generator().manual_seed(1000 * it + rank)).to(BF16)
        parts = [torch.empty(n) for _ in range(ws)]
        dist.all_gather(parts, Gl.float())
        out = _call(st, Gl, MIX)
        res = o.call([p.to(BF16) for p in parts])
        what = f"{kind}/{ef} call {it} rank {rank}"
        assert_bitwise(out, res["out"], what + " out")
        assert st.error_dict[0].dtype == F32
        assert_bitwise(st.error_dict[0].view(torch.int32), o.Es[rank].view(torch.int32), what + " E")
        if ef == "ef21":
            assert st.global_error_dict[0].dtype == F32
            assert_bitwise(st.global_error_dict[0].view(torch.int32), o.gE.view(torch.int32), what + " gE")
        if not res["dense"]:
            assert torch.equal(st.last_indices.cpu(), torch.cat(res["indices"][rank])), what + " indices"
        assert st.comm_bits_this_round == o.bits, what
    assert st.mixed_calls == 3 and o.bits > 0
    dist.destroy_process_group()


@pytest.mark.parametrize("kind,ef,decay", [("topk", "ef14", 1.0), ("topk", "ef21", 0.7), ("randk", "ef21", 1.0)])
def test_two_ranks_one_gpu(kind, ef, decay):
    mp.spawn(_two_rank_worker, args=(2, rendezvous(), kind, ef, decay), nprocs=2, join=True)


# ---- 6. checkpoints and refusals ---------------------------------------------------------
@pytest.mark.parametrize("kind,ef", [("topk", "ef14"), ("randk", "ef21")])
def test_resume_from_checkpoint_is_bit_identical(kind, ef, tmp_path):
    n = bucket_numel(MIX)
    Gs = [torch.randn(n, generator=torch.Generator().manual_seed(600 + it)).to(BF16) for it in range(5)]
    a = _state(kind, ef, "host", seed=5)
    outs = []
    for it, G in enumerate(Gs):
        if it == 3:
            torch.save(a.state_dict(), tmp_path / "ck.pt")
        outs.append(_call(a, G, MIX).cpu())
    sd = torch.load(tmp_path / "ck.pt", weights_only=True)
    assert sd["error_dtype"] == "fp32" and sd["mixed_buckets"] == [0] and sd["error_dict"][0].dtype == F32
    b = _state(kind, ef, "host", seed=999)
    b.load_state_dict(sd, device=DEV)
    assert b.error_dict[0].dtype == F32 and b.error_dict[0].is_cuda
    for it in (3, 4):
        assert_bitwise(_call(b, Gs[it], MIX), outs[it], f"resumed call {it} out")
    assert_bitwise(b.error_dict[0].view(torch.int32), a.error_dict[0].view(torch.int32), "E")
    if ef == "ef21":
        assert_bitwise(b.global_error_dict[0].view(torch.int32), a.global_error_dict[0].view(torch.int32), "gE")
    # the fp32 residuals of a bf16 bucket do not load into a state without the option
    c = _state(kind, ef, "host", option=False)
    with pytest.raises(ValueError, match="error_dtype"):
        c.load_state_dict(sd, device=DEV)
    assert not c.error_dict
    # a bf16-residual checkpoint is widened, exactly, and the run goes on with fp32 residuals
    old = _state(kind, ef, "host", seed=5, option=False)
    for G in Gs[:3]:
        _call(old, G, MIX)
    assert old.error_dict[0].dtype == BF16 and old.mixed_calls == 0
    d = _state(kind, ef, "host")
    d.load_state_dict(old.state_dict(), device=DEV)
    assert d.error_dict[0].dtype == F32 and torch.equal(d.error_dict[0].to(BF16), old.error_dict[0])
    _call(d, Gs[3], MIX)
    assert d.mixed_calls == 1 and d.error_dict[0].dtype == F32


def test_refusals():
    G = torch.randn(bucket_numel(TAIL)).to(BF16)
    st = _state("topk", "ef14")
    st.error_dtype = torch.float16  # any other value: ValueError at the first compressed call
    with pytest.raises(ValueError, match="error_dtype"):
        _call(st, G, TAIL)
    assert not st.error_dict
    st = _state("topk", "ef21")
    st.large_batch_init = True
    with pytest.raises(ValueError, match="large_batch_init"):
        _call(st, G, TAIL)
    # switching the option once a bucket has residuals is an error, not a reinterpretation
    st = _state("topk", "ef14", option=False)
    _call(st, G, TAIL)
    st.error_dtype = F32
    with pytest.raises(RuntimeError, match="error_dtype"):
        _call(st, G, TAIL)
    st = _state("topk", "ef14")
    _call(st, G, TAIL)
    st.error_dtype = None
    with pytest.raises(RuntimeError, match="float32"):
        _call(st, G, TAIL)
    # fp32 buckets and noef ignore it
    st = _state("topk", "ef14")
    _call(st, G.float(), TAIL)
    assert st.mixed_calls == 0 and st.error_dict[0].dtype == F32 and not st._mixed_buckets
    st = _state("topk", "noef")
    _call(st, G, TAIL)
    assert st.mixed_calls == 0 and not st.error_dict
