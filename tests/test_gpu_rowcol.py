"""Row- / column-wise TopK and RandK (sparse_type "row" / "column") on MI355X: the segmented
select (arctopk_seg_select) against the reference's own selections and the CPU restatement
(tests/rowcol_oracle.py), and the hooks built on it, bit for bit."""
import sys
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import rowcol_oracle as RC
from allreducetopk_amd import _native as N
from allreducetopk_amd.bucket import SyntheticBucket, bucket_numel
from allreducetopk_amd.comm_hooks import sparse_hook, sparse_hook_c4
from oracle import sparse as S
from parity import assert_bitwise, check_rows_tie_aware, ensure_group

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)

# the last row shape is longer than kMSmallSel (12,288): the multi-block select per segment
ROW = [[7], [40, 16], [4, 3, 3, 3], [96, 40], [3, 1000], [1, 5], [5, 1], [257, 130], [63, 65], [300, 1025],
       [2, 13000]]
# 1, 3, 63, 64 + 1, 128 + 1 and 4 x 64 + 1 columns: whole and partial strips of 16 columns (below
# 16,384 columns; COLUMN_SWITCH has the 64-column strips); the column strips have no row limit
COLUMN = [[7], [16, 40], [4, 3, 3, 3], [1000, 3], [130, 257], [5, 1], [1, 5], [65, 63], [64, 129], [3000, 70]]
# +-1 around the dispatch's switch points (csrc/seg_select.hip):
#   kSegWaveLen 512 (wave per segment / 256-thread block), kSegMidLen 4096 (256 / 1,024 threads),
#   kMSmallSel 12288 (LDS keys / multi-block select), kSegGridCap 2048 blocks per tensor
#   ([8200, 5]: 2,050 groups of four wave segments; [2049, 513]: 2,049 block segments: a second
#   walk of the grid), kSegBatch 32 tensors per launch (33 tensors of one class)
ROW_SWITCH = [[3, 512], [3, 513], [2, 4096], [2, 4097], [2, 12288], [2, 12289], [8200, 5], [2049, 513]] + \
    [[3, 20]] * 33
#   ARCTOPK_SEG_WIDE_STRIPS 256 strips of 64 = 16,384 columns (strips of 16 below, of 64 from there
#   on; 16,385: a partial wide strip), kSegBatch 32 (33 strip tensors), kStripWaves 16 (15, 16, 17
#   rows: the last waves own no row), kStripBatch 8 accesses x 4 rows ([600, 66]: 38 rows per wave)
COLUMN_SWITCH = [[15, 66], [16, 66], [17, 66], [600, 66], [6, 16383], [6, 16384], [70, 16385]] + [[20, 3]] * 33
SHAPES = {"row": ROW, "column": COLUMN}
SWITCH = {"row": ROW_SWITCH, "column": COLUMN_SWITCH}


@pytest.fixture(scope="module", autouse=True)
def group():
    ensure_group("nccl")
    yield


def _rand(shapes, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(bucket_numel(shapes), generator=g).to(dtype)


def _seg_select(x, shapes, ratio, mode, hashed=False, seed=0, zero=False, dtype=torch.float32):
    """arctopk_seg_select over a bucket; x None: indices only.  Returns per-tensor idx (and vals)."""
    L = N.lib()
    geo = [RC.geometry(s, ratio, mode) for s in shapes]
    rows, cols, kseg, tot = [g[0] for g in geo], [g[1] for g in geo], [g[4] for g in geo], [g[5] for g in geo]
    koff = [sum(tot[:i]) for i in range(len(tot))]
    numels = [r * c for r, c in zip(rows, cols)]
    offs = [sum(numels[:i]) for i in range(len(numels))]
    a = N.i64_array
    nb = int(L.arctopk_seg_workspace_bytes(len(shapes), a(rows), a(cols), a(kseg), int(mode == "column")))
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    idx = torch.full((sum(tot),), -1, dtype=torch.int32, device=DEV)
    vals = torch.zeros(sum(tot), dtype=dtype, device=DEV) if x is not None else None
    N.check(L.arctopk_seg_select(None if x is None else x.data_ptr(), len(shapes), None if x is None else a(offs),
                                 a(rows), a(cols), a(kseg), a(koff), int(mode == "column"), int(hashed), int(seed),
                                 idx.data_ptr(), None if x is None else vals.data_ptr(), ws.data_ptr(),
                                 N.DTYPE_CODE[dtype], int(zero), torch.cuda.current_stream().cuda_stream),
            "arctopk_seg_select")
    torch.cuda.synchronize()
    ic = idx.cpu()
    vc = vals.cpu() if vals is not None else None
    return ([ic[o:o + k] for o, k in zip(koff, tot)], None if vc is None else [vc[o:o + k] for o, k in zip(koff, tot)],
            offs)


# 1 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["row", "column"])
@pytest.mark.parametrize("ratio", [0.2, 0.01])
def test_kernel_matches_reference_segments(mode, ratio):
    """Every segment's index set equals the reference's own (tests/golden/rowcol_select.npz)."""
    gold = RC.golden_load()
    shapes = gold["shapes"][mode]
    assert shapes == SHAPES[mode]
    x = torch.cat([RC.golden_input(gold, i, s) for i, s in enumerate(shapes)])
    idx, vals, offs = _seg_select(x.to(DEV), shapes, ratio, mode)
    want = RC.golden_positions(gold, mode, ratio)
    for i, shape in enumerate(shapes):
        got = RC.payload_positions(idx[i], shape, ratio, mode)
        assert torch.equal(got, want[i]), f"{mode} {ratio} {shape}"
        n = bucket_numel([shape])
        assert torch.equal(vals[i], x[offs[i]:offs[i] + n][idx[i].long()])


# 2 ------------------------------------------------------------------------------------------
def _hook_vs_helper(mod, st, shapes, mode, ef, random, index_source, calls, dtype=torch.float32, ratio_of=None,
                    seed0=50):
    rng = torch.Generator().manual_seed(st.random_seed)
    E = gE = None
    for it in range(calls):
        G = _rand(shapes, seed0 + it, dtype)
        ratio = ratio_of() if ratio_of is not None else st.compress_ratio
        out = mod.sparse_hook_sync(st, SyntheticBucket(G.to(DEV), shapes)).wait()
        torch.cuda.synchronize()
        if ef == "ef21" and E is None:
            E, gE = G.clone(), G.clone()
            continue
        seed = int(torch.randint(0, 1_000_000_000, (1,), generator=rng).item()) if random else None
        res = RC.simulate_step([G], [E if not (ef == "ef14" and E is None) else None], gE, shapes, ratio, mode, ef,
                               random, seed, index_source)
        assert st.last_k == res["ks"]
        assert torch.equal(st.last_indices.cpu(), res["indices"][0]), f"it{it} indices"
        assert_bitwise(out, res["out"], f"it{it} out")
        if ef != "noef":
            assert_bitwise(st.error_dict[0], res["E_new"][0], f"it{it} E")
            E = res["E_new"][0]
        if ef == "ef21":
            assert_bitwise(st.global_error_dict[0], res["gE_new"], f"it{it} gE")
            gE = res["gE_new"]
        assert st.comm_bits_this_round == 0  # both formulas carry a factor (world_size - 1)


@pytest.mark.parametrize("mode", ["row", "column"])
@pytest.mark.parametrize("ef", ["noef", "ef14", "ef21"])
def test_topk_hook_vs_helper(mode, ef):
    st = sparse_hook.SparseState(None, compress_ratio=0.2, start_compress_iter=0, sparse_type=mode,
                                 random=False, use_error_feedback=ef)
    _hook_vs_helper(sparse_hook, st, SHAPES[mode], mode, ef, False, None, 3 + (ef == "ef21"))


@pytest.mark.parametrize("mode", ["row", "column"])
@pytest.mark.parametrize("ef,src", [("ef14", "hash"), ("ef21", "hash"), ("ef14", "host")])
def test_randk_hook_vs_helper(mode, ef, src):
    st = sparse_hook.SparseState(None, compress_ratio=0.2, start_compress_iter=0, sparse_type=mode,
                                 random=True, use_error_feedback=ef, random_seed=11, index_source=src)
    # "host" loops over segments in Python, as the reference does: the small shapes only
    shapes = SHAPES[mode] if src == "hash" else [s for s in SHAPES[mode] if bucket_numel([s]) <= 40000]
    _hook_vs_helper(sparse_hook, st, shapes, mode, ef, True, src, 3 + (ef == "ef21"))


@pytest.mark.parametrize("mode", ["row", "column"])
def test_switch_points_hook_vs_helper(mode):
    """Shapes one below and one above every switch point of the dispatch (SWITCH above)."""
    for random in (False, True):
        st = sparse_hook.SparseState(None, compress_ratio=0.01, start_compress_iter=0, sparse_type=mode,
                                     random=random, use_error_feedback="ef14", random_seed=3,
                                     index_source="hash")
        _hook_vs_helper(sparse_hook, st, SWITCH[mode], mode, "ef14", random, "hash", 2)


# 3 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["row", "column"])
def test_bf16_topk_hook_vs_helper(mode):
    """bf16 buckets tie at the threshold in many segments: the tie rule through the hook."""
    st = sparse_hook.SparseState(None, compress_ratio=0.2, start_compress_iter=0, sparse_type=mode,
                                 random=False, use_error_feedback="ef14")
    _hook_vs_helper(sparse_hook, st, SHAPES[mode], mode, "ef14", False, None, 2, dtype=torch.bfloat16)


# 4 ------------------------------------------------------------------------------------------
def _tie_tensor(nseg, seg_len, k, seed):
    """[nseg, seg_len]: 70 % exact zeros, blocks of +-2.5, one constant segment, one segment with
    fewer non-zeros than k."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(nseg, seg_len, generator=g)
    x[torch.rand(nseg, seg_len, generator=g) < 0.7] = 0.0
    blk = torch.rand(nseg, seg_len, generator=g) < 0.1
    x[blk] = torch.where(torch.rand(int(blk.sum()), generator=g) < 0.5, torch.tensor(2.5), torch.tensor(-2.5))
    x[3] = -0.75
    x[5] = 0.0
    x[5, :max(1, k // 2)] = torch.randn(max(1, k // 2), generator=g)
    return x


@pytest.mark.parametrize("mode,shape", [("row", [64, 200]), ("column", [200, 130])])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_ties_and_order_at_the_kernel_entry(mode, shape, dtype):
    ratio = 0.2
    r, c, nseg, seg_len, k, tot = RC.geometry(shape, ratio, mode)
    segs = _tie_tensor(nseg, seg_len, k, 9).to(dtype)
    x = (segs.t().contiguous() if mode == "column" else segs).flatten()  # the tensor, row-major
    for zero in (False, True):
        xd = x.to(DEV)
        idx, vals, _ = _seg_select(xd, [shape], ratio, mode, zero=zero, dtype=dtype)
        pos = RC.payload_positions(idx[0], shape, ratio, mode)
        for s in range(nseg):
            assert check_rows_tie_aware(pos[s], segs[s].float().abs(), k, band=0.0) == 0, f"segment {s}"
            assert torch.all(pos[s][1:] > pos[s][:-1]), f"segment {s} order"
        assert torch.equal(vals[0], x[idx[0].long()])
        want = x.clone()
        if zero:
            want[idx[0].long()] = 0
        assert torch.equal(xd.cpu(), want)  # zeroed exactly at idx, untouched elsewhere


# 5 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["row", "column"])
def test_hash_draw_matches_the_numpy_restatement(mode):
    shapes, ratio, seed = SHAPES[mode], 0.2, 987654321
    idx, _, _ = _seg_select(None, shapes, ratio, mode, hashed=True, seed=seed)
    for t, shape in enumerate(shapes):
        r, c, nseg, seg_len, k, _ = RC.geometry(shape, ratio, mode)
        want = RC.hash_positions(nseg, seg_len, k, seed, t)
        got = RC.payload_positions(idx[t], shape, ratio, mode)
        assert torch.equal(got, want), f"{mode} {shape}"
        if nseg > 1 and seg_len >= 40:  # two segments of one tensor draw different subsets
            assert not torch.equal(got[0], got[1])
        if len(shape) == 1:
            assert torch.equal(idx[t], S.randk_hash_indices(seg_len, k, seed, t))


# 6 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("random", [False, True])
def test_one_dimensional_bucket_equals_tensor_mode(random):
    shapes = [[7], [1000], [13000], [300], [5]]
    res = {}
    for mode in ("tensor", "row", "column"):
        st = sparse_hook.SparseState(None, compress_ratio=0.2, start_compress_iter=0, sparse_type=mode,
                                     random=random, use_error_feedback="ef14", random_seed=2,
                                     index_source="hash")
        outs = []
        for it in range(2):
            out = sparse_hook.sparse_hook_sync(st, SyntheticBucket(_rand(shapes, 80 + it).to(DEV), shapes)).wait()
            torch.cuda.synchronize()
            outs.append((out.cpu().clone(), st.error_dict[0].cpu().clone(), st.last_indices.cpu().clone()))
        res[mode] = outs
    for mode in ("row", "column"):
        for a, b in zip(res["tensor"], res[mode]):
            for u, v, what in zip(a, b, ("out", "E", "indices")):
                assert torch.equal(u, v), f"{mode} {what}"


# 7 ------------------------------------------------------------------------------------------
def test_c4_gradual_ratio_per_segment():
    shapes = ROW[:9]
    st = sparse_hook_c4.SparseState(None, compress_ratio=0.05, start_compress_iter=0, sparse_type="row",
                                    random=False, use_error_feedback="ef14", gradual_compression=True,
                                    warmup_iters=4)
    ratios = []

    def ratio_now():
        st.compression_started = True  # (the hook sets it before it reads the ratio)
        ratios.append(st.get_current_compress_ratio())
        return ratios[-1]

    _hook_vs_helper(sparse_hook_c4, st, shapes, "row", "ef14", False, None, 3, ratio_of=ratio_now)
    assert ratios[0] == 0.8 and ratios[0] > ratios[1] > ratios[2] > 0.05
    assert st.last_k == [RC.geometry(s, ratios[2], "row")[5] for s in shapes]


# 8 ------------------------------------------------------------------------------------------
def _worker(rank, ws, port, mode, ef, random):
    sys.path.insert(0, REPO)
    sys.path.insert(0, HERE)
    torch.set_num_threads(2)
    dist.init_process_group("gloo", init_method=port, rank=rank, world_size=ws)
    shapes = SHAPES[mode][:9]
    n = bucket_numel(shapes)
    st = sparse_hook.SparseState(None, compress_ratio=0.2, start_compress_iter=0, sparse_type=mode,
                                 random=random, use_error_feedback=ef, random_seed=5, index_source="hash")
    rng = torch.Generator().manual_seed(5)
    Es = gE = None
    bits = 0
    for it in range(3 + (ef == "ef21")):
        Gl = torch.randn(n, generator=torch.Generator().manual_seed(1000 * it + rank))
        allg = [torch.empty_like(Gl) for _ in range(ws)]
        dist.all_gather(allg, Gl)
        out = sparse_hook.sparse_hook_sync(st, SyntheticBucket(Gl.to("cuda:0"), shapes)).wait()
        torch.cuda.synchronize()
        if ef == "ef21" and Es is None:
            Es = [g.clone() for g in allg]
            gE = (allg[0] + allg[1]) / ws
            assert torch.equal(out.cpu(), gE)
            continue
        first = ef == "ef14" and Es is None
        seed = int(torch.randint(0, 1_000_000_000, (1,), generator=rng).item()) if random else None
        res = RC.simulate_step(allg, [None] * ws if first else Es, gE, shapes, 0.2, mode, ef, random, seed)
        assert torch.equal(out.cpu(), res["out"]), f"it{it} rank{rank} output"
        assert torch.equal(st.error_dict[0].cpu(), res["E_new"][rank]), f"it{it} E"
        Es = res["E_new"]
        if ef == "ef21":
            gE = res["gE_new"]
        bits += (2 * (ws - 1) if random else (ws - 1) * ws) * res["bits"]
        assert st.comm_bits_this_round == bits
    dist.destroy_process_group()


@pytest.mark.parametrize("mode,ef,random", [("column", "ef14", False), ("row", "ef21", False),
                                            ("column", "ef14", True)])
def test_two_ranks_one_gpu(mode, ef, random):
    from parity import rendezvous
    mp.spawn(_worker, args=(2, rendezvous(), mode, ef, random), nprocs=2, join=True)
