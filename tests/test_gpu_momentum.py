"""The native momentum fold (arctopk_momentum_fold, HookState.accumulate_momentum_on_bucket)
against the reference's own two torch ops run on the same GPU: bit for bit.

The expected value is always grad.mul_(1 - beta1).add_(exp_avg, alpha=beta1) per tensor
(comm_hooks/utils.py:54-65) on a clone of the bucket, on the GPU.  Bit patterns are compared
through integer views; where the expected value is NaN only NaN is required.

How torch rounds on the GPU is what the kernel has to reproduce, so the layout case also shows
that its inputs tell the candidate rules apart: the expected output differs, in at least one
element, from every rule the kernel does not implement (computed here in float64 with explicit
rounding).  The rule per (bucket, moment) dtype pair, as measured on MI355X / torch-ROCm: the
Python scalars enter as fp32, `mul_` rounds to the bucket dtype, `add_(m, alpha=b)` is one
fma(b, m, t) rounded to the bucket dtype.  The rule does not depend on beta1, so it is pinned at
beta1 = 0.9, where every rejected rule has telltale elements in these inputs (at 0.999 a bf16
bucket with fp32 moments has none between the fused and the separate add; at 0 every candidate is
the same function, a = 1 and b = 0 in every precision); the other betas are held to torch's bits.
"""
import functools

import pytest
import torch

from allreducetopk_amd.bucket import SyntheticBucket, bucket_numel
from allreducetopk_amd.comm_hooks import default_hooks, group_topk_hook_no_reshape, sparse_hook
from allreducetopk_amd.comm_hooks.utils import HookState
from parity import ensure_group

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAIRS = [(torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16), (torch.bfloat16, torch.float32)]
PAIR_IDS = ["f32-f32", "bf16-bf16", "bf16-f32"]
BETAS = [0.9, 0.999, 0.0]
# every view after the first starts at an odd element offset of a buffer that itself starts one
# element into its allocation; the last tensor spans many chunks with a ragged head and tail
LAYOUT = [(1,), (3,), (5,), (8,), (1023,), (4096,), (4097,), (2 * 4096 + 7,), (64, 18), (300001,)]
SLICED = {9: 3, 6: 1}  # moments that are slices buf[s : s + n] of a larger tensor: tensor -> s
GUARD = 77.0


@pytest.fixture(scope="module", autouse=True)
def group():
    ensure_group("nccl")
    yield


def ibits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def assert_same_bits(got, exp, what):
    nan = exp.isnan()
    assert bool(got.isnan()[nan].all()), f"{what}: NaN expected where torch gives NaN"
    bad = (ibits(got) != ibits(exp)) & ~nan
    nbad = int(bad.sum())
    if nbad:
        i = int(bad.nonzero()[0])
        raise AssertionError(f"{what}: {nbad} of {exp.numel()} elements differ from torch; first at {i}: "
                             f"got {got.flatten()[i].item()!r}, torch {exp.flatten()[i].item()!r}")


def specials(dtype):
    fi = torch.finfo(dtype)
    return torch.tensor([-0.0, float("inf"), float("-inf"), float("nan"), 1e-40, fi.max, -fi.max,
                         fi.tiny, 1.0], dtype=torch.float64).to(dtype)


def torch_loop(grads, moments, beta):
    for g, m in zip(grads, moments):
        g.mul_(1 - beta).add_(m, alpha=beta)


def make_state(params, moments, beta):
    st = HookState(None)
    st.init_momentum_field({p: {"exp_avg": m} for p, m in zip(params, moments)}, beta)
    return st


@functools.lru_cache(maxsize=None)
def layout_inputs(gdt, mdt):
    """(big, moment buffers): big[1 : 1 + N] is the bucket; N(0, 1) with -0.0, +-inf, NaN, a
    denormal, +-max planted in G and M: special against normal, normal against special and
    special against special (shifted by one, so inf meets -inf)."""
    gen = torch.Generator().manual_seed(20)
    n = bucket_numel(LAYOUT)
    big = torch.randn(n + 2, generator=gen).to(gdt)
    sg, sm = specials(gdt), specials(mdt)
    ns = sg.numel()
    bufs, off = [], 1
    for i, shape in enumerate(LAYOUT):
        k = bucket_numel([shape])
        s = SLICED.get(i, 0)
        buf = torch.randn(k + 2 * s, generator=gen).to(mdt)
        if s:
            buf[:s] = GUARD
            buf[s + k:] = GUARD
        if k >= 4 * ns:
            big[off + 2:off + 2 + ns] = sg                      # special G, normal M
            buf[s + 2 + ns:s + 2 + 2 * ns] = sm                 # normal G, special M
            big[off + k - 2 * ns:off + k - ns] = sg             # special both, M one ahead
            buf[s + k - 2 * ns:s + k - ns] = sm.roll(1)
        bufs.append(buf.to(DEV))
        off += k
    big[0], big[n + 1] = GUARD, -GUARD
    return big.to(DEV), bufs


def layout_case(gdt, mdt):
    """Fresh bucket (a copy of the inputs), its moments (views of the shared inputs) and guards."""
    big0, bufs = layout_inputs(gdt, mdt)
    big = big0.clone()
    n = bucket_numel(LAYOUT)
    moments = []
    for i, (shape, buf) in enumerate(zip(LAYOUT, bufs)):
        s = SLICED.get(i, 0)
        moments.append(buf[s:s + bucket_numel([shape])].view(shape))
    params = [torch.nn.Parameter(torch.empty(0)) for _ in LAYOUT]
    return big, SyntheticBucket(big[1:1 + n], LAYOUT, parameters=params), params, moments, bufs


def candidates(G, M, beta, gdt):
    """Outputs of the candidate rounding rules for bucket values G and moments M (flat tensors),
    in float64 with explicit rounding.  'fma_f32' is the rule the kernel implements."""
    def r32(x):
        return x.to(torch.float32).double()

    def rg(x):  # to the bucket dtype as the GPU does: the fp32 result, then the store's rounding
        return x.to(torch.float32).to(gdt).double()
    a64, b64 = 1 - beta, beta
    a32 = torch.tensor(a64, dtype=torch.float64).to(torch.float32).double().item()
    b32 = torch.tensor(b64, dtype=torch.float64).to(torch.float32).double().item()
    ag = torch.tensor(a64, dtype=torch.float64).to(gdt).double().item()
    bg = torch.tensor(b64, dtype=torch.float64).to(gdt).double().item()
    g, m = G.double(), M.double()
    t = rg(g * a32)
    out = {"fma_f32": rg(t + b32 * m), "mul_add_f32": rg(t + r32(b32 * m))}
    if gdt == torch.bfloat16:
        out["fma_alpha_bf16"] = rg(t + bg * m)
        out["mul_scalar_bf16"] = rg(rg(g * ag) + b32 * m)
    return {k: v.to(gdt) for k, v in out.items()}


@pytest.mark.parametrize("beta", BETAS)
@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
def test_layout_case_bits_guards_and_telltales(pair, beta):
    gdt, mdt = pair
    n = bucket_numel(LAYOUT)
    big, bucket, params, moments, bufs = layout_case(gdt, mdt)
    exp_big, exp_bucket, _, _, _ = layout_case(gdt, mdt)
    g0 = big[1:1 + n].clone()
    before = [buf.clone() for buf in bufs]
    torch_loop(exp_bucket.gradients(), moments, beta)
    st = make_state(params, moments, beta)
    st.accumulate_momentum_on_bucket(bucket)
    torch.cuda.synchronize()
    assert st.momentum_native_calls == 1
    exp = exp_big[1:1 + n]
    # guard elements around the bucket slice and the sliced moments; the moments themselves
    assert big[0].item() == GUARD and big[n + 1].item() == -GUARD
    for i, (buf, ref) in enumerate(zip(bufs, before)):
        assert torch.equal(ibits(buf), ibits(ref)), f"moment buffer {i} was written"
    off = 0
    for i, shape in enumerate(LAYOUT):
        k = bucket_numel([shape])
        assert_same_bits(bucket.buffer()[off:off + k], exp[off:off + k], f"tensor {i} {shape}")
        off += k
    # the inputs separate the rules: torch's result differs from every rejected candidate
    if beta != 0.0:
        M = torch.cat([m.flatten() for m in moments])
        cand = candidates(g0, M, beta, gdt)
        fin = ~exp.isnan()
        for name, c in cand.items():
            ndiff = int(((ibits(c) != ibits(exp)) & fin & ~c.isnan()).sum())
            print(f"{PAIR_IDS[PAIRS.index(pair)]} beta {beta}: rule {name} differs from torch in {ndiff} elements")
            if name != "fma_f32" and beta == 0.9:
                assert ndiff >= 1, f"the inputs do not tell rule {name} from torch's"


@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
def test_more_tensors_than_one_batch(pair):
    gdt, mdt = pair
    shapes = [(k,) for k in range(1, 71)] + [(5000,)]
    gen = torch.Generator().manual_seed(31)
    G = torch.randn(bucket_numel(shapes), generator=gen).to(gdt).to(DEV)
    moments = [torch.randn(s, generator=gen).to(mdt).to(DEV) for s in shapes]
    params = [torch.nn.Parameter(torch.empty(0)) for _ in shapes]
    exp = G.clone()
    torch_loop(SyntheticBucket(exp, shapes).gradients(), moments, 0.9)
    st = make_state(params, moments, 0.9)
    bucket = SyntheticBucket(G, shapes, parameters=params)
    st.accumulate_momentum_on_bucket(bucket)
    st.accumulate_momentum_on_bucket(bucket)  # the cached arrays
    torch_loop(SyntheticBucket(exp, shapes).gradients(), moments, 0.9)
    torch.cuda.synchronize()
    assert st.momentum_native_calls == 2
    assert_same_bits(G, exp, "71 tensors, two folds")


HOOK_SHAPES = [[40, 16], [10], [4, 3, 3, 3], [300, 128]]


def _hook_run(kind, native, monkeypatch):
    monkeypatch.setenv("ARCTOPK_MOMENTUM_NATIVE", "1" if native else "0")
    gen = torch.Generator().manual_seed(5)
    params = [torch.nn.Parameter(torch.empty(0)) for _ in HOOK_SHAPES]
    moments = [torch.randn(s, generator=gen).to(DEV) for s in HOOK_SHAPES]
    if kind == "arc":
        st = group_topk_hook_no_reshape.GroupTopKState(None, r=4, compress_ratio=0.2, start_compress_iter=0,
                                                       use_error_feedback="ef14", seed=1234)
        hook = group_topk_hook_no_reshape.group_topk_hook
    else:
        st = sparse_hook.SparseState(None, compress_ratio=0.2, start_compress_iter=0, sparse_type="tensor",
                                     random=False, use_error_feedback="ef14")
        hook = sparse_hook.sparse_hook_sync
    state = {p: {"exp_avg": m} for p, m in zip(params, moments)}
    st.init_momentum_field(state, 0.9)
    got = []
    for it in range(2):
        G = torch.randn(bucket_numel(HOOK_SHAPES), generator=gen).to(DEV)
        out = hook(st, SyntheticBucket(G, HOOK_SHAPES, parameters=params)).wait()
        torch.cuda.synchronize()
        got.append((out.clone(), st.error_dict[0].clone()))
        # the optimizer's step: moments updated in place, one replaced by a new tensor
        for p in params[:-1]:
            state[p]["exp_avg"].mul_(0.9).add_(0.25)
        state[params[-1]]["exp_avg"] = state[params[-1]]["exp_avg"] * 0.9 - 0.125
    return got, st.momentum_native_calls


@pytest.mark.parametrize("kind", ["arc", "topk"])
def test_through_the_hooks(kind, monkeypatch):
    native, ncalls = _hook_run(kind, True, monkeypatch)
    torch_, tcalls = _hook_run(kind, False, monkeypatch)
    assert ncalls == 2 and tcalls == 0
    for it, ((o1, e1), (o2, e2)) in enumerate(zip(native, torch_)):
        assert torch.equal(ibits(o1), ibits(o2)), f"{kind} call {it}: bucket differs"
        assert torch.equal(ibits(e1), ibits(e2)), f"{kind} call {it}: residual differs"
    assert not torch.equal(native[0][0], native[1][0])


def test_through_my_allreduce_hook():
    shapes = HOOK_SHAPES
    gen = torch.Generator().manual_seed(6)
    G = torch.randn(bucket_numel(shapes), generator=gen).to(DEV)
    moments = [torch.randn(s, generator=gen).to(DEV) for s in shapes]
    params = [torch.nn.Parameter(torch.empty(0)) for _ in shapes]
    exp = G.clone()
    torch_loop(SyntheticBucket(exp, shapes).gradients(), moments, 0.9)
    exp.div_(1)
    st = make_state(params, moments, 0.9)
    out = default_hooks.my_allreduce_hook(st, SyntheticBucket(G, shapes, parameters=params)).wait()
    torch.cuda.synchronize()
    assert st.momentum_native_calls == 1 and st.adam_freeze_key
    assert_same_bits(out, exp, "my_allreduce_hook")


def test_fallbacks_run_the_torch_loop():
    gen = torch.Generator().manual_seed(8)
    # a float16 bucket
    shapes = [(33,), (4, 5)]
    G = torch.randn(bucket_numel(shapes), generator=gen).to(torch.float16).to(DEV)
    moments = [torch.randn(s, generator=gen).to(torch.float16).to(DEV) for s in shapes]
    params = [torch.nn.Parameter(torch.empty(0)) for _ in shapes]
    exp = G.clone()
    torch_loop(SyntheticBucket(exp, shapes).gradients(), moments, 0.9)
    st = make_state(params, moments, 0.9)
    st.accumulate_momentum_on_bucket(SyntheticBucket(G, shapes, parameters=params))
    assert st.momentum_native_calls == 0
    assert torch.equal(G.view(torch.int16), exp.view(torch.int16))
    # a moment of broadcastable shape [1] against a [4] gradient
    shapes = [(4,), (6,)]
    G = torch.randn(10, generator=gen).to(DEV)
    moments = [torch.randn(1, generator=gen).to(DEV), torch.randn(6, generator=gen).to(DEV)]
    params = [torch.nn.Parameter(torch.empty(0)) for _ in shapes]
    exp = G.clone()
    torch_loop(SyntheticBucket(exp, shapes).gradients(), moments, 0.9)
    st = make_state(params, moments, 0.9)
    st.accumulate_momentum_on_bucket(SyntheticBucket(G, shapes, parameters=params))
    torch.cuda.synchronize()
    assert st.momentum_native_calls == 0
    assert torch.equal(ibits(G), ibits(exp))


def test_custom_op_equals_the_method():
    import allreducetopk_amd.ops  # noqa: F401  (registers torch.ops.arctopk.*)
    gdt, mdt = torch.bfloat16, torch.float32
    n = bucket_numel(LAYOUT)
    big, bucket, params, moments, _ = layout_case(gdt, mdt)
    big2 = big.clone()
    st = make_state(params, moments, 0.9)
    st.accumulate_momentum_on_bucket(bucket)
    offsets, numels, off = [], [], 0
    for shape in LAYOUT:
        offsets.append(off)
        numels.append(bucket_numel([shape]))
        off += numels[-1]
    torch.ops.arctopk.momentum_fold(big2[1:1 + n], [m.flatten() for m in moments], offsets, numels,
                                    1 - 0.9, 0.9)
    torch.cuda.synchronize()
    assert torch.equal(ibits(big2), ibits(big))
