"""A CPU rig that records which native calls and collectives the TopK / RandK hooks make.

The bucket lives in CPU tensors, the process group is a stand-in of size 1 or 2, libarctopk is an
object that records every call and returns 0, and the stream query, the is-CUDA check, the
all-reduce and the flat all-gather record instead of run.  Nothing is computed: what is pinned is
the order of the calls, every scalar, the contents of every int64 array, which buffer each pointer
is (by role) and what the call leaves in the state.

``python tests/sparse_hook_rig.py`` prints the whole matrix's trace as JSON lines, for comparing two
trees (tests/test_sparse_hook_calls_host.py checks it against a restatement of the docstring)."""
import contextlib
import ctypes
import hashlib
import itertools
import json
import logging
import types

import torch
import torch.distributed as dist

from allreducetopk_amd import _native as N
from allreducetopk_amd.bucket import SyntheticBucket, bucket_numel
from allreducetopk_amd.comm_hooks import sparse_hook as SH
from allreducetopk_amd.comm_hooks import sparse_hook_c4 as SH4

SHAPES = [[5], [16, 64], [3, 7], [8, 4, 3, 3]]
RATIO = 0.25
DECAY = 0.5  # error_decay: exact in fp32, and not the large-batch hook's alpha of 1
STREAM = 0x5712
WS_BYTES = 64  # what the two *_workspace_bytes calls answer

KINDS = [("topk", None), ("randk", "torch"), ("randk", "host"), ("randk", "hash")]
EFS = ["noef", "ef14", "ef21"]
SPARSE_TYPES = ["tensor", "row", "column"]
VARIANTS = ["fp32", "bf16", "fp32+wire_dtype", "bf16+error_dtype"]

# parameter names of the entry points the hooks call (include/arctopk.h)
ARGS = {
    "arctopk_sparse_workspace_bytes": "ntensors numels",
    "arctopk_seg_workspace_bytes": "ntensors rows cols k_seg by_column",
    "arctopk_topk_select": "x ntensors offsets numels ks k_off idx vals workspace dtype zero_selected stream",
    "arctopk_randk_select": "x ntensors offsets numels ks k_off seed idx vals workspace dtype zero_selected stream",
    "arctopk_topk_select_ef14": "g E err_in ntensors offsets numels ks k_off idx vals workspace dtype stream",
    "arctopk_randk_select_ef14": "g E err_in ntensors offsets numels ks k_off seed idx vals workspace dtype stream",
    "arctopk_seg_select": "x ntensors offsets rows cols k_seg k_off by_column hashed seed idx vals workspace dtype "
                          "zero_selected stream",
    "arctopk_sparse_gather": "x ntensors offsets ks k_off idx vals dtype stream",
    "arctopk_sparse_residual": "E ntensors offsets ks k_off idx vals ef decay dtype stream",
    "arctopk_sparse_decode": "out numel ntensors offsets ks k_off packed_len idx vals nranks world_size accumulate "
                             "gerr decay dtype stream",
    "arctopk_ef_apply": "x E numel ef err_in dtype stream",
    "arctopk_ef14_fold": "x E numel err_in dtype stream",
    "arctopk_sparse_fold_mixed": "g E D numel ef err_in stream",
    "arctopk_sparse_pack_mixed": "src E numel ntensors offsets ks k_off idx vals ef decay stream",
    "arctopk_sparse_decode_mixed21": "out gE scratch numel ntensors offsets ks k_off packed_len idx vals nranks "
                                     "world_size decay stream",
    "arctopk_sparse_pack_wire16": "values E numel ntensors offsets ks k_off idx vals16 ef decay stream",
    "arctopk_sparse_decode_wire16": "out numel ntensors offsets ks k_off packed_len idx vals16 nranks world_size "
                                    "accumulate gE decay stream",
}
_DT = {torch.float32: "f32", torch.bfloat16: "bf16", torch.int32: "i32", torch.uint8: "u8"}


class Recorder:
    """Stands in for libarctopk, and keeps the trace of one state's calls."""

    def __init__(self):
        self.trace = []
        self.state = None
        self.bucket = None
        self.made = []  # every tensor torch.empty returned during a hook call, kept alive

    def role(self, p) -> str:
        p = int(p or 0)
        if p == 0:
            return "NULL"
        if p == STREAM:
            return "stream"
        st, b = self.state, self.bucket.index()
        named = [("bucket", self.bucket.buffer()), ("error_dict[b]", st.error_dict.get(b)),
                 ("global_error_dict[b]", st.global_error_dict.get(b)), ("scratch", st._mixed_scratch),
                 ("workspace", st._workspace)]
        for name, t in named:
            if t is not None and t.data_ptr() == p:
                return name
        for t in self.made:
            if t.data_ptr() == p:
                kind = "indices" if t.dtype == torch.int32 else "values"
                return f"{kind}.{_DT[t.dtype]}[{t.numel()}]"
        return "unknown"

    def __getattr__(self, name):
        if not name.startswith("arctopk_"):
            raise AttributeError(name)
        names = ARGS[name].split()
        types_ = N._SIGS[name][1]

        def fn(*args):
            assert len(args) == len(names) == len(types_), name
            rec = {}
            for key, ty, a in zip(names, types_, args):
                if ty is ctypes.c_void_p:
                    rec[key] = self.role(a)
                elif ty is ctypes.c_float:
                    rec[key] = float(a)
                elif ty in (ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64):
                    rec[key] = int(a)
                else:  # an int64 array, or NULL
                    rec[key] = "NULL" if a is None else [int(v) for v in a]
            self.trace.append({"call": name, **rec})
            return WS_BYTES if name.endswith("_workspace_bytes") else 0

        return fn

    # the collectives
    def all_reduce(self, tensor, group=None, async_op=False):
        assert not async_op
        self.trace.append({"coll": "all_reduce", "dtype": _DT[tensor.dtype], "numel": tensor.numel(),
                           "buf": self.role(tensor.data_ptr())})

    def all_gather_flat(self, out, inp, group, world_size):
        self.trace.append({"coll": "all_gather", "dtype": _DT[inp.dtype], "numel": inp.numel(),
                           "out_numel": out.numel(), "buf": self.role(inp.data_ptr())})


def _digest(t: torch.Tensor) -> str:
    return hashlib.sha1(t.numpy().tobytes()).hexdigest()[:16]


def snapshot(st) -> dict:
    """What a hook call leaves in the state."""
    return {"comm_bits_this_round": int(st.comm_bits_this_round), "iter": int(st.iter),
            "mixed_calls": int(st.mixed_calls), "wire16_calls": int(st.wire16_calls),
            "last_k": [int(k) for k in getattr(st, "last_k", [])],
            "error_dtype": {int(b): _DT[t.dtype] for b, t in st.error_dict.items()},
            "global_error_dtype": {int(b): _DT[t.dtype] for b, t in st.global_error_dict.items()},
            "mixed_buckets": sorted(st._mixed_buckets),
            "cpu_rng": _digest(torch.get_rng_state()), "state_rng": _digest(st.rng.get_state())}


@contextlib.contextmanager
def patched(rec: Recorder):
    """libarctopk, the stream query, the is-CUDA check and the collectives replaced by ``rec``."""
    real_empty = torch.empty

    def empty(*a, **kw):
        t = real_empty(*a, **kw).zero_()
        rec.made.append(t)
        return t

    def check_compressible(state, input_tensor):
        if state.sparse_type not in ("tensor", "row", "column") or input_tensor.dtype not in N.DTYPE_CODE:
            raise ValueError("not compressible")

    saved = [(N, "lib", N.lib), (torch.cuda, "current_stream", torch.cuda.current_stream),
             (torch, "empty", real_empty), (SH, "_check_compressible", SH._check_compressible),
             (dist, "all_reduce", dist.all_reduce), (dist, "get_rank", dist.get_rank),
             (SH, "_all_gather_flat", SH._all_gather_flat)]
    N.lib = lambda: rec
    torch.cuda.current_stream = lambda device=None: types.SimpleNamespace(cuda_stream=STREAM)
    torch.empty = empty
    SH._check_compressible = check_compressible
    dist.all_reduce = rec.all_reduce
    dist.get_rank = lambda group=None: 0
    SH._all_gather_flat = rec.all_gather_flat
    try:
        yield
    finally:
        for obj, name, val in saved:
            setattr(obj, name, val)


def make_state(kind, source, ef, sparse_type, variant, ws, c4=False, **kw):
    cls = SH4.SparseState if c4 else SH.SparseState
    group = types.SimpleNamespace(size=lambda: ws)
    st = cls(group, compress_ratio=RATIO, start_compress_iter=kw.pop("start_compress_iter", 0),
             sparse_type=sparse_type, random=kind == "randk", use_error_feedback=ef, random_seed=7,
             index_source=source or "torch", **kw)
    st.error_decay = DECAY
    st.error_dtype = torch.float32 if variant == "bf16+error_dtype" else None
    st.wire_dtype = torch.bfloat16 if variant == "fp32+wire_dtype" else None
    return st


def run_case(kind, source, ef, sparse_type, variant, ws, ncalls=2, c4=False, large_batch=False):
    """The traces of ``ncalls`` hook calls of one fresh state on bucket 0: per call the list of
    native calls and collectives in order, ending in the state's snapshot (or the exception's name)."""
    rec = Recorder()
    dtype = torch.float32 if variant.startswith("fp32") else torch.bfloat16
    hook = SH4.sparse_hook_sync if c4 else SH.sparse_hook_sync
    log = logging.getLogger(SH.__name__)
    level = log.level
    out = []
    with patched(rec):
        torch.manual_seed(1234)
        st = make_state(kind, source, ef, sparse_type, variant, ws, c4=c4,
                        **({"start_compress_iter": 2} if large_batch else {}))
        if large_batch:
            st.large_batch_init = True
            log.setLevel(logging.INFO)  # the diff log, and with it on_values
        rec.state = st
        try:
            for i in range(ncalls):
                G = torch.ones(bucket_numel(SHAPES), dtype=dtype) * (i + 1)
                rec.bucket = SyntheticBucket(G, SHAPES, index=0)
                rec.trace, rec.made = [], []
                try:
                    fut = hook(st, rec.bucket)
                    assert fut.done() and fut.value() is G
                except TypeError as e:  # the large-batch hook's iteration 0
                    rec.trace.append({"raised": type(e).__name__})
                out.append(rec.trace + [{"state": snapshot(st)}])
        finally:
            log.setLevel(level)
    return out


def matrix():
    """(case id, arguments of run_case) of everything the test and the dump cover."""
    for (kind, source), ef, sp, variant, ws in itertools.product(KINDS, EFS, SPARSE_TYPES, VARIANTS, (1, 2)):
        cid = f"{kind}-{source}-{ef}-{sp}-{variant}-ws{ws}"
        yield cid, dict(kind=kind, source=source, ef=ef, sparse_type=sp, variant=variant, ws=ws)
    yield "large_batch-topk-ef21-tensor-bf16-ws2", dict(kind="topk", source=None, ef="ef21", sparse_type="tensor",
                                                      variant="bf16", ws=2, ncalls=4, large_batch=True)
    for variant in VARIANTS:
        yield f"c4-randk-hash-ef14-row-{variant}-ws2", dict(kind="randk", source="hash", ef="ef14", sparse_type="row",
                                                           variant=variant, ws=2, c4=True)


if __name__ == "__main__":
    for cid, kw in matrix():
        for i, trace in enumerate(run_case(**kw)):
            print(json.dumps({"case": cid, "call": i, "trace": trace}, sort_keys=True))
