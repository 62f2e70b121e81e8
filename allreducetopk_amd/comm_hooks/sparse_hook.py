"""TopK / RandK DDP comm hooks on MI355X -- drop-in for the reference's
comm_hooks/sparse_hook.py (``SparseState`` :127-160, ``cal_k`` :77-78,
``sparse_hook_sync`` :163-304).

Per bucket call (all on the caller's stream, no host synchronisation):

    ef_apply        (EF14: x += E, E = x | EF21: x -= E), one fused pass
    TopK : topk_select  exact element top-k of |x| per tensor (radix select),
                        ascending int32 indices + gathered values
    RandK: indices      torch.randperm(numel, device)[:k] after the shared reseed
                        (index_source="torch": the reference's own draw on a GPU), the
                        same draw on the CPU generator (index_source="host": the reference
                        run on CPU, as the golden vectors were made), then gather; or
                        (index_source="hash", perf mode) the k largest keyed-hash keys per
                        tensor -- a uniform k-subset -- through the TopK radix select:
                        ascending indices, gather (and EF14's E[idx] = 0) in its last pass
    residual        EF14: E[idx] = 0 | EF21: E[idx] += values
    RandK: all_reduce(values)              -> decode: zero + scatter(values / ws)
                                              (hash: one pass over whole chunks)
    TopK : all_gather(values), all_gather(indices)
                                           -> decode: zero + rank-ordered scatter-add, / ws
    EF21: gE += out; out = gE (fused into decode)

``sparse_type`` "row" / "column" (the reference's sparsify_by_row / sparsify_by_column, :36-75,
which its hook cannot reach: 2 values are unpacked where 3 are expected, :54, :75, :96) select per
row / per column of every tensor with the segmented select (arctopk_seg_select):

    2-D [R, C]   row: every row takes max(1, int(C * ratio)) entries; column: every column takes
                 max(1, int(R * ratio)) entries (cal_k_by_row / cal_k_by_column)
    1-D          one segment: exactly what "tensor" does (a RandK state draws RandK here too; the
                 reference forgets to forward ``random`` for 1-D tensors)
    N-D, N >= 3  viewed as [shape[0], numel / shape[0]] (the reference's ``num_rows, num_cols =
                 tensor.shape`` raises): a conv weight selects per output channel in row mode
    payload      int32 flat indices into the tensor; row: segment-major, ascending; column: the
                 reference's [k_seg, C] layout (entry j of column c at j * C + c)
    RandK        "torch" / "host": one torch.randperm(C)[:k] per row (column: randperm(R)[:k] per
                 column) in the reference's order; "hash": per segment s of tensor t the k largest
                 keys rk(hseed(t, s), j) (include/arctopk.h)
    EF14         arctopk_ef14_fold, then the select on E with the selected elements zeroed

Ties at the k-th |x| resolve lowest-index first.

Residuals are kept in the bucket's dtype by default: the bf16 entry points round after every add,
as the reference's torch ops do.  ``SparseState.error_dtype = torch.float32`` (DESIGN.md section
4g, not in the reference; environment default ``ARCTOPK_SPARSE_ERROR_DTYPE=fp32``) keeps a bf16
bucket's ``error_dict[b]`` -- and under EF21 ``global_error_dict[b]`` -- in fp32, as
``GroupTopKState.error_dtype`` / ``ef21_error_dtype`` do for ARC-TopK.  Such a call runs

    fold    arctopk_sparse_fold_mixed   EF14: E := f(G) + E | EF21: D := f(G) - E (fp32 scratch)
    select  the fp32 selects above on E / D (TopK's selection is finer than the bf16 path's);
            RandK's indices are the same draws
    pack    arctopk_sparse_pack_mixed   values = b(X); EF14: E := X - f(values), the remainder of
            the rounding, at the selected elements | EF21: E := fma(decay, f(values), E)
    decode  EF14: the bf16 decode above | EF21: arctopk_sparse_decode_mixed21: fp32 rank-ordered
            sums, gE := fma(decay, sum / ws, gE), out = b(gE)

in the default path's skeleton (``_compress_exchange(mixed=True)``), with its bf16 wire, index
exchange and bit accounting.  The option is ignored for fp32 buckets and "noef", and refused with
``large_batch_init`` on a bf16 bucket.

``SparseState.wire_dtype = torch.bfloat16`` (not in the reference; environment
default ``ARCTOPK_SPARSE_WIRE_DTYPE=bf16``) sends an fp32 bucket's values as bf16, as
``GroupTopKState.wire_dtype`` does for ARC-TopK: RandK's all-reduce carries half the bytes, TopK's
all-gathers three quarters (the indices stay int32).  Fold and selection are the fp32 path's, bit
for bit; behind them such a call runs

    pack    arctopk_sparse_pack_wire16  vals16 = b(values); EF14: E[idx] := values - f(vals16), the
            remainder of the rounding | EF21: E[idx] := fma(decay, f(vals16), E[idx])
            (in place of arctopk_sparse_residual); the exchange above then carries vals16
    decode  arctopk_sparse_decode_wire16  fp32 rank-ordered sums of f(vals16), / ws, EF21's gE; where
            every tensor's indices ascend (TopK, RandK "hash"; not the column layout) one block
            composes a whole chunk from all ranks in LDS and writes it once

also at world size 1, so one GPU produces what a rank of N would.  Residuals stay plain fp32.  The
option is ignored for bf16 buckets (their wire is bf16 already), in the dense warm-up calls and in
EF21's dense first call of a bucket, and refused with ``large_batch_init`` on an fp32 bucket.
"""

import logging
import os
from typing import Dict, List

import torch
import torch.distributed as dist

from allreducetopk_amd import _native as N
from allreducetopk_amd.comm_hooks import default_hooks
from allreducetopk_amd.comm_hooks.group_topk_hook_no_reshape import _residual_on
from allreducetopk_amd.comm_hooks.utils import (HookState, _get_allgather_out_list, dtype_bits,
                                                tensor_bits)

logger = logging.getLogger(__name__)

__all__ = ["SparseState", "sparse_hook_sync", "cal_k", "cal_k_by_row", "cal_k_by_column"]


def cal_k(tensor, compress_ratio):
    """k of a tensor (ref sparse_hook.py:77-78)."""
    return max(1, int(tensor.numel() * compress_ratio))


def _view_2d(shape):
    """(rows, cols) of a tensor for row / column selection; None for one segment (<= 1-D).
    N-D tensors are viewed as [shape[0], numel / shape[0]]."""
    if len(shape) <= 1:
        return None
    n = 1
    for d in shape:
        n *= int(d)
    rows = int(shape[0])
    return rows, n // max(rows, 1)


def cal_k_by_row(tensor, compress_ratio):
    """Entries of a tensor under sparse_type="row" (ref sparse_hook.py:80-84; N-D: per shape[0])."""
    v = _view_2d(tensor.shape)
    if v is None:
        return cal_k(tensor, compress_ratio)
    return max(1, int(v[1] * compress_ratio)) * v[0]


def cal_k_by_column(tensor, compress_ratio):
    """Entries of a tensor under sparse_type="column" (ref sparse_hook.py:86-90; N-D as above)."""
    v = _view_2d(tensor.shape)
    if v is None:
        return cal_k(tensor, compress_ratio)
    return max(1, int(v[0] * compress_ratio)) * v[1]


class SparseState(HookState):
    """State of the TopK/RandK hook (reference sparse_hook.py:127-160)."""

    def __init__(self, process_group: dist.ProcessGroup, compress_ratio: float = 0.01,
                 start_compress_iter: int = 2, sparse_type: str = "row", random: bool = False,
                 use_error_feedback: str = "noef", random_seed: int = 0,
                 index_source: str = "torch"):
        super().__init__(process_group)
        self.total_bit_before_compression = 0
        self.total_bit_after_compression = 0
        self.compress_ratio = compress_ratio
        self.iter = 0
        self.start_compress_iter = start_compress_iter
        self.error_decay = 1.0
        self.large_batch_init = False
        self.sparse_type = sparse_type
        self.compressor_name = f"{sparse_type}-wise sparsification"
        self.random = random
        self.rng = torch.Generator()
        self.rng.manual_seed(random_seed)
        self.use_error_feedback = use_error_feedback
        self.error_dict: Dict[int, torch.Tensor] = {}
        self.global_error_dict: Dict[int, torch.Tensor] = {}
        self.random_seed = random_seed
        if index_source not in ("torch", "host", "hash"):
            raise ValueError("index_source must be 'torch', 'host' or 'hash'")
        self.index_source = index_source
        self._workspace = None
        self._ws_bytes: Dict[tuple, int] = {}
        self._seg_geom: Dict[tuple, "_SegGeometry"] = {}  # row / column: per bucket layout and ratio
        self._fold_in = None  # RandK "hash" under EF14: the select applies E (1) or the first-call copy (2)
        # Residual dtype (not in the reference): None keeps E (and EF21's gE) in
        # the bucket's dtype; torch.float32 keeps them in fp32 under a bf16 bucket (4 B, under EF21
        # 8 B, per element of a 2-B bucket, plus EF21's fp32 scratch of the largest bucket), so unsent
        # mass below 2^-9 of a residual element is carried instead of rounded away.  One option for
        # both EF modes; ignored for fp32 buckets and noef.
        env = os.environ.get("ARCTOPK_SPARSE_ERROR_DTYPE", "")
        if env not in ("", "fp32"):
            raise ValueError(f"ARCTOPK_SPARSE_ERROR_DTYPE must be 'fp32' (or unset), got {env!r}")
        self.error_dtype = torch.float32 if env == "fp32" else None
        self.mixed_calls = 0  # compressed calls that ran with fp32 residuals under a bf16 bucket
        self._mixed_buckets = set()  # ... and the buckets whose residuals are such
        self._mixed_scratch = None  # EF21: D = f(G) - E, then the decode's fp32 sums (grown, never shrunk)
        # Wire dtype (not in the reference): None sends an fp32 bucket's values
        # as fp32; torch.bfloat16 sends them as bf16 and keeps the rounding remainder of what was sent
        # in the residual.  Ignored for bf16 buckets.
        env = os.environ.get("ARCTOPK_SPARSE_WIRE_DTYPE", "")
        if env not in ("", "bf16"):
            raise ValueError(f"ARCTOPK_SPARSE_WIRE_DTYPE must be 'bf16' (or unset), got {env!r}")
        self.wire_dtype = torch.bfloat16 if env == "bf16" else None
        self.wire16_calls = 0  # compressed calls that sent bf16 values of an fp32 bucket

    # ratio of this call; the c4 variant overrides (gradual compression)
    def _call_ratio(self) -> float:
        return self.compress_ratio

    def _on_compression_start(self):
        pass

    def _mixed_residual(self, bucket_dtype, ef: int) -> bool:
        """Whether this call keeps fp32 residuals under a bf16 bucket.  ValueError for an
        ``error_dtype`` other than None / torch.float32; ignored for fp32 buckets and without
        error feedback."""
        ed = self.error_dtype
        if ed is not None and ed is not torch.float32:
            raise ValueError(f"error_dtype must be None or torch.float32, got {ed!r}")
        return ed is not None and bucket_dtype == torch.bfloat16 and ef != N.EF_NONE

    def _wire16(self, bucket_dtype) -> bool:
        """Whether this call sends bf16 values of an fp32 bucket.  ValueError for a ``wire_dtype``
        other than None / torch.bfloat16; ignored for bf16 buckets."""
        wd = self.wire_dtype
        if wd is not None and wd is not torch.bfloat16:
            raise ValueError(f"wire_dtype must be None or torch.bfloat16, got {wd!r}")
        return wd is not None and bucket_dtype == torch.float32

    def state_dict(self) -> dict:
        out = super().state_dict()
        # for information: the residuals are plain fp32 either way, so loading needs no rule
        out["wire_dtype"] = "bf16" if self.wire_dtype is torch.bfloat16 else None
        # the residual dtype option, and the buckets whose fp32 residuals belong to a bf16 bucket
        out["error_dtype"] = "fp32" if self.error_dtype is torch.float32 else None
        out["mixed_buckets"] = sorted(self._mixed_buckets)
        return out

    def load_state_dict(self, sd: dict, device=None) -> None:
        """As HookState.load_state_dict.  A checkpoint written with ``error_dtype=torch.float32``
        (fp32 residuals of bf16 buckets) loads only into a state that has the option set: ValueError
        otherwise, since rounding those residuals to bf16 would drop what they exist to carry.  The
        other way round -- bf16 residuals into a state with the option -- converts them to fp32,
        which is exact."""
        mixed = [int(b) for b in sd.get("mixed_buckets", ())]
        if mixed and self.error_dtype is not torch.float32:
            raise ValueError(f"the checkpoint holds float32 residuals of bfloat16 buckets {mixed} "
                             "(error_dtype=torch.float32): set error_dtype=torch.float32 on this state "
                             "before loading it")
        super().load_state_dict(sd, device)
        self._mixed_buckets = set(mixed)
        if self.error_dtype is torch.float32 and self.use_error_feedback != "noef":
            for table in (self.error_dict, self.global_error_dict):
                for b, t in table.items():
                    if t.dtype == torch.bfloat16:
                        table[b] = t.float()
                        self._mixed_buckets.add(int(b))


def _workspace(state, device, numels) -> torch.Tensor:
    """Select workspace for this bucket's tensor sizes (grown, never shrunk)."""
    key = tuple(numels)
    nbytes = state._ws_bytes.get(key)
    if nbytes is None:
        nbytes = int(N.lib().arctopk_sparse_workspace_bytes(len(numels), N.i64_array(numels)))
        if nbytes < 0:
            N.check(-nbytes, "arctopk_sparse_workspace_bytes")
        state._ws_bytes[key] = nbytes
    ws = state._workspace
    if ws is None or ws.device != device or ws.numel() < nbytes:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        state._workspace = ws
    return ws


class _SegGeometry:
    """Row / column geometry of one bucket layout at one ratio: per tensor the [rows, cols] view,
    the entries per segment, the tensor's total (``ks``) and its offset in the payload."""

    def __init__(self, shapes, ratio: float, by_column: bool):
        self.by_column = by_column
        self.rows, self.cols, self.k_seg, self.ks, self.k_off = [], [], [], [], []
        acc = 0
        for shape in shapes:
            v = _view_2d(shape)
            if v is None:  # one segment; a column of n rows is the same contiguous segment
                n = int(shape[0]) if len(shape) else 1
                r, c = (n, 1) if by_column else (1, n)
            else:
                r, c = v
            seg_len, nseg = (r, c) if by_column else (c, r)
            k = max(1, int(seg_len * ratio))
            self.rows.append(r)
            self.cols.append(c)
            self.k_seg.append(k)
            self.ks.append(k * nseg)
            self.k_off.append(acc)
            acc += k * nseg
        self.sum_k = acc
        self.a_rows, self.a_cols, self.a_kseg = (N.i64_array(self.rows), N.i64_array(self.cols),
                                                 N.i64_array(self.k_seg))
        self.ws_bytes = int(N.lib().arctopk_seg_workspace_bytes(len(self.rows), self.a_rows, self.a_cols,
                                                                self.a_kseg, int(by_column)))
        if self.ws_bytes < 0:
            N.check(-self.ws_bytes, "arctopk_seg_workspace_bytes")


def _seg_geometry(state, tensors, ratio: float) -> _SegGeometry:
    key = (tuple(tuple(t.shape) for t in tensors), float(ratio), state.sparse_type)
    g = state._seg_geom.get(key)
    if g is None:
        g = state._seg_geom[key] = _SegGeometry(key[0], ratio, state.sparse_type == "column")
    return g


def _seg_reference_draws(g: _SegGeometry, device) -> torch.Tensor:
    """RandK "torch" / "host" under row / column: the reference's draws in its order
    (sparsify_by_row :46, sparsify_by_column :66, sparsify :20), as int32 flat indices.
    device None: the CPU generator."""
    kw = {} if device is None else {"device": device}
    parts = []
    for r, c, k in zip(g.rows, g.cols, g.k_seg):
        if g.by_column and c > 1:
            idx = torch.stack([torch.randperm(r, **kw)[:k] for _ in range(c)], dim=1)
            idx = idx * c + torch.arange(c, **kw).unsqueeze(0)
        elif not g.by_column and r > 1:
            idx = torch.stack([torch.randperm(c, **kw)[:k] for _ in range(r)], dim=0)
            idx = idx + torch.arange(r, **kw).unsqueeze(1) * c
        else:
            idx = torch.randperm(r * c, **kw)[:k]
        parts.append(idx.flatten().to(torch.int32))
    return torch.cat(parts)


def _done(state: SparseState, bucket, tensor) -> "torch.futures.Future[torch.Tensor]":
    """The end of a synchronous hook call: the iteration counter, and a completed Future."""
    state.maybe_increase_iter(bucket)
    fut = torch.futures.Future()
    fut.set_result(tensor)
    return fut


def _reseed(state: SparseState):
    """RandK's shared reseed, so every rank draws the same indices (:230-235); None for TopK."""
    if not state.random:
        return None
    seed = torch.randint(0, 1_000_000_000, (1,), generator=state.rng).item()
    torch.manual_seed(seed)
    return seed


def _sparse_hook_impl(state: SparseState, bucket, c4: bool = False) -> "torch.futures.Future[torch.Tensor]":
    if state.use_error_feedback == "ef21" and state.large_batch_init:
        # (sparse_hook.py:172-175, sparse_hook_c4.py:201-204)
        if state.iter < state.start_compress_iter:
            logger.info("Using large batch initialization in EF21!!")
        if state._mixed_residual(bucket.buffer().dtype, N.EF21):
            raise ValueError("error_dtype=torch.float32 does not run with large_batch_init: that hook "
                             "keeps a bfloat16 bucket's residuals in bfloat16")
        if state._wire16(bucket.buffer().dtype):
            raise ValueError("wire_dtype=torch.bfloat16 does not run with large_batch_init: that hook "
                             "keeps a float32 bucket's float32 wire")
        return _large_batch_ef21(state, bucket, c4)
    state.maybe_accumulate_momentum_on_bucket(bucket)
    group = state.process_group if state.process_group is not None else dist.group.WORLD
    world_size = group.size()
    input_tensor = bucket.buffer()

    if state.iter < state.start_compress_iter:  # (:190-193)
        state.maybe_increase_iter(bucket)
        return default_hooks._allreduce_fut(group, input_tensor, state)

    state._on_compression_start()
    _check_compressible(state, input_tensor)
    L = N.lib()
    device = input_tensor.device
    dtype = input_tensor.dtype
    b = bucket.index()
    total = input_tensor.shape[0]
    stream = torch.cuda.current_stream(device).cuda_stream
    ef = N.EF_CODE[state.use_error_feedback]
    dt = N.DTYPE_CODE[dtype]
    # EF21 residual scaling: E += error_decay * C(D), gE += error_decay * out (:265, :296)
    decay = float(state.error_decay)
    wire16 = state._wire16(dtype)  # bf16 values of this fp32 bucket on the wire (wire_dtype)
    mixed = state._mixed_residual(dtype, ef)  # fp32 residuals under this bf16 bucket (error_dtype)

    if ef == N.EF21 and b not in state.error_dict:
        return _ef21_dense_first_call(state, bucket, group, world_size, mixed)
    state._fold_in = None  # EF14's err_in where the select folds E itself
    if mixed:
        _mixed_fold(state, bucket, ef, stream)
    elif ef == N.EF14:
        err_in = b in state.error_dict
        if not err_in:
            logger.info("A zero tensor of length %s that represents local error is created.", total)
            state.error_dict[b] = torch.zeros(total, device=device, dtype=dtype)
        err = _residual_on(state.error_dict, b, input_tensor, "error_dict")
        # E := G + E (:205, :258); selection and gathers then read the pre-compression bucket
        # from E, and the decode writes the bucket once.  RandK's device draw folds E itself in
        # its write pass (arctopk_randk_select_ef14: its keys never read the data)
        # (and fp32 TopK folds it in its first pass: arctopk_topk_select_ef14)
        if _select_folds(state, dtype) and state.sparse_type == "tensor":
            state._fold_in = int(err_in)
        else:
            N.check(L.arctopk_ef14_fold(input_tensor.data_ptr(), err.data_ptr(), total, int(err_in),
                                        dt, stream), "arctopk_ef14_fold")
    elif ef == N.EF21:
        err = _residual_on(state.error_dict, b, input_tensor, "error_dict")
        _residual_on(state.global_error_dict, b, input_tensor, "global_error_dict")
        N.check(L.arctopk_ef_apply(input_tensor.data_ptr(), err.data_ptr(),
                                   total, N.EF21, 1, dt, stream), "arctopk_ef_apply")

    _compress_exchange(state, bucket, group, world_size, ef, state._call_ratio(), _reseed(state),
                       e_decay=decay, g_decay=decay, count_bits=True, ef14_folded=ef == N.EF14, wire16=wire16,
                       mixed=mixed)
    state.wire16_calls += int(wire16)
    state.mixed_calls += int(mixed)
    return _done(state, bucket, input_tensor)


def _ef21_dense_first_call(state: SparseState, bucket, group, world_size: int,
                           mixed: bool) -> "torch.futures.Future[torch.Tensor]":
    """EF21's first call of a bucket (:213-226): E_0 = G, the bucket is all-reduced and averaged,
    gE_0 = out.  ``mixed``: both are kept as fp32 copies of the bf16 bucket (``error_dtype``)."""
    input_tensor = bucket.buffer()
    b = bucket.index()

    def keep(t):  # a copy of its own either way: bf16 -> fp32 converts, so it copies
        return t.to(torch.float32, copy=True) if mixed else torch.clone(t).detach()

    logger.info("A tensor of length %s that represents local/global error is created.", input_tensor.shape[0])
    state.error_dict[b] = keep(input_tensor)
    dist.all_reduce(input_tensor, group=group, async_op=False)
    input_tensor.div_(world_size)
    state.global_error_dict[b] = keep(input_tensor)
    if mixed:
        state._mixed_buckets.add(int(b))
    return _done(state, bucket, input_tensor)


def _mixed_fold(state: SparseState, bucket, ef: int, stream) -> None:
    """The EF pre-apply of a bf16 bucket whose residuals are fp32 (``error_dtype``, DESIGN.md section
    4g): the residuals' bookkeeping and arctopk_sparse_fold_mixed.  EF14: X = f(G) + E then lives in
    E; EF21: D = f(G) - E lives in the state's fp32 scratch, which the decode reuses for its sums."""
    input_tensor = bucket.buffer()
    device = input_tensor.device
    b = bucket.index()
    total = input_tensor.shape[0]
    f32 = torch.float32
    err_in = b in state.error_dict
    if not err_in:  # EF14's first call: the fold writes every element
        logger.info("A zero tensor of length %s that represents local error is created.", total)
        state.error_dict[b] = torch.empty(total, device=device, dtype=f32)
        state._mixed_buckets.add(int(b))
    err = _residual_on(state.error_dict, b, input_tensor, "error_dict", f32)
    scratch = None
    if ef == N.EF21:
        _residual_on(state.global_error_dict, b, input_tensor, "global_error_dict", f32)
        scratch = state._mixed_scratch
        if scratch is None or scratch.device != device or scratch.numel() < total:
            scratch = state._mixed_scratch = torch.empty(total, dtype=f32, device=device)
    N.check(N.lib().arctopk_sparse_fold_mixed(input_tensor.data_ptr(), err.data_ptr(), N.ptr(scratch), total, ef,
                                              int(err_in), stream), "arctopk_sparse_fold_mixed")


def _select_folds(state: SparseState, dtype) -> bool:
    """EF14's E := G + E is applied by the select itself (RandK's device draw: in its write pass;
    fp32 TopK: in its first histogram pass), not by a fold pass of its own."""
    if state.random:
        return state.index_source == "hash"
    return dtype == torch.float32


def _check_compressible(state: SparseState, input_tensor: torch.Tensor) -> None:
    if state.sparse_type not in ("tensor", "row", "column"):
        raise ValueError(f"sparse_type must be 'tensor', 'row' or 'column', not {state.sparse_type!r}")
    if not input_tensor.is_cuda or input_tensor.dtype not in N.DTYPE_CODE:
        raise RuntimeError("sparse HIP codec needs a float32 or bfloat16 bucket on a GPU")


def _bucket_layout(state: SparseState, input_tensor, tensors, ratio: float):
    """(row / column geometry or None, numels, ks, element offsets, k offsets, sum of ks) of a
    bucket's tensors at this call's ratio."""
    numels = [t.numel() for t in tensors]
    # row / column: per-segment selection; ks are then the per-tensor totals
    seg = _seg_geometry(state, tensors, ratio) if state.sparse_type != "tensor" else None
    ks = seg.ks if seg is not None else [max(1, int(n * ratio)) for n in numels]
    offsets: List[int] = []
    off = 0
    for t in tensors:
        if (t.data_ptr() - input_tensor.data_ptr()) // input_tensor.element_size() != off:
            raise RuntimeError("bucket gradient views must tile the buffer in order")
        offsets.append(off)
        off += t.numel()
    k_off: List[int] = []
    acc = 0
    for k in ks:
        k_off.append(acc)
        acc += k
    return seg, numels, ks, offsets, k_off, acc


def _reference_draws(state: SparseState, indices: torch.Tensor, seg, numels, ks, k_off) -> None:
    """RandK "torch" / "host": the reference's own draws (:20; row / column: _seg_reference_draws)
    into ``indices``, per tensor in order.  "torch" draws on the bucket's device; "host" (parity
    mode: the reference run on CPU, sparse_hook_c4.py:20 with CPU tensors, after the reseed at
    :269-274) draws from the CPU generator in the same order, so that generator is left where the
    reference leaves it, and copies the draws to the device once."""
    on_device = state.index_source == "torch"
    if seg is not None:
        indices.copy_(_seg_reference_draws(seg, indices.device if on_device else None))
        return
    kw = {"device": indices.device} if on_device else {}
    out = indices if on_device else torch.empty(indices.numel(), dtype=torch.int32)
    for n, k, ko in zip(numels, ks, k_off):
        out[ko:ko + k].copy_(torch.randperm(n, **kw)[:k])
    if not on_device:
        indices.copy_(out)


def _seg_workspace(state: SparseState, seg: _SegGeometry, device) -> torch.Tensor:
    """Segmented-select workspace of this geometry (the state's one workspace, grown, never shrunk)."""
    ws = state._workspace
    if ws is None or ws.device != device or ws.numel() < seg.ws_bytes:
        ws = state._workspace = torch.empty(seg.ws_bytes, dtype=torch.uint8, device=device)
    return ws


def _exchange(state: SparseState, group, world_size: int, values, indices, value_bits: int, count_bits: bool,
              *, hashed: bool, by_column: bool):
    """The exchange of one compressed call, and its bit accounting (``count_bits``).  RandK:
    all-reduce of the values, every rank holding the same indices; TopK: all-gather of values and
    indices.  Returns what the decode reads: (values, indices, nranks, accumulate code).
    RandK "hash" outside the column layout: every tensor's indices ascend, so the decode may compose
    whole chunks in one pass (accumulate 2)."""
    sum_k = indices.numel()
    if state.random:
        if count_bits:
            state.comm_bits_this_round += 2 * (world_size - 1) * sum_k * value_bits
        if world_size > 1:
            dist.all_reduce(values, group=group, async_op=False)
        return values, indices, 1, 2 if hashed and not by_column else 0
    if count_bits:
        state.comm_bits_this_round += (world_size - 1) * world_size * sum_k * (value_bits + 32)
    if world_size > 1:
        all_vals = torch.empty(world_size * sum_k, dtype=values.dtype, device=values.device)
        all_idx = torch.empty(world_size * sum_k, dtype=torch.int32, device=values.device)
        _all_gather_flat(all_vals, values, group, world_size)
        _all_gather_flat(all_idx, indices, group, world_size)
        values, indices = all_vals, all_idx  # (gathering from one rank is the identity)
    return values, indices, world_size, 3 if by_column else 1


def _compress_exchange(state: SparseState, bucket, group, world_size: int, ef: int, ratio: float,
                       seed, e_decay: float, g_decay: float, count_bits: bool, on_values=None,
                       ef14_folded: bool = False, wire16: bool = False, mixed: bool = False) -> None:
    """The compressed call after the EF pre-apply, on the caller's stream: select (TopK) or draw
    (RandK) the indices, gather the values, persist the residual (EF14: E[idx] = 0; EF21:
    E[idx] += e_decay * values), exchange (RandK: all-reduce; TopK: all-gather of values and
    indices) and decode into the bucket (EF21: gE += g_decay * out, out = gE).
    ``sparse_type`` "row" / "column": the per-segment select (arctopk_seg_select) with the tensors'
    totals as ``ks``; under EF14 the caller has folded E := G + E already and says so with
    ``ef14_folded`` (the tensor path's fused folds go by ``state._fold_in`` as before).
    ``wire16`` (an fp32 bucket under ``wire_dtype=torch.bfloat16``): after the unchanged select,
    arctopk_sparse_pack_wire16 rounds the values to bf16 and writes the residual in place of
    arctopk_sparse_residual; the values travel and count as 16 bits; arctopk_sparse_decode_wire16
    decodes.
    ``mixed`` (a bf16 bucket under ``error_dtype=torch.float32``, after _mixed_fold): the selects
    read fp32 from E (EF14) or the scratch (EF21) and leave E alone; their own fp32 gather goes
    unused, and the reference draws and "hash" run none: arctopk_sparse_pack_mixed rounds the bf16
    values from the source and writes the residual; EF21 decodes with arctopk_sparse_decode_mixed21.
    Reference: sparse_hook.py:237-297 (and :363-410 for the large-batch hook)."""
    L = N.lib()
    input_tensor = bucket.buffer()
    tensors = bucket.gradients()
    device = input_tensor.device
    dtype = input_tensor.dtype
    b = bucket.index()
    total = input_tensor.shape[0]
    stream = torch.cuda.current_stream(device).cuda_stream
    dt = N.DTYPE_CODE[dtype]
    seg, numels, ks, offsets, k_off, sum_k = _bucket_layout(state, input_tensor, tensors, ratio)
    nt = len(tensors)
    fold14 = ef == N.EF14  # the pre-compression bucket lives in E (arctopk_ef14_fold)
    if seg is not None and fold14 and not ef14_folded:
        raise RuntimeError("row / column selection under EF14 needs the caller's arctopk_ef14_fold")
    hashed = state.random and state.index_source == "hash"
    drawn = state.random and not hashed  # the reference's own draws
    value_bits = 16 if wire16 else dtype_bits(dtype)
    a_off, a_n, a_k, a_ko = (N.i64_array(offsets), N.i64_array(numels), N.i64_array(ks),
                             N.i64_array(k_off))
    values = torch.empty(sum_k, dtype=dtype, device=device)
    indices = torch.empty(sum_k, dtype=torch.int32, device=device)
    x = input_tensor.data_ptr()
    err = state.error_dict[b].data_ptr() if ef != N.EF_NONE else None
    # what a select reads, as which dtype, where it gathers to, whether it zeroes EF14's E[idx]
    # (:104) in its last pass, and EF14's err_in where it also folds E := G + E (:205) itself
    if mixed:
        src = err if fold14 else state._mixed_scratch.data_ptr()
        sel_vals, sel_dt, zero, fold_in = None, N.F32, 0, None  # (sel_vals: allocated where a select gathers)
    else:
        src = err if fold14 else x
        sel_vals, sel_dt, zero, fold_in = values, dt, int(fold14), state._fold_in if fold14 else None
    if drawn:
        _reference_draws(state, indices, seg, numels, ks, k_off)
        if not mixed:
            N.check(L.arctopk_sparse_gather(src, nt, a_off, a_k, a_ko, indices.data_ptr(),
                                            values.data_ptr(), dt, stream), "arctopk_sparse_gather")
    elif seg is not None:
        ws = _seg_workspace(state, seg, device)
        if mixed:
            sel_vals = torch.empty(sum_k, dtype=torch.float32, device=device)
        N.check(L.arctopk_seg_select(src, nt, a_off, seg.a_rows, seg.a_cols, seg.a_kseg, a_ko,
                                     int(seg.by_column), int(hashed), int(seed) if hashed else 0,
                                     indices.data_ptr(), sel_vals.data_ptr(), ws.data_ptr(), sel_dt, zero, stream),
                "arctopk_seg_select")
    elif hashed:  # the k largest keyed-hash keys per tensor, ascending, gathered in the select
        ws_buf = _workspace(state, device, numels)
        if fold_in is not None:
            N.check(L.arctopk_randk_select_ef14(x, err, fold_in, nt, a_off, a_n, a_k, a_ko, int(seed),
                                                indices.data_ptr(), values.data_ptr(), ws_buf.data_ptr(), dt, stream),
                    "arctopk_randk_select_ef14")
        elif mixed:  # indices only: the keys never read the data
            N.check(L.arctopk_randk_select(None, nt, None, a_n, a_k, a_ko, int(seed), indices.data_ptr(), None,
                                           ws_buf.data_ptr(), N.F32, 0, stream), "arctopk_randk_select")
        else:
            N.check(L.arctopk_randk_select(src, nt, a_off, a_n, a_k, a_ko, int(seed), indices.data_ptr(),
                                           values.data_ptr(), ws_buf.data_ptr(), dt, zero, stream),
                    "arctopk_randk_select")
    else:
        ws_buf = _workspace(state, device, numels)
        if mixed:
            sel_vals = torch.empty(sum_k, dtype=torch.float32, device=device)
        rc = N.EINVAL
        if fold_in is not None:
            rc = L.arctopk_topk_select_ef14(x, err, fold_in, nt, a_off, a_n, a_k, a_ko,
                                            indices.data_ptr(), values.data_ptr(), ws_buf.data_ptr(), dt, stream)
            if rc == N.EINVAL:  # (a tensor not 16-B aligned / of numel % 4 != 0): fold, then select
                N.check(L.arctopk_ef14_fold(x, err, total, fold_in, dt, stream), "arctopk_ef14_fold")
            else:
                N.check(rc, "arctopk_topk_select_ef14")
        if rc == N.EINVAL:
            N.check(L.arctopk_topk_select(src, nt, a_off, a_n, a_k, a_ko, indices.data_ptr(),
                                          sel_vals.data_ptr(), ws_buf.data_ptr(), sel_dt, zero, stream),
                    "arctopk_topk_select")

    # the call's selection, for inspection and tests (int32 indices per tensor, concatenated
    # in bucket order at the k offsets; TopK: ascending within a tensor)
    state.last_indices, state.last_k = indices, ks
    if on_values is not None:
        on_values(values)
    if wire16:  # the values as they travel, and the residual with what the rounding drops
        vals16 = torch.empty(sum_k, dtype=torch.bfloat16, device=device)
        N.check(L.arctopk_sparse_pack_wire16(values.data_ptr(), err, total, nt, a_off, a_k, a_ko, indices.data_ptr(),
                                             vals16.data_ptr(), ef, e_decay, stream), "arctopk_sparse_pack_wire16")
        values = vals16
    elif mixed:
        N.check(L.arctopk_sparse_pack_mixed(src, err, total, nt, a_off, a_k, a_ko, indices.data_ptr(),
                                            values.data_ptr(), ef, e_decay, stream), "arctopk_sparse_pack_mixed")
    elif ef == N.EF21 or (fold14 and drawn):  # residual persistence (:257-267); the selects did EF14's
        N.check(L.arctopk_sparse_residual(err, nt, a_off, a_k, a_ko, indices.data_ptr(), values.data_ptr(), ef,
                                          e_decay, dt, stream), "arctopk_sparse_residual")

    by_column = seg is not None and seg.by_column
    vals, idx, nranks, accumulate = _exchange(state, group, world_size, values, indices, value_bits, count_bits,
                                              hashed=hashed, by_column=by_column)
    gerr = state.global_error_dict[b].data_ptr() if ef == N.EF21 else None
    if wire16:
        N.check(L.arctopk_sparse_decode_wire16(x, total, nt, a_off, a_k, a_ko, sum_k, idx.data_ptr(), vals.data_ptr(),
                                               nranks, world_size, accumulate, gerr, g_decay, stream),
                "arctopk_sparse_decode_wire16")
    elif mixed and ef == N.EF21:  # the fold's scratch is free again: it takes the fp32 sums
        N.check(L.arctopk_sparse_decode_mixed21(x, gerr, src, total, nt, a_off, a_k, a_ko, sum_k, idx.data_ptr(),
                                                vals.data_ptr(), nranks, world_size, g_decay, stream),
                "arctopk_sparse_decode_mixed21")
    else:
        N.check(L.arctopk_sparse_decode(x, total, nt, a_off, a_k, a_ko, sum_k, idx.data_ptr(), vals.data_ptr(),
                                        nranks, world_size, accumulate, gerr, g_decay, dt, stream),
                "arctopk_sparse_decode")


def _large_batch_ef21(state: SparseState, bucket, c4: bool) -> "torch.futures.Future[torch.Tensor]":
    """EF21 with large-batch initialisation (reference sparse_hook.py:307-416; the registered
    copy sparse_hook_c4.py:353-457), reached when ``state.large_batch_init`` is set by hand:

    - iteration 0: the reference calls ``default_hooks._allreduce_fut`` without its required
      ``hook_state`` argument, so it raises TypeError (after advancing ``iter``); so does this;
    - 1 <= iter < start_compress_iter: E += G; the bucket is all-reduced and averaged; gE += it;
    - iter == start_compress_iter: E and gE are divided by start_compress_iter - 1;
    - compressed calls: D = G - E, C(D) at ``compress_ratio`` (never the gradual ratio),
      E += C(D) (alpha 1), the exchange, gE += error_decay * out, out = gE.  No communication
      bits are counted (the reference counts none in this hook).  The registered copy then
      fails in the reference (its ``cal_k(state, tensor)`` is called as ``cal_k(tensor,
      ratio)``: AttributeError, sparse_hook_c4.py:421); with ``c4`` so does this, at the same
      point (after the residual division, the pre-apply and the reseed)."""
    assert state.use_error_feedback == "ef21", "This hook is only for EF21"
    assert state.large_batch_init, "This hook is only for large batch initialization"
    state.maybe_accumulate_momentum_on_bucket(bucket)
    group = state.process_group if state.process_group is not None else dist.group.WORLD
    world_size = group.size()
    input_tensor = bucket.buffer()
    b = bucket.index()
    total = input_tensor.shape[0]
    if state.iter < 1:
        state.maybe_increase_iter(bucket)
        raise TypeError("_allreduce_fut() missing 1 required positional argument: 'hook_state'")
    if state.iter < state.start_compress_iter:
        if b not in state.error_dict:
            logger.info("A tensor of length %s that represents local/global error is created.", total)
            state.error_dict[b] = torch.zeros(total, device=input_tensor.device, dtype=input_tensor.dtype)
            state.global_error_dict[b] = torch.zeros(total, device=input_tensor.device, dtype=input_tensor.dtype)
        state.error_dict[b].add_(input_tensor, alpha=1.0)
        dist.all_reduce(input_tensor, group=group, async_op=False)
        input_tensor.div_(world_size)
        state.global_error_dict[b].add_(input_tensor, alpha=1.0)
        return _done(state, bucket, input_tensor)
    if state.iter == state.start_compress_iter:
        state.error_dict[b].div_(state.start_compress_iter - 1)
        state.global_error_dict[b].div_(state.start_compress_iter - 1)
    _check_compressible(state, input_tensor)
    err = _residual_on(state.error_dict, b, input_tensor, "error_dict")
    _residual_on(state.global_error_dict, b, input_tensor, "global_error_dict")
    L = N.lib()
    stream = torch.cuda.current_stream(input_tensor.device).cuda_stream
    N.check(L.arctopk_ef_apply(input_tensor.data_ptr(), err.data_ptr(), total, N.EF21, 1,
                               N.DTYPE_CODE[input_tensor.dtype], stream), "arctopk_ef_apply")
    seed = _reseed(state)
    if c4:
        raise AttributeError("'Tensor' object has no attribute 'get_current_compress_ratio'")
    log_diff = bucket.is_last() and dist.get_rank() == 0 and logger.isEnabledFor(logging.INFO)
    sq = [None]
    if log_diff:  # |D - C(D)| = sqrt(|D|^2 - |values|^2): only computed when the log is on
        dn = input_tensor.float().pow(2).sum()
        sq[0] = lambda v: float((dn - v.float().pow(2).sum()).clamp_min(0).sqrt())
    vals_seen = []
    _compress_exchange(state, bucket, group, world_size, N.EF21, state.compress_ratio, seed,
                       e_decay=1.0, g_decay=float(state.error_decay), count_bits=False,
                       on_values=vals_seen.append if log_diff else None)
    if log_diff:
        logger.info(f"Rank[{dist.get_rank()}] Iter[{state.iter}], Diff error{sq[0](vals_seen[0])}")
    return _done(state, bucket, input_tensor)


def _all_gather_flat(out: torch.Tensor, inp: torch.Tensor, group, world_size: int) -> None:
    try:
        dist.all_gather_into_tensor(out, inp, group=group, async_op=False)
    except (RuntimeError, NotImplementedError, AttributeError):  # backends without the flat form
        parts = _get_allgather_out_list(inp, world_size)
        dist.all_gather(parts, inp, group=group, async_op=False)
        torch.cat(parts, out=out)


def sparse_hook_sync(state: SparseState, bucket: dist.GradBucket
                     ) -> torch.futures.Future[torch.Tensor]:
    return _sparse_hook_impl(state, bucket)


# bits helpers kept for drivers that import them from here
__all__ += ["tensor_bits", "dtype_bits"]
