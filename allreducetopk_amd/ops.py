"""PyTorch operator layer over libarctopk's C ABI (``torch.ops.arctopk.*``).

The hook itself calls the C entry points directly (one foreign call per step, see
DESIGN.md section 7).  These registrations expose the same codec phases to the PyTorch
dispatcher, so a caller can use them inside code that torch.compile traces or that is
captured in a CUDA/HIP graph: each op declares which tensors it mutates and has a fake
(meta) implementation, and it enqueues on the current stream of the tensors' device.

A plan is passed as its integer handle (``BucketPlan.handle.value``); buffers are the
plan's own (``BucketPlan.sketch`` / ``rowlist`` / ``slotmap`` / ``packed`` / ``V_ring[0]``)
or any tensors of the sizes ``BucketPlan.info`` gives.

    import allreducetopk_amd.ops  # registers torch.ops.arctopk.*
    torch.ops.arctopk.draw_projections(h, seed, V)
    torch.ops.arctopk.encode(h, grad, err, ef, True, V, sketch)
    dist.all_reduce(sketch)
    torch.ops.arctopk.select(h, sketch, ws, rowlist, slotmap)
    torch.ops.arctopk.pack(h, grad, err, ef, rowlist, slotmap, packed)
    dist.all_reduce(packed)
    torch.ops.arctopk.decode(h, packed, slotmap, ws, ef, gerr, grad)

``torch.ops.arctopk.momentum_fold(bucket, moments, offsets, numels, 1 - beta1, beta1)`` is the
momentum compression that precedes a hook call (HookState.accumulate_momentum_on_bucket).

``torch.ops.arctopk.encode_mixed`` / ``pack_mixed`` are the encode and pack of a bf16 bucket whose EF14
residual is a float32 tensor (``GroupTopKState.error_dtype``); select and decode
are the ops above.

``torch.ops.arctopk.encode_mixed21`` / ``pack_mixed21`` / ``decode_mixed21`` are the three phases of a
bf16 bucket whose EF21 residuals are both float32 tensors (``GroupTopKState.ef21_error_dtype``, DESIGN.md
section 4e); the select between them is the op above.

``torch.ops.arctopk.pack_wire16`` / ``decode_wire16`` are the pack and decode of an fp32 bucket whose
packed values travel as bfloat16 (``GroupTopKState.wire_dtype``); encode and
select are the ops above.

Each op replaces the same reference code as the C entry point it calls (include/arctopk.h).
"""
from __future__ import annotations

import ctypes
from typing import List, Optional

import torch

from allreducetopk_amd import _native as N


def _stream(t: torch.Tensor) -> int:
    return torch._C._cuda_getCurrentRawStream(t.device.index or 0)


def _ptr(t: Optional[torch.Tensor]) -> int:
    return 0 if t is None else t.data_ptr()


@torch.library.custom_op("arctopk::draw_projections", mutates_args=("V",))
def draw_projections(plan: int, seed: int, V: torch.Tensor) -> None:
    """V := the reference's torch.randn(m, r, device=...) draws after manual_seed(seed)."""
    N.check(N.lib().arctopk_draw_projections(plan, seed, V.data_ptr(), _stream(V)),
            "arctopk_draw_projections")


@torch.library.custom_op("arctopk::encode", mutates_args=("err", "sketch"))
def encode(plan: int, grad: torch.Tensor, err: Optional[torch.Tensor], ef: int, err_in: bool,
           V: torch.Tensor, sketch: torch.Tensor) -> None:
    """EF pre-apply + rank-r sketch of every tensor of the bucket (K1)."""
    N.check(N.lib().arctopk_encode(plan, grad.data_ptr(), _ptr(err), ef, int(err_in), V.data_ptr(),
                                   sketch.data_ptr(), _stream(grad)), "arctopk_encode")


@torch.library.custom_op("arctopk::select", mutates_args=("rowlist", "slotmap"))
def select(plan: int, sketch: torch.Tensor, world_size: int, rowlist: torch.Tensor,
           slotmap: torch.Tensor) -> None:
    """Mean sketch -> row energies -> exact top-k rows per tensor (K2)."""
    N.check(N.lib().arctopk_select(plan, sketch.data_ptr(), world_size, rowlist.data_ptr(),
                                   slotmap.data_ptr(), _stream(sketch)), "arctopk_select")


@torch.library.custom_op("arctopk::pack", mutates_args=("err", "packed"))
def pack(plan: int, grad: torch.Tensor, err: Optional[torch.Tensor], ef: int, rowlist: torch.Tensor,
         slotmap: torch.Tensor, packed: torch.Tensor) -> None:
    """Selected rows -> packed values; EF14 / EF21 residual updates (K3)."""
    N.check(N.lib().arctopk_pack(plan, grad.data_ptr(), _ptr(err), ef, rowlist.data_ptr(),
                                 slotmap.data_ptr(), packed.data_ptr(), _stream(grad)), "arctopk_pack")


@torch.library.custom_op("arctopk::decode", mutates_args=("gerr", "out"))
def decode(plan: int, packed: torch.Tensor, slotmap: torch.Tensor, world_size: int, ef: int,
           gerr: Optional[torch.Tensor], out: torch.Tensor) -> None:
    """Bucket := mean of the selected rows (+ EF21 global residual) (K4)."""
    N.check(N.lib().arctopk_decode(plan, packed.data_ptr(), slotmap.data_ptr(), world_size, ef,
                                   _ptr(gerr), out.data_ptr(), _stream(out)), "arctopk_decode")


@torch.library.custom_op("arctopk::momentum_fold", mutates_args=("bucket",))
def momentum_fold(bucket: torch.Tensor, moments: List[torch.Tensor], offsets: List[int],
                  numels: List[int], one_minus_beta: float, beta: float) -> None:
    """bucket[offsets[i] : offsets[i] + numels[i]] := one_minus_beta * itself + beta * moments[i],
    rounded as grad.mul_(one_minus_beta).add_(moment, alpha=beta) rounds on the GPU; one launch.
    ``moments`` are contiguous, all of one dtype, each of numels[i] elements."""
    if not (len(moments) == len(offsets) == len(numels)):
        raise ValueError("momentum_fold: moments, offsets and numels must have the same length")
    if any(not m.is_contiguous() or m.numel() != n or m.device != bucket.device
           for m, n in zip(moments, numels)):
        raise ValueError("momentum_fold: every moment must be contiguous, on the bucket's device "
                         "and of numels[i] elements")
    if not bucket.is_contiguous() or any(o < 0 or n < 0 or o + n > bucket.numel()
                                         for o, n in zip(offsets, numels)):
        raise ValueError("momentum_fold: a range lies outside the (contiguous) bucket")
    mom_dtype = moments[0].dtype if moments else bucket.dtype
    if bucket.dtype not in N.DTYPE_CODE or any(m.dtype != mom_dtype for m in moments) \
            or mom_dtype not in N.DTYPE_CODE:
        raise ValueError("momentum_fold: fp32 or bf16 bucket, moments of one fp32 or bf16 dtype")
    ptrs = (ctypes.c_void_p * len(moments))(*[m.data_ptr() for m in moments])
    N.check(N.lib().arctopk_momentum_fold(bucket.data_ptr(), len(moments), N.i64_array(offsets),
                                          N.i64_array(numels), ptrs, one_minus_beta, beta,
                                          N.DTYPE_CODE[bucket.dtype], N.DTYPE_CODE[mom_dtype],
                                          _stream(bucket)), "arctopk_momentum_fold")


def _check_mixed(grad: Optional[torch.Tensor], err: torch.Tensor, what: str) -> None:
    if err.dtype != torch.float32 or not err.is_contiguous():
        raise ValueError(f"{what}: the residual must be a contiguous float32 tensor")
    if grad is not None and (grad.dtype != torch.bfloat16 or grad.numel() != err.numel()
                             or grad.device != err.device):
        raise ValueError(f"{what}: a bfloat16 bucket of the residual's length, on its device")


@torch.library.custom_op("arctopk::encode_mixed", mutates_args=("err", "sketch"))
def encode_mixed(plan: int, grad: torch.Tensor, err: torch.Tensor, err_in: bool, V: torch.Tensor,
                 sketch: torch.Tensor) -> None:
    """EF14 pre-apply into an fp32 residual + the bf16 sketch of a bf16 bucket (arctopk_encode_mixed)."""
    _check_mixed(grad, err, "encode_mixed")
    N.check(N.lib().arctopk_encode_mixed(plan, grad.data_ptr(), err.data_ptr(), int(err_in), V.data_ptr(),
                                         sketch.data_ptr(), _stream(grad)), "arctopk_encode_mixed")


@torch.library.custom_op("arctopk::pack_mixed", mutates_args=("err", "packed"))
def pack_mixed(plan: int, grad: Optional[torch.Tensor], err: torch.Tensor, err_in: bool,
               rowlist: torch.Tensor, slotmap: torch.Tensor, packed: torch.Tensor) -> None:
    """Selected rows -> bf16 packed values; the fp32 residual keeps X - packed (arctopk_pack_mixed)."""
    _check_mixed(grad, err, "pack_mixed")
    N.check(N.lib().arctopk_pack_mixed(plan, _ptr(grad), err.data_ptr(), int(err_in), rowlist.data_ptr(),
                                       slotmap.data_ptr(), packed.data_ptr(), _stream(err)),
            "arctopk_pack_mixed")


@torch.library.custom_op("arctopk::encode_mixed21", mutates_args=("sketch",))
def encode_mixed21(plan: int, grad: torch.Tensor, err: torch.Tensor, V: torch.Tensor, sketch: torch.Tensor) -> None:
    """The bf16 sketch of D = float(G) - E for an fp32 EF21 residual E, which is only read
    (arctopk_encode_mixed21)."""
    _check_mixed(grad, err, "encode_mixed21")
    N.check(N.lib().arctopk_encode_mixed21(plan, grad.data_ptr(), err.data_ptr(), V.data_ptr(),
                                           sketch.data_ptr(), _stream(grad)), "arctopk_encode_mixed21")


@torch.library.custom_op("arctopk::pack_mixed21", mutates_args=("err", "packed"))
def pack_mixed21(plan: int, grad: torch.Tensor, err: torch.Tensor, rowlist: torch.Tensor, slotmap: torch.Tensor,
                 packed: torch.Tensor) -> None:
    """Selected rows -> packed = bf16(D); the fp32 residual E += float(packed) (arctopk_pack_mixed21)."""
    _check_mixed(grad, err, "pack_mixed21")
    N.check(N.lib().arctopk_pack_mixed21(plan, grad.data_ptr(), err.data_ptr(), rowlist.data_ptr(),
                                         slotmap.data_ptr(), packed.data_ptr(), _stream(grad)),
            "arctopk_pack_mixed21")


@torch.library.custom_op("arctopk::decode_mixed21", mutates_args=("gerr", "out"))
def decode_mixed21(plan: int, packed: torch.Tensor, slotmap: torch.Tensor, world_size: int, gerr: torch.Tensor,
                   out: torch.Tensor) -> None:
    """Selected elements: gE += float(packed) / world_size in fp32; out = bf16(gE) everywhere
    (arctopk_decode_mixed21)."""
    _check_mixed(out, gerr, "decode_mixed21")
    N.check(N.lib().arctopk_decode_mixed21(plan, packed.data_ptr(), slotmap.data_ptr(), world_size,
                                           gerr.data_ptr(), out.data_ptr(), _stream(out)),
            "arctopk_decode_mixed21")


def _check_wire16(what: str, packed: torch.Tensor, **fp32) -> None:
    if packed.dtype != torch.bfloat16 or not packed.is_contiguous():
        raise ValueError(f"{what}: the packed values must be a contiguous bfloat16 tensor")
    n = None
    for name, t in fp32.items():
        if t is None:
            continue
        if t.dtype != torch.float32 or not t.is_contiguous() or t.device != packed.device:
            raise ValueError(f"{what}: {name} must be a contiguous float32 tensor on the packed values' device")
        if n is not None and t.numel() != n:
            raise ValueError(f"{what}: {name} must have the bucket's length")
        n = t.numel()


@torch.library.custom_op("arctopk::pack_wire16", mutates_args=("err", "packed"))
def pack_wire16(plan: int, grad: Optional[torch.Tensor], err: Optional[torch.Tensor], ef: int, err_in: bool,
                rowlist: torch.Tensor, slotmap: torch.Tensor, packed: torch.Tensor) -> None:
    """Selected rows of an fp32 bucket -> bf16 packed values; the fp32 residual keeps the rounding
    remainder (EF14: E = X - float(packed); EF21: E += float(packed)) (arctopk_pack_wire16)."""
    _check_wire16("pack_wire16", packed, grad=grad, err=err)
    N.check(N.lib().arctopk_pack_wire16(plan, _ptr(grad), _ptr(err), ef, int(err_in), rowlist.data_ptr(),
                                        slotmap.data_ptr(), packed.data_ptr(), _stream(packed)),
            "arctopk_pack_wire16")


@torch.library.custom_op("arctopk::decode_wire16", mutates_args=("gerr", "out"))
def decode_wire16(plan: int, packed: torch.Tensor, slotmap: torch.Tensor, world_size: int, ef: int,
                  gerr: Optional[torch.Tensor], out: torch.Tensor) -> None:
    """fp32 bucket := float(packed) / world_size on the selected rows, zero elsewhere; EF21: added
    to the global residual, which is written everywhere (arctopk_decode_wire16)."""
    _check_wire16("decode_wire16", packed, out=out, gerr=gerr)
    N.check(N.lib().arctopk_decode_wire16(plan, packed.data_ptr(), slotmap.data_ptr(), world_size, ef,
                                          _ptr(gerr), out.data_ptr(), _stream(out)), "arctopk_decode_wire16")


# fake implementations: the ops only mutate their declared outputs
@draw_projections.register_fake
def _(plan, seed, V):
    return None


@encode.register_fake
def _(plan, grad, err, ef, err_in, V, sketch):
    return None


@select.register_fake
def _(plan, sketch, world_size, rowlist, slotmap):
    return None


@pack.register_fake
def _(plan, grad, err, ef, rowlist, slotmap, packed):
    return None


@decode.register_fake
def _(plan, packed, slotmap, world_size, ef, gerr, out):
    return None


@momentum_fold.register_fake
def _(bucket, moments, offsets, numels, one_minus_beta, beta):
    return None


@encode_mixed.register_fake
def _(plan, grad, err, err_in, V, sketch):
    return None


@pack_mixed.register_fake
def _(plan, grad, err, err_in, rowlist, slotmap, packed):
    return None


@encode_mixed21.register_fake
def _(plan, grad, err, V, sketch):
    return None


@pack_mixed21.register_fake
def _(plan, grad, err, rowlist, slotmap, packed):
    return None


@decode_mixed21.register_fake
def _(plan, packed, slotmap, world_size, gerr, out):
    return None


@pack_wire16.register_fake
def _(plan, grad, err, ef, err_in, rowlist, slotmap, packed):
    return None


@decode_wire16.register_fake
def _(plan, packed, slotmap, world_size, ef, gerr, out):
    return None
