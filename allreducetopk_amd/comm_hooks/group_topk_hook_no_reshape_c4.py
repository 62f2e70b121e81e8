"""ARC-TopK hook, c4 variant -- drop-in for the reference's
comm_hooks/group_topk_hook_no_reshape_c4.py (``GroupTopKState`` :147-200, ``cal_k``
:202-219, ``group_topk_hook`` :222-352), the hook its registry imports for the Llama / C4
runs (comm_hooks/utils.py:109-110).

Differences from ``group_topk_hook_no_reshape`` (whose plans, exchange step, deferral and
streams this hook shares):

* 1-D tensors are not compressed (:19-25): they are DENSE segments of the native plan
  (``ARCTOPK_PLAN_DENSE_1D``) -- no sketch, no place in the sketch all-reduce, no select;
  their values ride the packed all-reduce once and ``P_bits`` is 0.
* ``gradual_compression`` (default True) ramps the ratio from 0.8 down to ``compress_ratio``
  over ``start_compress_iter + warmup_iters`` iterations after compression starts
  (:186-200); ``cal_k`` takes the ratio in force.  Each ratio is a plan of its own; the
  bucket's previous plan is dropped when the ratio moves.
* During the ramp every 2-D / ND tensor's V comes from a fresh generator seeded with the
  call's seed (:31-39, :296-301; ``ARCTOPK_PLAN_RESTART_DRAWS``): with device projections
  Philox offset 0 for every tensor and the global generator left where
  ``torch.manual_seed(seed)`` puts it; with host projections one mt19937 draw per tensor.

Deviation: with ``use_error_feedback="ef21"`` and a 1-D tensor in
the bucket the reference raises at its first compressed call (:25 returns the tensor itself
as the values that :130-132 write back into it after zeroing it).  This hook does what that
code evidently means, the 1-D tensor as a tensor whose rows are all selected:
D = G - E; E += D; out = gE + mean(D); gE := out.

``fake_group_topk_hook`` (:356-433), an ablation tool, is not provided.
"""

import logging

import torch
import torch.distributed as dist

from allreducetopk_amd import _native as N
from allreducetopk_amd.comm_hooks import group_topk_hook_no_reshape as _base

logger = logging.getLogger(__name__)

__all__ = ["GroupTopKState", "cal_k", "group_topk_hook"]


class GroupTopKState(_base.GroupTopKState):
    """State of the c4 ARC-TopK hook (reference :147-184; same constructor)."""

    _CKPT_SCALARS = _base.GroupTopKState._CKPT_SCALARS + ("compression_started",)

    def __init__(self, process_group: dist.ProcessGroup, r: int = 4, compress_ratio: float = 0.08,
                 start_compress_iter: int = 2, use_error_feedback="noef", seed=0, error_decay=1.0,
                 gradual_compression=True, warmup_iters=100):
        super().__init__(process_group, r=r, compress_ratio=compress_ratio,
                         start_compress_iter=start_compress_iter,
                         use_error_feedback=use_error_feedback, seed=seed, error_decay=error_decay)
        self.base_compress_ratio = compress_ratio
        self.gradual_compression = gradual_compression
        # note: the ramp spans start_compress_iter + warmup_iters iterations (ref :164)
        self.warmup_iters = start_compress_iter + warmup_iters
        self.compression_started = False

    def get_current_compress_ratio(self):
        """0.8 -> base ratio, linear in iterations since compression started (ref :186-200)."""
        if not self.gradual_compression or not self.compression_started:
            return self.base_compress_ratio
        progress = self.iter - self.start_compress_iter
        if progress < self.warmup_iters:
            start_ratio = 0.8
            cur = start_ratio - (start_ratio - self.base_compress_ratio) * (progress / self.warmup_iters)
            return max(cur, self.base_compress_ratio)
        return self.base_compress_ratio

    def _deterministic_projections(self) -> bool:
        """Whether this call draws every V from a fresh generator (ref :300)."""
        return self.compression_started and self.iter - self.start_compress_iter < self.warmup_iters

    def _plan_ratio(self) -> float:
        return float(self.get_current_compress_ratio())

    def _plan_flags(self) -> int:
        return N.PLAN_DENSE_1D | (N.PLAN_RESTART_DRAWS if self._deterministic_projections() else 0)


def cal_k(state, tensor) -> int:
    """Selected elements of one tensor at the ratio in force (reference :202-219)."""
    ratio = state.get_current_compress_ratio()
    kind, n, m = _base._geometry(tensor.shape)
    if kind == N.SEG_RAW:  # 1-D: every element
        return n
    return max(1, int(n * ratio)) * m


def group_topk_hook(state: GroupTopKState, bucket: dist.GradBucket
                    ) -> torch.futures.Future[torch.Tensor]:
    # past the dense warm-up: compression has started (ref :250-254), before the ratio is read
    if state.iter >= state.start_compress_iter and not state.compression_started:
        state.compression_started = True
        logger.info("Starting compression at iteration %s with gradual compression enabled: %s",
                    state.iter, state.gradual_compression)
    return _base.group_topk_hook(state, bucket)
