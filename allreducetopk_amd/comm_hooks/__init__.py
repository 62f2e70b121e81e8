"""Drop-in DDP comm hooks (same module layout as the reference's ``comm_hooks``):
``group_topk_hook_no_reshape`` (ARC-TopK), ``group_topk_hook_no_reshape_c4`` (its c4 variant:
dense 1-D tensors, gradual ratio), ``sparse_hook`` / ``sparse_hook_c4`` (TopK / RandK),
``default_hooks``, and the registry in ``utils``."""
