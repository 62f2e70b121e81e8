"""NumPy restatement of the "idx16" index wire format (include/arctopk.h), test infrastructure only."""
import numpy as np

BLOCK = 65536


def blocks(numels) -> int:
    return sum(-(-n // BLOCK) for n in numels)


def wire_bytes(numels, ks) -> int:
    return -(-2 * sum(ks) // 16) * 16 + -(-4 * blocks(numels) // 16) * 16


def encode(numels, ks, idx) -> np.ndarray:
    """One rank's payload bytes from its int32 indices (per tensor ascending, concatenated)."""
    idx = np.asarray(idx, dtype=np.int64)
    starts = np.cumsum([0] + list(ks))
    T = [np.searchsorted(idx[a:a + k], np.arange(-(-n // BLOCK)) * BLOCK) for n, k, a in zip(numels, ks, starts)]
    parts = [(idx & 0xFFFF).astype("<u2").tobytes(), np.concatenate(T).astype("<i4").tobytes()]
    return np.frombuffer(b"".join(p + bytes(-len(p) % 16) for p in parts), dtype=np.uint8)
