"""NumPy restatement of the "bitmap" index wire format (include/arctopk.h), test infrastructure only."""
import numpy as np

GROUP = 4096


def info_bits(numels) -> int:
    return sum(n + 32 * -(-n // GROUP) for n in numels)


def wire_bytes(numels, ks=None) -> int:
    return -(-4 * sum(-(-n // 32) for n in numels) // 16) * 16 + -(-4 * sum(-(-n // GROUP) for n in numels) // 16) * 16


def encode(numels, ks, idx) -> np.ndarray:
    """One rank's payload bytes from its int32 indices (per tensor ascending, concatenated)."""
    idx = np.asarray(idx, dtype=np.int64)
    W, C = [], []
    for n, k, a in zip(numels, ks, np.cumsum([0] + list(ks))):
        member = np.zeros(-(-n // 32) * 32, dtype=np.uint8)
        member[idx[a:a + k]] = 1
        W.append(np.packbits(member, bitorder="little"))
        C.append(np.searchsorted(idx[a:a + k], np.arange(-(-n // GROUP)) * GROUP).astype("<i4").tobytes())
    parts = [b"".join(w.tobytes() for w in W), b"".join(C)]
    return np.frombuffer(b"".join(p + bytes(-len(p) % 16) for p in parts), dtype=np.uint8)
