"""CPU restatement of the TopK / RandK hooks with fp32 residuals under a bf16 bucket
(``SparseState.error_dtype``), test infrastructure only.

Plain torch fp32 / bf16 ops in the order of the contract, per rank and for N ranks in one process.
f = ``.float()`` (bf16 -> fp32, exact), b = ``.to(torch.bfloat16)`` (round to nearest even, NaN ->
0x7FC0).

  EF14  fold   X = f(G) + E (one fp32 add; the first call: X = f(G));  E := X
        pack   selected: vals = b(X), E := X - f(vals) (exact);  others keep E = X
        decode the bf16 decode of oracle.sparse on the bf16 values
  EF21  first  out = (bf16 sum of the ranks' G in rank order) / ws in bf16;  E_0 = f(G), gE_0 = f(out)
        fold   D = f(G) - E (one fp32 subtract);  E is not written
        pack   selected: vals = b(D), E := fma(d, f(vals), E)
        decode s = fp32 sum of the payloads in rank order from 0 (RandK: f of the bf16 all-reduced
               payload);  m = s / ws;  gE := fma(d, m, gE) everywhere;  out = b(gE)
  indices TopK: stable descending sort of |X| (or |D|) in fp32, the first k, ascending;
          RandK: the draws of the state's index_source, which never read the data;
          row / column: rowcol_oracle's segmented rules and layouts
"""
from __future__ import annotations

from fractions import Fraction
from typing import List, Optional

import numpy as np
import torch

import rowcol_oracle as RC
from oracle import sparse as S

BF16 = torch.bfloat16


def f(t: torch.Tensor) -> torch.Tensor:
    return t.float()


def b(t: torch.Tensor) -> torch.Tensor:
    return t.to(BF16)


def fma32(d: float, m: torch.Tensor, e: torch.Tensor) -> torch.Tensor:
    """fma(d, m, e) in fp32, one rounding.  The product of two fp32 numbers is exact in fp64; the
    fp64 sum is rounded once to 53 bits and once more to 24, which differs from one rounding only
    where the fp64 sum sits exactly halfway between two fp32 numbers: those are settled exactly."""
    d32 = float(np.float32(d))
    s = m.double() * d32 + e.double()
    r = s.float()
    rd = r.double()
    inf = torch.full_like(r, float("inf"))
    other = torch.nextafter(r, torch.where(s > rd, inf, -inf))
    tie = (s != rd) & ((s - rd).abs() == (other.double() - s).abs())
    for i in tie.nonzero().flatten().tolist():
        exact = Fraction(float(m[i])) * Fraction(d32) + Fraction(float(e[i]))
        lo, hi = sorted((float(r[i]), float(other[i])))
        mid = (Fraction(lo) + Fraction(hi)) / 2
        if exact > mid:
            r[i] = hi
        elif exact < mid:
            r[i] = lo
    return r


def topk_indices(x: torch.Tensor, k: int) -> torch.Tensor:
    """The k largest |x|, ties at the k-th lowest index first, ascending (int32)."""
    order = torch.sort(x.abs(), descending=True, stable=True).indices[:k]
    return torch.sort(order).values.to(torch.int32)


def layout_ks(shapes, ratio: float, sparse_type: str) -> List[int]:
    if sparse_type == "tensor":
        return [S.cal_k(S.numel_of(s), ratio) for s in shapes]
    return [RC.geometry(s, ratio, sparse_type)[5] for s in shapes]


def select(X: Optional[torch.Tensor], shapes, ratio: float, sparse_type: str, random: bool, index_source: str,
           seed: Optional[int], device=None) -> List[torch.Tensor]:
    """Per tensor the payload's int32 indices.  `device`: where index_source "torch" draws."""
    if sparse_type != "tensor":
        if random and index_source == "host":
            return RC.host_draws(shapes, ratio, sparse_type, seed)
        assert not random or index_source == "hash", "row / column 'torch' draws are not restated"
        return RC.select_indices(X, shapes, ratio, sparse_type, random, seed)[0]
    out, off = [], 0
    if random and index_source in ("host", "torch"):
        torch.manual_seed(int(seed))
    for t, s in enumerate(shapes):
        n = S.numel_of(s)
        k = S.cal_k(n, ratio)
        if not random:
            out.append(topk_indices(X[off:off + n], k))
        elif index_source == "hash":
            out.append(S.randk_hash_indices(n, k, int(seed), t))
        elif index_source == "host":
            out.append(torch.randperm(n)[:k].to(torch.int32))
        else:
            out.append(torch.randperm(n, device=device)[:k].to(torch.int32).cpu())
        off += n
    return out


def _flat(shapes, idxs) -> torch.Tensor:
    """Per-tensor indices as int64 bucket positions."""
    parts, off = [], 0
    for s, idx in zip(shapes, idxs):
        parts.append(idx.long() + off)
        off += S.numel_of(s)
    return torch.cat(parts)


def fold14(G: torch.Tensor, E: Optional[torch.Tensor]) -> torch.Tensor:
    assert G.dtype == BF16 and (E is None or E.dtype == torch.float32)
    return f(G) if E is None else f(G) + E


def fold21(G: torch.Tensor, E: torch.Tensor) -> torch.Tensor:
    assert G.dtype == BF16 and E.dtype == torch.float32
    return f(G) - E


def pack14(X: torch.Tensor, shapes, idxs):
    """(bf16 values, E_new): E_new = X with the rounding remainder at the selected elements."""
    pos = _flat(shapes, idxs)
    vals = b(X[pos])
    E = X.clone()
    E[pos] = X[pos] - f(vals)
    return vals, E


def pack21(D: torch.Tensor, E: torch.Tensor, shapes, idxs, decay: float):
    """(bf16 values, E_new): E_new = fma(decay, f(vals), E) at the selected elements."""
    pos = _flat(shapes, idxs)
    vals = b(D[pos])
    E = E.clone()
    E[pos] = fma32(decay, f(vals), E[pos])
    return vals, E


def decode21(all_vals: List[torch.Tensor], all_idxs, shapes, ws: int, gE: torch.Tensor, decay: float):
    """(out bf16, gE_new) from `len(all_vals)` payloads in rank order (RandK: the one all-reduced)."""
    s = torch.zeros_like(gE)
    for vals, idxs in zip(all_vals, all_idxs):
        pos = _flat(shapes, idxs)
        s[pos] = s[pos] + f(vals)
    m = s / float(ws)  # fp32 division, correctly rounded
    gE = fma32(decay, m, gE)
    return b(gE), gE


def first21(Gs: List[torch.Tensor]):
    """EF21's dense first call: (out bf16, [E_0 per rank], gE_0)."""
    acc = Gs[0].clone()
    for G in Gs[1:]:
        acc = acc + G
    out = acc / len(Gs)
    assert out.dtype == BF16
    return out, [f(G) for G in Gs], f(out)


class SparseMixedOracle:
    """The hook's state and calls with error_dtype=torch.float32 on `ws` ranks (one bf16 bucket,
    index 0, is_last, start_compress_iter 0).  c4: the gradual ratio of sparse_hook_c4."""

    def __init__(self, ws: int, shapes, ratio: float, ef: str, random: bool = False, index_source: str = "host",
                 sparse_type: str = "tensor", seed: int = 0, decay: float = 1.0, c4: bool = False,
                 warmup_iters: int = 100, device=None):
        self.ws, self.shapes, self.base_ratio, self.ef = ws, [list(s) for s in shapes], ratio, ef
        self.random, self.index_source, self.sparse_type = random, index_source, sparse_type
        self.decay, self.c4, self.warmup_iters, self.device = decay, c4, warmup_iters, device
        self.rng = torch.Generator().manual_seed(seed)
        self.Es: Optional[List[torch.Tensor]] = None
        self.gE: Optional[torch.Tensor] = None
        self.iter = 0
        self.bits = 0

    def ratio_now(self) -> float:
        return S.gradual_ratio(self.base_ratio, self.iter, 0, self.warmup_iters) if self.c4 else self.base_ratio

    def call(self, Gs: List[torch.Tensor], indices=None) -> dict:
        """One hook call on every rank.  `indices`: per rank the per-tensor index lists to use in
        place of the restated selection.  Returns dict(out, indices per rank, ks, E_old)."""
        ws, shapes = self.ws, self.shapes
        E_old = None if self.Es is None else [E.clone() for E in self.Es]
        if self.ef == "ef21" and self.Es is None:
            out, self.Es, self.gE = first21(Gs)
            self.iter += 1
            return dict(out=out, indices=None, ks=None, E_old=E_old, dense=True)
        ratio = self.ratio_now()
        seed = int(torch.randint(0, 1_000_000_000, (1,), generator=self.rng).item()) if self.random else None
        ks = layout_ks(shapes, ratio, self.sparse_type)
        vals, idxs, Es = [], [], []
        for q, G in enumerate(Gs):
            src = fold14(G, None if self.Es is None else self.Es[q]) if self.ef == "ef14" else fold21(G, self.Es[q])
            ix = indices[q] if indices is not None else select(src, shapes, ratio, self.sparse_type, self.random,
                                                               self.index_source, seed, self.device)
            assert [i.numel() for i in ix] == ks
            v, E = pack14(src, shapes, ix) if self.ef == "ef14" else pack21(src, self.Es[q], shapes, ix, self.decay)
            vals.append(v), idxs.append(ix), Es.append(E)
        self.Es = Es
        n = Gs[0].numel()
        bits_sum = sum(ks) * (16 + (0 if self.random else 32))
        self.bits += (2 * (ws - 1) if self.random else (ws - 1) * ws) * bits_sum
        if self.random:
            vsum = vals[0].clone()
            for q in range(1, ws):
                vsum = vsum + vals[q]  # bf16: b(f(v0) + f(v1)), what the bf16 collective returns
            if self.ef == "ef14":
                out = S.decode_randk(vsum, torch.cat(idxs[0]), shapes, ks, ws, n)
            else:
                out, self.gE = decode21([vsum], [idxs[0]], shapes, ws, self.gE, self.decay)
        elif self.ef == "ef14":
            out = S.decode_topk(vals, [torch.cat(ix) for ix in idxs], shapes, ks, ws, n)
        else:
            out, self.gE = decode21(vals, idxs, shapes, ws, self.gE, self.decay)
        self.iter += 1
        return dict(out=out, indices=idxs, ks=ks, E_old=E_old, dense=False, values=vals)
