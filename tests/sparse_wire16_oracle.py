"""CPU restatement of the TopK / RandK hooks with bf16 values on the wire of an fp32 bucket
(``SparseState.wire_dtype``), test infrastructure only.

Plain torch fp32 / bf16 ops in the order of the contract, per rank and for N ranks in one process.
f = ``.float()`` (bf16 -> fp32, exact), b = ``.to(torch.bfloat16)`` (round to nearest even, NaN ->
0x7FC0); fp32 fma in float64, rounded once (sparse_mixed_oracle.fma32).

  fold    noef: X = G | EF14: X = G + E (one fp32 add; the first call: X = G), E := X |
          EF21: D = G - E (the first call of a bucket is dense: E_0 = G, gE_0 = mean of the ranks' G)
  select  the fp32 path's: sparse_mixed_oracle.select on X (or D); v = X[idx]
  pack    vals16 = b(v) | EF14: E[idx] := v - f(vals16) | EF21: E[idx] := fma(d, f(vals16), E[idx])
          an index outside its tensor: vals16 = 0, E untouched
  wire    RandK: the bf16 all-reduce, b(f(p0) + f(p1)) on two ranks; TopK: every rank's payload
  decode  s = 0.0f + f(v_0) + f(v_1) + ... in rank order; m = s / ws; out = m, or under EF21
          gE := fma(d, m, gE), out = gE on every element
"""
from __future__ import annotations

from typing import List, Optional

import torch

import sparse_mixed_oracle as SM
from oracle import sparse as S

BF16 = torch.bfloat16
f, b, fma32 = SM.f, SM.b, SM.fma32


def _positions(shapes, idxs):
    """(positions into the payload, bucket positions) of the indices that lie in their tensor."""
    keep, pos, off, koff = [], [], 0, 0
    for s, idx in zip(shapes, idxs):
        n = S.numel_of(s)
        ok = ((idx >= 0) & (idx < n)).nonzero().flatten()
        keep.append(ok + koff)
        pos.append(idx[ok].long() + off)
        off += n
        koff += idx.numel()
    return torch.cat(keep), torch.cat(pos)


def pack(v: torch.Tensor, E: Optional[torch.Tensor], shapes, idxs, ef: str, decay: float = 1.0):
    """(vals16, E_new) from the selects' contiguous fp32 values; E may hold anything at idx under
    EF14 (the remainder is stored, not added)."""
    assert v.dtype == torch.float32 and (E is None or E.dtype == torch.float32)
    keep, pos = _positions(shapes, idxs)
    vals = torch.zeros(v.numel(), dtype=BF16)
    vals[keep] = b(v[keep])
    if ef == "noef":
        return vals, None
    E = E.clone()
    if ef == "ef14":
        E[pos] = v[keep] - f(vals[keep])
    else:
        E[pos] = fma32(decay, f(vals[keep]), E[pos])
    return vals, E


def sums(all_vals: List[torch.Tensor], all_idxs, shapes, n: int, order=None) -> torch.Tensor:
    """fp32 sums of the payloads at their elements, from 0.0f, in rank order (`order`: another)."""
    s = torch.zeros(n)
    for q in (range(len(all_vals)) if order is None else order):
        keep, pos = _positions(shapes, all_idxs[q])
        s[pos] = s[pos] + f(all_vals[q][keep])
    return s


def decode(all_vals: List[torch.Tensor], all_idxs, shapes, ws: int, n: int, gE: Optional[torch.Tensor] = None,
           decay: float = 1.0):
    """(out, gE_new) from `len(all_vals)` payloads in rank order (RandK: the one all-reduced)."""
    m = sums(all_vals, all_idxs, shapes, n) / float(ws)  # fp32 division, correctly rounded
    if gE is None:
        return m, None
    gE = fma32(decay, m, gE)
    return gE.clone(), gE


def comm_bits(sum_k: int, ws: int, random: bool) -> int:
    if random:
        return 2 * (ws - 1) * sum_k * 16
    return (ws - 1) * ws * sum_k * (16 + 32)


class SparseWire16Oracle:
    """The hook's state and calls with wire_dtype=torch.bfloat16 on `ws` ranks (one fp32 bucket,
    index 0, is_last, start_compress_iter 0).  c4: the gradual ratio of sparse_hook_c4."""

    def __init__(self, ws: int, shapes, ratio: float, ef: str, random: bool = False, index_source: str = "host",
                 sparse_type: str = "tensor", seed: int = 0, decay: float = 1.0, c4: bool = False,
                 warmup_iters: int = 100):
        self.ws, self.shapes, self.base_ratio, self.ef = ws, [list(s) for s in shapes], ratio, ef
        self.random, self.index_source, self.sparse_type = random, index_source, sparse_type
        self.decay, self.c4, self.warmup_iters = decay, c4, warmup_iters
        self.rng = torch.Generator().manual_seed(seed)
        self.Es: Optional[List[torch.Tensor]] = None
        self.gE: Optional[torch.Tensor] = None
        self.iter = 0
        self.bits = 0
        self.wire16_calls = 0

    def ratio_now(self) -> float:
        return S.gradual_ratio(self.base_ratio, self.iter, 0, self.warmup_iters) if self.c4 else self.base_ratio

    def call(self, Gs: List[torch.Tensor]) -> dict:
        """One hook call on every rank: dict(out, indices per rank, ks, dense, values)."""
        ws, shapes, ef = self.ws, self.shapes, self.ef
        n = Gs[0].numel()
        if ef == "ef21" and self.Es is None:  # the dense first call: fp32 on the wire
            acc = Gs[0].clone()
            for G in Gs[1:]:
                acc = acc + G
            out = acc / float(ws)
            self.Es, self.gE = [G.clone() for G in Gs], out.clone()
            self.iter += 1
            return dict(out=out, indices=None, ks=None, dense=True)
        ratio = self.ratio_now()
        seed = int(torch.randint(0, 1_000_000_000, (1,), generator=self.rng).item()) if self.random else None
        ks = SM.layout_ks(shapes, ratio, self.sparse_type)
        vals, idxs, Es = [], [], []
        for q, G in enumerate(Gs):
            assert G.dtype == torch.float32
            if ef == "noef":
                src, E = G, None
            elif ef == "ef14":
                src = G if self.Es is None else G + self.Es[q]
                E = src
            else:
                src, E = G - self.Es[q], self.Es[q]
            ix = SM.select(src, shapes, ratio, self.sparse_type, self.random, self.index_source, seed)
            assert [i.numel() for i in ix] == ks
            v16, E = pack(src[SM._flat(shapes, ix)], E, shapes, ix, ef, self.decay)
            vals.append(v16), idxs.append(ix), Es.append(E)
        if ef != "noef":
            self.Es = Es
        self.bits += comm_bits(sum(ks), ws, self.random)
        if self.random:
            vsum = vals[0].clone()
            for q in range(1, ws):
                vsum = vsum + vals[q]  # bf16: b(f(p0) + f(p1)), what the bf16 collective returns
            out, gE = decode([vsum], [idxs[0]], shapes, ws, n, self.gE, self.decay)
        else:
            out, gE = decode(vals, idxs, shapes, ws, n, self.gE, self.decay)
        if ef == "ef21":
            self.gE = gE
        self.iter += 1
        self.wire16_calls += 1
        return dict(out=out, indices=idxs, ks=ks, dense=False, values=vals)
