"""CPU restatement of an fp32 bucket whose packed values travel as bf16 (test infrastructure only).

The rules of DESIGN.md section 4f in plain torch ops, per rank and for N ranks in one process, with
the selected rows supplied by the caller (the device's own: encode and select are the existing
ones and are checked elsewhere).  f = ``.float()`` (bf16 -> fp32, exact), b =
``.to(torch.bfloat16)`` (round to nearest even, NaN -> 0x7FC0).

  pack   : selected rows (every element of a DENSE segment):
           noef: packed = b(G)
           ef14: X = G + E (one fp32 add; G on the first call); packed = b(X); E := X - f(packed);
                 other rows keep E = X
           ef21: D = G - E; packed = b(D); E := E + f(packed); other rows untouched
  wire   : the ranks' packed values summed in bf16 (torch's own bf16 add, in rank order)
  decode : mean = f(sum) / ws in fp32; noef, ef14: out = mean on the selection, 0 elsewhere;
           ef21: gE := gE + mean on the selection, out = gE everywhere

Gather and scatter reuse the slicing of ``oracle.arctopk`` (segments, pack, decode); 1-D tensors
are RAW under the base hook and DENSE (every element selected) under the c4 hook, whose ratio ramp
and restarted draws come from ``arc_c4_oracle``.
"""
from __future__ import annotations

from typing import List, Optional

import torch

import arc_c4_oracle as C4
from oracle import arctopk as A

RAW, SKETCH, DENSE = A.RAW, A.SKETCH, C4.DENSE
BF16 = torch.bfloat16
F32 = torch.float32


def f(t: torch.Tensor) -> torch.Tensor:
    return t.float()


def b(t: torch.Tensor) -> torch.Tensor:
    return t.to(BF16)


def segments(shapes, ratio: float, dense_1d: bool = False):
    return C4.segments(shapes, ratio) if dense_1d else A.segments(shapes, ratio)


def full_rows(rows, segs):
    """`rows` with every row of a DENSE segment."""
    return [torch.arange(s.n) if s.kind == DENSE else torch.as_tensor(x, dtype=torch.int64)
            for s, x in zip(segs, rows)]


def pre_apply(G: torch.Tensor, E: Optional[torch.Tensor], ef: str) -> torch.Tensor:
    """X (ef14: G + E, or G when E is None: the first call), D (ef21: G - E) or G (noef)."""
    assert G.dtype == F32 and (E is None or E.dtype == F32)
    if ef == "ef14" and E is not None:
        return G + E
    if ef == "ef21":
        return G - E
    return G.clone()


def pack(G: torch.Tensor, E: Optional[torch.Tensor], ef: str, rows, segs):
    """(bf16 values in oracle.arctopk's layout, E_new fp32 or None).  Nothing is modified."""
    X = pre_apply(G, E, ef)
    vals = b(A.pack(X.clone(), rows, segs, "noef"))  # the gather of A.pack, then one rounding
    if ef == "noef":
        return vals, None
    En = X.clone() if ef == "ef14" else E.clone()
    off = 0
    for s, idx in zip(segs, rows):
        v2 = En[s.offset:s.offset + s.numel].view(s.n, s.m)
        y = f(vals[off:off + s.k]).view(-1, s.m)
        v2[idx] = (v2[idx] - y) if ef == "ef14" else (v2[idx] + y)
        off += s.k
    return vals, En


def wire_sum(vals: List[torch.Tensor]) -> torch.Tensor:
    """The bf16 all-reduce: torch's bf16 add in rank order (b(f(a) + f(b)))."""
    acc = vals[0].clone()
    for v in vals[1:]:
        acc = acc + v
    assert acc.dtype == BF16
    return acc


def decode(values_sum: torch.Tensor, ws: int, rows, segs, numel: int, ef: str, gE: Optional[torch.Tensor]):
    """(out fp32, gE_new fp32 or None) from the all-reduced bf16 values.  gE is not modified."""
    assert values_sum.dtype == BF16
    mean = A.decode(f(values_sum), ws, rows, segs, numel, F32)  # fp32 division, scattered into zeros
    if ef != "ef21":
        return mean, None
    sel = A.decode(torch.ones(values_sum.numel()), 1, rows, segs, numel, F32) != 0
    gE_new = torch.where(sel, gE + mean, gE)  # unselected elements keep their bits
    return gE_new.clone(), gE_new


def sketch_elems(segs, r: int) -> int:
    return sum(s.n * r if s.kind == SKETCH else s.n if s.kind == RAW else 0 for s in segs)


def bits_per_call(segs, r: int) -> int:
    """The sketch in fp32 (none for DENSE) + the selected values in bf16."""
    return sketch_elems(segs, r) * 32 + sum(s.k for s in segs) * 16


def simulate_step(Gs: List[torch.Tensor], Es: List[Optional[torch.Tensor]], gE: Optional[torch.Tensor], shapes,
                  ratio: float, r: int, ef: str, rows, dense_1d: bool = False):
    """One compressed call on len(Gs) ranks given the selected `rows` per segment (DENSE segments:
    ignored, every element)."""
    ws = len(Gs)
    segs = segments(shapes, ratio, dense_1d)
    rows = full_rows(rows, segs)
    vals, E_new = [], []
    for G, E in zip(Gs, Es):
        v, En = pack(G, E, ef, rows, segs)
        vals.append(v), E_new.append(En)
    vsum = wire_sum(vals)
    out, gE_new = decode(vsum, ws, rows, segs, Gs[0].numel(), ef, gE)
    return dict(segs=segs, rows=rows, values=vals, values_sum=vsum, out=out, E_new=E_new, gE_new=gE_new,
                bits=bits_per_call(segs, r))


class Wire16Oracle:
    """The hook's state and calls with wire_dtype=torch.bfloat16 on `ws` ranks (one fp32 bucket,
    index 0, is_last; start_compress_iter 0).  ef21's first call is the dense fp32 one, which draws
    no seed.  c4: the c4 hook (DENSE 1-D tensors and the ratio ramp of arc_c4_oracle)."""

    def __init__(self, ws: int, shapes, ratio: float, ef: str, r: int = 4, c4: bool = False, gradual: bool = True,
                 warmup_iters: int = 100):
        self.ws, self.shapes, self.base_ratio, self.r, self.c4 = ws, [tuple(s) for s in shapes], ratio, r, c4
        self.ef = ef
        self.gradual, self.warmup_sum = gradual, warmup_iters  # (start 0: the ramp spans warmup_iters)
        self.iter = 0
        self.bits = 0
        self.Es: Optional[List[Optional[torch.Tensor]]] = None
        self.gE: Optional[torch.Tensor] = None

    def ratio_now(self) -> float:
        if not self.c4:
            return self.base_ratio
        return C4.current_ratio(self.base_ratio, self.iter, 0, self.warmup_sum, self.gradual, True)

    def call(self, Gs, rows=None):
        if self.Es is None:
            if self.ef == "ef21":  # E_0 = G; the dense all-reduce; gE_0 = mean
                acc = Gs[0].clone()
                for G in Gs[1:]:
                    acc = acc + G
                out = acc / self.ws
                self.Es, self.gE = [G.clone() for G in Gs], out.clone()
                self.bits += Gs[0].numel() * 32
                self.iter += 1
                return dict(out=out, first=True)
            self.Es = [None] * self.ws
        ratio = self.ratio_now()
        res = simulate_step(Gs, self.Es, self.gE, self.shapes, ratio, self.r, self.ef, rows, dense_1d=self.c4)
        self.Es, self.gE = res["E_new"], res["gE_new"]
        self.bits += 2 * (self.ws - 1) * res["bits"]
        self.iter += 1
        return dict(out=res["out"], ratio=ratio, res=res, first=False)
