"""CPU restatement of EF21 with both residuals in fp32 under a bf16 bucket (test infrastructure only).

The rules of DESIGN.md section 4e in plain torch ops, per rank and for N ranks in one process,
with the selected rows supplied by the caller (the device's own: the select is the existing one
and is checked elsewhere).  f = ``.float()`` (bf16 -> fp32, exact), b = ``.to(torch.bfloat16)``
(round to nearest even, NaN -> 0x7FC0).

  first  : out = (sum of the ranks' G in bf16, rank order) / ws in bf16;  E_0 = f(G), gE_0 = f(out)
  encode : D = f(G) - E (one fp32 subtract);  E is not written
           sketch = b(D.view(n, m) @ f(V)) (SKETCH), b(D) (RAW), none (DENSE)
  pack   : selected rows: packed = b(D);  E := E + f(packed) (one fp32 add);  other rows untouched
  decode : selected elements: gE := gE + f(P) / ws, P the bf16 sum of the ranks' packed values in
           rank order, the quotient in fp32 and not rounded to bf16;  out = b(gE) everywhere

Every rank holds the same gE (it starts from the same mean and adds the same sums), so one copy is
kept.  1-D tensors are RAW under the base hook and DENSE (every element selected) under the c4
hook, whose ratio ramp and restarted draws come from ``arc_c4_oracle``.
"""
from __future__ import annotations

from typing import List, Optional

import torch

import arc_c4_oracle as C4
from oracle import arctopk as A

RAW, SKETCH, DENSE = A.RAW, A.SKETCH, C4.DENSE
BF16 = torch.bfloat16


def f(t: torch.Tensor) -> torch.Tensor:
    return t.float()


def b(t: torch.Tensor) -> torch.Tensor:
    return t.to(BF16)


def segments(shapes, ratio: float, dense_1d: bool = False):
    return C4.segments(shapes, ratio) if dense_1d else A.segments(shapes, ratio)


def first_call(Gs: List[torch.Tensor]):
    """(out bf16, [E_0 per rank], gE_0): the dense all-reduce of the bf16 buckets, divided by ws."""
    acc = Gs[0].clone()
    for G in Gs[1:]:
        acc = acc + G
    out = acc / len(Gs)
    assert out.dtype == BF16
    return out, [f(G) for G in Gs], f(out)


def encode(G: torch.Tensor, E: torch.Tensor, segs, Vs):
    """(D fp32, [bf16 sketch per segment, None for DENSE])."""
    assert G.dtype == BF16 and E.dtype == torch.float32
    D = f(G) - E
    Ps = []
    for s, V in zip(segs, Vs):
        d = D[s.offset:s.offset + s.numel]
        if s.kind == SKETCH:
            Ps.append(b(d.view(s.n, s.m) @ f(V)))
        else:
            Ps.append(b(d) if s.kind == RAW else None)
    return D, Ps


def pack(D: torch.Tensor, E: torch.Tensor, rows, segs):
    """(bf16 values in oracle.arctopk's layout, E_new fp32).  D and E are not modified."""
    vals = b(A.pack(D.clone(), rows, segs, "noef"))  # the gather of A.pack, then one rounding
    E = E.clone()
    off = 0
    for s, idx in zip(segs, rows):
        v2 = E[s.offset:s.offset + s.numel].view(s.n, s.m)
        v2[idx] = v2[idx] + f(vals[off:off + s.k]).view(-1, s.m)
        off += s.k
    return vals, E


def decode(values_sum: torch.Tensor, ws: int, rows, segs, gE: torch.Tensor):
    """(out bf16, gE_new fp32) from the all-reduced bf16 values.  gE is not modified."""
    assert values_sum.dtype == BF16 and gE.dtype == torch.float32
    mean = f(values_sum) / float(ws)  # fp32 division, correctly rounded
    gE = gE.clone()
    off = 0
    for s, idx in zip(segs, rows):
        v2 = gE[s.offset:s.offset + s.numel].view(s.n, s.m)
        v2[idx] = v2[idx] + mean[off:off + s.k].view(-1, s.m)
        off += s.k
    return b(gE), gE


def bits_per_call(segs, r: int) -> int:
    """The base hook's accounting in bf16: sketch elements (none for DENSE) + selected values."""
    return sum(((s.n * r if s.kind == SKETCH else s.n if s.kind == RAW else 0) + s.k) * 16 for s in segs)


def simulate_step(Gs: List[torch.Tensor], Es: List[torch.Tensor], gE: torch.Tensor, shapes, ratio: float,
                  r: int, seed: int, rows, dense_1d: bool = False, restart: bool = False, proj_device=None,
                  Vs=None):
    """One compressed call on len(Gs) ranks (sums in rank order, in bf16 as the wire carries
    them).  `rows`: per segment the selected rows (DENSE segments: ignored, every element)."""
    ws = len(Gs)
    segs = segments(shapes, ratio, dense_1d)
    if Vs is None:
        Vs = C4.draw_projections(seed, segs, r, BF16, restart, device=proj_device)
    rows = [torch.arange(s.n) if s.kind == DENSE else torch.as_tensor(x, dtype=torch.int64)
            for s, x in zip(segs, rows)]
    Ds, Pls, vals, E_new = [], [], [], []
    for G, E in zip(Gs, Es):
        D, Ps = encode(G, E, segs, Vs)
        v, En = pack(D, E, rows, segs)
        Ds.append(D), Pls.append(Ps), vals.append(v), E_new.append(En)
    vsum = vals[0].clone()
    for q in range(1, ws):
        vsum = vsum + vals[q]
    out, gE_new = decode(vsum, ws, rows, segs, gE)
    return dict(segs=segs, V=Vs, D=Ds, P_local=Pls, rows=rows, values=vals, values_sum=vsum, out=out,
                E_new=E_new, gE_new=gE_new, bits=bits_per_call(segs, r))


class Mixed21Oracle:
    """The hook's state and calls with ef21_error_dtype=torch.float32 on `ws` ranks (one bucket,
    index 0, is_last; start_compress_iter 0): the first call is the dense one, which draws no
    seed.  c4: the c4 hook (DENSE 1-D tensors, the ratio ramp and the restarted draws of
    arc_c4_oracle)."""

    def __init__(self, ws: int, shapes, ratio: float, r: int = 4, seed: int = 0, c4: bool = False,
                 gradual: bool = True, warmup_iters: int = 100):
        self.ws, self.shapes, self.base_ratio, self.r, self.c4 = ws, [tuple(s) for s in shapes], ratio, r, c4
        self.gradual, self.warmup_sum = gradual, warmup_iters  # (start 0: the ramp spans warmup_iters)
        self.iter = 0
        self.bits = 0
        self.rng = torch.Generator().manual_seed(seed)
        self.Es: Optional[List[torch.Tensor]] = None
        self.gE: Optional[torch.Tensor] = None

    def ratio_now(self) -> float:
        if not self.c4:
            return self.base_ratio
        return C4.current_ratio(self.base_ratio, self.iter, 0, self.warmup_sum, self.gradual, True)

    def call(self, Gs, rows=None, proj_device=None):
        if self.Es is None:
            out, self.Es, self.gE = first_call(Gs)
            self.bits += Gs[0].numel() * 16
            self.iter += 1
            return dict(out=out, first=True)
        ratio = self.ratio_now()
        seed = int(torch.randint(0, 1_000_000_000, (1,), generator=self.rng).item())
        restart = self.c4 and C4.deterministic(self.iter, 0, self.warmup_sum, True)
        res = simulate_step(Gs, self.Es, self.gE, self.shapes, ratio, self.r, seed, rows, dense_1d=self.c4,
                            restart=restart, proj_device=proj_device)
        self.Es, self.gE = res["E_new"], res["gE_new"]
        self.bits += 2 * (self.ws - 1) * res["bits"]
        self.iter += 1
        return dict(out=res["out"], ratio=ratio, seed=seed, restart=restart, res=res, first=False)
