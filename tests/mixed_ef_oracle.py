"""CPU restatement of EF14 with an fp32 residual under a bf16 bucket (test infrastructure only).

The rules of DESIGN.md section 4d in plain torch ops, per rank and for N ranks in one process,
with the selected rows supplied by the caller (the device's own: the select is the existing one
and is checked elsewhere).  f = ``.float()`` (bf16 -> fp32, exact), b = ``.to(torch.bfloat16)``
(round to nearest even, NaN -> 0x7FC0).

  encode : X = f(G) + E (one fp32 add) or f(G) on the first call;  E := X
           sketch = b(X.view(n, m) @ f(V)) (SKETCH), b(X) (RAW), none (DENSE)
  pack   : selected rows: packed = b(X); E := X - f(packed);  other rows keep E = X
  decode : unchanged -- the bf16 mean of the summed packed values, scattered into zeros

Pack and decode reuse the slicing of ``oracle.arctopk`` (segments, row order, values layout);
1-D tensors are RAW under the base hook and DENSE (every element selected) under the c4 hook,
whose ratio ramp and restarted draws come from ``arc_c4_oracle``.
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


def encode(G: torch.Tensor, E: Optional[torch.Tensor], segs, Vs):
    """(X fp32, [bf16 sketch per segment, None for DENSE]); E None: the bucket's first call."""
    assert G.dtype == BF16 and (E is None or E.dtype == torch.float32)
    X = f(G) if E is None else f(G) + E
    Ps = []
    for s, V in zip(segs, Vs):
        x = X[s.offset:s.offset + s.numel]
        if s.kind == SKETCH:
            Ps.append(b(x.view(s.n, s.m) @ f(V)))
        else:
            Ps.append(b(x) if s.kind == RAW else None)
    return X, Ps


def pack(X: torch.Tensor, rows, segs):
    """(bf16 values in oracle.arctopk's layout, E_new fp32).  X is not modified."""
    vals = b(A.pack(X.clone(), rows, segs, "noef"))  # the gather of A.pack, then one rounding
    E = X.clone()
    off = 0
    for s, idx in zip(segs, rows):
        v2 = E[s.offset:s.offset + s.numel].view(s.n, s.m)
        v2[idx] = v2[idx] - f(vals[off:off + s.k]).view(-1, s.m)
        off += s.k
    return vals, E


def bits_per_call(segs, r: int) -> int:
    """The base hook's accounting in bf16: sketch elements (none for DENSE) + selected values."""
    return sum(((s.n * r if s.kind == SKETCH else s.n if s.kind == RAW else 0) + s.k) * 16 for s in segs)


def simulate_step(Gs: List[torch.Tensor], Es: List[Optional[torch.Tensor]], shapes, ratio: float, r: int,
                  seed: int, rows, dense_1d: bool = False, restart: bool = False, proj_device=None,
                  Vs=None):
    """One compressed call on len(Gs) ranks (sums in rank order, in bf16 as the wire carries
    them).  `rows`: per segment the selected rows (DENSE segments: ignored, every element)."""
    ws = len(Gs)
    segs = segments(shapes, ratio, dense_1d)
    if Vs is None:
        Vs = C4.draw_projections(seed, segs, r, BF16, restart, device=proj_device)
    rows = [torch.arange(s.n) if s.kind == DENSE else torch.as_tensor(x, dtype=torch.int64)
            for s, x in zip(segs, rows)]
    Xs, Pls, vals, E_new = [], [], [], []
    for G, E in zip(Gs, Es):
        X, Ps = encode(G, E, segs, Vs)
        v, En = pack(X, rows, segs)
        Xs.append(X), Pls.append(Ps), vals.append(v), E_new.append(En)
    P_sum = []
    for j, s in enumerate(segs):
        if s.kind == DENSE:
            P_sum.append(None)
            continue
        acc = Pls[0][j].clone()
        for q in range(1, ws):
            acc = acc + Pls[q][j]
        P_sum.append(acc)
    vsum = vals[0].clone()
    for q in range(1, ws):
        vsum = vsum + vals[q]
    out = A.decode(vsum, ws, rows, segs, Gs[0].numel(), BF16)
    return dict(segs=segs, V=Vs, X=Xs, P_local=Pls, P_sum=P_sum, rows=rows, values=vals, values_sum=vsum,
                out=out, E_new=E_new, bits=bits_per_call(segs, r))


class MixedOracle:
    """The hook's state and calls with error_dtype=torch.float32 on `ws` ranks (one bucket, index
    0, is_last; start_compress_iter 0).  c4: the c4 hook (DENSE 1-D tensors, the ratio ramp and
    the restarted draws of arc_c4_oracle)."""

    def __init__(self, ws: int, shapes, ratio: float, r: int = 4, seed: int = 0, c4: bool = False,
                 gradual: bool = True, warmup_iters: int = 100):
        self.ws, self.shapes, self.base_ratio, self.r, self.c4 = ws, [tuple(s) for s in shapes], ratio, r, c4
        self.gradual, self.warmup_sum = gradual, warmup_iters  # (start 0: the ramp spans warmup_iters)
        self.iter = 0
        self.bits = 0
        self.rng = torch.Generator().manual_seed(seed)
        self.Es: List[Optional[torch.Tensor]] = [None] * ws

    def ratio_now(self) -> float:
        if not self.c4:
            return self.base_ratio
        return C4.current_ratio(self.base_ratio, self.iter, 0, self.warmup_sum, self.gradual, True)

    def call(self, Gs, rows, proj_device=None):
        ratio = self.ratio_now()
        seed = int(torch.randint(0, 1_000_000_000, (1,), generator=self.rng).item())
        restart = self.c4 and C4.deterministic(self.iter, 0, self.warmup_sum, True)
        res = simulate_step(Gs, self.Es, self.shapes, ratio, self.r, seed, rows, dense_1d=self.c4,
                            restart=restart, proj_device=proj_device)
        self.Es = res["E_new"]
        self.bits += 2 * (self.ws - 1) * res["bits"]
        self.iter += 1
        return dict(out=res["out"], ratio=ratio, seed=seed, restart=restart, res=res)
