"""CPU restatement of the c4 variant of the ARC-TopK hook (test infrastructure only).

Written from the semantics of the reference's comm_hooks/group_topk_hook_no_reshape_c4.py
(line numbers below are that file's), on top of the base hook's restatement in
``oracle.arctopk`` (whose encode / select / pack / decode helpers it reuses):

* 1-D tensors are DENSE (:19-25): no sketch, no select, every element a selected "row";
* the ratio ramps from 0.8 to the base ratio (:186-200) once compression has started (:250-251),
  and ``cal_k`` uses the ratio in force (:202-219);
* during the ramp (:300) every 2-D / ND tensor's V is drawn by a fresh generator seeded with
  the call's seed (:31-39); afterwards by the global stream, as the base hook.

Deviation, on purpose: with EF21 a 1-D tensor is treated as a tensor whose rows are all
selected (D = G - E; packed = D; E += D; out = gE + mean(D); gE := out), where the reference
raises (tests/golden/c4arc_ef21_1d_error.json).

``C4Oracle`` replays whole calls on ``ws`` ranks in one process (sums in rank order: bitwise
what gloo computes for ws <= 2); ``simulate_step`` is one compressed call, with
``rows_override`` / ``proj_device`` as ``oracle.arctopk.simulate_step`` has them.
"""
from __future__ import annotations

from typing import List, Optional

import torch

from oracle import arctopk as A

RAW, SKETCH, DENSE = A.RAW, A.SKETCH, 2
PLAN_DENSE_1D, PLAN_RESTART_DRAWS = 1, 2


def bucket_grad(numel: int, it: int, rank: int, dtype=torch.float32) -> torch.Tensor:
    """The gradient bucket of (iteration, rank) in the c4arc_* fixtures, which store its digest
    instead of the values: make_golden.make_grad's rule (a private CPU generator, randn)."""
    g = torch.Generator().manual_seed(1000 + 100 * it + rank)
    return torch.randn(numel, generator=g).to(dtype)


def digest(t: torch.Tensor) -> str:
    """SHA-256 of a tensor's bytes: the fixtures pin E / gE of every call by digest (bitwise) and
    hold the arrays themselves for the last call only, to stay small."""
    import hashlib
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def current_ratio(base: float, it: int, start: int, warmup_sum: int, gradual: bool = True,
                  started: bool = True) -> float:
    """get_current_compress_ratio (:186-200); warmup_sum = start_compress_iter + warmup_iters."""
    if not gradual or not started:
        return base
    p = it - start
    if p < warmup_sum:
        return max(0.8 - (0.8 - base) * (p / warmup_sum), base)
    return base


def deterministic(it: int, start: int, warmup_sum: int, started: bool = True) -> bool:
    """use_deterministic (:300)."""
    return started and it - start < warmup_sum


def segments(shapes, ratio: float) -> List[A.Segment]:
    out, off = [], 0
    for s in shapes:
        kind, n, m = A.geometry(s)
        if kind == RAW:
            out.append(A.Segment(DENSE, off, n, n, 1, n, tuple(s)))
        else:
            out.append(A.Segment(kind, off, n * m, n, m, max(1, int(n * ratio)), tuple(s)))
        off += n * m
    return out


def cal_k(shape, ratio: float) -> int:
    """cal_k (:202-219) at the ratio in force."""
    kind, n, m = A.geometry(shape)
    return n if kind == RAW else max(1, int(n * ratio)) * m


def plan_geometry(shapes, ratio: float, r: int):
    """What arctopk_plan_describe_ex(..., ARCTOPK_PLAN_DENSE_1D) must report: per segment
    (kind, offset, n, m, k_rows, sketch_off, v_off, packed_off, row_off, sel_off) and the totals."""
    rows, sk, vo, po, ro, so, vals = [], 0, 0, 0, 0, 0, 0
    for s in segments(shapes, ratio):
        rows.append(dict(kind=s.kind, offset=s.offset, n=s.n, m=s.m, k_rows=s.k_rows, sketch_off=sk,
                         v_off=vo if s.kind == SKETCH else -1, packed_off=po, row_off=ro, sel_off=so))
        if s.kind == SKETCH:
            sk += s.n * r
            vo += s.m * r
        po = (po + s.k + 3) // 4 * 4  # segments start 16-B aligned in the packed buffer
        vals += s.k
        ro += s.n
        so += s.k_rows
    info = dict(numel=sum(s.numel for s in segments(shapes, ratio)), sketch_len=sk, v_len=vo, packed_len=po,
                sel_rows=so, rows_total=ro, nseg=len(rows), r=r, values_len=vals)
    return rows, info


def draw_projections(seed: int, segs, r: int, dtype=torch.float32, restart: bool = False, device=None):
    """V per SKETCH tensor.  restart (the ramp, :31-39): ``torch.empty(m, r).normal_(generator=g)``
    with g a NEW generator on the tensor's device seeded with the call's seed, per tensor.
    Otherwise the base hook's stream (V.normal_() after torch.manual_seed(seed), :39, :297)."""
    if not restart:
        return A.draw_projections(seed, segs, r, dtype, device=device)
    out = []
    for s in segs:
        if s.kind != SKETCH:
            out.append(None)
            continue
        g = torch.Generator(device=device if device is not None else "cpu")
        g.manual_seed(int(seed))
        out.append(torch.empty(s.m, r, dtype=dtype, device=device).normal_(generator=g).cpu())
    return out


def threshold_gap(norms: torch.Tensor, k: int) -> float:
    """Relative gap between the k-th and (k+1)-th largest energy (inf when k = n)."""
    if k >= norms.numel():
        return float("inf")
    top = torch.sort(norms.double(), descending=True).values
    a, b = float(top[k - 1]), float(top[k])
    return (a - b) / a if a > 0 else 0.0


def bits_per_call(segs, r: int, dtype_bits: int) -> int:
    """P_bits + comm_bits per tensor (:22-23, :43, :59): a DENSE tensor has no sketch."""
    return sum(((s.n * r if s.kind == SKETCH else 0) + s.k) * dtype_bits for s in segs)


def simulate_step(Gs, Es, gE, shapes, ratio: float, r: int, ef: str, seed: int, restart: bool,
                  rows_override=None, proj_device=None):
    """One compressed call on len(Gs) ranks.  rows_override: per segment the selected rows (None
    entries, and every DENSE segment, keep the restatement's own)."""
    ws = len(Gs)
    segs = segments(shapes, ratio)
    Vs = draw_projections(seed, segs, r, Gs[0].dtype, restart, device=proj_device)
    Xs, Pls = [], []
    for G, E in zip(Gs, Es):
        X = G.clone()
        if E is not None and ef in ("ef14", "ef21"):  # (:266-276); the first EF14 call adds nothing
            X.add_(E, alpha=1.0 if ef == "ef14" else -1.0)
        Xs.append(X)
        Pls.append([X[s.offset:s.offset + s.numel].view(s.n, s.m) @ V if s.kind == SKETCH else None
                    for s, V in zip(segs, Vs)])
    norms, rows, gaps = [], [], []
    for j, s in enumerate(segs):
        if s.kind != SKETCH:  # (:24) indices = arange(d)
            norms.append(None)
            rows.append(torch.arange(s.n))
            continue
        acc = Pls[0][j].clone()
        for q in range(1, ws):
            acc = acc + Pls[q][j]
        acc /= ws
        nrm = torch.sum(acc.square(), dim=1)
        _, idx = torch.topk(nrm, k=s.k_rows, largest=True, sorted=False)
        norms.append(nrm)
        rows.append(idx)
        gaps.append((j, threshold_gap(nrm.float(), s.k_rows)))
    if rows_override is not None:
        rows = [rows[j] if (x is None or segs[j].kind != SKETCH) else torch.as_tensor(x, dtype=torch.int64)
                for j, x in enumerate(rows_override)]
    vals = [A.pack(X, rows, segs, ef) for X in Xs]
    vsum = vals[0].clone()
    for q in range(1, ws):
        vsum = vsum + vals[q]
    out = A.decode(vsum, ws, rows, segs, Gs[0].numel(), Gs[0].dtype)
    E_new = []
    for X, E in zip(Xs, Es):
        E_new.append(X.clone() if ef == "ef14" else (E + X if ef == "ef21" else None))
    gE_new = None
    if ef == "ef21":
        gE_new = gE + out
        out = gE_new.clone()
    return dict(segs=segs, V=Vs, norms=norms, rows=rows, gaps=gaps, out=out, E_new=E_new, gE_new=gE_new,
                bits=bits_per_call(segs, r, torch.finfo(Gs[0].dtype).bits))


class C4Oracle:
    """The c4 hook's state and calls on `ws` ranks (one bucket, index 0, is_last)."""

    def __init__(self, ws: int, shapes, ratio: float, r: int = 4, start: int = 2, ef: str = "noef",
                 seed: int = 0, gradual: bool = True, warmup_iters: int = 100):
        self.ws, self.shapes, self.base_ratio, self.r = ws, [tuple(s) for s in shapes], ratio, r
        self.start, self.ef, self.gradual = start, ef, gradual
        self.warmup_sum = start + warmup_iters  # (:164)
        self.iter = 0
        self.started = False
        self.bits = 0
        self.rng = torch.Generator().manual_seed(seed)
        self.Es: List[Optional[torch.Tensor]] = [None] * ws
        self.gE = None

    def ratio_now(self) -> float:
        return current_ratio(self.base_ratio, self.iter, self.start, self.warmup_sum, self.gradual,
                             self.started)

    def call(self, Gs, rows_override=None, proj_device=None):
        """One hook call per rank; returns dict(kind, out, ratio, seed, restart, res)."""
        ws, eb = self.ws, torch.finfo(Gs[0].dtype).bits
        if self.iter < self.start:  # dense warm-up (default_hooks._allreduce_fut)
            acc = Gs[0] / ws
            for q in range(1, ws):
                acc = acc + Gs[q] / ws
            self.bits += 2 * (ws - 1) * Gs[0].numel() * eb
            self.iter += 1
            return dict(kind="warmup", out=acc, ratio=None)
        self.started = True  # (:250-251), before the ratio is read
        ratio = self.ratio_now()
        if self.ef == "ef21" and self.Es[0] is None:  # EF21 init (:273-292)
            self.Es = [G.clone() for G in Gs]
            acc = Gs[0].clone()
            for q in range(1, ws):
                acc = acc + Gs[q]
            acc.div_(ws)
            self.gE = acc.clone()
            self.bits += Gs[0].numel() * eb
            self.iter += 1
            return dict(kind="ef21_init", out=acc.clone(), ratio=ratio)
        seed = int(torch.randint(0, 1_000_000_000, (1,), generator=self.rng).item())
        restart = deterministic(self.iter, self.start, self.warmup_sum, self.started)
        res = simulate_step(Gs, self.Es, self.gE, self.shapes, ratio, self.r, self.ef, seed, restart,
                            rows_override=rows_override, proj_device=proj_device)
        if self.ef in ("ef14", "ef21"):
            self.Es = res["E_new"]
        if self.ef == "ef21":
            self.gE = res["gE_new"]
        self.bits += 2 * (ws - 1) * res["bits"]
        self.iter += 1
        return dict(kind="compressed", out=res["out"], ratio=ratio, seed=seed, restart=restart, res=res)
