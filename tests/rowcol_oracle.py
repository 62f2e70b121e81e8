"""CPU restatement of row- / column-wise TopK and RandK (sparse_type "row" / "column"), test
infrastructure only.  The contract (include/arctopk.h, arctopk_seg_select):

  geometry   1-D: one segment of numel keys; 2-D [R, C]: rows (row mode) or columns (column mode);
             N-D: viewed as [shape[0], numel / shape[0]].  k_seg = max(1, int(seg_len * ratio))
  TopK       per segment the k_seg largest |x|, ties lowest position first: a stable descending
             sort of |x| along the segment, its first k_seg positions, ascending
  RandK hash per segment s of tensor t the k_seg largest keys rk(hseed(t, s), j)
  layout     int32 flat indices into the tensor; row mode: segment-major, ascending inside a
             segment; column mode: [k_seg, C] (entry j of column c at j * C + c)
"""
from __future__ import annotations

from typing import List, Optional

import numpy as np
import torch

from oracle import sparse as S

_M64 = (1 << 64) - 1


def view_2d(shape):
    """(rows, cols, by_segments) -- 1-D tensors are one segment."""
    shape = [int(d) for d in shape]
    n = S.numel_of(shape)
    if len(shape) <= 1:
        return None
    return shape[0], n // shape[0]


def geometry(shape, ratio: float, mode: str):
    """(rows, cols, nseg, seg_len, k_seg, total) of one tensor; mode 'row' / 'column'."""
    v = view_2d(shape)
    if v is None:
        n = S.numel_of(shape)
        r, c = (n, 1) if mode == "column" else (1, n)
    else:
        r, c = v
    nseg, seg_len = (c, r) if mode == "column" else (r, c)
    k = max(1, int(seg_len * ratio))
    return r, c, nseg, seg_len, k, k * nseg


def segments(x: torch.Tensor, shape, mode: str) -> torch.Tensor:
    """The tensor as [nseg, seg_len] (a copy for column mode)."""
    r, c, nseg, seg_len, _, _ = geometry(shape, 1.0, mode)
    m = x.reshape(r, c)
    return m.t().contiguous() if mode == "column" else m


def topk_positions(seg: torch.Tensor, k: int) -> torch.Tensor:
    """[nseg, k] positions within each segment, ascending: strict-above, then lowest position."""
    order = torch.sort(seg.abs().float(), dim=1, descending=True, stable=True).indices[:, :k]
    return torch.sort(order, dim=1).values


def hseed(seed: int, t: int, s: int) -> int:
    z = (seed + 0x9E3779B97F4A7C15 * (t + 1) + 0xD1B54A32D192ED03 * s) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return (z ^ (z >> 31)) & 0xFFFFFFFF


def rk_keys(hs: int, n: int) -> np.ndarray:
    s = np.uint64(hs)
    j = np.arange(n, dtype=np.uint64)
    inner = S._rk_mix(j ^ s)
    m32 = np.uint64(0xFFFFFFFF)
    return S._rk_mix((inner + np.uint64((0x9E3779B9 * (int(s) | 1)) & 0xFFFFFFFF)) & m32)


def hash_positions(nseg: int, seg_len: int, k: int, seed: int, t: int) -> torch.Tensor:
    out = np.empty((nseg, k), dtype=np.int64)
    for s in range(nseg):
        key = rk_keys(hseed(seed, t, s), seg_len).astype(np.int64)
        out[s] = np.sort(np.argsort(-key, kind="stable")[:k])
    return torch.from_numpy(out)


def layout(pos: torch.Tensor, rows: int, cols: int, mode: str) -> torch.Tensor:
    """[nseg, k] positions -> the payload's int32 flat indices."""
    if mode == "column" and cols > 1:  # pos[c, j] = row_j(c): entry j * C + c = row * C + c
        flat = pos.t() * cols + torch.arange(cols).unsqueeze(0)
    elif mode == "column":
        flat = pos
    else:
        flat = pos + torch.arange(pos.shape[0]).unsqueeze(1) * cols
    return flat.flatten().to(torch.int32)


def select_indices(X: torch.Tensor, shapes, ratio: float, mode: str, random: bool,
                   seed: Optional[int]) -> (List[torch.Tensor], List[int]):
    """Per tensor: the payload indices (TopK, or RandK 'hash') and the totals ks."""
    idxs, ks, off = [], [], 0
    for t, shape in enumerate(shapes):
        r, c, nseg, seg_len, k, tot = geometry(shape, ratio, mode)
        if random:
            pos = hash_positions(nseg, seg_len, k, int(seed), t)
        else:
            pos = topk_positions(segments(X[off:off + r * c], shape, mode), k)
        idxs.append(layout(pos, r, c, mode))
        ks.append(tot)
        off += r * c
    return idxs, ks


def host_draws(shapes, ratio: float, mode: str, seed: int) -> List[torch.Tensor]:
    """RandK index_source='host': the reference's CPU draws after torch.manual_seed(seed)
    (sparsify_by_row :46, sparsify_by_column :66; 1-D: randperm(numel)[:k])."""
    torch.manual_seed(int(seed))
    out = []
    for shape in shapes:
        r, c, nseg, seg_len, k, _ = geometry(shape, ratio, mode)
        if mode == "column" and c > 1:
            idx = torch.stack([torch.randperm(r)[:k] for _ in range(c)], dim=1)
            idx = idx * c + torch.arange(c).unsqueeze(0)
        elif mode == "row" and r > 1:
            idx = torch.stack([torch.randperm(c)[:k] for _ in range(r)], dim=0)
            idx = idx + torch.arange(r).unsqueeze(1) * c
        else:
            idx = torch.randperm(r * c)[:k]
        out.append(idx.flatten().to(torch.int32))
    return out


def pack(X: torch.Tensor, shapes, idxs, ks, ef: str, random: bool):
    """oracle.sparse.pack with given indices and totals; mutates X per EF mode."""
    vals, bits, off = [], 0, 0
    for shape, idx, k in zip(shapes, idxs, ks):
        n = S.numel_of(shape)
        v = X[off:off + n]
        val = v[idx.long()].clone()
        assert val.numel() == k
        vals.append(val)
        bits += k * torch.finfo(X.dtype).bits + (0 if random else k * 32)
        if ef == "ef14":
            v[idx.long()] = 0
        elif ef == "ef21":
            v.zero_()
            v[idx.long()] = val
        off += n
    return torch.cat(vals), torch.cat(idxs), bits


def simulate_step(Gs, Es, gE, shapes, ratio: float, mode: str, ef: str, random: bool, seed=None,
                  index_source: str = "hash", error_decay: float = 1.0):
    """One compressed call on len(Gs) ranks (the structure of oracle.sparse.simulate_step)."""
    ws = len(Gs)
    Xs, packs = [], []
    ks = None
    for G, E in zip(Gs, Es):
        X = S.encode(G, E, ef)
        if random and index_source == "host":
            idxs = host_draws(shapes, ratio, mode, seed)
            ks = [geometry(s, ratio, mode)[5] for s in shapes]
        else:
            idxs, ks = select_indices(X, shapes, ratio, mode, random, seed)
        packs.append(pack(X, shapes, idxs, ks, ef, random))
        Xs.append(X)
    numel = Gs[0].numel()
    if random:
        vsum = packs[0][0].clone()
        for q in range(1, ws):
            vsum = vsum + packs[q][0]
        out = S.decode_randk(vsum, packs[0][1], shapes, ks, ws, numel)
    else:
        out = S.decode_topk([p[0] for p in packs], [p[1] for p in packs], shapes, ks, ws, numel)
    E_new = []
    for X, E in zip(Xs, Es):
        if ef == "ef14":
            E_new.append(X.clone())
        elif ef == "ef21":
            E_new.append(E.clone().add_(X, alpha=error_decay))
        else:
            E_new.append(None)
    gE_new = None
    if ef == "ef21":
        gE_new = gE.clone().add_(out, alpha=error_decay)
        out = gE_new.clone()
    return dict(values=[p[0] for p in packs], indices=[p[1] for p in packs], ks=ks,
                bits=packs[0][2], out=out, E_new=E_new, gE_new=gE_new)


# ---- the reference's own selections (tests/golden/rowcol_select.npz, make_golden_rowcol.py) ----

def golden_load():
    import json
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rowcol_select.npz"))
    return dict(z=z, pool=torch.from_numpy(z["pool"]),
                shapes={m: json.loads(str(z[f"{m}_shapes"])) for m in ("row", "column")})


def golden_input(g, i: int, shape) -> torch.Tensor:
    n = S.numel_of(shape)
    pool = g["pool"]
    return pool[(torch.arange(n) + 1009 * i) % pool.numel()].clone()


def golden_positions(g, mode: str, ratio: float) -> List[torch.Tensor]:
    """Per tensor the reference's [nseg, k_seg] positions within each segment, ascending."""
    flat = torch.from_numpy(g["z"][f"{mode}_r{ratio}_pos"].astype(np.int64))
    out, off = [], 0
    for shape in g["shapes"][mode]:
        _, _, nseg, _, k, tot = geometry(shape, ratio, mode)
        out.append(flat[off:off + tot].reshape(nseg, k))
        off += tot
    assert off == flat.numel()
    return out


def payload_positions(idx: torch.Tensor, shape, ratio: float, mode: str) -> torch.Tensor:
    """A tensor's payload indices back as [nseg, k_seg] positions (checks the layout: every
    entry lies in the segment its place in the payload says)."""
    r, c, nseg, seg_len, k, tot = geometry(shape, ratio, mode)
    idx = idx.long()
    assert idx.numel() == tot
    if mode == "column" and c > 1:
        grid = idx.reshape(k, c)
        assert torch.equal(grid % c, torch.arange(c).unsqueeze(0).expand_as(grid)), "column layout"
        return (grid // c).t().contiguous()
    if mode == "column":
        return idx.reshape(1, k)
    grid = idx.reshape(nseg, k)
    assert torch.equal(grid // c, torch.arange(nseg).unsqueeze(1).expand_as(grid)), "row layout"
    return grid % c
