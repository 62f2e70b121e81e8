"""Generate tests/golden/rowcol_select.npz: the reference's own row- and column-wise TopK
selections (sparsify_by_row / sparsify_by_column, cal_k_by_row / cal_k_by_column of
comm_hooks/sparse_hook.py, imported from the read-only reference checkout on the build machine
only; no reference source is written anywhere).

Stored:
  pool            a seeded fp32 vector of POOL elements.  Tensor number i of a shape list is
                  pool[(arange(numel) + 1009 * i) % POOL]: POOL is a prime above every segment
                  length and no stride of a column is a multiple of it, so no segment sees a pool
                  element twice, and the inputs of the largest shapes need no storage of their own
  {mode}_shapes   the shape lists, as json (N-D shapes are handed to the reference as their
                  [shape[0], numel / shape[0]] view: its own unpack of tensor.shape raises for them)
  {mode}_r{ratio}_k     per tensor, the reference's cal_k_by_{row,column}
  {mode}_r{ratio}_pos   per tensor, concatenated: the reference's selected positions within each
                        segment, sorted ascending, segment-major, as uint16

The generator asserts that no segment has a tie at its threshold, so every segment of the fixture
has exactly one right answer.

Usage:  python tests/golden/make_golden_rowcol.py REFERENCE_CHECKOUT
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
POOL = 65521
ROW = [[7], [40, 16], [4, 3, 3, 3], [96, 40], [3, 1000], [1, 5], [5, 1], [257, 130], [63, 65], [300, 1025],
       [2, 13000]]
COLUMN = [[7], [16, 40], [4, 3, 3, 3], [1000, 3], [130, 257], [5, 1], [1, 5], [65, 63], [64, 129], [3000, 70]]
RATIOS = [0.2, 0.01]


def tensor_input(pool: torch.Tensor, i: int, shape) -> torch.Tensor:
    n = int(np.prod(shape))
    return pool[(torch.arange(n) + 1009 * i) % pool.numel()].clone()


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    sys.path.insert(0, sys.argv[1])
    from comm_hooks import sparse_hook as R  # the reference
    pool = torch.randn(POOL, generator=torch.Generator().manual_seed(20251))
    out = {"pool": pool.numpy(), "row_shapes": np.array(json.dumps(ROW)),
           "column_shapes": np.array(json.dumps(COLUMN))}
    for mode, shapes, fn, calk in (("row", ROW, R.sparsify_by_row, R.cal_k_by_row),
                                   ("column", COLUMN, R.sparsify_by_column, R.cal_k_by_column)):
        for ratio in RATIOS:
            ks, pos = [], []
            for i, shape in enumerate(shapes):
                x = tensor_input(pool, i, shape)
                t = x.reshape(shape) if len(shape) <= 2 else x.reshape(shape[0], -1)
                k = int(calk(t, ratio))
                res = fn(t, ratio)
                idx = res[1].long().flatten()
                assert idx.numel() == k
                if t.dim() == 1:
                    nseg, seg_len, seg, p = 1, t.numel(), t.abs().unsqueeze(0), idx.unsqueeze(0)
                elif mode == "row":
                    nseg, seg_len, seg = t.shape[0], t.shape[1], t.abs()
                    p = (idx % seg_len).reshape(nseg, -1)
                    assert torch.equal(idx.reshape(nseg, -1) // seg_len,
                                       torch.arange(nseg).unsqueeze(1).expand(nseg, k // nseg))
                else:
                    nseg, seg_len, seg = t.shape[1], t.shape[0], t.abs().t()
                    grid = idx.reshape(-1, nseg)  # [k_seg, C]
                    assert torch.equal(grid % nseg, torch.arange(nseg).unsqueeze(0).expand_as(grid))
                    p = (grid // nseg).t()
                p = torch.sort(p, dim=1).values
                kseg = p.shape[1]
                srt = torch.sort(seg, dim=1, descending=True).values
                if kseg < seg_len:  # no tie at the threshold, in any segment
                    assert bool((srt[:, kseg - 1] > srt[:, kseg]).all()), (mode, ratio, shape)
                assert seg_len < 65536
                ks.append(k)
                pos.append(p.flatten().numpy().astype(np.uint16))
            out[f"{mode}_r{ratio}_k"] = np.array(ks, dtype=np.int64)
            out[f"{mode}_r{ratio}_pos"] = np.concatenate(pos)
    path = os.path.join(HERE, "rowcol_select.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
