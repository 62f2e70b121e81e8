"""Shapes, inputs and expectations shared by the sketch-rank tests (test infrastructure only).

RANK_MIX holds, at every sketch rank r = 1 .. 8 and in both dtypes, every encode path of the plan
(csrc/plan.hip; bounds re-derived in tests/test_sketch_rank_host.py):

  [10]                     1-D pass-through; at r = 4 every later sketch offset is 10, 17 or 22 plus
                           a multiple of 4, so the select's aligned-quad energy path (R == 4 and
                           sketch_off % 4 == 0) is not taken: r = 4 runs the generic code here too
  [40, 16] .. [512, 2]     thread-per-row LDS tiles (m < 64), ND shapes among them
  [300, 62], [300, 63]     (256 m + m r) * 4 <= 65536 holds for m = 62 at every r, for m = 63 only
                           up to r = 4: [300, 63] is an LDS tile at r <= 4, wave-per-row at r >= 5
  [7]                      1-D; the bucket offset behind it is odd
  [33, 130], [64, 72]      wave-per-row at an odd offset: the scalar path
  [5]                      1-D; brings the offset to 48320, a multiple of 8 (see below)
  [130, 2048]              wave-per-row, 16-byte loads, unsplit at every r (max_cols(8) = 2048)
  [5, 2056], [6, 2049]     16-byte and scalar; split only at r = 8, and only there m * r * 4 > 65536
                           (the fp32-residual encode then reads V from global memory)
  [9, 5632], [6, 4101]     scalar; 1, 1, 2, 2, 2, 3, 3, 3 and 1, 1, 1, 2, 2, 2, 2, 3 column parts
  [3, 16388]               two parts even at r = 1; 16-byte loads in fp32 (offset 412428 = 4 * 103107),
                           scalar in bf16

A 16-byte path needs m and the bucket offset to be multiples of 4 (fp32) or 8 (bf16).  As the list
was first proposed, without the [5], every wave-per-row tensor sat at an odd offset and the set held
no ENC_ROW_VEC tile in either dtype; with it [130, 2048] and [5, 2056] take 16-byte loads in both
dtypes.  test_gpu_sketch_rank.py asserts the modes with arctopk_diag_encode_tiles.
"""
import torch

RANK_MIX = [[10], [40, 16], [4, 3, 3, 3], [16, 8, 1, 1], [512, 2], [300, 62], [300, 63], [7],
            [33, 130], [64, 72], [5], [130, 2048], [5, 2056], [6, 2049], [9, 5632], [6, 4101], [3, 16388]]
RANK_LARGE = [[20000, 8], [30], [16000, 72], [20000], [7, 9]]
# column-split tensors of RANK_MIX per rank, fp32: m > (65536 / (4 r)) rounded down to a multiple of 4
N_SPLIT_F32 = {1: 1, 2: 1, 3: 2, 4: 3, 5: 3, 6: 3, 7: 3, 8: 5}
# (dtype, r) for which torch's CPU sum over dim 1 -- the oracle's row energy -- does not add in the
# kernels' sequential order.  fp32 r = 5, 6, 7: about 40 % of rows differ in the last bits.  bf16
# r = 5 .. 8: the fp32 accumulation order differs too, but shows only where the two fp32 sums fall on
# either side of a bf16 rounding boundary (measured: 0 to 8 of 2,000,000 random rows per rank)
ORDER_DEPENDENT = {(torch.float32, 5), (torch.float32, 6), (torch.float32, 7),
                   (torch.bfloat16, 5), (torch.bfloat16, 6), (torch.bfloat16, 7), (torch.bfloat16, 8)}


def max_cols(r: int, dtype) -> int:
    """Columns of one column part: V^T [r][cols] fp32 within 64 KiB, in whole 16-byte units."""
    va = 8 if dtype == torch.bfloat16 else 4
    return 65536 // (4 * r) // va * va


def sequential_energy(P: torch.Tensor) -> torch.Tensor:
    """sum_j P[:, j]^2 as the kernels form it: ((q0 + q1) + q2) + ..., squares in P's dtype (as
    the oracle's P ** 2), the sum in fp32, one rounding to P's dtype."""
    q = P ** 2
    s = q[:, 0].float()
    for j in range(1, P.shape[1]):
        s = s + q[:, j].float()
    return s.to(P.dtype)


def energy_band(r: int, dtype=torch.float32) -> float:
    """Relative distance of two summation orders of r non-negative terms added in fp32: each order
    is within (r - 1) roundings of 2^-24 relative of the exact sum.  Rounded once to bf16 the two are
    equal or neighbouring bf16 values: at most 2^-7 apart, relative."""
    return 2.0 ** -7 if dtype == torch.bfloat16 else 2.0 * (r - 1) * 2.0 ** -24


# Integer inputs: every product, partial sum and sum of X.view(n, m) @ V is an integer of magnitude
# at most 5 * 16388 < 2^24, so fp32 accumulation is exact in any order (column-split partials
# included) and the sketch is known bit for bit.  (The multipliers are coprime to the moduli: with
# G[i] = (7 i + 3) % 7 - 3 the bucket would be all zeros, and ((3 c + 5 j) % 3) - 1 does not depend
# on the column c, so neither could show a wrong column.)
def integer_bucket(n: int, mul: int = 5, add: int = 3, mod: int = 7) -> torch.Tensor:
    """G[i] = (mul * i + add) % mod - mod // 2, int64: integers in [-3, 3] by default."""
    return (torch.arange(n, dtype=torch.int64) * mul + add) % mod - mod // 2


def integer_residual(n: int) -> torch.Tensor:
    """E[i] = (3 i + 1) % 5 - 2, int64: integers in [-2, 2]."""
    return integer_bucket(n, 3, 1, 5)


def integer_projection(m: int, r: int) -> torch.Tensor:
    """V[c][j] = ((3 c + 5 j) % 7) % 3 - 1, [m, r] int64: integers in [-1, 1] that depend on both the
    column and the projection column."""
    c = torch.arange(m, dtype=torch.int64)[:, None]
    j = torch.arange(r, dtype=torch.int64)[None, :]
    return (3 * c + 5 * j) % 7 % 3 - 1
