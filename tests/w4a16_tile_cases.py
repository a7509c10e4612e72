"""Inputs and a numpy restatement for k_gemm_w4a16_tile (vsim_amd/csrc/gemm_w4a16_tile.hip), shared by
tests/test_gpu_w4a16_tile_ops.py (the device against k_gemm_w4a16_rows, bit for bit) and
tests/test_w4a16_tile_cpu.py (the inputs have teeth: a kernel that split the strands, added the
partials or rounded the fma another way would change bits on them).

The product per (weight row, activation row), as gemm_w4a16_rows.hip states it:
  dot_b   = the matrix core's sum, from C = 0, of block b's 32 products (q - 8) * h;
  part[p] = fmaf(d_w[b], dot_b, part[p]) over b = p, p + 16, ... in ascending b, p = 0 .. 15;
  sum     = ((0 + part[0]) + part[1]) + ... + part[15];
  y       = ldexpf(sum, -e) (+ bias).
numpy cannot restate the matrix core's inner order, so dot_b here is a stand-in shared by every
variant: the exact sum (fp64 holds it: 32 terms of 4 + 11 bits over at most 41 binades) rounded once
to fp32.  Everything after it is restated exactly, the fma by a round-to-odd fp64 sum.
"""
import numpy as np

import fast_ref as R
import w4a16_ref as W

QK = 32
P = 16
N_ROWS = 300
PERIOD = 37       # the 32 row families, then 5 fresh random rows
MS = (16, 40, 96, 200)
KS = (32, 64, 544, 1056, 2080)
NS = (1, 16, 17, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300)
VARIANTS = ("contiguous_strands", "pairwise_tree", "two_roundings")
# families' rows whose operand is non-zero in one block only (one 1e30 outlier, one last element):
# a single non-zero term, on which every order and every rounding of the later steps agrees
ONE_BLOCK_FAMILIES = (3, 13)
ZERO_FAMILIES = (5, 6)
# ... and the row of f32 subnormals: its outputs are f32 subnormals, which the final scaling rounds
# once more, so that differences in the sum's low bits do not reach the output
SUBNORMAL_FAMILY = 4


def activations(K, seed):
    """x [300][K] float32: copies of tests/test_gpu_w4a16_ops.py's 32 row families (fresh random
    draws per copy) with 5 fresh random rows of mixed scales after each.  A copy starts at 37 k, and
    37 = 5 mod 16, so the families' NaN and Inf rows (8, 10, 12 of a copy) stand at another position
    of their 16-row tile in every copy (row 8: 8, 13, 2, 7, 12, 1, 6, 11)."""
    from test_gpu_w4a16_ops import families
    rng = np.random.default_rng(1000 + seed)
    x = np.empty((N_ROWS, K), np.float32)
    for r0 in range(0, N_ROWS, PERIOD):
        blk = np.concatenate([families(K, seed + r0), (rng.standard_normal((5, K)) * 10.0 ** rng.integers(-3, 4, (5, 1))).astype(np.float32)])
        x[r0:r0 + PERIOD] = blk[:N_ROWS - r0]
    return x


def family_of(j):
    """The family index of row j of activations(), or -1 for a random row between the copies."""
    return j % PERIOD if j % PERIOD < 32 else -1


def bad_rows(n=N_ROWS):
    from test_gpu_w4a16_ops import BAD_ROWS
    return [j for j in range(n) if family_of(j) in BAD_ROWS]


def weight(M, K):
    """(AoS Q4_0 blocks, bias [M]) of the case (M, K): tests/test_gpu_w4a16_ops.py's weights()."""
    from test_gpu_w4a16_ops import weights
    return weights(M, K, 31 * M + K)


# The activations of a case depend on K alone: the four weights of a K meet the same 300 rows, and
# tests/test_w4a16_tile_cpu.py asks every wrong variant to bite every row in at least one output of
# the four (352 outputs per row; at K = 544 a single weight of 16 rows would not do: a row then has
# 16 outputs with one two-block strand each, and the two-rounding fma differs from the true one in
# about one such output in twenty).  SEEDS: an offset per K should a seed not bite (none needed).
SEEDS = {}


def case_seed(K):
    return K + 7919 * SEEDS.get(K, 0)


# ------------------------------------------------------------------ the restatement
def block_dots(wq, h):
    """[n][M][nb] float32: the stand-in for the matrix core's block sums (exact, rounded once)."""
    M, nb, _ = wq.shape
    hv = np.asarray(h, np.float16).astype(np.float64).reshape(-1, nb, QK)
    return np.einsum("mbi,nbi->nmb", wq.astype(np.float64), hv).astype(np.float32)


def fma32(a, b, c):
    """fmaf(a, b, c) on float32 arrays, one rounding: a * b is exact in fp64, the sum with c is taken
    to fp64 by round-to-odd (TwoSum gives the error's sign), which a final rounding to 24 bits cannot
    tell from the exact sum."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c64 = c.astype(np.float64)
    t = p + c64
    bb = t - p
    err = (p - (t - bb)) + (c64 - bb)
    even = (t.view(np.int64) & 1) == 0
    t = np.where((err != 0) & even, np.nextafter(t, np.where(err > 0, np.inf, -np.inf)), t)
    return t.astype(np.float32)


def emulate(wd, dots, e, bias=None, wrong=None):
    """y [n][M] float32 of the formula on the block sums `dots` [n][M][nb]; rows with e == NONFINITE
    are NaN (0x7FC00000).  wrong: None, or one of VARIANTS --
      contiguous_strands: strand p takes blocks p L .. p L + L - 1, L = ceil(nb / 16), not b mod 16;
      pairwise_tree:      the sixteen partials added as a balanced tree, not in order from 0;
      two_roundings:      part = fl(fl(d * dot) + part), not the fma."""
    assert wrong is None or wrong in VARIANTS
    wd = np.asarray(wd, np.float32)
    n, M, nb = dots.shape
    L = -(-nb // P)
    part = np.zeros((P, n, M), np.float32)
    for p in range(P):
        blocks = range(p * L, min(nb, p * L + L)) if wrong == "contiguous_strands" else range(p, nb, P)
        for b in blocks:
            d = np.broadcast_to(wd[None, :, b], (n, M))
            if wrong == "two_roundings":
                part[p] = (d * dots[:, :, b]).astype(np.float32) + part[p]
            else:
                part[p] = fma32(d, dots[:, :, b], part[p])
    if wrong == "pairwise_tree":
        lvl = [part[p] for p in range(P)]
        while len(lvl) > 1:
            lvl = [lvl[i] + lvl[i + 1] for i in range(0, len(lvl), 2)]
        s = lvl[0]
    else:
        s = np.zeros((n, M), np.float32)
        for p in range(P):
            s = s + part[p]
    y = np.empty((n, M), np.float32)
    for j in range(n):
        if e[j] == W.NONFINITE:
            y[j] = np.uint32(W.QNAN_BITS).view(np.float32)
            continue
        v = np.ldexp(s[j], -int(e[j])).astype(np.float32)
        y[j] = v + np.asarray(bias, np.float32) if bias is not None else v
    return y


def case(M, K):
    """(aos, bias, wd, wq, x, h, e) of the GPU test's case (M, K)."""
    aos, b = weight(M, K)
    wd, wq = R.q4_parse(aos, K)
    x = activations(K, case_seed(K))
    h, e = W.row_operand(x)
    return aos, b, wd, wq, x, h, e
