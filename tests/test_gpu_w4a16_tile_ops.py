"""k_gemm_w4a16_tile through its op entry (vsim_op_q4_gemm_w4a16_tile) against the kernel it must equal
bit for bit: vsim_op_q4_gemm_w4a16_rows on consecutive 32-row chunks of the same operand.

Shapes: M in {16, 40, 96, 200} (half a W4T32 tile, ragged tiles, one beyond any TM <= 128 with a ragged
rest) x K in {32, 64, 544, 1056, 2080} (one block, fewer blocks than partials, ragged strands on both
sides of 16, a long strand), 300 activation rows (tests/w4a16_tile_cases.py), every n at the seams of
a 16-, 32-, 64-, 128- or 256-row tile.  The launcher takes 64 weight rows per workgroup from 256
workgroups on and 32 below; M = 4,104 (129 W4T32 tiles: the last 64-row group has one tile only) is
there for the first form, at the n on both sides of that threshold.
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import w4a16_ref as W  # noqa: E402
import w4a16_tile_cases as C  # noqa: E402
from test_gpu_w4a16_ops import DEV, EINVAL, bits, dev, host, product, repack  # noqa: E402
from vsim_amd import hip  # noqa: E402

pytestmark = pytest.mark.gpu

N = C.N_ROWS
M_WIDE = 4104


def operand_rows(x, n, K, guard=1, guard_value=7.0):
    """vsim_op_w4a16_rows of the first n rows of the device tensor x [>= n][K] in chunks of 32 rows,
    into buffers of exactly n rows followed by `guard` guard rows; returns (x16, e) on the device."""
    x16 = torch.full(((n + guard) * K,), guard_value, dtype=torch.float16, device=DEV)
    e = torch.full((n + guard,), 12345, dtype=torch.int32, device=DEV)
    for r0 in range(0, n, 32):
        c = min(32, n - r0)
        hip.w4a16_rows(x[r0:r0 + c].contiguous(), K, c, x16[r0 * K:], e[r0:])
    return x16, e


def chunked(w, M, K, x16, e, n, bias):
    """The reference: the rows entry on consecutive chunks of 32 rows."""
    out = np.empty((n, M), np.float32)
    for r0 in range(0, n, 32):
        c = min(32, n - r0)
        out[r0:r0 + c] = product(w, M, K, x16[r0 * K:], e[r0:], c, bias)
    return out


def tile(w, M, K, x16, e, n, bias, rows=N + 1):
    """The tile entry on a NaN-prefilled y of `rows` rows."""
    y = torch.full((rows * M,), float("nan"), dtype=torch.float32, device=DEV)
    hip.q4_gemm_w4a16_tile(w, M, K, x16, e, n, bias, y)
    out = host(y).reshape(rows, M)
    assert np.isnan(out[n:]).all(), "rows >= n written"
    return out[:n]


@functools.lru_cache(maxsize=None)
def activations(K):
    """The 300 rows of a K, their operand on the device and on the host: made once per K."""
    x = C.activations(K, C.case_seed(K))
    x16, e = operand_rows(dev(x), N, K)
    hr, er = W.row_operand(x)
    hh, eh = host(x16).reshape(N + 1, K), host(e)
    assert np.array_equal(eh[:N], er) and np.array_equal(hh[:N].view(np.uint16), hr.view(np.uint16))
    assert (hh[N] == 7.0).all() and eh[N] == 12345
    return x, x16, e, hr, er


@functools.lru_cache(maxsize=None)
def reference(M, K):
    """The weight of a case and the chunked rows kernel's 300 rows, without and with bias: once."""
    aos, b = C.weight(M, K)
    w, bd = repack(aos, M, K), dev(b)
    _, x16, e, _, _ = activations(K)
    return aos, w, bd, chunked(w, M, K, x16, e, N, None), chunked(w, M, K, x16, e, N, bd)


def same(got, want, what):
    if not np.array_equal(bits(got), bits(want)):
        bad = np.argwhere(bits(got) != bits(want))
        pytest.fail(f"{what}: {len(bad)} values differ, first (row, weight row) {bad[:4].tolist()}")


@pytest.mark.parametrize("K", C.KS)
@pytest.mark.parametrize("M", C.MS)
def test_bit_for_bit_the_rows_kernel(M, K):
    _, w, bd, ref, refb = reference(M, K)
    _, x16, e, _, er = activations(K)
    bad = C.bad_rows()
    good = [j for j in range(N) if j not in bad]
    # the reference does what the contract says: the non-finite rule, the neighbours untouched
    assert all(er[j] == W.NONFINITE for j in bad) and (bits(ref[bad]) == W.QNAN_BITS).all() and (bits(refb[bad]) == W.QNAN_BITS).all()
    assert np.isfinite(ref[good]).all() and np.isfinite(refb[good]).all()
    for n in C.NS:
        same(tile(w, M, K, x16, e, n, None), ref[:n], f"M={M} K={K} n={n}")
        same(tile(w, M, K, x16, e, n, bd), refb[:n], f"M={M} K={K} n={n} with bias")


@pytest.mark.parametrize("K", [544, 2080])
def test_the_64_row_form_at_a_ragged_wide_weight(K):
    """M = 4,104: 65 groups of 64 weight rows, so n >= 193 (4 tiles of 64 rows) launches the 64-row
    form and n <= 192 the 32-row one; the last group's second W4T32 tile does not exist."""
    _, w, bd, ref, refb = reference(M_WIDE, K)
    _, x16, e, _, _ = activations(K)
    for n in (192, 193, 255, 256, 257, 300):
        same(tile(w, M_WIDE, K, x16, e, n, None), ref[:n], f"M={M_WIDE} K={K} n={n}")
        same(tile(w, M_WIDE, K, x16, e, n, bd), refb[:n], f"M={M_WIDE} K={K} n={n} with bias")


@pytest.mark.parametrize("M,K", [(40, 544), (200, 1056), (M_WIDE, 544)])
def test_a_permutation_of_the_rows_gives_the_permuted_bits(M, K):
    _, w, bd, ref, refb = reference(M, K)
    x = activations(K)[0]
    perm = np.random.default_rng(M + K).permutation(N)
    for n in (N, 77):
        xp16, ep = operand_rows(dev(x[perm[:n]]), n, K)
        same(tile(w, M, K, xp16, ep, n, bd), refb[perm[:n]], f"M={M} K={K}: {n} permuted rows")
    # a row alone, from every place of a 16-row tile and from the non-finite rows
    for j in list(range(37, 53)) + C.bad_rows()[:3]:
        x1, e1 = operand_rows(dev(x[j:j + 1]), 1, K)
        same(tile(w, M, K, x1, e1, 1, None, rows=2), ref[j:j + 1], f"M={M} K={K}: row {j} alone")


@pytest.mark.parametrize("M,K", [(40, 544), (200, 2080), (M_WIDE, 544)])
def test_nothing_read_behind_the_operands(M, K):
    aos, _, bd, _, refb = reference(M, K)
    x = activations(K)[0]
    w = repack(aos, M, K, slack=8192)              # a NaN-patterned region behind the weight
    for n in (5, 17, 64, 65, 130, 257):
        xg = np.concatenate([x[:n], np.full((3, K), np.nan, np.float32)])
        x16, e = operand_rows(dev(xg), n, K, guard=70, guard_value=float("nan"))  # NaN rows behind row n - 1
        e[n:] = W.NONFINITE
        same(tile(w, M, K, x16, e, n, bd), refb[:n], f"M={M} K={K} n={n}")


def test_within_the_bound_of_the_fp64_product():
    """Not merely self-consistent with its twin: inside the derived bound of the same formula in fp64."""
    import fast_ref as R
    M, K = 96, 1056
    aos, w, bd, _, _ = reference(M, K)
    _, x16, e, hr, er = activations(K)
    wd, wq = R.q4_parse(aos, K)
    good = [j for j in range(N) if er[j] != W.NONFINITE]
    y64, tol = W.product64(wd, wq, hr, er, host(bd))
    got = tile(w, M, K, x16, e, N, bd)
    ratio = W.bound_ratio(got[good], y64[good], tol[good])
    print(f"gemm_w4a16_tile M={M} K={K}: worst error {ratio:.4f} x bound over {len(good)} rows")
    assert ratio <= 1.0


def test_argument_errors():
    M, K = 32, 64
    w = torch.zeros(hip.q4_bytes(M, K), dtype=torch.uint8, device=DEV)
    x16 = torch.zeros(70 * K, dtype=torch.float16, device=DEV)
    e = torch.zeros(70, dtype=torch.int32, device=DEV)
    y = torch.zeros(70 * M, dtype=torch.float32, device=DEV)
    g = hip.lib().vsim_op_q4_gemm_w4a16_tile
    H, Ex, Wp, Y = x16.data_ptr(), e.data_ptr(), w.data_ptr(), y.data_ptr()
    assert g(Wp, M, K, H, Ex, 0, None, Y, None) == EINVAL
    assert g(Wp, M, K, H, Ex, -3, None, Y, None) == EINVAL
    assert g(Wp, M, 48, H, Ex, 2, None, Y, None) == EINVAL
    assert g(Wp, M, 0, H, Ex, 2, None, Y, None) == EINVAL
    assert g(Wp, 0, K, H, Ex, 2, None, Y, None) == EINVAL
    assert g(Wp, -5, K, H, Ex, 2, None, Y, None) == EINVAL
    assert g(None, M, K, H, Ex, 2, None, Y, None) == EINVAL
    assert g(Wp, M, K, None, Ex, 2, None, Y, None) == EINVAL
    assert g(Wp, M, K, H, None, 2, None, Y, None) == EINVAL
    assert g(Wp, M, K, H, Ex, 2, None, None, None) == EINVAL
    assert b"q4_gemm_w4a16_tile" in hip.lib().vsim_last_error()
    assert g(Wp, M, K, H, Ex, 32, None, Y, None) == 0
    assert g(Wp, M, K, H, Ex, 33, None, Y, None) == 0      # (the rows entry's limit does not apply)
    assert g(Wp, M, K, H, Ex, 70, None, Y, None) == 0
    torch.cuda.synchronize()
