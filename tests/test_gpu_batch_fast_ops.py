"""k_gemm_fast_rows through its op entry (vsim_op_q4_gemm_fast_rows), held to two independent checks.

* Bit equality, row by row, with the fast decode GEMV (vsim_op_q4_gemv, n = 1, MODE_FAST: k_gemv_fast,
  itself held to an fp64 bound in tests/test_gpu_ops.py) on that row quantized alone: the entry's
  contract, for any n and any rows beside it.
* Every value within fast_ref.gemv_tol(nb, sum_b |d_w d_x s_b|) of fast_ref.q4_dot's fp64 product,
  the bound test_gpu_fast_ops.py derives for k_fast_gemv (the same sixteen fp32 strands).
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import fast_ref as R  # noqa: E402
from vsim_amd import hip  # noqa: E402
from vsim_amd import modelgen as mg  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
EINVAL = -1
U = R.U


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def repack(aos_np, rows, k):
    """W4T32 image of the AoS blocks in a buffer of exactly q4_bytes: no slack behind the weight."""
    src = dev(aos_np)
    dst = torch.empty(hip.q4_bytes(rows, k), dtype=torch.uint8, device=DEV)
    hip.check(hip.lib().vsim_op_q4_repack(src.data_ptr(), dst.data_ptr(), rows, k, None), "repack")
    return dst


def quantize(x, k, n):
    """x: device float32 [n][k] -> xq Q4 SoA rows (vsim_op_q4_quantize), in a buffer of exactly n rows."""
    xq = torch.empty(n * k // 32 * 20, dtype=torch.uint8, device=DEV)
    xd = torch.empty(n * k, dtype=torch.float32, device=DEV)
    hip.check(hip.lib().vsim_op_q4_quantize(x.data_ptr(), k, n, xq.data_ptr(), xd.data_ptr(), None), "quantize")
    return xq


def act_parse(xq, k, n):
    aos = torch.empty(n * k // 32 * 20, dtype=torch.uint8, device=DEV)
    hip.check(hip.lib().vsim_op_act_unpack(xq.data_ptr(), aos.data_ptr(), n, k, None), "act_unpack")
    return R.q4_parse(host(aos), k)  # d [n][nb], q [n][nb][32]


def gemv_fast_row(w, M, K, xq1, bias):
    y = torch.full((M,), float("nan"), dtype=torch.float32, device=DEV)
    hip.check(hip.lib().vsim_op_q4_gemv(w.data_ptr(), M, K, xq1.data_ptr(), None, 1,
                                        None if bias is None else bias.data_ptr(), y.data_ptr(), hip.MODE_FAST,
                                        None), "gemv")
    return host(y)


def fast_rows(w, M, K, xq, n, bias, rows=33):
    """The entry on a NaN-prefilled y of `rows` rows."""
    y = torch.full((rows * M,), float("nan"), dtype=torch.float32, device=DEV)
    hip.q4_gemm_fast_rows(w, M, K, xq, n, bias, y)
    return host(y).reshape(rows, M)


@pytest.fixture
def fast_gemm_setting():
    old = hip.batch_set_fast_gemm(1)
    yield
    hip.batch_set_fast_gemm(old)


def operands(M, K, n):
    rng = np.random.default_rng(M * 7 + K * 3 + n)
    w_aos = mg.quantize_q4_0(rng.standard_normal(M * K).astype(np.float32) * np.float32(0.02))
    x = (rng.standard_normal((n, K)) * 1.5).astype(np.float32)
    b = rng.standard_normal(M).astype(np.float32)
    return w_aos, x, b


# one block (fifteen empty partials); a ragged tile; nb = 15 / 16 / 17 round the sixteen strands with
# n round 16 (one MFMA column group or two); a ragged half tile; many blocks per strand with n = 31;
# K = 16384 at n = 32; every tile of a 4096-row product; pythia's ragged vocabulary tile at nb = 160
SHAPES = [(1, 32, 1), (33, 64, 3), (48, 480, 15), (32, 512, 16), (40, 544, 17), (100, 96, 5), (257, 4096, 31),
          (96, 16384, 32), (4096, 128, 32), (50288 - 50272 + 32, 5120, 2)]


@pytest.mark.parametrize("M,K,n", SHAPES)
def test_fast_rows_vs_gemv_and_fp64(M, K, n, fast_gemm_setting):
    hip.batch_set_fast_gemm(2)  # the kernel at every n
    w_aos, x, b = operands(M, K, n)
    w, bd = repack(w_aos, M, K), dev(b)
    xd_ = dev(x)
    xq = quantize(xd_, K, n)
    y, yb = fast_rows(w, M, K, xq, n, None), fast_rows(w, M, K, xq, n, bd)
    assert np.isnan(y[n:]).all() and np.isnan(yb[n:]).all(), "rows >= n written"
    wd, wq = R.q4_parse(w_aos, K)
    ad, aq = act_parse(xq, K, n)
    nb = K // 32
    worst = 0.0
    for j in range(n):
        # the row quantized alone: the same blocks as inside the batch, and the decode GEMV on them
        xq1 = quantize(xd_[j:j + 1].contiguous(), K, 1)
        for bias, got in ((None, y), (bd, yb)):
            want = gemv_fast_row(w, M, K, xq1, bias)
            if not np.array_equal(bits(got[j]), bits(want)):
                bad = np.nonzero(bits(got[j]) != bits(want))[0]
                pytest.fail(f"({M}, {K}, {n}) row {j} bias {bias is not None}: {bad.size} of {M} differ from "
                            f"k_gemv_fast, first {bad[:5]}: {got[j][bad[:3]]} against {want[bad[:3]]}")
            # the entry at n = 1 on that row alone: the bits it gave inside the batch
            alone = fast_rows(w, M, K, xq1, 1, bias, rows=2)
            assert np.array_equal(bits(alone[0]), bits(got[j])) and np.isnan(alone[1]).all(), (j, "alone")
        y64, ab = R.q4_dot(wd, wq, ad[j], aq[j])
        tol = R.gemv_tol(nb, ab)
        worst = max(worst, R.bound_ratio(y[j], y64, tol))
        y64b = y64 + b
        worst = max(worst, R.bound_ratio(yb[j], y64b, tol + U * np.abs(y64b)))
    print(f"gemm_fast_rows M={M} K={K} n={n}: worst error {worst:.3f} x bound")
    assert worst <= 1.0


def test_fast_rows_settings_give_equal_bits(fast_gemm_setting):
    M, K, n = 70, 1056, 9
    w_aos, x, b = operands(M, K, n)
    w, bd = repack(w_aos, M, K), dev(b)
    xq = quantize(dev(x), K, n)
    got = []
    for setting in (2, 0, 1):
        hip.batch_set_fast_gemm(setting)
        got.append((fast_rows(w, M, K, xq, n, None), fast_rows(w, M, K, xq, n, bd)))
    assert hip.batch_set_fast_gemm(7) == 1 and hip.batch_set_fast_gemm(1) == 1  # other values select 1
    for y, yb in got:
        assert not np.isnan(y[:n]).any() and np.isnan(y[n:]).all() and np.isnan(yb[n:]).all()
    for y, yb in got[1:]:
        assert np.array_equal(bits(y[:n]), bits(got[0][0][:n]))
        assert np.array_equal(bits(yb[:n]), bits(got[0][1][:n]))


def test_fast_rows_argument_errors(fast_gemm_setting):
    M, K = 32, 64
    w = torch.zeros(hip.q4_bytes(M, K), dtype=torch.uint8, device=DEV)
    xq = torch.zeros(33 * K // 32 * 20, dtype=torch.uint8, device=DEV)
    y = torch.zeros(33 * M, dtype=torch.float32, device=DEV)
    f = hip.lib().vsim_op_q4_gemm_fast_rows
    for setting in (2, 0):
        hip.batch_set_fast_gemm(setting)
        assert f(w.data_ptr(), M, K, xq.data_ptr(), 0, None, y.data_ptr(), None) == EINVAL
        assert f(w.data_ptr(), M, K, xq.data_ptr(), 33, None, y.data_ptr(), None) == EINVAL
        assert f(w.data_ptr(), M, 48, xq.data_ptr(), 2, None, y.data_ptr(), None) == EINVAL
        assert f(w.data_ptr(), M, K, None, 2, None, y.data_ptr(), None) == EINVAL
        assert f(None, M, K, xq.data_ptr(), 2, None, y.data_ptr(), None) == EINVAL
        assert f(w.data_ptr(), M, K, xq.data_ptr(), 2, None, None, None) == EINVAL
        assert f(w.data_ptr(), 0, K, xq.data_ptr(), 2, None, y.data_ptr(), None) == EINVAL
        assert f(w.data_ptr(), M, K, xq.data_ptr(), 32, None, y.data_ptr(), None) == 0
    torch.cuda.synchronize()
