"""The weight-only mode's checkers (tests/w4a16_ref.py) bite, shown without a GPU: an honest
emulation of the kernel passes the operand's bit check and the product's bound, and each emulation
of a wrong kernel leaves one of them.  Also records, from the oracle alone, the two distances the
GPU quality checks use (tests/test_gpu_w4a16_model.py).  Nothing here reads the code under test.
"""
import numpy as np
import pytest

import fast_ref as R
import w4a16_ref as W
from vsim_amd import modelgen as mg

M, K, N = 40, 544, 6


@pytest.fixture(scope="module")
def case():
    rng = np.random.default_rng(3)
    wd, wq = R.q4_parse(mg.quantize_q4_0(rng.standard_normal(M * K).astype(np.float32) * np.float32(0.02)), K)
    x = (rng.standard_normal((N, K)) * 1.5).astype(np.float32)
    x[2] *= np.float32(2.0 ** -32)  # a row far below the batch's maximum: fp16 subnormals on the batch's scale
    h, e = W.row_operand(x)
    y64, tol = W.product64(wd, wq, h, e)
    return wd, wq, x, h, e, y64, tol


def test_operand_rules():
    x = np.zeros((7, 64), np.float32)
    rng = np.random.default_rng(1)
    x[0] = rng.standard_normal(64)
    x[1] = x[0] * np.float32(3e-7)
    x[1, 5] = 1e30                       # an outlier: the rest underflows to fp16 subnormals and zeros
    x[2] = np.float32(1e-40) * rng.standard_normal(64).astype(np.float32)   # f32 subnormals
    x[3, 3] = -0.0
    x[4] = x[0]; x[4, 9] = np.nan
    x[5] = x[0]; x[5, 0] = -np.inf
    x[6] = np.float32(2.0 ** 14)         # exactly at the lower edge
    h, e = W.row_operand(x)
    for j in (0, 1, 2, 6):
        top = np.abs(x[j]).max().astype(np.float64) * 2.0 ** float(e[j])
        assert 2.0 ** 14 <= top < 2.0 ** 15, j
        assert np.isfinite(h[j]).all()
        assert np.array_equal(h[j], np.ldexp(x[j].astype(np.float64), int(e[j])).astype(np.float16))
    assert e[6] == 0 and e[3] == 0 and not h[3].any() and np.signbit(h[3, 3]) and not np.signbit(h[3, 2])
    assert e[1] == 14 - 99 and h[1, 5] == np.float16(2.0 ** 14 * (1e30 / 2.0 ** 99))
    assert (np.abs(h[1][np.arange(64) != 5]) < 2.0 ** -14).all()         # subnormal or zero
    assert e[2] > 127 and np.abs(h[2]).max() >= 2.0 ** 14                 # 2^e itself is no float32
    assert e[4] == W.NONFINITE and e[5] == W.NONFINITE and not h[4].any() and not h[5].any()
    # a row's operand is a function of that row: any subset, any order
    h2, e2 = W.row_operand(x[[6, 2, 0]])
    assert np.array_equal(e2, e[[6, 2, 0]]) and np.array_equal(h2.view(np.uint16), h[[6, 2, 0]].view(np.uint16))


def test_bound_constant():
    assert W.c_of_k(32) == 32 + 1 + 16 + 1 and W.c_of_k(544) == 32 + 2 + 16 + 1 and W.c_of_k(16384) == 32 + 32 + 16 + 1


def test_honest_orders_pass(case):
    wd, wq, x, h, e, y64, tol = case
    r = W.bound_ratio(W.product32_reversed(wd, wq, h, e), y64, tol)
    print(f"fp32, reversed order: {r:.3f} x bound")
    assert r <= 1.0
    b = np.linspace(-1, 1, M).astype(np.float32)
    y64b, tolb = W.product64(wd, wq, h, e, b)
    yb = W.product32_reversed(wd, wq, h, e) + b[None]
    assert W.bound_ratio(yb, y64b, tolb) <= 1.0


def test_activations_through_q4_leave_the_bound(case):
    wd, wq, x, h, e, y64, tol = case
    W64 = (wd.astype(np.float64)[:, :, None] * wq).reshape(M, K)
    xq = np.stack([(lambda d, q: (d[:, None].astype(np.float64) * q).reshape(-1))(*R.q4_quantize_ref(r)) for r in x])
    assert W.bound_ratio(xq @ W64.T, y64, tol) > 100.0


def test_fp16_weights_leave_the_bound(case):
    wd, wq, x, h, e, y64, tol = case
    w16 = (wd.astype(np.float64)[:, :, None] * wq).astype(np.float16).astype(np.float64).reshape(M, K)
    y = np.stack([(h[j].astype(np.float64) @ w16.T) * 2.0 ** -float(e[j]) for j in range(N)])
    assert W.bound_ratio(y, y64, tol) > 1.0


def test_skipped_block_leaves_the_bound(case):
    wd, wq, x, h, e, y64, tol = case
    wd2 = wd.copy()
    wd2[:, K // 32 - 1] = 0.0   # the last block never added
    assert W.bound_ratio(W.product64(wd2, wq, h, e)[0], y64, tol) > 100.0


def test_batch_maximum_scaling_leaves_the_bit_check(case):
    wd, wq, x, h, e, y64, tol = case
    eb = int(W.row_operand(np.abs(x).max(axis=0, keepdims=True))[1][0])   # one exponent for the batch
    hb = np.ldexp(x.astype(np.float64), eb).astype(np.float16)
    assert eb != e[2] and not np.array_equal(hb[2].view(np.uint16), h[2].view(np.uint16))
    # ... and the small row's values then depend on its neighbours: most of its bits are gone
    yb = W.product64(wd, wq, hb[2:3], np.array([eb], np.int32))[0]
    assert W.bound_ratio(yb, y64[2:3], tol[2:3]) > 1.0


def test_exponent_off_by_one_leaves_both(case):
    wd, wq, x, h, e, y64, tol = case
    h1 = np.ldexp(x.astype(np.float64), (e + 1)[:, None]).astype(np.float16)
    assert not np.array_equal(e + 1, e) and not np.array_equal(h1.view(np.uint16), h.view(np.uint16))
    assert W.bound_ratio(W.product64(wd, wq, h, e + 1)[0], y64, tol) > 1000.0   # the right h, 2^-(e+1)


def test_flushed_subnormals_are_visible():
    """The subnormal rule is checkable: on an outlier row the subnormal h carry enough of the
    product that a flushing matrix core would leave the bound."""
    wd, wq, x, _ = W.subnormal_case()
    h, e = W.row_operand(x)
    assert ((np.abs(h) < 2.0 ** -14) & (h != 0)).sum() >= 32
    y64, tol = W.product64(wd, wq, h, e)
    flushed = np.where(np.abs(h.astype(np.float64)) < 2.0 ** -14, 0.0, h.astype(np.float64)).astype(np.float16)
    assert W.bound_ratio(W.product64(wd, wq, flushed, e)[0], y64, tol) > 100.0


def test_quality_distances_recorded(tmp_path):
    """The two recorded distances, recomputed from the oracle and the restatement alone."""
    path, tokens, ideal, rest64 = W.quality_case(str(tmp_path))
    exact = W.oracle_exact_rows(path, tokens)
    rest32 = W.neox_forward(path, tokens, W.mm_rest32)
    d_exact, d_rest, d_order = W.rms(exact, ideal), W.rms(rest64, ideal), W.rms(rest64, rest32)
    print(f"seed {W.QUALITY_SEED}: logits RMS {np.sqrt(np.mean(ideal.astype(np.float64) ** 2)):.4f}; exact mode to ideal "
          f"{d_exact!r}; restatement to ideal {d_rest!r} (ratio {d_exact / d_rest:.1f}); restatement fp64 against "
          f"fp32 reversed {d_order!r}")
    assert d_exact == pytest.approx(W.EXACT_TO_IDEAL, rel=1e-6)
    assert d_order == pytest.approx(W.REST_ORDER_DIST, rel=0.02)
    assert W.REST_TOL == 4.0 * W.REST_ORDER_DIST
    # exact mode is well clear of zero and the restatement well inside the floor: the ratio test tests something
    assert d_exact > 0.1 * np.sqrt(np.mean(ideal.astype(np.float64) ** 2))
    assert d_exact / d_rest > 10 * W.QUALITY_FLOOR
    # the forward is the oracle's graph: with the oracle's own product it is the oracle's eval, bit for bit
    import oracle_py as O

    def mm_exact(w, x):
        return O.mul_mat(R.q4_pack(w[0], w[1]), w[0].shape[0], w[0].shape[1] * 32, x, x.shape[0]).reshape(x.shape[0], -1)

    assert np.array_equal(W.neox_forward(path, tokens, mm_exact).view(np.uint32), exact.view(np.uint32))
