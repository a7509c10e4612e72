"""tests/w4a16_step_cases.py on the CPU: the restatements agree with their parts, and every row family
bites -- its named wrong variant changes at least one bit of (h, e) on at least one row -- so that
tests/test_gpu_w4a16_step_ops.py cannot pass vacuously on a kernel that fuses wrongly."""
import numpy as np
import pytest

import w4a16_ref as W
import w4a16_step_cases as C

LN_N = [32, 128, 160]
GELU_K = [32, 512]


def bites(rows, make, wrong):
    """How many rows of the family the wrong variant changes."""
    return sum(0 if C.same(make(r, None), make(r, wrong)) else 1 for r in rows)


@pytest.mark.parametrize("n", LN_N)
def test_ln_restatement_and_maximum_after_the_affine(n):
    rows = C.ln_family(n)
    for x, w, b in rows:
        y = C.O.norm(x, n, 1)
        z = C.affine(w, y, b)
        h, e = C.ln_operand(x, w, b)
        hr, er = W.row_operand(z[None])
        assert e == int(er[0]) and np.array_equal(h.view(np.uint16), hr[0].view(np.uint16))
        assert int(np.abs(z).argmax()) != int(np.abs(y).argmax())      # the family does what it says
    assert bites(rows, lambda r, wr: C.ln_operand(*r, wrong=wr), "max_before_affine") == len(rows)


@pytest.mark.parametrize("K", GELU_K)
def test_gelu_families_bite(K):
    neg = C.gelu_negative_max(K)
    for x, bias in neg:
        s, g = C.gelu_rows(x, bias)
        j = int(np.abs(s).argmax())
        assert s[j] < 0 and g[j] == 0.0 and np.abs(g).max() > 0
    assert bites(neg, lambda r, wr: C.gelu_operand(*r, wrong=wr), "max_over_inputs") == len(neg)
    zero = C.gelu_all_zero(K)
    for x, bias in zero:
        h, e = C.gelu_operand(x, bias)
        assert not C.gelu_rows(x, bias)[1].any() and e == 0 and not (h.view(np.uint16) & 0x7FFF).any()
    assert bites(zero, lambda r, wr: C.gelu_operand(*r, wrong=wr), "zero_unhandled") == len(zero)
    big = C.gelu_beyond_f16(K)
    for x, bias in big:
        s, g = C.gelu_rows(x, bias)
        assert np.isfinite(s).all() and not np.isfinite(g).all()      # finite in, the table's inf / NaN out
        h, e = C.gelu_operand(x, bias)
        assert e == W.NONFINITE and not h.view(np.uint16).any()
    assert bites(big, lambda r, wr: C.gelu_operand(*r, wrong=wr), "nonfinite_ignored") == len(big)


@pytest.mark.parametrize("K", GELU_K)
def test_power_of_two_maxima_bite(K):
    rows = C.power_of_two_rows(K)
    make = lambda r, wr: C.gelu_operand(r[0], r[1], wrong=wr)  # noqa: E731
    exact, below = [r for r in rows if r[2] == "exact"], [r for r in rows if r[2] == "below"]
    for x, bias, kind in rows:
        g = C.gelu_rows(x, bias)[1]
        m, ex = np.frexp(float(np.abs(g).max()))
        assert (m == 0.5) == (kind == "exact")
        h, _ = C.gelu_operand(x, bias)
        top = float(np.abs(h.astype(np.float64)).max())
        assert 2.0 ** 14 <= top < 2.0 ** 15 and (top == 2.0 ** 14) == (kind == "exact")
    assert bites(exact, make, "interval_closed_above") == len(exact)
    assert bites(below, make, "log2_rounded") == len(below)
    ln = C.power_of_two_ln_rows(128)
    mk = lambda r, wr: C.ln_operand(r[0], r[1], r[2], wrong=wr)  # noqa: E731
    assert bites([r for r in ln if r[3] == "exact"], mk, "interval_closed_above") == 3
    assert bites([r for r in ln if r[3] == "below"], mk, "log2_rounded") == 3


def test_subnormal_maximum_bites():
    rows = C.subnormal_ln_rows(128)
    for x, w, b in rows:
        h, e = C.ln_operand(x, w, b)
        assert e > 14 + 126 and 2.0 ** 14 <= float(np.abs(h.astype(np.float64)).max()) < 2.0 ** 15
    assert bites(rows, lambda r, wr: C.ln_operand(*r, wrong=wr), "field_only") == len(rows)


@pytest.mark.parametrize("M", [17, 130])
def test_join_order_bites(M):
    v, res, res_a = C.join_rows(M)
    a, b = C.join(v, res, res_a), C.join(v, res, res_a, wrong="join_left_first")
    assert (a.view(np.uint32) != b.view(np.uint32)).sum() >= 1
    assert np.array_equal(C.join(v, res).view(np.uint32), (v + res).view(np.uint32))
