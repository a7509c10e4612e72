"""No GPU: the float64 restatement of vsim_op_logprob that the GPU tests check against
(score_ref.py), its tolerance, and score.perplexity's windowing on a stub model."""
import math

import numpy as np
import pytest

import score_ref as R
from vsim_amd import score


# ------------------------------------------------------------------ the restatement
def test_matches_the_naive_formula_on_benign_rows():
    g = np.random.default_rng(1)
    for V in (1, 2, 63, 1025, 50400):
        x = (g.standard_normal(V) * 2).astype(np.float32)
        naive = np.log(np.sum(np.exp(x.astype(np.float64))))
        assert R.lse_row(x) == pytest.approx(naive, rel=0, abs=1e-12 * max(1.0, abs(naive)))
        t = int(g.integers(0, V))
        lp, am = R.score_row(x, t)
        assert lp == pytest.approx(float(x[t]) - naive, rel=0, abs=1e-11)
        assert am == int(np.argmax(x))


def test_huge_maximum_with_the_rest_far_below():
    x = np.full(100, -1e30, np.float32)
    x[37] = 1e30
    assert R.lse_row(x) == float(np.float32(1e30))
    assert R.score_row(x, 37) == (0.0, 37)
    lp, _ = R.score_row(x, 0)
    assert lp == float(np.float32(-1e30)) - float(np.float32(1e30))


def test_minus_infinity_entries_contribute_nothing():
    x = np.array([0.5, -np.inf, 0.5, -np.inf, -np.inf], np.float32)
    assert R.lse_row(x) == pytest.approx(0.5 + math.log(2.0), abs=1e-15)
    lp, am = R.score_row(x, 1)
    assert lp == -math.inf and am == 0


def test_all_equal_rows_and_one_entry():
    for V in (1, 2, 64, 4099):
        x = np.full(V, 3.25, np.float32)
        lp, am = R.score_row(x, V - 1)
        assert lp == pytest.approx(-math.log(V), abs=1e-14) and am == 0
    assert R.score_row(np.array([-7.5], np.float32), 0) == (0.0, 0)


def test_nan_and_infinity_rules():
    x = np.array([1.0, np.nan, 5.0, np.nan], np.float32)
    lp, am = R.score_row(x, 0)
    assert math.isnan(lp) and am == 1  # the first NaN
    x = np.array([1.0, np.inf, 5.0, np.inf], np.float32)
    lp, am = R.score_row(x, 0)
    assert math.isnan(lp) and am == 1
    x = np.full(9, -np.inf, np.float32)
    lp, am = R.score_row(x, 3)
    assert math.isnan(lp) and am == 0
    # no target: 0.0 whatever the row holds, argmax still by the rule
    assert R.score_row(np.array([np.nan, 1.0], np.float32), -1) == (0.0, 0)
    # -0.0 and +0.0 are one value: the first wins
    assert R.argmax_row(np.array([-1.0, -0.0, 0.0], np.float32)) == 1
    assert R.tol_row(np.array([np.nan, 1.0], np.float32), 0) == 0.0


def test_the_checker_bites():
    """One float ulp on a dominant logit moves logprob of another token by about that ulp: far
    more than the tolerance."""
    g = np.random.default_rng(2)
    x = (g.standard_normal(4099) * 2).astype(np.float32)
    x[100] = 30.0
    y = x.copy()
    y[100] = np.nextafter(np.float32(30.0), np.float32(np.inf))
    a, _ = R.score_row(x, 7)
    b, _ = R.score_row(y, 7)
    ulp = float(y[100]) - float(x[100])
    assert abs(a - b) == pytest.approx(ulp, rel=1e-3)
    assert abs(a - b) > 1000 * R.tol_row(x, 7)
    lp, am = R.score_rows(x[None, :], [7])
    R.check_rows(x[None, :], [7], lp, am)
    with pytest.raises(AssertionError):
        R.check_rows(x[None, :], [7], np.array([b]), am)
    with pytest.raises(AssertionError):
        R.check_rows(x[None, :], [7], lp, am + 1)


# ------------------------------------------------------------------ perplexity's windowing
class Stub:
    """A model whose logprob for (position p of the text, target) is canned: -(p + 1) / 8 when the
    target is the text's next token; records every call."""

    def __init__(self, ids, n_ctx):
        self.ids, self.n_ctx, self.calls = list(ids), n_ctx, []

    def score(self, n_past, tokens, targets):
        tokens, targets = list(tokens), list(targets)
        assert n_past == 0 and len(tokens) == len(targets) <= self.n_ctx
        # the window is a contiguous piece of the text: find it by the scored positions' targets
        start = next(s for s in range(len(self.ids)) if self.ids[s:s + len(tokens)] == tokens
                     and all(t == -1 or t == self.ids[s + i + 1] for i, t in enumerate(targets)))
        self.calls.append((start, len(tokens), [start + i for i, t in enumerate(targets) if t != -1]))
        lp = np.array([-(start + i + 1) / 8.0 if t != -1 else 0.0 for i, t in enumerate(targets)])
        am = np.array([t if (start + i) % 2 == 0 else -5 for i, t in enumerate(targets)], np.int32)
        return lp, am


def distinct_ids(n):
    return [(7 * i + 3) % 1009 for i in range(n)]  # distinct for n <= 1009: a window occurs once


@pytest.mark.parametrize("n,window,stride", [(40, 16, 16), (40, 16, 4), (41, 16, 5), (10, 16, None), (16, 16, 8),
                                             (17, 16, 16), (2, 16, None), (33, None, None)])
def test_perplexity_windows(n, window, stride):
    ids = distinct_ids(n)
    m = Stub(ids, 16 if window is None else 64)
    r = score.perplexity(m, ids, window=window, stride=stride)
    w = window or m.n_ctx
    s = stride or w
    scored = [p for c in m.calls for p in c[2]]
    assert scored == list(range(n - 1))  # every position once, in order
    assert r["n_scored"] == n - 1
    assert np.array_equal(r["logprob"], -(np.arange(n - 1) + 1) / 8.0)
    assert r["nll"] == pytest.approx(np.mean((np.arange(n - 1) + 1) / 8.0), rel=1e-15)
    assert r["ppl"] == pytest.approx(math.exp(r["nll"]), rel=1e-15)
    assert r["top1"] == pytest.approx(len(range(0, n - 1, 2)) / (n - 1))
    # the first window starts the text and scores everything it holds; later ones hold a full
    # window (w - s context rows with -1 targets, then at most s scored ones)
    first = m.calls[0]
    assert first[0] == 0 and first[1] == min(n, w) and first[2] == list(range(min(n, w) if n > w else n - 1))
    for start, length, pos in m.calls[1:]:
        assert length == w and 1 <= len(pos) <= s
        assert pos[0] >= start + (w - s)  # the context rows are not scored


def test_perplexity_of_an_empty_or_one_token_text():
    m = Stub([5], 8)
    r = score.perplexity(m, [5])
    assert r["n_scored"] == 0 and math.isnan(r["nll"]) and not m.calls
    with pytest.raises(ValueError):
        score.perplexity(m, [1, 2, 3], window=4, stride=5)


def test_agreement():
    a = score.agreement([-1.0, -2.0, -3.0], [1, 2, 3], [-1.5, -2.0, -2.0], [1, 9, 3])
    assert a["mean_abs_dlogprob"] == pytest.approx(0.5) and a["max_abs_dlogprob"] == 1.0
    assert a["argmax_agree"] == pytest.approx(2 / 3) and a["n"] == 3
    with pytest.raises(ValueError):
        score.agreement([0.0], [1], [0.0, 1.0], [1, 2])
