"""float64 restatement of vsim_op_logprob (include/vsim_hip.h) and the checker's tolerance.

Per row x (float32), target t:
    m   = max(x)                              a float, exact
    s   = fsum_j exp(float64(x[j]) - float64(m))     math.fsum: the correctly rounded sum
    lse = float64(m) + log(s)
    logprob = float64(x[t]) - lse             t == -1: 0.0
    argmax  = the first maximum (-0.0 == +0.0), or the first NaN if the row has one
A row with a NaN, or whose maximum is +inf or -inf, has logprob NaN; -inf entries contribute 0.

Tolerance.  tol(row) = 2^-50 * (V + |m| + |x_t| + 64), an absolute bound on |device - this file|:
  * the subtraction float64(x) - float64(m) is one IEEE operation on the same operands on both
    sides: identical;
  * the device's double exp and log are within a few ulp of glibc's: each term of s is off by
    a few 2^-53 relative, so is s, and log(s) moves by that many 2^-53 absolute (d log s = ds / s),
    plus log's own few ulp of |log s| <= log V <= 13 (V < 4e5);
  * the device adds the V positive terms in its own fixed order: at most (V - 1) 2^-53 relative in
    s against the exact sum (every partial sum is at most s), i.e. (V - 1) 2^-53 absolute in log s;
    fsum's result is the exact sum rounded once;
  * the two final roundings (m + log s, x_t - lse) cost 2^-53 (|lse| + |logprob|)
    <= 2^-53 (2 |m| + |x_t| + 3 * 13).
  Total <= 2^-53 (V + 2 |m| + |x_t| + c) with c a few dozen: under half of 2^-50 (V + |m| + |x_t| + 64).
"""
import math

import numpy as np


def argmax_row(x) -> int:
    """numpy.argmax's conventions, as vsim_op_argmax states them: the first NaN if any, else the
    first maximum (-0.0 == +0.0 as values)."""
    x = np.asarray(x, np.float32)
    nan = np.flatnonzero(np.isnan(x))
    if nan.size:
        return int(nan[0])
    return int(np.argmax(x))  # value comparison: first of equal maxima, -0.0 == +0.0


def lse_row(x) -> float:
    """(float64(m) + log(fsum exp(float64(x) - float64(m))); NaN by the NaN / Inf rule."""
    x = np.asarray(x, np.float32)
    if np.isnan(x).any():
        return math.nan
    m = float(np.max(x))
    if math.isinf(m):
        return math.nan
    d = x.astype(np.float64) - m
    with np.errstate(under="ignore"):
        s = math.fsum(math.exp(v) for v in d.tolist())
    return m + math.log(s)


def score_row(x, t):
    """(logprob, argmax) of one row; t == -1: logprob 0.0."""
    x = np.asarray(x, np.float32)
    am = argmax_row(x)
    if t < 0:
        return 0.0, am
    lse = lse_row(x)
    return (math.nan if math.isnan(lse) else float(x[t]) - lse), am


def score_rows(x, targets):
    """score_row over x [R][V]: (logprob float64 [R], argmax int32 [R])."""
    x = np.asarray(x, np.float32)
    out = [score_row(x[i], int(targets[i])) for i in range(x.shape[0])]
    return np.array([o[0] for o in out], np.float64), np.array([o[1] for o in out], np.int32)


def tol_row(x, t) -> float:
    """The checker's absolute tolerance for one row (derivation above)."""
    x = np.asarray(x, np.float32)
    if t < 0 or np.isnan(x).any() or np.isinf(np.max(x)):
        return 0.0
    return 2.0 ** -50 * (x.size + abs(float(np.max(x))) + abs(float(x[t])) + 64.0)


def check_rows(x, targets, lp, am, what=""):
    """Assert a device result (lp, am) for rows x against this file: argmax equal, logprob within
    tol_row (NaN where the rule says NaN, exactly 0.0 without a target, -inf for a -inf logit)."""
    x = np.asarray(x, np.float32)
    wlp, wam = score_rows(x, targets)
    assert np.array_equal(np.asarray(am, np.int32), wam), (what, "argmax")
    for i in range(x.shape[0]):
        t = int(targets[i])
        if math.isnan(wlp[i]):
            assert math.isnan(lp[i]), (what, i, lp[i])
        elif t < 0 or math.isinf(wlp[i]):  # no target: 0.0; a -inf target logit: -inf
            assert lp[i] == wlp[i], (what, i, lp[i])
        else:
            assert abs(float(lp[i]) - wlp[i]) <= tol_row(x[i], t), (what, i, float(lp[i]), wlp[i], tol_row(x[i], t))
