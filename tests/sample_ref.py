"""A numpy restatement of the sampler's candidate stage (sample_top_p_top_k_repeat_penalty,
utils.cpp:339-371), shared by the tests of the batched device stage: float64 arithmetic in the
reference's order of operations, the k largest in a stable order by (value descending, id
ascending) -- the reference's order wherever values are distinct, the header's tie rule otherwise.
"""
import numpy as np


def widen(f):
    """A float parameter passed to a double argument (vsim.cpp:866-873)."""
    return float(np.float32(f))


def candidates(x, win, temp, penalty):
    """Every id's candidate as float64: x * (1 / temp), and for the ids of `win` (duplicates and
    ids outside [0, n) match nothing more) that times the penalty when x < 0, over it otherwise."""
    x = np.asarray(x, np.float32)
    scale, pen = 1.0 / widen(temp), widen(penalty)
    c = x.astype(np.float64) * scale
    w = np.asarray(win, np.int64).reshape(-1)
    inwin = np.zeros(x.size, bool)
    inwin[w[(w >= 0) & (w < x.size)]] = True
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(inwin, np.where(x < 0, c * pen, c / pen), c)


def topk(x, win, temp, penalty, k):
    """(val float64 [k], ids int32 [k]) of one row: the k best candidates, best first."""
    c = candidates(x, win, temp, penalty)
    order = np.lexsort((np.arange(c.size), -c))[:k]
    return c[order], order.astype(np.int32)


def check_rows(rows, params, vals, ids):
    """Row b of (vals, ids) -- arrays of at least params[b]["k"] entries per row -- must be
    topk(rows[b], **params[b]): values as bits, ids exactly.  Raises AssertionError naming the
    first row that is not."""
    assert len(rows) == len(params) == len(vals) == len(ids)
    for b, (x, p) in enumerate(zip(rows, params)):
        k = p["k"]
        wv, wi = topk(x, p["win"], p["temp"], p["penalty"], k)
        gi = np.asarray(ids[b], np.int32)[:k]
        gv = np.ascontiguousarray(np.asarray(vals[b], np.float64)[:k])
        assert np.array_equal(gi, wi), f"row {b}: ids {gi[:8]}.. against {wi[:8]}.."
        assert np.array_equal(gv.view(np.uint64), wv.view(np.uint64)), f"row {b}: values differ"
