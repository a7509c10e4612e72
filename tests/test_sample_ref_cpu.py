"""No GPU: tests/sample_ref.py against the library's host sampler, and its checker against the
mistakes a batched device stage could make (a window id lost, two rows' parameters swapped)."""
import numpy as np
import pytest

import sample_ref as R
from vsim_amd import hip

PARAMS = [dict(seed=42, top_k=20, top_p=0.95, temp=0.85, repeat_last_n=64, repeat_penalty=1.3),
          dict(seed=43, top_k=40, top_p=0.95, temp=0.8, repeat_last_n=64, repeat_penalty=1.3),
          dict(seed=7, top_k=64, top_p=1.0, temp=1.3, repeat_last_n=8, repeat_penalty=1.1),
          dict(seed=9, top_k=1, top_p=0.5, temp=0.5, repeat_last_n=0, repeat_penalty=1.0),
          dict(seed=11, top_k=5, top_p=0.9, temp=1.0, repeat_last_n=256, repeat_penalty=2.0)]


def distinct_row(n, seed):
    g = np.random.default_rng(seed)
    v = ((np.arange(n, dtype=np.float64) - n / 2 + 0.25) * 3e-3).astype(np.float32)
    assert np.unique(v).size == n
    return g.permutation(v)


@pytest.mark.parametrize("p", PARAMS, ids=[f"seed{p['seed']}" for p in PARAMS])
@pytest.mark.parametrize("n", [64, 257, 4099])
def test_restatement_feeds_pick_what_sample_host_chooses(n, p):
    """Two samplers of equal seed and window: one draws with sample_host (the reference's code on
    the whole row), the other with pick on the restatement's candidates.  Equal tokens draw after
    draw, with the window moving, mean equal candidate lists where it matters: the generator's
    state and the top-p cut depend on every value."""
    a, b = hip.Sampler(**p), hip.Sampler(**p)
    g = np.random.default_rng(n + p["seed"])
    win = [0] * p["repeat_last_n"]
    for t in g.integers(0, n, 5):
        a.accept(int(t))
        b.accept(int(t))
        win = (win + [int(t)])[1:] if win else win
    for step in range(12):
        x = distinct_row(n, 100 * step + n)
        k = p["top_k"]
        val, ids = R.topk(x, win, p["temp"], p["repeat_penalty"], k)
        assert np.unique(R.candidates(x, win, p["temp"], p["repeat_penalty"])).size == n  # tie-free
        ta, tb = a.sample_host(x), b.pick(val, ids)
        assert ta == tb, step
        win = (win + [ta])[1:] if win else win
    assert a.stats() == {"device": 0, "host": 12} and b.stats() == {"device": 12, "host": 0}


def _batch():
    n, B = 1025, 4
    rows = [distinct_row(n, 50 + b) for b in range(B)]
    params = []
    for b, x in enumerate(rows):
        top = [int(t) for t in np.argsort(-x.astype(np.float64))[:6]]  # the penalty reorders the head
        params.append(dict(win=top + [n + 3, -2, top[0]], temp=0.7 + 0.1 * b, penalty=1.2 + 0.1 * b, k=(20, 40, 64, 5)[b]))
    outs = [R.topk(x, p["win"], p["temp"], p["penalty"], p["k"]) for x, p in zip(rows, params)]
    return rows, params, [o[0] for o in outs], [o[1] for o in outs]


def test_checker_accepts_the_restatement():
    rows, params, vals, ids = _batch()
    R.check_rows(rows, params, vals, ids)


@pytest.mark.parametrize("b", range(4))
def test_checker_bites_when_one_window_id_of_one_row_is_dropped(b):
    rows, params, vals, ids = _batch()
    bad = [dict(p) for p in params]
    bad[b]["win"] = bad[b]["win"][1:-1]  # the row's best id leaves the window (its duplicate too)
    with pytest.raises(AssertionError, match=f"row {b}"):
        R.check_rows(rows, bad, vals, ids)


def test_checker_bites_when_two_rows_swap_parameters():
    rows, params, vals, ids = _batch()
    for a, b in ((0, 1), (1, 2), (0, 3)):
        bad = list(params)
        bad[a], bad[b] = dict(params[b], k=params[a]["k"]), dict(params[a], k=params[b]["k"])  # (k alone would show in the shapes)
        with pytest.raises(AssertionError, match=f"row {a}"):
            R.check_rows(rows, bad, vals, ids)
    bad = list(params)
    bad[0], bad[1] = params[1], params[0]
    with pytest.raises(AssertionError):
        R.check_rows(rows, bad, vals, ids)


def test_checker_bites_on_one_flipped_value_bit_and_one_swapped_pair():
    rows, params, vals, ids = _batch()
    v = [np.array(a) for a in vals]
    v[2].view(np.uint64)[7] ^= 1
    with pytest.raises(AssertionError, match="row 2"):
        R.check_rows(rows, params, v, ids)
    i = [np.array(a) for a in ids]
    i[1][[3, 4]] = i[1][[4, 3]]
    with pytest.raises(AssertionError, match="row 1"):
        R.check_rows(rows, params, vals, i)


def test_tie_rule_and_signed_zeros():
    x = np.array([0.0, -0.0, 1.0, 1.0, -0.0, 0.0], np.float32)
    val, ids = R.topk(x, [], 1.0, 1.0, 6)
    assert list(ids) == [2, 3, 0, 1, 4, 5]
    assert list(np.signbit(val)) == [False, False, False, True, True, False]
