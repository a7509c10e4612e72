"""Scoring a text with a model: per-position log-probabilities, perplexity, and the agreement of
two runs (exact vs fast or weight-only mode, an F16-quantized vs a Q4_0 file).

The numbers come from Model.score (vsim_model_eval_score, include/vsim_hip.h): one prompt pass per
window, the log-sum-exp of every logits row taken on the device.  This module only cuts the text
into windows and averages; it needs nothing but an object with `n_ctx` and
`score(n_past, tokens, targets) -> (logprob, argmax)`.
"""
from __future__ import annotations

import math

import numpy as np


def windows(n_tokens: int, window: int, stride: int):
    """The evaluation windows of a text of n_tokens ids: (start, end, first) triples -- the window
    is ids[start:end], evaluated from n_past = 0, and its positions first..end-1 are the ones it
    scores (position p scores ids[p + 1]; the text's last position has nothing to score).  The
    first window scores all its positions; each later one moves `stride` positions on and keeps
    the window - stride tokens before them as context.  Every position 0..n_tokens-2 is scored
    exactly once."""
    if window < 1 or stride < 1 or stride > window:
        raise ValueError("windows: need 1 <= stride <= window")
    out, done, last = [], 0, n_tokens - 1  # positions [0, done) are scored; `last` has no target
    while done < last:
        end = min(n_tokens, window if not out else done + stride)
        out.append((max(0, end - window), end, done))
        done = end
    return out


def perplexity(model, ids, window=None, stride=None) -> dict:
    """Log-probability of every token of `ids` after the first, given the tokens before it (at
    most window - 1 of them), and the perplexity from it.
    Returns dict(nll, ppl, n_scored, top1, logprob): the mean negative log-probability, exp(nll),
    the number of scored positions, the share of them whose greedy id is the token that followed,
    and logprob[p] = log P(ids[p + 1] | ids[..p]) for p in 0..len(ids)-2."""
    ids = [int(t) for t in ids]
    window = int(window) if window else int(model.n_ctx)
    stride = int(stride) if stride else window
    lps, hits = [], 0
    for start, end, first in windows(len(ids), window, stride):
        toks = ids[start:end]
        tgt = [ids[p + 1] if first <= p < len(ids) - 1 else -1 for p in range(start, end)]
        lp, am = model.score(0, toks, tgt)[:2]
        for p in range(first, min(end, len(ids) - 1)):
            lps.append(float(lp[p - start]))
            hits += int(am[p - start]) == ids[p + 1]
    n = len(lps)
    nll = -math.fsum(lps) / n if n else float("nan")
    return {"nll": nll, "ppl": math.exp(nll) if n else float("nan"), "n_scored": n,
            "top1": hits / n if n else float("nan"), "logprob": np.asarray(lps, np.float64)}


def agreement(lp_a, am_a, lp_b, am_b) -> dict:
    """Two runs over the same positions: the mean and the largest |delta logprob|, and the share of
    positions whose greedy ids agree."""
    lp_a, lp_b = np.asarray(lp_a, np.float64), np.asarray(lp_b, np.float64)
    am_a, am_b = np.asarray(am_a), np.asarray(am_b)
    if lp_a.shape != lp_b.shape or am_a.shape != am_b.shape:
        raise ValueError("agreement: the runs cover different positions")
    d = np.abs(lp_a - lp_b)
    return {"mean_abs_dlogprob": float(d.mean()) if d.size else float("nan"),
            "max_abs_dlogprob": float(d.max()) if d.size else float("nan"),
            "argmax_agree": float((am_a == am_b).mean()) if am_a.size else float("nan"), "n": int(d.size)}
