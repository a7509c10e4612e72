"""The sampler object's host stages (vsim_sampler_* in include/vsim_hip.h); no GPU needed.

* pick: the k-element finishing stage against a restatement in Python floats (IEEE doubles,
  math.exp = the C library's exp) of utils.cpp:373-421 and of libstdc++'s
  std::discrete_distribution over std::mt19937;
* sample_host: the whole sampler inside a Python copy of the reference main loop's bookkeeping,
  against the oracle's own loop (oracle_py.Model.generate);
* the window rules.
"""
import ctypes
import math

import numpy as np
import pytest

import oracle_py as O
from vsim_amd import hip
from vsim_amd import modelgen as mg

GOLDEN_PARAMS = dict(seed=42, top_k=20, top_p=0.95, temp=0.85, repeat_last_n=64, repeat_penalty=1.3)
CLI_DEFAULTS = dict(seed=42, top_k=40, top_p=0.95, temp=0.8, repeat_last_n=64, repeat_penalty=1.3)


class Mt19937:
    """std::mt19937(seed)'s 32-bit output stream."""

    def __init__(self, seed):
        self.bg = np.random.RandomState(seed)._bit_generator
        self.draws = 0

    def __call__(self):
        self.draws += 1
        return int(self.bg.random_raw())


def ref_pick(rng, val, ids, top_p):
    """utils.cpp:373-421 on ordered candidates, then libstdc++'s discrete_distribution."""
    top_p = float(np.float32(top_p))  # a float parameter widened to the double argument
    maxl = -math.inf
    for v in val:
        maxl = max(maxl, v)
    probs = [math.exp(v - maxl) for v in val]
    s = 0.0
    for p in probs:
        s += p
    probs = [p / s for p in probs]
    if top_p < 1.0:
        cum = 0.0
        for i in range(len(probs)):
            cum += probs[i]
            if cum >= top_p:
                probs = probs[:i + 1]
                break
        cum = 1.0 / cum
        probs = [p * cum for p in probs]
    if len(probs) < 2:  # no draw at all
        return int(ids[0])
    s = 0.0
    for p in probs:
        s += p
    cp, acc = [], 0.0
    for p in probs:
        acc += p / s
        cp.append(acc)
    cp[-1] = 1.0
    x1, x2 = rng(), rng()
    u = (float(x1) + float(x2) * 4294967296.0) / 18446744073709551616.0
    if u >= 1.0:
        u = math.nextafter(1.0, 0.0)
    return int(ids[int(np.searchsorted(np.array(cp), u, "left"))])


def candidates(g, k, spread):
    val = np.sort(g.standard_normal(k) * spread)[::-1].astype(np.float64)
    ids = g.permutation(50400)[:k].astype(np.int32)
    return np.ascontiguousarray(val), ids


@pytest.mark.parametrize("top_p", [0.5, 0.95, 1.0])
@pytest.mark.parametrize("k", [1, 2, 20, 64])
def test_pick_matches_restatement(k, top_p):
    g = np.random.default_rng(1000 * k + int(100 * top_p))
    s = hip.Sampler(seed=7 + k, top_k=k, top_p=top_p, temp=0.85, repeat_last_n=64, repeat_penalty=1.3)
    rng = Mt19937(7 + k)
    got, want = [], []
    for _ in range(200):
        val, ids = candidates(g, k, spread=g.choice([0.3, 2.0, 8.0]))
        got.append(s.pick(val, ids))
        want.append(ref_pick(rng, list(val), ids, top_p))
    assert got == want
    assert s.stats() == {"device": 200, "host": 0}


def test_pick_cut_to_one_candidate_consumes_no_draw():
    """Every third list's head holds all the mass, so the top-p cut leaves it alone: no draw, and
    the picks after it show a draw consumed by mistake."""
    g = np.random.default_rng(5)
    s = hip.Sampler(seed=11, top_k=20, top_p=0.95, temp=1.0, repeat_last_n=8, repeat_penalty=1.0)
    rng = Mt19937(11)
    got, want, single = [], [], 0
    for it in range(200):
        val, ids = candidates(g, 20, spread=0.5)
        if it % 3 == 1:
            val[0] += 60.0
        before = rng.draws
        want.append(ref_pick(rng, list(val), ids, 0.95))
        single += rng.draws == before
        got.append(s.pick(val, ids))
    assert single >= 60
    assert got == want


def _loop_with_sample_host(om, prompt, n_predict, params, n_batch=8, n_ctx=512):
    """vsim.cpp:749-910's bookkeeping around oracle evals and the library's sampler."""
    s = hip.Sampler(**params)
    n_predict = min(n_predict, n_ctx - len(prompt))
    logits = om.eval(0, [1, 2, 3, 4, 5])  # the warm-up eval
    embd, out, n_past = [], [], 0
    i = 0
    while i < len(prompt) + n_predict:
        if embd:
            logits = om.eval(n_past, embd)
        n_past += len(embd)
        embd = []
        if i >= len(prompt):
            embd.append(s.sample_host(logits))
        else:
            for k in range(i, len(prompt)):
                embd.append(prompt[k])
                s.accept(prompt[k])
                if len(embd) > n_batch:
                    break
            i += len(embd) - 1
        out += embd
        if embd[-1] == 2:
            break
        i += 1
    return out, s


@pytest.mark.parametrize("params", [GOLDEN_PARAMS, CLI_DEFAULTS], ids=["golden", "cli-defaults"])
@pytest.mark.parametrize("cfg", ["tiny-neox", "tiny-gptj"])
def test_sample_host_matches_oracle_loop(cfg, params, tmp_path):
    arch_s, hp = mg.CONFIGS[cfg]
    path = str(tmp_path / f"{cfg}.bin")
    mg.write_model(path, arch_s, hp, seed=5, std=0.08)
    om = O.Model(path, 1 if arch_s == "gptj" else 0)
    prompt = [3, 1, 4, 1, 5, 9, 7, 6, 5, 3, 5]
    want = om.generate(prompt, 24, **params)
    got, s = _loop_with_sample_host(om, prompt, 24, params)
    assert got == want
    assert s.stats() == {"device": 0, "host": len(got) - len(prompt)}


def test_window_rules():
    logits = np.full(128, -4.0, np.float32)
    logits[0], logits[9] = 2.0, 1.5
    # the window starts as zeros: id 0 is penalised (2.0 / 2 < 1.5) before anything is accepted
    s = hip.Sampler(seed=1, top_k=1, top_p=1.0, temp=1.0, repeat_last_n=4, repeat_penalty=2.0)
    assert s.sample_host(logits) == 9
    # ... and once the zeros are pushed out it no longer is (9 now is: 1.5 / 2 < 2.0)
    for t in (9, 9, 9):
        s.accept(t)
    assert s.sample_host(logits) == 0
    # repeat_last_n = 0: no window, accept does nothing, nothing is ever penalised
    s0 = hip.Sampler(seed=1, top_k=1, top_p=1.0, temp=1.0, repeat_last_n=0, repeat_penalty=2.0)
    s0.accept(0)
    assert s0.sample_host(logits) == 0
    assert s0.sample_host(logits) == 0
    assert s0.pick(np.array([1.0]), np.array([5], np.int32)) == 5


@pytest.mark.parametrize("k", [0, -1, hip.TOPK_MAX + 1])
def test_pick_rejects_out_of_range_k(k):
    s = hip.Sampler()
    val, ids = np.zeros(hip.TOPK_MAX + 1), np.arange(hip.TOPK_MAX + 1, dtype=np.int32)
    tok = ctypes.c_int32()
    assert hip.lib().vsim_sampler_pick(s.h, hip.ptr(val), hip.ptr(ids), k, ctypes.byref(tok)) == -1  # VSIM_EINVAL
    assert s.stats() == {"device": 0, "host": 0}
