"""Exact decode on both sides of the fused layer tail's context-length seam, to the last cache
row, bit for bit against oracle_py.Model.

The executor fuses the heads into k_layer_tail only while attn_lds_floats(d, n_ctx) * 4 <= 75264,
that is n_ctx + 2 d <= 2432: n_ctx <= 1920 at d = 256, 2304 at d = 64.  Past that the step is
k_attn_decode plus a chain GEMV for the out-projection, and no LayerNorm runs inside a tail; GPT-J
and CodeGen (d = 256) at their own n_ctx = 2048 decode that way.  Each test asserts from the
profile which of the two steps ran, so a moved threshold fails here instead of un-covering the seam.

Per graph one oracle trajectory serves every context length: an exact prompt of n_ctx_min - 8
tokens, then greedy steps to the largest n_ctx - 1.  Each device model evaluates the prompt and
walks the oracle's tokens to its own last row.
"""
import functools
import os

import numpy as np
import pytest

from vsim_amd import hip
from vsim_amd import modelgen as mg

pytestmark = pytest.mark.gpu

ARCH = {"gptj": hip.ARCH_GPTJ, "gptneox": hip.ARCH_GPTNEOX, "bloom": hip.ARCH_BLOOM}
ORACLE_ARCH = {"gptneox": 0, "gptj": 1, "bloom": 2}
NTH = max(1, min(16, os.cpu_count() or 1))  # the oracle's rows are independent chains: same bits
EINVAL = -1
# config -> context lengths, the first the largest fused one, the second the smallest unfused one
SEAMS = {"seam-gptj": (1920, 1924, 2048),   # GPT-J, d = 256, parallel residual, in-tail LayerNorm
         "small-neox": (2304, 2308),        # d = 64, heads split over two workgroups (c = 32), two norms, biases
         "small-bloom": (2304, 2308)}       # serial residual, ALiBi: tail without fc_out
PARAMS = [(cfg, n) for cfg, ns in SEAMS.items() for n in ns]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def fused(cfg, n_ctx):
    hp = mg.CONFIGS[cfg][1]
    return n_ctx + 2 * (hp.n_embd // hp.n_head) <= 2432


@pytest.fixture(scope="module")
def model_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("seams"))


@functools.lru_cache(maxsize=None)
def _trajectory(cfg, root):
    """(path, prompt, prompt logits, [token fed at P + i], [its logits]) from one oracle model at
    the config's largest context."""
    import oracle_py as O
    arch_s, hp = mg.CONFIGS[cfg]
    path = os.path.join(root, f"{cfg}.bin")
    mg.write_model(path, arch_s, hp, seed=11, std=0.05)
    ns = SEAMS[cfg]
    om = O.Model(path, ORACLE_ARCH[arch_s], n_ctx=max(ns))
    prompt = [int(t) for t in np.random.default_rng(1).integers(0, hp.n_vocab, min(ns) - 8)]
    lg0 = om.eval(0, prompt, nthreads=NTH)
    toks, lgs, lg = [], [], lg0
    for n_past in range(len(prompt), max(ns)):
        toks.append(int(np.argmax(lg)))
        lg = om.eval(n_past, [toks[-1]], nthreads=NTH)
        lgs.append(lg)
    return path, prompt, lg0, toks, lgs


def _decode_kernels(dm, n_past, tok):
    """The kernel names of one profiled single-token step (and its logits)."""
    dm.set_profile(True)
    lg = dm.eval(n_past, [tok])
    names = [k["name"] for k in dm.profile_kernels()]
    dm.set_profile(False)
    return lg, names


def _assert_step(cfg, n_ctx, names):
    tail = [n for n in names if n.startswith("k_layer_tail")]
    if fused(cfg, n_ctx):
        assert tail and "k_attn_decode" not in names, names
    else:
        assert not tail and "k_attn_decode" in names, names


@pytest.mark.parametrize("cfg,n_ctx", PARAMS, ids=[f"{c}-{n}" for c, n in PARAMS])
def test_walk_to_the_last_row(cfg, n_ctx, model_dir):
    path, prompt, lg0, toks, lgs = _trajectory(cfg, model_dir)
    assert fused(cfg, SEAMS[cfg][0]) and not fused(cfg, SEAMS[cfg][1]) and SEAMS[cfg][1] - SEAMS[cfg][0] == 4
    arch_s, _ = mg.CONFIGS[cfg]
    spin0 = hip.spin_timeouts()
    dm = hip.Model.load(path, ARCH[arch_s], n_ctx=n_ctx)
    dm.set_mode(hip.MODE_EXACT)
    P = len(prompt)
    assert np.array_equal(bits(dm.eval(0, prompt)), bits(lg0)), "prompt"
    lg, names = _decode_kernels(dm, P, toks[0])
    assert np.array_equal(bits(lg), bits(lgs[0])), ("profiled step", P)
    _assert_step(cfg, n_ctx, names)
    for n_past in range(P, n_ctx):  # (the first step again, unprofiled, then on to the last cache row)
        lg = dm.eval(n_past, [toks[n_past - P]])
        if not np.array_equal(bits(lg), bits(lgs[n_past - P])):
            bad = np.nonzero(bits(lg) != bits(lgs[n_past - P]))[0]
            pytest.fail(f"{cfg} n_ctx {n_ctx}: n_past {n_past}: {bad.size} logits differ, first {bad[:5]}")
    # the context is full: a host check refuses the next position, whatever the token
    tok, out = np.zeros(1, np.int32), np.zeros(dm.n_vocab, np.float32)
    assert hip.lib().vsim_model_eval(dm.h, n_ctx, hip.ptr(tok), 1, None, None, hip.ptr(out)) == EINVAL
    assert "exceeds n_ctx" in hip.lib().vsim_last_error().decode()
    assert hip.spin_timeouts() == spin0
    dm.close()


def test_batch_with_a_row_at_the_last_position(model_dir):
    """decode_batch, B = 2, at the smallest unfused context of the d = 256 graph: one slot at
    n_ctx - 1 beside one at position 3, each against the oracle's row for that sequence."""
    import oracle_py as O
    cfg, n_ctx = "seam-gptj", 1924
    path, prompt, lg0, toks, lgs = _trajectory(cfg, model_dir)
    arch_s, _ = mg.CONFIGS[cfg]
    P = len(prompt)
    om = O.Model(path, ORACLE_ARCH[arch_s], n_ctx=8)
    om.eval(0, prompt[:3], nthreads=NTH)
    short = om.eval(3, [prompt[3]], nthreads=NTH)
    dm = hip.Model.load(path, ARCH[arch_s], n_ctx=n_ctx)
    dm.set_mode(hip.MODE_EXACT)
    dm.seq_reserve(3)
    assert np.array_equal(bits(dm.eval_seq(1, 0, prompt)), bits(lg0))
    for n_past in range(P, n_ctx - 1):  # slot 1 alone, as batches of one
        lg, nxt = dm.decode_batch([1], [n_past], [toks[n_past - P]])
        assert np.array_equal(bits(lg[0]), bits(lgs[n_past - P])), n_past
        assert int(nxt[0]) == toks[n_past - P + 1]
    dm.eval_seq(2, 0, prompt[:3], want_logits=False)
    last = n_ctx - 1
    for order in ((0, 1), (1, 0)):
        rows = [(1, last, toks[last - P], lgs[last - P]), (2, 3, prompt[3], short)]
        rows = [rows[i] for i in order]
        lg, nxt = dm.decode_batch([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows])
        for b, r in enumerate(rows):
            assert np.array_equal(bits(lg[b]), bits(r[3])), (order, r[:2])
            assert int(nxt[b]) == int(np.argmax(r[3]))
    with pytest.raises(hip.VsimError, match="n_past outside"):  # the context is full
        dm.decode_batch([1], [n_ctx], [0])
    dm.close()
