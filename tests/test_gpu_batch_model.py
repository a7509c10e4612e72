"""Batched decode (vsim_model_seq_reserve / _eval_seq / _decode_batch), exact mode: every row of
every step is, bit for bit, the logits row the CPU oracle gives for that sequence run alone with
the same history -- whatever shares the batch, in whatever order, at whatever positions.

The reference of a sequence is an oracle model holding the device model's weights
(oracle_py.Model.from_device) that sees that sequence only: its prompt, then its greedy tokens one
at a time.  Small models get one oracle instance per sequence; at full width one instance serves
the sequences one after another (each starts again at position 0), which gives the same rows.
"""
import os

import numpy as np
import pytest

from vsim_amd import hip
from vsim_amd import modelgen as mg
from vsim_amd.batch import generate_many

pytestmark = pytest.mark.gpu

ARCH = {"gptj": hip.ARCH_GPTJ, "gptneox": hip.ARCH_GPTNEOX, "bloom": hip.ARCH_BLOOM}
NTH = max(1, min(16, os.cpu_count() or 1))  # the oracle's rows are independent chains: same bits
EINVAL = -1


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _trajectory(om, prompt, steps, nthreads=1):
    """The sequence alone on the oracle: [(n_past, tokens fed, logits)] for the prompt and then
    `steps` greedy tokens."""
    lg = om.eval(0, prompt, nthreads=nthreads)
    tr, n_past = [(0, list(prompt), lg)], len(prompt)
    for _ in range(steps):
        t = int(np.argmax(lg))
        lg = om.eval(n_past, [t], nthreads=nthreads)
        tr.append((n_past, [t], lg))
        n_past += 1
    return tr


class Seq:
    """A sequence on a device slot, walking its oracle trajectory."""

    def __init__(self, slot, tr):
        self.slot, self.tr, self.i = slot, tr, 1  # tr[0] is the prompt

    def row(self):
        n_past, toks, _ = self.tr[self.i]
        return self.slot, n_past, toks[0]

    def check(self, lg, nxt, what):
        want = self.tr[self.i][2]
        if not np.array_equal(bits(lg), bits(want)):
            bad = np.nonzero(bits(lg) != bits(want))[0]
            pytest.fail(f"{what}: slot {self.slot} at n_past {self.tr[self.i][0]}: {bad.size} logits differ, "
                        f"first {bad[:5]} oracle {want[bad[:3]]} device {lg[bad[:3]]}")
        assert int(nxt) == int(np.argmax(lg)), (what, self.slot)
        self.i += 1


def _step(dm, seqs, what):
    rows = [s.row() for s in seqs]
    lg, nxt = dm.decode_batch([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows])
    assert lg.shape == (len(seqs), dm.n_vocab) and nxt.shape == (len(seqs),)
    for b, s in enumerate(seqs):
        s.check(lg[b], nxt[b], what)
    # the ids alone (no logits copy) are the same ids
    return nxt


@pytest.fixture
def gemm_setting():
    old = hip.batch_set_gemm(1)
    yield
    hip.batch_set_gemm(old)


@pytest.mark.parametrize("gemm", [2, 0, 1], ids=["rows-gemm", "gemv-jobs", "default"])
@pytest.mark.parametrize("cfg", ["small-neox", "small-gptj", "small-bloom"])
def test_small_models_changing_batches(cfg, gemm, tmp_path, gemm_setting):
    import oracle_py as O
    arch_s, hp = mg.CONFIGS[cfg]
    path = str(tmp_path / f"{cfg}.bin")
    mg.write_model(path, arch_s, hp, seed=11, std=0.05)
    dm = hip.Model.load(path, ARCH[arch_s])
    dm.set_mode(hip.MODE_EXACT)
    dm.set_graph(True)
    hip.batch_set_gemm(gemm)
    rng = np.random.default_rng(5)
    # lengths 9 and 33 take eval_seq through the prompt GEMV-job and GEMM regimes
    prompts = [list(rng.integers(0, hp.n_vocab, n)) for n in (1, 3, 5, 9, 33)]
    STEPS = 16
    oms = [O.Model.from_device(dm, arch_s) for _ in prompts]
    trs = [_trajectory(om, p, STEPS) for om, p in zip(oms, prompts)]
    dm.seq_reserve(5)
    dm.seq_reserve(5)  # the same count again: nothing to do
    seqs = [Seq(s, trs[s]) for s in range(5)]
    # slot 0 through the plain eval: the prompt, then three single-token steps on the captured graph
    assert np.array_equal(bits(dm.eval(0, prompts[0])), bits(trs[0][0][2]))
    for _ in range(3):
        n_past, toks, want = trs[0][seqs[0].i]
        assert np.array_equal(bits(dm.eval(n_past, toks)), bits(want))
        seqs[0].i += 1
    assert dm.info()["graph"]
    for s in range(1, 5):
        assert np.array_equal(bits(dm.eval_seq(s, 0, prompts[s])), bits(trs[s][0][2])), f"eval_seq prompt {s}"
    for k in range(4):  # all five, rows in a different order each step
        order = [seqs[(i + k) % 5] for i in range(5)] if k % 2 == 0 else list(reversed(seqs))
        _step(dm, order, f"step {k} (all)")
    for k in range(4, 7):  # one dropped
        _step(dm, [seqs[4], seqs[0], seqs[1], seqs[3]], f"step {k} (without slot 2)")
    for k in range(7, 9):  # B = 1
        _step(dm, [seqs[3]], f"step {k} (alone)")
    # slot 2 retired: a new prompt restarts it
    p2 = list(rng.integers(0, hp.n_vocab, 4))
    om2 = O.Model.from_device(dm, arch_s)
    tr2 = _trajectory(om2, p2, 4)
    assert np.array_equal(bits(dm.eval_seq(2, 0, p2)), bits(tr2[0][2])), "restarted slot's prompt"
    seqs[2] = Seq(2, tr2)
    for k in range(9, 12):
        _step(dm, [seqs[2], seqs[0], seqs[4]], f"step {k} (restarted slot 2)")
    # only the ids asked for: the same ids, and the cache advanced as with the logits copy
    rows = [s.row() for s in (seqs[1], seqs[3])]
    lg, nxt = dm.decode_batch([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], want_logits=False)
    assert lg is None
    assert [int(t) for t in nxt] == [int(np.argmax(s.tr[s.i][2])) for s in (seqs[1], seqs[3])]
    for s in (seqs[1], seqs[3]):
        s.i += 1
    _step(dm, [seqs[1], seqs[3]], "after an ids-only step")
    # slot 0's cache is intact for the single-sequence entry points
    n_past, toks, want = trs[0][seqs[0].i]
    assert np.array_equal(bits(dm.eval(n_past, toks)), bits(want)), "plain eval on slot 0 after the batches"
    # eval_seq with N = 1 is the same row too (general path)
    n_past, toks, want = seqs[4].tr[seqs[4].i]
    assert np.array_equal(bits(dm.eval_seq(4, n_past, toks)), bits(want)), "eval_seq N = 1"
    dm.close()


def _pair(cfg, n_layer=2, seed=7, n_ctx=512):
    import oracle_py as O
    arch_s, hp = mg.CONFIGS[cfg]
    dm = hip.Model.create(ARCH[arch_s], dict(n_vocab=hp.n_vocab, n_embd=hp.n_embd, n_head=hp.n_head,
                                             n_layer=n_layer, n_rot=hp.n_rot,
                                             use_parallel_residual=hp.use_parallel_residual), n_ctx=n_ctx)
    dm.randomize(seed=seed, std=0.02)
    om = O.Model.from_device(dm, arch_s, n_ctx=n_ctx)
    return arch_s, hp, dm, om


@pytest.mark.parametrize("cfg", ["gpt-j-6B", "gpt-neoxt-20b", "bloom-560m"])
def test_full_width_batches(cfg, gemm_setting):
    """Two layers at the real widths: GPT-J d = 256 with M = 4096 / 16384 / 50400, GPT-NeoXT-20B
    d = 96 and E = 6144, bloom-560m ALiBi and the 250,880-row head; B = 5 at ragged positions."""
    arch_s, hp, dm, om = _pair(cfg)
    dm.set_mode(hip.MODE_EXACT)
    rng = np.random.default_rng(3)
    prompts = [list(rng.integers(0, hp.n_vocab, n)) for n in (2, 5, 1, 7, 3)]
    STEPS = 6  # with k_gemm_exact_rows, then one through the GEMV-job path and one with the default choice
    trs = [_trajectory(om, p, STEPS + 2, nthreads=NTH) for p in prompts]  # one after another, each from 0
    spin0 = hip.spin_timeouts()
    dm.seq_reserve(5)
    dm.debug_poison(32)  # every slot and the scratch NaN: nothing unwritten may be read
    seqs = [Seq(s, trs[s]) for s in range(5)]
    for s in range(5):
        assert np.array_equal(bits(dm.eval_seq(s, 0, prompts[s])), bits(trs[s][0][2])), f"prompt {s}"
    for k in range(STEPS + 2):
        hip.batch_set_gemm(2 if k < STEPS else k - STEPS)
        _step(dm, seqs if k % 2 == 0 else list(reversed(seqs)), f"{cfg} step {k}")
    assert hip.spin_timeouts() == spin0
    dm.close()


def test_argument_errors(tmp_path, gemm_setting):
    arch_s, hp = mg.CONFIGS["tiny-gptj"]
    path = str(tmp_path / "tiny.bin")
    mg.write_model(path, arch_s, hp, seed=2, std=0.05)
    L = hip.lib()
    dm = hip.Model.load(path, hip.ARCH_GPTJ, n_ctx=64)
    dm.seq_reserve(3)

    def call(m, seqs, n_past, toks):
        a, b, c = (np.ascontiguousarray(v, np.int32) for v in (seqs, n_past, toks))
        nxt = np.zeros(64, np.int32)
        return L.vsim_model_decode_batch(m.h, len(seqs), a.ctypes.data, b.ctypes.data, c.ctypes.data, None,
                                         nxt.ctypes.data)

    assert call(dm, [0, 1, 2], [0, 0, 0], [1, 2, 3]) == 0
    assert call(dm, [0, 1, 1], [1, 1, 1], [1, 2, 3]) == EINVAL       # a duplicate slot
    assert call(dm, [0, 3], [1, 1], [1, 2]) == EINVAL                # a slot beyond the reserve
    assert call(dm, [0, -1], [1, 1], [1, 2]) == EINVAL
    assert call(dm, [0, 1], [1, 64], [1, 2]) == EINVAL               # n_past == n_ctx
    assert call(dm, [0, 1], [1, -1], [1, 2]) == EINVAL
    assert call(dm, [0, 1], [1, 1], [1, hp.n_vocab]) == EINVAL       # a token outside the vocabulary
    assert call(dm, [], [], []) == EINVAL                            # B = 0
    assert call(dm, [0, 1], [63, 1], [1, 2]) == 0                    # the last position is in range
    assert L.vsim_model_seq_reserve(dm.h, 2) == EINVAL               # shrinking
    assert L.vsim_model_seq_reserve(dm.h, 0) == EINVAL
    tok = np.ascontiguousarray([1], np.int32)
    assert L.vsim_model_eval_seq(dm.h, 3, 0, tok.ctypes.data, 1, None) == EINVAL
    assert L.vsim_model_eval_seq(dm.h, 1, 64, tok.ctypes.data, 1, None) == EINVAL
    dm.seq_reserve(33)
    assert call(dm, list(range(33)), [0] * 33, [1] * 33) == EINVAL   # B = 33
    assert call(dm, list(range(32)), [0] * 32, [1] * 32) == 0
    dm.set_mode(hip.MODE_FAST)                                       # a fast-mode model
    assert call(dm, [0, 1], [1, 1], [1, 2]) == EINVAL
    assert b"exact mode" in L.vsim_last_error()
    assert L.vsim_model_eval_seq(dm.h, 1, 1, tok.ctypes.data, 1, None) == 0  # eval_seq works in both modes
    dm.close()
    # a pipeline stage that is not a whole model
    st = hip.Model.load(path, hip.ARCH_GPTJ, n_ctx=64, layer_begin=0, layer_end=1)
    assert L.vsim_model_seq_reserve(st.h, 2) == EINVAL
    assert call(st, [0], [0], [1]) == EINVAL
    assert L.vsim_model_eval_seq(st.h, 0, 0, tok.ctypes.data, 1, None) == EINVAL
    st.close()


def test_generate_many_equals_single_sequence_runs(tmp_path, gemm_setting):
    arch_s, hp = mg.CONFIGS["small-gptj"]
    path = str(tmp_path / "small-gptj.bin")
    mg.write_model(path, arch_s, hp, seed=4, std=0.05)
    rng = np.random.default_rng(9)
    prompts = [list(int(t) for t in rng.integers(0, hp.n_vocab, n)) for n in (4, 1, 9, 2, 6, 3, 12)]
    dm = hip.Model.load(path, hip.ARCH_GPTJ)
    dm.set_mode(hip.MODE_EXACT)
    got = generate_many(dm, prompts, 10, n_slots=3)
    dm.close()
    one = hip.Model.load(path, hip.ARCH_GPTJ)
    one.set_mode(hip.MODE_EXACT)
    for p, g in zip(prompts, got):
        t0 = int(np.argmax(one.eval(0, p)))
        assert g == [t0] + one.generate(len(p), t0, 9), p
    # with an eos: each sequence stops at its first occurrence
    eos = got[0][3]
    dm = hip.Model.load(path, hip.ARCH_GPTJ)
    dm.set_mode(hip.MODE_EXACT)
    got_e = generate_many(dm, prompts, 10, eos=eos, n_slots=3)
    dm.close()
    for g, ge in zip(got, got_e):
        assert ge == (g[:g.index(eos) + 1] if eos in g else g)
    assert len(got_e[0]) <= 4
    one.close()
