"""The fast batched decode step (vsim_model_decode_batch_fast): every row of every step is, bit for
bit, the logits row vsim_model_eval_seq(N = 1) gives on the same model in MODE_FAST from the same
cache state -- whatever shares the batch, in whatever order, at whatever positions, under every
setting of vsim_batch_set_fast_gemm, and whatever mode the model itself is in.

Slots come in pairs with the same prompt, fed by identical calls: slot 2 i advances by
decode_batch_fast, its twin 2 i + 1 by eval_seq with the model in MODE_FAST.  The token streams are
teacher-forced from a fixed RNG (not the argmax), so both sides see the same tokens even where a
logit tie would split a greedy pair.
"""
import numpy as np
import pytest

from vsim_amd import hip
from vsim_amd import modelgen as mg
from vsim_amd.batch import generate_many

pytestmark = pytest.mark.gpu

ARCH = {"gptj": hip.ARCH_GPTJ, "gptneox": hip.ARCH_GPTNEOX, "bloom": hip.ARCH_BLOOM}
EINVAL = -1


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture
def fast_gemm_setting():
    old = hip.batch_set_fast_gemm(1)
    yield
    hip.batch_set_fast_gemm(old)


class Pair:
    """A sequence twice: on slot `a` (the batch's) and on its twin `b` (eval_seq's)."""

    def __init__(self, i, n_past=0):
        self.a, self.b, self.n_past = 2 * i, 2 * i + 1, n_past


class Twins:
    def __init__(self, dm, model_mode, seed):
        self.dm, self.mode, self.rng = dm, model_mode, np.random.default_rng(seed)
        dm.set_mode(model_mode)

    def token(self):
        return int(self.rng.integers(0, self.dm.n_vocab))

    def prefill(self, pair, n):
        """The same prompt into both slots by the same call, in the model's own mode."""
        prompt = [self.token() for _ in range(n)]
        la, lb = self.dm.eval_seq(pair.a, 0, prompt), self.dm.eval_seq(pair.b, 0, prompt)
        assert np.array_equal(bits(la), bits(lb)), "the pair's prompts differ"
        pair.n_past = n

    def twin_row(self, slot, n_past, tok):
        """eval_seq (N = 1) in MODE_FAST, the model put back into its own mode afterwards."""
        self.dm.set_mode(hip.MODE_FAST)
        lg = self.dm.eval_seq(slot, n_past, [tok])
        self.dm.set_mode(self.mode)
        return lg

    def step(self, pairs, what, want_logits=True):
        toks = [self.token() for _ in pairs]
        lg, nxt = self.dm.decode_batch_fast([p.a for p in pairs], [p.n_past for p in pairs], toks,
                                            want_logits=want_logits)
        assert nxt.shape == (len(pairs),)
        assert (lg is None) if not want_logits else lg.shape == (len(pairs), self.dm.n_vocab)
        for r, (p, t) in enumerate(zip(pairs, toks)):
            want = self.twin_row(p.b, p.n_past, t)
            if want_logits and not np.array_equal(bits(lg[r]), bits(want)):
                bad = np.nonzero(bits(lg[r]) != bits(want))[0]
                pytest.fail(f"{what}: slot {p.a} at n_past {p.n_past}: {bad.size} logits differ from eval_seq, "
                            f"first {bad[:5]}: {lg[r][bad[:3]]} against {want[bad[:3]]}")
            assert int(nxt[r]) == int(np.argmax(want)), (what, p.a)
            p.n_past += 1

    def step_by_eval_seq(self, pair, what):
        """Both slots by eval_seq in MODE_FAST: the batch's slot may be advanced by either call."""
        t = self.token()
        la = self.twin_row(pair.a, pair.n_past, t)
        lb = self.twin_row(pair.b, pair.n_past, t)
        assert np.array_equal(bits(la), bits(lb)), what
        pair.n_past += 1


def _small(cfg, tmp_path, seed=11):
    arch_s, hp = mg.CONFIGS[cfg]
    path = str(tmp_path / f"{cfg}.bin")
    mg.write_model(path, arch_s, hp, seed=seed, std=0.05)
    return hip.Model.load(path, ARCH[arch_s]), hp


@pytest.mark.parametrize("model_mode", [hip.MODE_FAST, hip.MODE_EXACT], ids=["model-fast", "model-exact"])
@pytest.mark.parametrize("gemm", [2, 0, 1], ids=["rows-kernel", "gemv-per-row", "default"])
@pytest.mark.parametrize("cfg", ["small-neox", "small-gptj", "small-bloom"])
def test_small_models_changing_batches(cfg, gemm, model_mode, tmp_path, fast_gemm_setting):
    dm, hp = _small(cfg, tmp_path)
    hip.batch_set_fast_gemm(gemm)
    dm.seq_reserve(8)
    dm.debug_poison(32)  # every slot and the scratch NaN: nothing unwritten may be read
    T = Twins(dm, model_mode, seed=5)
    pairs = [Pair(i) for i in range(4)]
    for p, n in zip(pairs, (1, 3, 5, 9)):  # (9: the prompt GEMM regime of a fast-mode model)
        T.prefill(p, n)
    for k in range(3):  # all four, rows in a different order each step
        order = [pairs[(i + k) % 4] for i in range(4)] if k % 2 == 0 else list(reversed(pairs))
        T.step(order, f"step {k} (all)")
    for k in range(3, 5):  # one dropped
        T.step([pairs[3], pairs[0], pairs[1]], f"step {k} (without pair 2)")
    T.step([pairs[3]], "B = 1")
    T.prefill(pairs[2], 4)  # a retired pair restarts with a new prompt
    for k in range(6, 8):
        T.step([pairs[2], pairs[0], pairs[3]], f"step {k} (restarted pair 2)")
    T.step([pairs[1], pairs[3]], "ids only", want_logits=False)
    T.step([pairs[1], pairs[3]], "after an ids-only step")
    # mixed feeding: the batch's slot alternately by the two calls
    for k in range(4):
        if k % 2 == 0:
            T.step_by_eval_seq(pairs[0], f"mixed {k}")
        else:
            T.step([pairs[0], pairs[2]], f"mixed {k}")
    dm.close()


@pytest.mark.parametrize("cfg", ["gpt-j-6B", "pythia-12b", "bloom-560m"])
def test_full_width_batches(cfg, fast_gemm_setting):
    """Two layers at the real widths: GPT-J E = 4096 with M = 4096 / 16384 / 50400, pythia-12b E = 5120
    and the ragged 50,288-row head, bloom-560m ALiBi and the 250,880-row head.  B = 5 at ragged
    positions, then one B = 32 step."""
    arch_s, hp = mg.CONFIGS[cfg]
    dm = hip.Model.create(ARCH[arch_s], dict(n_vocab=hp.n_vocab, n_embd=hp.n_embd, n_head=hp.n_head, n_layer=2,
                                             n_rot=hp.n_rot, use_parallel_residual=hp.use_parallel_residual),
                          n_ctx=64)
    dm.randomize(seed=7, std=0.02)
    spin0 = hip.spin_timeouts()
    dm.seq_reserve(64)
    dm.debug_poison(32)
    T = Twins(dm, hip.MODE_FAST, seed=3)
    pairs = [Pair(i) for i in range(32)]
    for p, n in zip(pairs[:5], (2, 5, 1, 7, 3)):
        T.prefill(p, n)
    for k in range(4):
        hip.batch_set_fast_gemm((2, 2, 0, 1)[k])
        T.step(pairs[:5] if k % 2 == 0 else list(reversed(pairs[:5])), f"{cfg} step {k}")
    hip.batch_set_fast_gemm(2)
    T.step(pairs, f"{cfg} B = 32")  # (pairs 5..31 start at position 0)
    assert hip.spin_timeouts() == spin0
    dm.close()


def test_gap_to_exact_mode_is_printed(tmp_path, fast_gemm_setting):
    """Sanity, not asserted beyond finiteness: how far a fast row lies from the exact row of the same
    cache state (fast mode's own error, that of eval_seq in MODE_FAST)."""
    dm, hp = _small("small-gptj", tmp_path)
    dm.set_mode(hip.MODE_EXACT)
    dm.seq_reserve(2)
    prompt = [3, 1, 4, 1, 5]
    dm.eval_seq(0, 0, prompt)
    dm.eval_seq(1, 0, prompt)
    fast, _ = dm.decode_batch_fast([0], [5], [9])
    exact, _ = dm.decode_batch([1], [5], [9])
    f, e = fast[0].astype(np.float64), exact[0].astype(np.float64)
    cos = float(f @ e / np.sqrt((f @ f) * (e @ e)))
    rel = float(np.abs(f - e).max() / np.abs(e).max())
    print(f"fast row against exact row (small-gptj): cos {cos:.6f}, max-rel {rel:.3e}")
    assert np.isfinite(f).all() and np.isfinite(e).all()
    dm.close()


def test_generate_many_fast_equals_eval_seq_loops(tmp_path, fast_gemm_setting):
    dm, hp = _small("small-gptj", tmp_path, seed=4)
    dm.set_mode(hip.MODE_FAST)
    rng = np.random.default_rng(9)
    prompts = [list(int(t) for t in rng.integers(0, hp.n_vocab, n)) for n in (4, 1, 9, 2, 6, 3, 12)]
    got = generate_many(dm, prompts, 8, n_slots=3, fast=True)
    for p, g in zip(prompts, got):
        want, n_past = [int(np.argmax(dm.eval_seq(0, 0, p)))], len(p)
        while len(want) < 8:
            want.append(int(np.argmax(dm.eval_seq(0, n_past, [want[-1]]))))
            n_past += 1
        assert g == want, p
    dm.close()


def test_argument_errors(tmp_path, fast_gemm_setting):
    arch_s, hp = mg.CONFIGS["tiny-gptj"]
    path = str(tmp_path / "tiny.bin")
    mg.write_model(path, arch_s, hp, seed=2, std=0.05)
    L = hip.lib()
    dm = hip.Model.load(path, hip.ARCH_GPTJ, n_ctx=64)
    dm.seq_reserve(3)

    def call(m, seqs, n_past, toks, fn=None):
        a, b, c = (np.ascontiguousarray(v, np.int32) for v in (seqs, n_past, toks))
        nxt = np.zeros(64, np.int32)
        return (fn or L.vsim_model_decode_batch_fast)(m.h, len(seqs), a.ctypes.data, b.ctypes.data, c.ctypes.data,
                                                      None, nxt.ctypes.data)

    for mode in (hip.MODE_EXACT, hip.MODE_FAST):  # the call names its path: both model modes serve
        dm.set_mode(mode)
        assert call(dm, [0, 1, 2], [0, 0, 0], [1, 2, 3]) == 0
        assert call(dm, [0, 1, 1], [1, 1, 1], [1, 2, 3]) == EINVAL       # a duplicate slot
        assert call(dm, [0, 3], [1, 1], [1, 2]) == EINVAL                # a slot beyond the reserve
        assert call(dm, [0, -1], [1, 1], [1, 2]) == EINVAL
        assert call(dm, [0, 1], [1, 64], [1, 2]) == EINVAL               # n_past == n_ctx
        assert call(dm, [0, 1], [1, -1], [1, 2]) == EINVAL
        assert call(dm, [0, 1], [1, 1], [1, hp.n_vocab]) == EINVAL       # a token outside the vocabulary
        assert call(dm, [], [], []) == EINVAL                            # B = 0
        assert call(dm, [0, 1], [63, 1], [1, 2]) == 0                    # the last position is in range
    assert L.vsim_model_decode_batch_fast(None, 1, None, None, None, None, None) == EINVAL
    dm.seq_reserve(33)
    assert call(dm, list(range(33)), [0] * 33, [1] * 33) == EINVAL       # B = 33
    assert call(dm, list(range(32)), [0] * 32, [1] * 32) == 0
    # decode_batch still refuses a fast-mode model, and says why
    assert call(dm, [0, 1], [1, 1], [1, 2], L.vsim_model_decode_batch) == EINVAL
    assert b"exact mode" in L.vsim_last_error()
    dm.close()
    # a pipeline stage that is not a whole model
    st = hip.Model.load(path, hip.ARCH_GPTJ, n_ctx=64, layer_begin=0, layer_end=1)
    assert call(st, [0], [0], [1]) == EINVAL
    st.close()
