"""No GPU: generate_many(fast=...) on a stub model picks the step call by the keyword alone --
fast=True only decode_batch_fast, fast=False (the default) only decode_batch -- with the same
schedule and the same outputs either way; prompts go through eval_seq in both."""
import numpy as np

from vsim_amd.batch import generate_many

V = 97


def _next(history):
    h = 7
    for i, t in enumerate(history):
        h = (h * 31 + (t + 1) * (i + 3)) % 1000003
    return h % V


class Stub:
    def __init__(self, n_ctx=64):
        self.n_ctx, self.n_vocab = n_ctx, V
        self.hist = {}
        self.calls = []  # "eval" / "step" / "step_fast", in order

    def seq_reserve(self, n):
        pass

    def eval_seq(self, seq, n_past, tokens, want_logits=True):
        assert n_past == 0
        self.hist[seq] = list(tokens)
        self.calls.append("eval")
        lg = np.zeros(V, np.float32)
        lg[_next(self.hist[seq])] = 1.0
        return lg

    def _step(self, name, seqs, n_past, tokens, want_logits):
        assert not want_logits and len(set(seqs)) == len(list(seqs))
        nxt = []
        for s, p, t in zip(seqs, n_past, tokens):
            assert p == len(self.hist[s])
            self.hist[s].append(int(t))
            nxt.append(_next(self.hist[s]))
        self.calls.append(name)
        return None, np.asarray(nxt, np.int32)

    def decode_batch(self, seqs, n_past, tokens, want_logits=True):
        return self._step("step", seqs, n_past, tokens, want_logits)

    def decode_batch_fast(self, seqs, n_past, tokens, want_logits=True):
        return self._step("step_fast", seqs, n_past, tokens, want_logits)


PROMPTS = [[1], [2, 3, 4], [5, 6], [7, 8, 9, 10, 11], [12]]


def test_fast_keyword_picks_the_step_call():
    fast, exact, default = Stub(), Stub(), Stub()
    got_f = generate_many(fast, PROMPTS, 6, n_slots=2, fast=True)
    got_e = generate_many(exact, PROMPTS, 6, n_slots=2, fast=False)
    got_d = generate_many(default, PROMPTS, 6, n_slots=2)
    assert got_f == got_e == got_d and all(len(g) == 6 for g in got_f)
    assert "step_fast" in fast.calls and "step" not in fast.calls
    assert "step" in exact.calls and "step_fast" not in exact.calls
    assert default.calls == exact.calls
    # the same schedule: only the step call's name differs; every prompt through eval_seq
    assert [c.replace("step_fast", "step") for c in fast.calls] == exact.calls
    assert fast.calls.count("eval") == len(PROMPTS)
