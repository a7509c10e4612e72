"""No GPU: the continuous-batching loop (vsim_amd/batch.py generate_many) on a stub model whose
next token is a deterministic function of the slot's history, so every schedule decision shows in
the outputs: retirement on eos / n_predict / n_ctx, slot reuse order, no slot twice in a step,
one output list per prompt in the prompts' order."""
import numpy as np
import pytest

from vsim_amd.batch import generate_many

V = 97


def _next(history):
    """The stub's greedy token after `history`: depends on every token and on the length."""
    h = 7
    for i, t in enumerate(history):
        h = (h * 31 + (t + 1) * (i + 3)) % 1000003
    return h % V


def _alone(prompt, n_predict, eos, n_ctx):
    """What one sequence run alone produces under generate_many's retirement rules."""
    hist, out = list(prompt), []
    while True:
        t = _next(hist)
        out.append(t)
        if t == eos or len(out) >= n_predict or len(hist) >= n_ctx:
            return out
        hist.append(t)


class Stub:
    def __init__(self, n_ctx=64):
        self.n_ctx, self.n_vocab = n_ctx, V
        self.reserved = 1
        self.hist = {}
        self.log = []  # ("eval", slot, n_tokens) / ("step", slots, n_past)

    def seq_reserve(self, n):
        assert n >= self.reserved
        self.reserved = n

    def eval_seq(self, seq, n_past, tokens, want_logits=True):
        assert 0 <= seq < self.reserved and n_past == 0 and 0 < len(tokens) <= self.n_ctx
        self.hist[seq] = list(tokens)
        self.log.append(("eval", seq, len(tokens)))
        lg = np.zeros(V, np.float32)
        lg[_next(self.hist[seq])] = 1.0
        return lg

    def decode_batch(self, seqs, n_past, tokens, want_logits=True):
        seqs, n_past, tokens = list(seqs), list(n_past), list(tokens)
        assert 1 <= len(seqs) <= 32 and len(set(seqs)) == len(seqs), "a slot twice in one step"
        assert not want_logits
        nxt = []
        for s, p, t in zip(seqs, n_past, tokens):
            assert 0 <= s < self.reserved
            assert p == len(self.hist[s]) and p < self.n_ctx, "position is the slot's history length"
            self.hist[s].append(int(t))
            nxt.append(_next(self.hist[s]))
        self.log.append(("step", tuple(seqs), tuple(n_past)))
        return None, np.asarray(nxt, np.int32)


PROMPTS = [[1], [2, 3, 4], [5, 6], [7, 8, 9, 10, 11], [12], [13, 14], [15, 16, 17]]


def test_outputs_are_each_sequence_alone_in_prompt_order():
    m = Stub()
    got = generate_many(m, PROMPTS, 9, n_slots=3)
    assert got == [_alone(p, 9, -1, m.n_ctx) for p in PROMPTS]
    assert all(len(g) == 9 for g in got)
    assert m.reserved == 3


def test_slot_reuse_order_and_batch_composition():
    m = Stub()
    # different budgets through eos: pick each prompt's eos-free length by its own stream
    got = generate_many(m, PROMPTS, 4, n_slots=3)
    evals = [e for e in m.log if e[0] == "eval"]
    # the first three prompts take slots 0, 1, 2 in order, before any step
    assert m.log[:3] == [("eval", 0, 1), ("eval", 1, 3), ("eval", 2, 2)]
    # all retire together after n_predict = 4 tokens (1 from the prompt + 3 steps), and the next
    # three prompts reuse the slots lowest first; the last prompt runs alone
    assert [e[1] for e in evals] == [0, 1, 2, 0, 1, 2, 0]
    steps = [e for e in m.log if e[0] == "step"]
    assert [s[1] for s in steps] == [(0, 1, 2)] * 6 + [(0,)] * 3
    assert steps[0][2] == (1, 3, 2) and steps[3][2] == (5, 1, 2)
    assert [len(g) for g in got] == [4] * 7


def test_retirement_on_eos_frees_the_slot_for_the_next_prompt():
    m = Stub()
    base = _alone(PROMPTS[1], 12, -1, m.n_ctx)
    eos = base[2]  # prompt 1 stops at its third token (if no earlier token equals it)
    got = generate_many(m, PROMPTS, 12, eos=eos, n_slots=2)
    want = [_alone(p, 12, eos, m.n_ctx) for p in PROMPTS]
    assert got == want
    assert got[1][-1] == eos and len(got[1]) <= 3
    for g in got:  # eos only ever as the last token
        assert eos not in g[:-1]
    # a step never names a slot twice and never more slots than reserved (the stub asserts the
    # first); every step's rows are in slot order
    for e in m.log:
        if e[0] == "step":
            assert list(e[1]) == sorted(e[1]) and len(e[1]) <= 2


def test_retirement_at_the_context_end():
    m = Stub(n_ctx=8)
    prompts = [[1, 2, 3, 4, 5, 6], [7], [1, 2, 3, 4, 5, 6, 7, 8]]
    got = generate_many(m, prompts, 20, n_slots=2)
    assert got == [_alone(p, 20, -1, 8) for p in prompts]
    # 6-token prompt: positions 6 and 7 remain, so 1 + 2 tokens; the full-context prompt yields
    # its one token and never enters a step
    assert [len(g) for g in got] == [3, 8, 1]
    for e in m.log:
        if e[0] == "step":
            assert max(e[2]) < 8


def test_edge_arguments():
    m = Stub()
    assert generate_many(m, [], 5) == []
    assert generate_many(m, [[1], [2]], 0) == [[], []]
    assert m.log == []
    with pytest.raises(ValueError):
        generate_many(m, [[]], 3)
    with pytest.raises(ValueError):
        generate_many(m, [[1]], 3, n_slots=33)
    one = generate_many(m, [[4, 5]], 1)
    assert one == [[_next([4, 5])]] and [e[0] for e in m.log] == ["eval"]
