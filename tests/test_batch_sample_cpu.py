"""No GPU: the sampled side of vsim_amd/batch.py (generate_many(samplers=...), sample_n) on a stub
model with real Sampler objects.  The stub's logits row is a deterministic function of the slot's
history, and its sampled step draws with the sampler it is handed (sample_host), so a sampler that
met the wrong sequence, missed a prompt token or drew out of turn shows in the streams."""
import numpy as np
import pytest

from vsim_amd import hip
from vsim_amd.batch import generate_many, sample_n

V = 97
PARAMS = [dict(seed=42, top_k=20, top_p=0.95, temp=0.85, repeat_last_n=64, repeat_penalty=1.3),
          dict(seed=43, top_k=40, top_p=0.95, temp=0.8, repeat_last_n=64, repeat_penalty=1.3),
          dict(seed=7, top_k=64, top_p=1.0, temp=1.3, repeat_last_n=4, repeat_penalty=1.1),
          dict(seed=9, top_k=3, top_p=0.5, temp=0.5, repeat_last_n=0, repeat_penalty=1.0),
          dict(seed=11, top_k=5, top_p=0.9, temp=1.0, repeat_last_n=16, repeat_penalty=2.0)]
PROMPTS = [[1], [2, 3, 4], [5, 6], [7, 8, 9, 10, 11], [12, 13]]


def _row(history):
    h = 7
    for i, t in enumerate(history):
        h = (h * 31 + (t + 1) * (i + 3)) % 1000003
    return (np.random.default_rng(h).standard_normal(V) * 2).astype(np.float32)


class Rec(hip.Sampler):
    """A Sampler that records what reaches it."""

    def __init__(self, **p):
        super().__init__(**p)
        self.events = []

    def accept(self, token):
        self.events.append(("accept", int(token)))
        super().accept(token)

    def sample_host(self, logits):
        t = super().sample_host(logits)
        self.events.append(("draw", t))
        return t


def _alone(prompt, p, n_predict, eos, n_ctx):
    """The reference's loop for one sequence on the stub's rows, under batch.py's retirement rules."""
    s = hip.Sampler(**p)
    for t in prompt:
        s.accept(t)
    hist, out = list(prompt), []
    while True:
        t = s.sample_host(_row(hist))
        out.append(t)
        if t == eos or len(out) >= n_predict or len(hist) >= n_ctx:
            return out
        hist.append(t)


class Stub:
    def __init__(self, n_ctx=64, greedy_only=False):
        self.n_ctx, self.n_vocab = n_ctx, V
        self.reserved, self.hist, self.log = 1, {}, []
        self.greedy_only = greedy_only

    def seq_reserve(self, n):
        assert n >= self.reserved
        self.reserved = n
        self.log.append(("reserve", n))

    def eval_seq(self, seq, n_past, tokens, want_logits=True):
        assert 0 <= seq < self.reserved and n_past == 0 and 0 < len(tokens) <= self.n_ctx
        self.hist[seq] = list(tokens)
        self.log.append(("eval", seq, len(tokens)))
        return _row(self.hist[seq])

    def seq_copy(self, dst, src, n_tokens):
        assert dst != src and 0 <= dst < self.reserved and 0 <= src < self.reserved
        assert n_tokens == len(self.hist[src])
        self.hist[dst] = list(self.hist[src][:n_tokens])
        self.log.append(("copy", dst, src, n_tokens))

    def decode_batch(self, seqs, n_past, tokens, want_logits=True):
        assert not want_logits
        rows = self._advance(seqs, n_past, tokens)
        self.log.append(("step", tuple(seqs), tuple(n_past)))
        return None, np.asarray([int(np.argmax(r)) for r in rows], np.int32)

    def decode_batch_sample(self, seqs, n_past, tokens, samplers, fast=False):
        assert not self.greedy_only, "the greedy loop must not reach the sampled step"
        samplers = list(samplers)
        assert len(samplers) == len(seqs) and len({id(s) for s in samplers}) == len(samplers)
        rows = self._advance(seqs, n_past, tokens)
        self.log.append(("sstep", tuple(seqs), tuple(n_past), tuple(id(s) for s in samplers), fast))
        return np.asarray([s.sample_host(r) for s, r in zip(samplers, rows)], np.int32)  # in row order

    def _advance(self, seqs, n_past, tokens):
        seqs, n_past, tokens = list(seqs), list(n_past), list(tokens)
        assert 1 <= len(seqs) <= 32 and len(set(seqs)) == len(seqs), "a slot twice in one step"
        assert seqs == sorted(seqs)
        rows = []
        for s, p, t in zip(seqs, n_past, tokens):
            assert 0 <= s < self.reserved
            assert p == len(self.hist[s]) and p < self.n_ctx, "position is the slot's history length"
            self.hist[s].append(int(t))
            rows.append(_row(self.hist[s]))
        return rows


def test_streams_are_each_sequence_alone_across_slot_reuse():
    m = Stub()
    sm = [Rec(**p) for p in PARAMS]
    got = generate_many(m, PROMPTS, 9, n_slots=2, samplers=sm)
    assert got == [_alone(pr, p, 9, -1, m.n_ctx) for pr, p in zip(PROMPTS, PARAMS)]
    # every step hands each slot the sampler of the sequence that lives there
    owner, waiting = {}, list(range(len(PROMPTS)))
    for e in m.log:
        if e[0] == "eval":
            owner[e[1]] = waiting.pop(0)
        elif e[0] == "sstep":
            assert [id(sm[owner[s]]) for s in e[1]] == list(e[3])
            assert e[4] is False
    assert sorted(set(owner)) == [0, 1] and not waiting
    assert not any(e[0] == "step" for e in m.log)


def test_prompt_tokens_are_accepted_before_the_first_draw():
    m = Stub()
    sm = [Rec(**p) for p in PARAMS]
    got = generate_many(m, PROMPTS, 4, n_slots=3, samplers=sm)
    for pr, s, g in zip(PROMPTS, sm, got):
        assert s.events[:len(pr)] == [("accept", t) for t in pr]
        assert [e for e in s.events[len(pr):]] == [("draw", t) for t in g]  # nothing else is ever accepted
        assert s.stats() == {"device": 0, "host": len(g)}


def test_retirement_on_eos_n_predict_and_context_end():
    base = _alone(PROMPTS[1], PARAMS[1], 12, -1, 64)
    eos = base[2]
    m = Stub()
    got = generate_many(m, PROMPTS, 12, eos=eos, n_slots=2, samplers=[hip.Sampler(**p) for p in PARAMS])
    assert got == [_alone(pr, p, 12, eos, 64) for pr, p in zip(PROMPTS, PARAMS)]
    assert got[1][-1] == eos and len(got[1]) <= 3
    assert all(eos not in g[:-1] and len(g) <= 12 for g in got)
    m = Stub(n_ctx=8)
    prompts = [[1, 2, 3, 4, 5, 6], [7], [1, 2, 3, 4, 5, 6, 7, 8]]
    got = generate_many(m, prompts, 20, n_slots=2, samplers=[hip.Sampler(**p) for p in PARAMS[:3]])
    assert got == [_alone(pr, p, 20, -1, 8) for pr, p in zip(prompts, PARAMS)]
    assert [len(g) for g in got] == [3, 8, 1]
    assert all(max(e[2]) < 8 for e in m.log if e[0] == "sstep")


def test_without_samplers_the_greedy_calls_are_unchanged():
    m = Stub(greedy_only=True)
    got = generate_many(m, PROMPTS, 4, n_slots=3)
    assert [len(g) for g in got] == [4] * 5
    assert m.log == [("reserve", 3), ("eval", 0, 1), ("eval", 1, 3), ("eval", 2, 2),
                     ("step", (0, 1, 2), (1, 3, 2)), ("step", (0, 1, 2), (2, 4, 3)), ("step", (0, 1, 2), (3, 5, 4)),
                     ("eval", 0, 5), ("eval", 1, 2),
                     ("step", (0, 1), (5, 2)), ("step", (0, 1), (6, 3)), ("step", (0, 1), (7, 4))]
    m2 = Stub(greedy_only=True)
    assert generate_many(m2, PROMPTS, 4, n_slots=3, samplers=None) == got and m2.log == m.log


def test_fast_flag_reaches_the_sampled_step_and_argument_checks():
    m = Stub()
    generate_many(m, PROMPTS[:2], 3, fast=True, samplers=[hip.Sampler(**p) for p in PARAMS[:2]])
    assert [e[4] for e in m.log if e[0] == "sstep"] == [True, True]
    with pytest.raises(ValueError):
        generate_many(m, PROMPTS, 3, samplers=[hip.Sampler()])
    with pytest.raises(ValueError):
        sample_n(m, [], [hip.Sampler()], 3)
    with pytest.raises(ValueError):
        sample_n(m, [1], [hip.Sampler() for _ in range(33)], 3)
    assert sample_n(m, [1], [], 3) == [] and sample_n(m, [1], [hip.Sampler()], 0) == [[]]


def test_sample_n_evaluates_the_prompt_once_and_forks():
    m = Stub()
    prompt = [3, 1, 4, 1, 5]
    sm = [Rec(**p) for p in PARAMS[:4]]
    base = _alone(prompt, PARAMS[2], 10, -1, 64)
    eos = base[3]  # one stream retires early; the others go on in smaller batches
    got = sample_n(m, prompt, sm, 10, eos=eos)
    assert got == [_alone(prompt, p, 10, eos, 64) for p in PARAMS[:4]]
    assert m.log[:5] == [("reserve", 4), ("eval", 0, 5), ("copy", 1, 0, 5), ("copy", 2, 0, 5), ("copy", 3, 0, 5)]
    assert sum(e[0] == "eval" for e in m.log) == 1
    for s, g in zip(sm, got):
        assert s.events == [("accept", t) for t in prompt] + [("draw", t) for t in g]
    steps = [e for e in m.log if e[0] == "sstep"]
    assert steps[0][1] == (0, 1, 2, 3) and len(steps[-1][1]) < 4
    for e in steps:
        assert list(e[3]) == [id(sm[s]) for s in e[1]]
