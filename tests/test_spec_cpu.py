"""No GPU: the speculative loop (vsim_amd/spec.py) on a stub model whose greedy token is a
deterministic function of the slot's history, so a wrong acceptance, a stale cache row that is read,
or a run at the wrong position shows in the ids."""
import numpy as np
import pytest

from vsim_amd import hip
from vsim_amd.spec import ModelDrafter, NgramDrafter, ReplayDrafter, accept, generate_speculative

V = 97


def _next(history):
    h = 7
    for i, t in enumerate(history):
        h = (h * 31 + (t + 1) * (i + 3)) % 1000003
    return h % V


def plain(prompt, n_predict, eos=-1, n_ctx=64):
    """The loop that feeds one token per step."""
    hist, out = list(prompt[:-1]), []
    last = prompt[-1]
    while len(out) < n_predict and len(hist) < n_ctx:
        hist.append(last)
        last = _next(hist)
        out.append(last)
        if last == eos:
            break
    return out


class Stub:
    """Slot caches as token lists; a row at position p overwrites row p and sees rows 0..p only."""

    def __init__(self, n_ctx=64):
        self.n_ctx, self.n_vocab = n_ctx, V
        self.cache = {}
        self.log = []

    def eval_seq(self, seq, n_past, tokens, want_logits=True):
        assert n_past == 0 and 0 < len(tokens) <= self.n_ctx
        self.cache[seq] = list(tokens)
        self.log.append(("eval_seq", seq, len(tokens)))

    def decode_runs(self, seqs, n_past, runs, mode, want_logits=True):
        assert len(seqs) == len(n_past) == len(runs) == 1 and not want_logits
        assert mode == self.mode
        s, p, run = seqs[0], n_past[0], list(runs[0])
        c = self.cache.setdefault(s, [])
        assert 1 <= len(run) <= hip.BATCH_MAX and 0 <= p <= len(c) and p + len(run) <= self.n_ctx
        nxt = []
        for j, t in enumerate(run):
            del c[p + j:]  # (rows past the position are never read)
            c.append(int(t))
            nxt.append(_next(c))
        self.log.append(("runs", s, p, len(run)))
        return None, [np.asarray(nxt, np.int32)]

    mode = hip.MODE_W4A16


class Fixed:
    """Proposes whatever `fn(ids, k)` says; records the calls."""

    def __init__(self, fn):
        self.fn, self.calls, self.seen = fn, [], []

    def propose(self, ids, k):
        self.calls.append((len(ids), k))
        return self.fn(list(ids), k)

    def accepted(self, ids):
        self.seen.append(len(ids))


def perfect(ids, k):
    out, h = [], list(ids)
    for _ in range(k):
        out.append(_next(h))
        h.append(out[-1])
    return out


PROMPT = [3, 1, 4, 1, 5]


def test_accept_hand_cases():
    assert accept([5], [9]) == 1
    assert accept([5, 9, 2], [9, 2, 7]) == 3
    assert accept([5, 9, 2], [9, 3, 2]) == 2
    assert accept([5, 9, 2], [8, 2, 7]) == 1
    assert accept([5, 8, 2, 7], [9, 2, 7, 1]) == 1   # later matches do not count after a miss
    assert accept([5, 9, 2, 6], [9, 2, 7, 6]) == 3
    assert accept([5, 9], np.asarray([9, 4], np.int32)) == 2


def test_perfect_drafter_ids_and_steps():
    m = Stub(n_ctx=128)
    ids, st = generate_speculative(m, PROMPT, 64, Fixed(perfect), k=7)
    assert ids == plain(PROMPT, 64, n_ctx=128)
    assert st == {"steps": 8, "drafted": 56, "accepted": 56, "tokens": 64}
    assert m.log[0] == ("eval_seq", 1, 4)


def test_always_wrong_drafter():
    m = Stub()
    d = Fixed(lambda ids, k: [(t + 1) % V for t in perfect(ids, k)])
    ids, st = generate_speculative(m, PROMPT, 20, d, k=5)
    assert ids == plain(PROMPT, 20)
    assert st["steps"] == 20 and st["accepted"] == 0 and st["tokens"] == 20
    assert st["drafted"] == sum(k for _, k in d.calls)
    assert d.seen == [len(PROMPT) + i for i in range(1, 21)]


@pytest.mark.parametrize("off", range(7))
def test_wrong_at_one_offset(off):
    def fn(ids, k):
        p = perfect(ids, k)
        if off < len(p):
            p[off] = (p[off] + 1) % V
        return p
    m = Stub()
    ids, st = generate_speculative(m, PROMPT, 30, Fixed(fn), k=7)
    assert ids == plain(PROMPT, 30)
    assert st["tokens"] == 30 == st["steps"] + st["accepted"]


def test_empty_and_short_drafts():
    m = Stub()
    ids, st = generate_speculative(m, PROMPT, 10, Fixed(lambda ids, k: []), k=7)
    assert ids == plain(PROMPT, 10) and st == {"steps": 10, "drafted": 0, "accepted": 0, "tokens": 10}
    assert all(e[3] == 1 for e in m.log if e[0] == "runs")
    ids, st = generate_speculative(Stub(), PROMPT, 10, Fixed(lambda ids, k: perfect(ids, 2)), k=7)
    assert ids == plain(PROMPT, 10)
    # a drafter that offers more than k is cut to k
    m = Stub()
    ids, _ = generate_speculative(m, PROMPT, 12, Fixed(lambda ids, k: perfect(ids, k + 5)), k=3)
    assert ids == plain(PROMPT, 12) and max(e[3] for e in m.log if e[0] == "runs") == 4


def test_eos_inside_an_accepted_run():
    full = plain(PROMPT, 20)
    eos = full[10]
    want = plain(PROMPT, 20, eos=eos)
    assert want[-1] == eos and len(want) <= 11
    ids, st = generate_speculative(Stub(), PROMPT, 20, Fixed(perfect), k=7, eos=eos)
    assert ids == want and st["tokens"] == len(want)


def test_n_predict_ends_inside_a_run():
    for n in (1, 5, 8, 9, 13):
        m = Stub()
        ids, st = generate_speculative(m, PROMPT, n, Fixed(perfect), k=7)
        assert ids == plain(PROMPT, n) and len(ids) == n
        assert sum(e[3] for e in m.log if e[0] == "runs") == n  # no row beyond what is needed


def test_run_clipped_at_n_ctx():
    m = Stub(n_ctx=16)
    ids, st = generate_speculative(m, PROMPT, 100, Fixed(perfect), k=7)
    assert ids == plain(PROMPT, 100, n_ctx=16) and len(ids) == 16 - 4
    runs = [e for e in m.log if e[0] == "runs"]
    assert all(e[2] + e[3] <= 16 for e in runs) and runs[-1][2] + runs[-1][3] == 16


def test_single_token_prompt_and_other_slot_and_mode():
    m = Stub()
    m.mode = hip.MODE_EXACT
    ids, _ = generate_speculative(m, [9], 12, Fixed(perfect), k=4, mode=hip.MODE_EXACT, slot=3)
    assert ids == plain([9], 12)
    assert all(e[0] == "runs" and e[1] == 3 for e in m.log)
    with pytest.raises(ValueError):
        generate_speculative(m, [], 4, Fixed(perfect))


def test_stats_add_up():
    rng = np.random.default_rng(0)

    def fn(ids, k):
        p = perfect(ids, k)
        return [t if rng.random() < 0.7 else (t + 1) % V for t in p]
    d = Fixed(fn)
    ids, st = generate_speculative(Stub(n_ctx=128), PROMPT, 90, d, k=6)
    assert ids == plain(PROMPT, 90, n_ctx=128)
    assert st["tokens"] == len(ids) == st["steps"] + st["accepted"]
    assert st["accepted"] <= st["drafted"] == sum(k for _, k in d.calls)
    assert len(d.calls) == st["steps"]


def test_ngram_drafter_on_a_periodic_stream():
    d = NgramDrafter(n=3)
    ids = [1, 2, 3, 4, 5] * 3 + [1, 2]
    assert d.propose(ids, 4) == [3, 4, 5, 1]
    assert d.propose(ids, 40) == [3, 4, 5, 1, 2]  # the latest earlier occurrence, to the end of ids
    assert d.propose([7, 8, 9], 4) == []
    assert d.propose([7, 8, 7], 2) == [8, 7]     # falls back to shorter n-grams
    assert d.propose([5], 3) == []
    # in the loop: right or wrong, the ids are the plain loop's
    ids, st = generate_speculative(Stub(), PROMPT, 25, NgramDrafter(2), k=5)
    assert ids == plain(PROMPT, 25)


def test_replay_drafter():
    stream = plain(PROMPT, 40)
    for wrong in ((), (0,), (3, 4, 20), range(40), lambda i: i % 3 == 1):
        d = ReplayDrafter(stream, wrong=wrong, n_vocab=V)
        ids, st = generate_speculative(Stub(), PROMPT, 40, d, k=7)
        assert ids == stream
    d = ReplayDrafter(stream)
    ids, st = generate_speculative(Stub(), PROMPT, 40, d, k=7)
    assert ids == stream and st["steps"] == 5 and st["accepted"] == st["drafted"] == 35
    d = ReplayDrafter([10, 11, 12, 13], wrong=(1,))
    assert d.propose([1, 2], 3) == [10, 10, 12] and d.propose([1, 2, 10], 5) == [10, 12, 13]


class DraftStub:
    """A draft model that records what it was fed: eval and generate on slot 0."""

    def __init__(self, n_ctx=64):
        self.n_ctx, self.n_vocab = n_ctx, V
        self.cache, self.log, self.modes = [], [], []

    def set_mode(self, mode):
        self.modes.append(mode)

    def eval(self, n_past, tokens, want_logits=True):
        assert n_past <= len(self.cache) and not want_logits and len(tokens) > 0
        self.cache[n_past:] = [int(t) for t in tokens]
        self.log.append(("eval", n_past, list(tokens)))

    def generate(self, n_past, token, n_steps):
        assert n_past <= len(self.cache) and n_past + n_steps <= self.n_ctx
        out = []
        for i in range(n_steps):
            self.cache[n_past + i:] = [int(token)]
            token = (_next(self.cache) + (1 if len(self.cache) in self.bad else 0)) % V
            out.append(token)
        self.log.append(("generate", n_past, n_steps))
        return out

    bad = ()


def test_model_drafter_catch_up():
    dm = DraftStub()
    d = ModelDrafter(dm)
    ids = list(PROMPT)
    p = d.propose(ids, 4)
    assert dm.log == [("eval", 0, PROMPT[:-1]), ("generate", 4, 4)] and p == perfect(PROMPT, 4)
    # full acceptance: ids grew by the draft and the bonus token; only the draft's last token is fed
    bonus = _next(ids + p)
    ids2 = ids + p + [bonus]
    dm.log.clear()
    p2 = d.propose(ids2, 4)
    assert dm.log == [("eval", 8, [p[-1]]), ("generate", 9, 4)]
    assert p2 == perfect(ids2, 4)
    # partial acceptance: two drafted tokens kept, then the verifier's own token: nothing to feed
    ids3 = ids2 + p2[:2] + [(p2[2] + 1) % V]
    dm.log.clear()
    p3 = d.propose(ids3, 4)
    assert dm.log == [("generate", 12, 4)]
    assert p3 == perfect(ids3, 4)
    assert dm.cache[:len(ids3)] == ids3
    # clipped at the draft model's context; mode switching around the calls
    dm2 = DraftStub(n_ctx=8)
    d2 = ModelDrafter(dm2, mode=hip.MODE_FAST, back=hip.MODE_W4A16)
    assert len(d2.propose(PROMPT, 7)) == 4 and d2.propose(list(range(9)), 3) == []
    assert dm2.modes == [hip.MODE_FAST, hip.MODE_W4A16]


def test_model_drafter_in_the_loop():
    """A draft model that is wrong at some positions: the ids stay the plain loop's."""
    dm = DraftStub(n_ctx=128)
    dm.bad = {9, 10, 17, 30, 31, 32, 45}
    ids, st = generate_speculative(Stub(n_ctx=128), PROMPT, 60, ModelDrafter(dm), k=6)
    assert ids == plain(PROMPT, 60, n_ctx=128)
    assert 0 < st["accepted"] < st["drafted"]
