"""Greedy speculative decoding on Model.decode_runs (host Python only).

One verify step feeds [last token] + draft to one slot as one run (vsim_model_decode_runs): row i's
greedy id is the plain loop's token after row i wherever rows 1..i were the plain loop's own
tokens, bit for bit, so the accepted tokens are exactly those of the loop that feeds one token per
step -- for every drafter, right or wrong.  A rejected draft needs no undo: the next run starts at a
smaller n_past and overwrites the rows the rejected tokens wrote before anything reads them.

Drafters are objects with propose(ids, k) -> list of at most k token ids that may follow ids (the
prompt and everything generated so far), and accepted(ids), called after every verify step.
"""
from . import hip


def accept(run_tokens, next_ids):
    """The number a in 1..len(run_tokens) of rows of a verified run whose output is a valid
    continuation: row 0 always (its input is the last accepted token), row i iff next_ids[i - 1] ==
    run_tokens[i] and every row before it counts.  The step yields the tokens next_ids[:a]."""
    a = 1
    while a < len(run_tokens) and int(next_ids[a - 1]) == int(run_tokens[a]):
        a += 1
    return a


def generate_speculative(model, prompt, n_predict, drafter, k=7, eos=-1, mode=hip.MODE_W4A16, slot=1):
    """Greedy generation of up to n_predict tokens after `prompt` on cache slot `slot`, `k` drafted
    tokens per verify step.  prompt[:-1] goes in through model.eval_seq (in the model's mode, which
    should be `mode`); then every step verifies [last] + drafter.propose(ids, k) as one run of
    model.decode_runs in `mode`, clipped to n_ctx and to what n_predict still needs; an empty draft is a
    plain one-row step.  Stops after `eos`, after n_predict tokens or at n_ctx.  Returns (ids, stats):
    the generated tokens -- those of the loop that feeds one token per step -- and {"steps": verify
    steps, "drafted": tokens proposed and verified, "accepted": drafted tokens that were right,
    "tokens": len(ids)}."""
    prompt = [int(t) for t in prompt]
    if not prompt:
        raise ValueError("generate_speculative: empty prompt")
    if len(prompt) > model.n_ctx:
        raise ValueError("generate_speculative: prompt longer than n_ctx")
    out = []
    stats = {"steps": 0, "drafted": 0, "accepted": 0, "tokens": 0}
    n_past, last = len(prompt) - 1, prompt[-1]
    if n_past:
        model.eval_seq(slot, 0, prompt[:-1], want_logits=False)
    while len(out) < n_predict and n_past < model.n_ctx:
        rows = min(n_predict - len(out), model.n_ctx - n_past, hip.BATCH_MAX)  # each row yields one token
        want = min(int(k), rows - 1)
        draft = [int(t) for t in drafter.propose(prompt + out, want)][:want] if want > 0 else []
        run = [last] + draft
        _, nxt = model.decode_runs([slot], [n_past], [run], mode, want_logits=False)
        nxt = [int(t) for t in nxt[0]]
        a = accept(run, nxt)
        stats["steps"] += 1
        stats["drafted"] += len(draft)
        stats["accepted"] += a - 1
        new = nxt[:a]
        if eos in new:
            out += new[:new.index(eos) + 1]
            break
        out += new
        n_past += a
        last = new[-1]
        drafter.accepted(prompt + out)
    stats["tokens"] = len(out)
    return out, stats


class NgramDrafter:
    """Prompt lookup: the latest earlier occurrence of the last n tokens (then n - 1, .., 1) in the
    ids so far, and the tokens that followed it."""

    def __init__(self, n=3):
        self.n = int(n)

    def propose(self, ids, k):
        L = len(ids)
        for n in range(min(self.n, L - 1), 0, -1):
            tail = ids[L - n:]
            for s in range(L - n - 1, -1, -1):
                if ids[s:s + n] == tail:
                    return list(ids[s + n:s + n + k])
        return []

    def accepted(self, ids):
        pass


class ModelDrafter:
    """A draft model: Model.generate of k greedy tokens on the draft model's slot 0 (the cache of
    Model.eval / Model.generate).  It keeps that cache in step by itself: before drafting it feeds,
    through Model.eval, whatever tokens of ids[:-1] the cache does not hold yet (after a fully
    accepted draft: the draft's last token; after a rejection: nothing, the rows past the accepted
    prefix are simply overwritten).
    The draft model may be the verifier's own object (self-speculation: fast-mode drafts verified by
    weight-only runs of the same weights): give mode=hip.MODE_FAST and back=the verifier's mode, and
    the drafter switches the model to `mode` around its own calls and to `back` after them; the verify
    slot must then not be 0.  Another model needs the same vocabulary."""

    def __init__(self, model, mode=None, back=None):
        self.m, self.mode, self.back = model, mode, back
        self.fed = []  # the tokens whose rows slot 0 holds, by position

    def propose(self, ids, k):
        ids = [int(t) for t in ids]
        want = ids[:-1]
        k = min(int(k), self.m.n_ctx - len(want))
        if k < 1:
            return []
        c = 0
        while c < len(want) and c < len(self.fed) and self.fed[c] == want[c]:
            c += 1
        if self.mode is not None:
            self.m.set_mode(self.mode)
        try:
            if c < len(want):
                self.m.eval(c, want[c:], want_logits=False)
            draft = [int(t) for t in self.m.generate(len(want), ids[-1], k)]
        finally:
            if self.back is not None:
                self.m.set_mode(self.back)
        self.fed = ids + draft[:-1]  # generate fed ids[-1] and all but the last token it produced
        return draft

    def accepted(self, ids):
        pass  # (propose compares its cache's tokens with ids and catches up from there)


class ReplayDrafter:
    """Proposes a recorded continuation: stream[i] is the token generated i places after the prompt.
    `wrong` corrupts chosen places: a collection of stream indices, or a function of the index.  A
    corrupted place proposes another token (t ^ 1, or (t + 1) % n_vocab with n_vocab given).  For
    tests and for a benchmark's acceptance sweep."""

    def __init__(self, stream, wrong=(), n_vocab=None):
        self.stream = [int(t) for t in stream]
        self.wrong = wrong if callable(wrong) else (lambda i, w=frozenset(wrong): i in w)
        self.n_vocab = n_vocab
        self.prompt_len = None

    def propose(self, ids, k):
        if self.prompt_len is None:
            self.prompt_len = len(ids)  # (the first call comes before anything was generated)
        off = len(ids) - self.prompt_len
        out = []
        for i in range(off, min(off + k, len(self.stream))):
            t = self.stream[i]
            if self.wrong(i):
                t = t ^ 1 if self.n_vocab is None else (t + 1) % self.n_vocab
            out.append(t)
        return out

    def accepted(self, ids):
        pass
