"""Continuous batching over one model's sequence slots, greedy or sampled.

generate_many() and sample_n() drive a model through its Model methods only (n_ctx, seq_reserve,
eval_seq, decode_batch, decode_batch_fast, decode_batch_w4a16, and for sampling decode_batch_sample
and seq_copy), so
anything with those methods serves: the device model, or a stub on the CPU.
"""
from __future__ import annotations

import numpy as np

BATCH_MAX = 32  # VSIM_BATCH_MAX: rows of one decode_batch step


MODE_W4A16 = 2  # VSIM_MODE_W4A16


def generate_many(model, prompts, n_predict, eos=-1, n_slots=None, fast=False, samplers=None, w4a16=False):
    """Greedy (samplers=None) or sampled continuations of `prompts` (token-id lists), up to n_predict tokens each.

    Prompts are admitted in order, each into the lowest free slot: the prompt is evaluated there
    with eval_seq, and the argmax of its last row is the sequence's first token.  Then decode_batch
    advances all live sequences by one token per step, rows in slot order.  A sequence retires when
    it has produced `eos` (kept as its last token; -1: none), n_predict tokens, or when its next
    token would have no position left in the context (n_ctx); its slot goes to the next waiting
    prompt before the following step.  Returns one token list per prompt, in the prompts' order.

    n_slots: how many sequences run at once (default: min(len(prompts), BATCH_MAX)); the model is
    asked for that many slots once (seq_reserve).  In exact mode every sequence's tokens are those
    of the sequence run alone: a row's logits do not depend on what shares its batch.

    fast: the steps go through decode_batch_fast (fast-mode products, one weight pass per step for
    all rows) instead of decode_batch.  Prompts still go through eval_seq, in the model's mode; on a
    model in fast mode every sequence's tokens are then those of its own eval_seq loop.

    w4a16: the steps go through decode_batch_w4a16 (weight-only products: Q4_0 weights, fp16
    activation rows) instead; not together with fast.  On a model in weight-only mode every
    sequence's tokens are those of its own eval_seq loop, bit for bit.

    samplers: one Sampler per prompt; it follows its sequence through whatever slots and batches
    the sequence meets.  On admission the prompt's tokens enter the sampler's window (accept), and
    the first token is sample_host on eval_seq's logits row, as the reference's loop does after a
    prompt; from then on the steps go through decode_batch_sample.  In exact mode every sequence's
    tokens are the reference's for that prompt and those parameters alone.
    """
    prompts = [list(p) for p in prompts]
    out = [[] for _ in prompts]
    if fast and w4a16:
        raise ValueError("generate_many: fast and w4a16 name two numeric paths")
    if not prompts or n_predict <= 0:
        return out
    for p in prompts:
        if not p or len(p) > model.n_ctx:
            raise ValueError("generate_many: a prompt must have 1..n_ctx tokens")
    if samplers is not None:
        samplers = list(samplers)
        if len(samplers) != len(prompts):
            raise ValueError("generate_many: one sampler per prompt")
    n_slots = min(len(prompts), BATCH_MAX) if n_slots is None else int(n_slots)
    if not 1 <= n_slots <= BATCH_MAX:
        raise ValueError(f"generate_many: n_slots must be in 1..{BATCH_MAX}")
    model.seq_reserve(n_slots)
    free = list(range(n_slots))  # ascending: the lowest free slot is taken first
    live = {}                    # slot -> [prompt index, n_past, last token]
    waiting = list(range(len(prompts)))

    def push(slot, i, n_past, tok):
        """Record sequence i's new token; keep the sequence live unless it retires."""
        out[i].append(tok)
        if tok == eos or len(out[i]) >= n_predict or n_past >= model.n_ctx:
            free.append(slot)
            free.sort()
        else:
            live[slot] = [i, n_past, tok]

    while waiting or live:
        while waiting and free:
            slot, i = free.pop(0), waiting.pop(0)
            lg = model.eval_seq(slot, 0, prompts[i])
            if samplers is None:
                first = int(np.argmax(lg))
            else:
                for t in prompts[i]:
                    samplers[i].accept(t)
                first = samplers[i].sample_host(lg)
            push(slot, i, len(prompts[i]), first)
        if not live:
            continue
        slots = sorted(live)
        if samplers is None:
            step = model.decode_batch_w4a16 if w4a16 else model.decode_batch_fast if fast else model.decode_batch
            _, nxt = step(slots, [live[s][1] for s in slots], [live[s][2] for s in slots],
                          want_logits=False)
        else:
            nxt = model.decode_batch_sample(slots, [live[s][1] for s in slots], [live[s][2] for s in slots],
                                            [samplers[live[s][0]] for s in slots],
                                            **({"mode": MODE_W4A16} if w4a16 else {"fast": fast}))
        for s, t in zip(slots, nxt):
            i, n_past, _ = live.pop(s)
            push(s, i, n_past + 1, int(t))
    return out


def sample_n(model, prompt, samplers, n_predict, eos=-1, fast=False, w4a16=False):
    """len(samplers) sampled continuations of one prompt, the prompt evaluated once.

    The prompt goes through eval_seq into slot 0; seq_copy forks that cache into slots 1.., one per
    sampler.  Every sampler takes the prompt into its window and draws its first token from the one
    logits row (sample_host); then decode_batch_sample advances the live sequences, rows in slot
    order, until each has produced `eos` (kept; -1: none), n_predict tokens, or has no position
    left in the context.  Returns one token list per sampler: in exact mode the reference's stream
    for that prompt and that sampler's parameters alone.  w4a16: the steps run with weight-only
    products (decode_batch_sample's mode), not together with fast.
    """
    if fast and w4a16:
        raise ValueError("sample_n: fast and w4a16 name two numeric paths")
    prompt, samplers = list(prompt), list(samplers)
    n = len(samplers)
    out = [[] for _ in samplers]
    if not n or n_predict <= 0:
        return out
    if not prompt or len(prompt) > model.n_ctx:
        raise ValueError("sample_n: the prompt must have 1..n_ctx tokens")
    if n > BATCH_MAX:
        raise ValueError(f"sample_n: at most {BATCH_MAX} samplers")
    model.seq_reserve(n)
    lg = model.eval_seq(0, 0, prompt)
    for slot in range(1, n):
        model.seq_copy(slot, 0, len(prompt))
    live = {}  # slot -> [n_past, last token]

    def push(slot, n_past, tok):
        out[slot].append(tok)
        if not (tok == eos or len(out[slot]) >= n_predict or n_past >= model.n_ctx):
            live[slot] = [n_past, tok]

    for slot, sm in enumerate(samplers):
        for t in prompt:
            sm.accept(t)
        push(slot, len(prompt), sm.sample_host(lg))
    while live:
        slots = sorted(live)
        nxt = model.decode_batch_sample(slots, [live[s][0] for s in slots], [live[s][1] for s in slots],
                                        [samplers[s] for s in slots],
                                        **({"mode": MODE_W4A16} if w4a16 else {"fast": fast}))
        for s, t in zip(slots, nxt):
            n_past, _ = live.pop(s)
            push(s, n_past + 1, int(t))
    return out
