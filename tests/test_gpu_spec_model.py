"""Greedy speculative decoding on the device (vsim_amd/spec.py over Model.decode_runs): the ids are
those of the plain loop, bit for bit, for every drafter.

Weight-only mode, tiny GPT-J and GPT-NeoX (two layers, E 128, vocabulary 128): the ids equal
Model.generate's (the fused single-token step has the general path's bits) with ReplayDrafter (no,
some and every place wrong), with NgramDrafter, and with ModelDrafter on the same model object in fast
mode (self-speculation; the verify slot is 1).  Exact mode with mode=MODE_EXACT: Model.generate's ids
too.  Fast mode: the ids of the one-row decode_batch_fast loop.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from vsim_amd import hip  # noqa: E402
from vsim_amd import modelgen as mg  # noqa: E402
from vsim_amd.spec import ModelDrafter, NgramDrafter, ReplayDrafter, generate_speculative  # noqa: E402

pytestmark = pytest.mark.gpu

ARCH = {"gptj": hip.ARCH_GPTJ, "gptneox": hip.ARCH_GPTNEOX}
N_CTX = 96
N_PREDICT = 40
PROMPT = [5, 9, 2, 77, 31, 8]


def load(name, mode, tmp_path):
    arch_s, hp = mg.CONFIGS[name]
    path = str(tmp_path / f"{name}.bin")
    mg.write_model(path, arch_s, hp, seed=31, std=0.05)
    dm = hip.Model.load(path, ARCH[arch_s], n_ctx=N_CTX)
    dm.set_mode(mode)
    dm.seq_reserve(3)
    return dm, hp


def generate_ids(dm):
    """Model.generate after the prompt, on slot 0."""
    dm.eval(0, PROMPT[:-1], want_logits=False)
    return [int(t) for t in dm.generate(len(PROMPT) - 1, PROMPT[-1], N_PREDICT)]


@pytest.mark.parametrize("name", ["tiny-gptj", "tiny-neox"])
def test_w4a16_ids_are_generates(name, tmp_path):
    dm, hp = load(name, hip.MODE_W4A16, tmp_path)
    want = generate_ids(dm)
    drafters = {
        "replay, all right": ReplayDrafter(want, n_vocab=hp.n_vocab),
        "replay, some wrong": ReplayDrafter(want, wrong=(0, 3, 4, 11, 12, 13, 30), n_vocab=hp.n_vocab),
        "replay, all wrong": ReplayDrafter(want, wrong=lambda i: True, n_vocab=hp.n_vocab),
        "ngram": NgramDrafter(3),
        "self-speculation": ModelDrafter(dm, mode=hip.MODE_FAST, back=hip.MODE_W4A16),
    }
    for what, d in drafters.items():
        dm.debug_poison(N_CTX)
        ids, st = generate_speculative(dm, PROMPT, N_PREDICT, d, k=7, slot=1)
        assert ids == want, (name, what)
        assert st["tokens"] == N_PREDICT == st["steps"] + st["accepted"], (what, st)
        if what == "replay, all right":
            assert st["steps"] == N_PREDICT // 8 and st["accepted"] == st["drafted"]
        if what == "replay, all wrong":
            assert st["accepted"] == 0 and st["steps"] == N_PREDICT
    # an eos inside an accepted run
    eos = want[10]
    ids, _ = generate_speculative(dm, PROMPT, N_PREDICT, ReplayDrafter(want), k=7, eos=eos, slot=2)
    assert ids == want[:want.index(eos) + 1]
    dm.close()


@pytest.mark.parametrize("name", ["tiny-gptj", "tiny-neox"])
def test_exact_ids_are_generates(name, tmp_path):
    dm, hp = load(name, hip.MODE_EXACT, tmp_path)
    want = generate_ids(dm)
    for wrong in ((), (1, 2, 9, 20, 21), range(N_PREDICT)):
        ids, st = generate_speculative(dm, PROMPT, N_PREDICT, ReplayDrafter(want, wrong=wrong, n_vocab=hp.n_vocab), k=5,
                                       mode=hip.MODE_EXACT, slot=1)
        assert ids == want, (name, wrong)
    dm.close()


@pytest.mark.parametrize("name", ["tiny-gptj", "tiny-neox"])
def test_fast_ids_are_the_one_row_loops(name, tmp_path):
    dm, hp = load(name, hip.MODE_FAST, tmp_path)
    dm.eval_seq(2, 0, PROMPT[:-1], want_logits=False)
    want, last = [], PROMPT[-1]
    for i in range(N_PREDICT):
        _, nx = dm.decode_batch_fast([2], [len(PROMPT) - 1 + i], [last], want_logits=False)
        last = int(nx[0])
        want.append(last)
    for wrong in ((), (0, 5, 6, 7, 25), range(N_PREDICT)):
        ids, st = generate_speculative(dm, PROMPT, N_PREDICT, ReplayDrafter(want, wrong=wrong, n_vocab=hp.n_vocab), k=7,
                                       mode=hip.MODE_FAST, slot=1)
        assert ids == want, (name, wrong)
    ids, _ = generate_speculative(dm, PROMPT, N_PREDICT, NgramDrafter(2), k=4, mode=hip.MODE_FAST, slot=1)
    assert ids == want
    dm.close()
