"""vsim_model_decode_runs (Model.decode_runs): a run of tokens per slot in one batched step.

Contract, every mode: row j of a slot's run is bit for bit row 0 of the one-row decode_batch* step the
mode names on that slot at n_past + j after the j rows before it, and the caches end up the same.
Twin slots check it: seq_copy forks one prompt into slots 1..8; slots 1..4 advance by decode_runs in
ragged batches ([1,5,2], [8], [3,3,3,3] = 12 rows and [4,4,3] = 11 rows, the exact product's kernel
threshold, and [32]), slots 5..8 one row per decode_batch* step; every logits row and every next id is
compared bitwise, then both twins take the same one-row step (the caches).  Two-layer models of
modelgen.CONFIGS (E 128, 4 heads of 32, vocabulary 128): the three architectures in exact mode,
GPT-J and GPT-NeoX in fast mode, all three in weight-only mode, and weight-only mode under
vsim_w4a16_set_attn(1) on the architectures without ALiBi -- there also at head dim 64, where the
switch takes the fp16 kernels (at 32 it keeps the exact path's).
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from vsim_amd import hip  # noqa: E402
from vsim_amd import modelgen as mg  # noqa: E402

pytestmark = pytest.mark.gpu

ARCH = {"gptj": hip.ARCH_GPTJ, "gptneox": hip.ARCH_GPTNEOX, "bloom": hip.ARCH_BLOOM}
MODELS = {
    "tiny-gptj": mg.CONFIGS["tiny-gptj"],
    "tiny-neox": mg.CONFIGS["tiny-neox"],
    "tiny-bloom": mg.CONFIGS["tiny-bloom"],
    "gptj-d64": ("gptj", mg.HParams(128, 128, 2, 2, 32)),
    "neox-d64": ("gptneox", mg.HParams(128, 128, 2, 2, 16)),
}
EXACT, FAST, W4 = hip.MODE_EXACT, hip.MODE_FAST, hip.MODE_W4A16
# (model, mode, vsim_w4a16_set_attn)
CASES = [("tiny-gptj", EXACT, 0), ("tiny-neox", EXACT, 0), ("tiny-bloom", EXACT, 0),
         ("tiny-gptj", FAST, 0), ("tiny-neox", FAST, 0),
         ("tiny-gptj", W4, 0), ("tiny-neox", W4, 0), ("tiny-bloom", W4, 0),
         ("tiny-gptj", W4, 1), ("tiny-neox", W4, 1), ("gptj-d64", W4, 1), ("neox-d64", W4, 1)]
IDS = [f"{c[0]}-{('exact', 'fast', 'w4a16')[c[1]]}" + ("-attn16" if c[2] else "") for c in CASES]
N_CTX = 64
PROMPT = 5


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b, what):
    if not np.array_equal(bits(a), bits(b)):
        bad = np.argwhere(bits(a) != bits(b))
        pytest.fail(f"{what}: {len(bad)} values differ, first {bad[:4].tolist()}")


@pytest.fixture
def switch():
    old = hip.w4a16_set_attn(0)
    yield
    hip.w4a16_set_attn(old)


def load(name, mode, tmp_path, slots=9):
    arch_s, hp = MODELS[name]
    path = str(tmp_path / f"{name}.bin")
    mg.write_model(path, arch_s, hp, seed=21, std=0.05)
    dm = hip.Model.load(path, ARCH[arch_s], n_ctx=N_CTX)
    dm.set_mode(mode)
    dm.seq_reserve(slots)
    return dm, hp


def one_row(dm, mode):
    return {EXACT: dm.decode_batch, FAST: dm.decode_batch_fast, W4: dm.decode_batch_w4a16}[mode]


def stepped(dm, mode, slot, n_past, toks):
    """The reference: one row per decode_batch* step.  (logits [n][V], next [n])."""
    rows, nxt = [], []
    for j, t in enumerate(toks):
        lg, nx = one_row(dm, mode)([slot], [n_past + j], [t])
        rows.append(lg[0])
        nxt.append(int(nx[0]))
    return np.stack(rows), nxt


def tokens_of(hp, n, seed):
    return [int(t) for t in np.random.default_rng(seed).integers(0, hp.n_vocab, n)]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_twin_slots(case, tmp_path, switch):
    name, mode, attn = case
    dm, hp = load(name, mode, tmp_path)
    hip.w4a16_set_attn(attn)
    dm.debug_poison(N_CTX)
    dm.eval_seq(1, 0, tokens_of(hp, PROMPT, 1), want_logits=False)
    for s in range(2, 9):
        dm.seq_copy(s, 1, PROMPT)
    pos = [PROMPT] * 4  # pair i: slot 1 + i by runs, slot 5 + i by single steps
    # (pairs, run lengths); the last batch ends pair 3 on the last cache row
    batches = [([0, 1, 2], [1, 5, 2]), ([3], [8]), ([0, 1, 2, 3], [3, 3, 3, 3]), ([2, 1, 0], [4, 4, 3]), ([0], [32]),
               ([3], [32]), ([3, 1], [N_CTX - PROMPT - 43, 2])]
    for bi, (pairs, lens) in enumerate(batches):
        runs = [tokens_of(hp, n, 100 + 10 * bi + i) for i, n in enumerate(lens)]
        lg, nxt = dm.decode_runs([1 + p for p in pairs], [pos[p] for p in pairs], runs, mode)
        assert np.isfinite(lg).all()
        r0 = 0
        for p, run, nx in zip(pairs, runs, nxt):
            want, want_nx = stepped(dm, mode, 5 + p, pos[p], run)
            same(lg[r0:r0 + len(run)], want, f"{IDS[CASES.index(case)]} batch {lens}: slot {1 + p}'s rows at {pos[p]}")
            assert [int(x) for x in nx] == want_nx, (lens, p)
            assert [int(x) for x in nx] == [int(np.argmax(r)) for r in want]
            r0 += len(run)
            pos[p] += len(run)
    assert pos[3] == N_CTX
    # the caches: the same one-row step on both twins
    for p in range(3):
        a = one_row(dm, mode)([1 + p], [pos[p]], [7])[0]
        b = one_row(dm, mode)([5 + p], [pos[p]], [7])[0]
        same(a, b, f"pair {p}: the step after the runs")
    dm.close()


@pytest.mark.parametrize("name,attn", [("tiny-gptj", 0), ("tiny-bloom", 0), ("neox-d64", 1)])
def test_w4a16_run_from_zero_is_the_prompt(name, attn, tmp_path, switch):
    """Weight-only mode: every path gives a row one set of bits, so a run of n from position 0 is
    eval_seq of the same n tokens -- the last row's logits and the cache it leaves."""
    dm, hp = load(name, W4, tmp_path, slots=3)
    hip.w4a16_set_attn(attn)
    dm.debug_poison(N_CTX)
    toks = tokens_of(hp, 32, 2)
    for n in (1, 7, 32):
        lg, _ = dm.decode_runs([1], [0], [toks[:n]], W4)
        same(lg[n - 1], dm.eval_seq(2, 0, toks[:n]), f"run of {n} from 0 against eval_seq")
        same(dm.eval_seq(1, n, [3]), dm.eval_seq(2, n, [3]), f"the step after a run of {n}")
    dm.close()


@pytest.mark.parametrize("case", [CASES[0], CASES[4], CASES[7], CASES[11]], ids=[IDS[0], IDS[4], IDS[7], IDS[11]])
def test_rollback_and_independence(case, tmp_path, switch):
    name, mode, attn = case
    dm, hp = load(name, mode, tmp_path, slots=6)
    hip.w4a16_set_attn(attn)
    dm.debug_poison(N_CTX)
    dm.eval_seq(1, 0, tokens_of(hp, PROMPT, 1), want_logits=False)
    for s in (2, 3, 4, 5):
        dm.seq_copy(s, 1, PROMPT)
    t = tokens_of(hp, 6, 5)
    wrong = [(x + 1) % hp.n_vocab for x in t]
    # slot 1 sees three wrong rows after t[0], then continues from PROMPT + 1; slot 2 never saw them
    dm.decode_runs([1], [PROMPT], [[t[0]] + wrong[1:4]], mode)
    a, an = dm.decode_runs([1], [PROMPT + 1], [t[1:]], mode)
    dm.decode_runs([2], [PROMPT], [[t[0]]], mode)
    b, bn = dm.decode_runs([2], [PROMPT + 1], [t[1:]], mode)
    same(a, b, "rows after a rollback")
    assert [int(x) for x in an[0]] == [int(x) for x in bn[0]]
    same(one_row(dm, mode)([1], [PROMPT + 6], [9])[0], one_row(dm, mode)([2], [PROMPT + 6], [9])[0], "step after a rollback")
    # independence: slot 3's run alone, and beside two other slots' runs in another order
    alone, _ = dm.decode_runs([3], [PROMPT], [t], mode)
    other = tokens_of(hp, 9, 6)
    mixed, _ = dm.decode_runs([5, 4, 1], [PROMPT, PROMPT, PROMPT + 6], [other[:2], t, other[2:]], mode)
    same(mixed[2:8], alone, "a slot's rows beside other runs")
    dm.close()


@pytest.mark.parametrize("mode", [EXACT, W4], ids=["exact", "w4a16"])
def test_errors_leave_the_caches_alone(mode, tmp_path):
    dm, hp = load("tiny-gptj", mode, tmp_path, slots=4)
    dm.debug_poison(N_CTX)
    dm.eval_seq(1, 0, tokens_of(hp, PROMPT, 1), want_logits=False)
    dm.seq_copy(2, 1, PROMPT)
    V = hp.n_vocab
    bad = [
        ([], [], [], "S < 1"),
        ([1, 2], [PROMPT, PROMPT], [[1], []], "len < 1"),
        ([1, 2], [PROMPT, PROMPT], [[1] * 30, [1] * 3], "N > 32"),
        ([1], [PROMPT], [[1] * 33], "len > 32"),
        ([4], [PROMPT], [[1]], "slot outside the reserve"),
        ([-1], [PROMPT], [[1]], "negative slot"),
        ([1, 1], [PROMPT, PROMPT + 1], [[1], [2]], "slot named twice"),
        ([1], [-1], [[1]], "n_past < 0"),
        ([1], [N_CTX - 2], [[1, 2, 3]], "run past n_ctx"),
        ([1], [N_CTX], [[1]], "n_past = n_ctx"),
        ([1], [PROMPT], [[1, V]], "token = n_vocab"),
        ([1], [PROMPT], [[-1]], "token < 0"),
        ([1, 2], [PROMPT, PROMPT], [[1, 2], [3, V]], "a later run's token outside the vocabulary"),
    ]
    for seqs, npast, runs, what in bad:
        with pytest.raises(hip.VsimError, match="decode_runs"):
            dm.decode_runs(seqs, npast, runs, mode)
    with pytest.raises(hip.VsimError, match="decode_runs"):
        dm.decode_runs([1], [PROMPT], [[1]], 3)   # no such mode
    L = hip.lib()
    one = np.ones(1, np.int32)
    for args in [(None, mode, 1, hip.ptr(one), hip.ptr(one), hip.ptr(one), hip.ptr(one)),
                 (dm.h, mode, 1, None, hip.ptr(one), hip.ptr(one), hip.ptr(one)),
                 (dm.h, mode, 1, hip.ptr(one), None, hip.ptr(one), hip.ptr(one)),
                 (dm.h, mode, 1, hip.ptr(one), hip.ptr(one), None, hip.ptr(one)),
                 (dm.h, mode, 1, hip.ptr(one), hip.ptr(one), hip.ptr(one), None)]:
        assert L.vsim_model_decode_runs(*args, None, None) == -1
    if mode != EXACT:  # exact products are refused on a model that is not in exact mode
        with pytest.raises(hip.VsimError, match="decode_runs"):
            dm.decode_runs([1], [PROMPT], [[1]], EXACT)
    # nothing was enqueued: slot 1 still is slot 2's twin, NaN rows past the prompt included
    a, _ = dm.decode_runs([1], [PROMPT], [[4, 5, 6]], mode)
    b, _ = dm.decode_runs([2], [PROMPT], [[4, 5, 6]], mode)
    assert np.isfinite(a).all()
    same(a, b, "the caches after the refused calls")
    dm.close()


def test_stage_model_is_refused(tmp_path):
    arch_s, hp = MODELS["tiny-gptj"]
    path = str(tmp_path / "stage.bin")
    mg.write_model(path, arch_s, hp, seed=21, std=0.05)
    dm = hip.Model.load(path, ARCH[arch_s], n_ctx=N_CTX, layer_begin=0, layer_end=1)
    with pytest.raises(hip.VsimError, match="decode_runs"):
        dm.decode_runs([0], [0], [[1]], EXACT)
    dm.close()


def test_profile_names_the_two_launches(tmp_path):
    dm, hp = load("tiny-neox", W4, tmp_path, slots=2)
    dm.set_profile(True)
    dm.decode_runs([1], [0], [[1, 2, 3]], W4)
    names = [k["name"] for k in dm.profile_kernels()]
    dm.set_profile(False)
    assert "k_kv_rows + k_attn_decode_runs" in names and "k_attn_decode_batch" not in names, names
    dm.close()
