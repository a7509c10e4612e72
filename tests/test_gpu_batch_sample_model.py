"""The sampled batched step (vsim_model_decode_batch_sample), slot fork (vsim_model_seq_copy) and the
loops on them (generate_many(samplers=...), sample_n): every sequence's sampled stream is the one
it has alone -- the oracle's loop, the reference's golden streams, eval_sample on a twin model --
whatever shares its batch."""
import ctypes
import functools
import os
import tempfile

import numpy as np
import pytest
import torch

import oracle_py as O
from golden_util import e2e, model_path, prompt_ids
from vsim_amd import hip
from vsim_amd import modelgen as mg
from vsim_amd.batch import generate_many, sample_n

pytestmark = pytest.mark.gpu

ARCH = {"gptneox": hip.ARCH_GPTNEOX, "gptj": hip.ARCH_GPTJ, "bloom": hip.ARCH_BLOOM}
DEV = "cuda:0"
EINVAL = -1
GOLDEN_PARAMS = dict(seed=42, top_k=20, top_p=0.95, temp=0.85, repeat_last_n=64, repeat_penalty=1.3)  # interface.py's
CLI_DEFAULTS = dict(seed=42, top_k=40, top_p=0.95, temp=0.8, repeat_last_n=64, repeat_penalty=1.3)
PARAMS = [GOLDEN_PARAMS, CLI_DEFAULTS,
          dict(seed=7, top_k=64, top_p=1.0, temp=1.2, repeat_last_n=8, repeat_penalty=1.1),
          dict(seed=1234, top_k=1, top_p=0.5, temp=0.5, repeat_last_n=1, repeat_penalty=1.0),  # (the reference's loop needs a window)
          dict(seed=99, top_k=5, top_p=0.9, temp=1.0, repeat_last_n=256, repeat_penalty=1.6)]
N_PREDICT = 24


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def model_file(cfg):
    arch_s, hp = mg.CONFIGS[cfg]
    path = os.path.join(tempfile.mkdtemp(), f"{cfg}.bin")
    mg.write_model(path, arch_s, hp, seed=5, std=0.08)
    return path, arch_s


@functools.lru_cache(maxsize=None)
def prompts(cfg):
    g = np.random.default_rng(17)
    V = mg.CONFIGS[cfg][1].n_vocab
    return tuple(tuple(int(t) for t in g.integers(3, V, n)) for n in (4, 1, 12, 10, 7))  # (no eos id 2 inside)


@functools.lru_cache(maxsize=None)
def oracle_stream(cfg, prompt, params):
    """The reference's own loop for one sequence alone: the generated tokens after the prompt."""
    path, arch_s = model_file(cfg)
    out = O.Model(path, ARCH[arch_s]).generate(list(prompt), N_PREDICT, **dict(params))
    assert out[:len(prompt)] == list(prompt)
    return out[len(prompt):]


def frozen(p):
    return tuple(sorted(p.items()))


# ------------------------------------------------------------------ against the oracle
@pytest.mark.parametrize("cfg", ["small-neox", "small-gptj", "small-bloom"])
def test_generate_many_sampled_matches_the_oracle_loop(cfg):
    path, arch_s = model_file(cfg)
    dm = hip.Model.load(path, ARCH[arch_s])
    sm = [hip.Sampler(**p) for p in PARAMS]
    got = generate_many(dm, prompts(cfg), N_PREDICT, eos=2, n_slots=3, samplers=sm)  # slots reused, batches change
    for pr, p, g, s in zip(prompts(cfg), PARAMS, got, sm):
        assert g == oracle_stream(cfg, pr, frozen(p)), (pr, p)
        assert s.stats() == {"device": len(g) - 1, "host": 1}  # the first token: sample_host on the prompt's row
    dm.close()


def test_golden_sampled_streams_in_one_batch():
    ent = e2e()["models"]["small-neox"]
    dm = hip.Model.load(model_path("small-neox"), hip.ARCH_GPTNEOX)
    ps = sorted(ent["sampled"])
    got = generate_many(dm, [prompt_ids(p) for p in ps], N_PREDICT, eos=2, samplers=[hip.Sampler(**GOLDEN_PARAMS) for _ in ps])
    for p, g in zip(ps, got):
        assert prompt_ids(p) + g == ent["sampled"][p], p
    dm.close()


def test_a_host_path_sampler_among_device_path_ones():
    cfg = "small-gptj"
    path, arch_s = model_file(cfg)
    dm = hip.Model.load(path, ARCH[arch_s])
    params = [GOLDEN_PARAMS, dict(GOLDEN_PARAMS, top_k=100, seed=5), PARAMS[2], dict(CLI_DEFAULTS, seed=8)]
    sm = [hip.Sampler(**p) for p in params]
    got = generate_many(dm, prompts(cfg)[:4], N_PREDICT, eos=2, samplers=sm)
    for i, (pr, p, g, s) in enumerate(zip(prompts(cfg), params, got, sm)):
        assert g == oracle_stream(cfg, pr, frozen(p)), i
        assert s.stats() == ({"device": 0, "host": len(g)} if i == 1 else {"device": len(g) - 1, "host": 1})
    dm.close()


def test_sample_n_forks_one_prompt_evaluation():
    cfg = "small-neox"
    path, arch_s = model_file(cfg)
    dm = hip.Model.load(path, ARCH[arch_s])
    calls = {"eval_seq": 0, "seq_copy": 0}

    class Counting:
        """The model, counting the prompt evaluations and forks that pass through."""

        def __getattr__(self, name):
            f = getattr(dm, name)
            if name not in calls:
                return f

            def counted(*a, **k):
                calls[name] += 1
                return f(*a, **k)
            return counted

    pr = prompts(cfg)[2]
    got = sample_n(Counting(), pr, [hip.Sampler(**p) for p in PARAMS[:4]], N_PREDICT, eos=2)
    assert calls == {"eval_seq": 1, "seq_copy": 3}
    for p, g in zip(PARAMS, got):
        assert g == oracle_stream(cfg, pr, frozen(p)), p
    dm.close()


# ------------------------------------------------------------------ fast mode: twin slots
@pytest.fixture
def fast_gemm_setting():
    old = hip.batch_set_fast_gemm(1)
    yield
    hip.batch_set_fast_gemm(old)


def twin_token(dm, model_mode, slot, n_past, tok, s):
    """eval_seq (N = 1) in MODE_FAST + vsim_op_topk on that row + Sampler.pick: what the fast sampled
    step promises for the row."""
    dm.set_mode(hip.MODE_FAST)
    lg = dm.eval_seq(slot, n_past, [tok])
    dm.set_mode(model_mode)
    p = s.params
    xd = torch.tensor(lg, device=DEV)
    wd = torch.tensor(np.asarray(s.win, np.int32), device=DEV) if s.win else None
    val = torch.zeros(p["top_k"], dtype=torch.float64, device=DEV)
    ids = torch.zeros(p["top_k"], dtype=torch.int32, device=DEV)
    hip.topk(xd, lg.size, wd, 1.0 / float(np.float32(p["temp"])), float(np.float32(p["repeat_penalty"])), p["top_k"], val, ids)
    torch.cuda.synchronize()
    return s.draw(val.cpu().numpy(), ids.cpu().numpy())


class Tracked:
    """A Sampler and a host copy of its window, for the twin's vsim_op_topk call."""

    def __init__(self, **p):
        self.params, self.s = p, hip.Sampler(**p)
        self.win = [0] * p["repeat_last_n"]

    def _push(self, t):
        if self.win:
            self.win = self.win[1:] + [int(t)]

    def accept(self, t):
        self.s.accept(t)
        self._push(t)

    def draw(self, val, ids):
        t = self.s.pick(val, ids)
        self._push(t)
        return t


@pytest.mark.parametrize("model_mode", [hip.MODE_FAST, hip.MODE_EXACT], ids=["model-fast", "model-exact"])
@pytest.mark.parametrize("gemm", [2, 0, 1], ids=["rows-kernel", "gemv-per-row", "default"])
def test_fast_sampled_step_equals_eval_seq_topk_pick(gemm, model_mode, fast_gemm_setting):
    path, arch_s = model_file("small-gptj")
    dm = hip.Model.load(path, ARCH[arch_s])
    hip.batch_set_fast_gemm(gemm)
    dm.set_mode(model_mode)
    dm.seq_reserve(8)
    n = 4
    plist = PARAMS[:3] + [PARAMS[4]]
    a = [hip.Sampler(**p) for p in plist]       # the batch's samplers, slots 0, 2, 4, 6
    b = [Tracked(**p) for p in plist]           # the twins', slots 1, 3, 5, 7
    n_past, tok = [], []
    for i, pr in enumerate(prompts("small-gptj")[:n]):
        la, lb = dm.eval_seq(2 * i, 0, pr), dm.eval_seq(2 * i + 1, 0, pr)
        assert np.array_equal(bits(la), bits(lb))
        for t in pr:
            a[i].accept(t)
            b[i].accept(t)
        n_past.append(len(pr))
        tok.append(int(pr[-1]) % 7 + 3)
    for step in range(6):
        rows = list(range(n)) if step % 2 == 0 else [3, 0, 2]
        nxt = dm.decode_batch_sample([2 * i for i in rows], [n_past[i] for i in rows], [tok[i] for i in rows],
                                     [a[i] for i in rows], fast=True)
        for r, i in enumerate(rows):
            want = twin_token(dm, model_mode, 2 * i + 1, n_past[i], tok[i], b[i])
            assert int(nxt[r]) == want, (step, i)
            assert a[i].stats() == b[i].s.stats(), (step, i)
            n_past[i] += 1
            tok[i] = want
    assert all(s.stats()["host"] == 0 for s in a)
    dm.close()


# ------------------------------------------------------------------ full vocabulary, B = 32
@pytest.mark.parametrize("cfg", ["gpt-j-6B", "bloom-560m"])
def test_full_vocabulary_rows_equal_eval_sample_on_a_twin_model(cfg):
    """Two layers at the real widths (n_vocab 50,400 / 250,880), 32 rows with their own samplers
    (k, window length up to the device limit, temperature and penalty per row).  The twin model has the
    same weights; each row's history is replayed into it and its eval_sample draws the row's token."""
    arch_s, hp = mg.CONFIGS[cfg]
    hpd = dict(n_vocab=hp.n_vocab, n_embd=hp.n_embd, n_head=hp.n_head, n_layer=2, n_rot=hp.n_rot,
               use_parallel_residual=hp.use_parallel_residual)
    dm, tw = (hip.Model.create(ARCH[arch_s], hpd, n_ctx=16) for _ in range(2))
    for m in (dm, tw):
        m.randomize(seed=7, std=0.02)
    B = 32
    dm.seq_reserve(B)
    plist = [dict(seed=100 + b, top_k=(1, 20, 40, 64)[b % 4], top_p=0.95, temp=0.6 + 0.03 * b,
                  repeat_last_n=(0, 1, 64, 1024)[(b // 4) % 4], repeat_penalty=1.0 + 0.02 * b) for b in range(B)]
    a, t = [hip.Sampler(**p) for p in plist], [hip.Sampler(**p) for p in plist]
    g = np.random.default_rng(3)
    hist = [[int(g.integers(0, hp.n_vocab))] for _ in range(B)]
    for step in range(3):
        nxt = dm.decode_batch_sample(list(range(B)), [step] * B, [h[-1] for h in hist], a)
        for b in range(B):
            if step:
                tw.eval(0, hist[b][:-1], want_logits=False)
            want = tw.eval_sample(t[b], step, hist[b][-1])
            assert int(nxt[b]) == want, (step, b)
            assert a[b].stats() == t[b].stats() == {"device": step + 1, "host": 0}
            hist[b].append(want)
    assert len({h[-1] for h in hist}) > 1
    dm.close()
    tw.close()


# ------------------------------------------------------------------ seq_copy
def test_seq_copy_forks_a_slot():
    path, arch_s = model_file("small-gptj")
    dm = hip.Model.load(path, ARCH[arch_s], n_ctx=64)
    dm.seq_reserve(6)
    dm.debug_poison(16)  # every slot NaN: nothing but the copied rows may be read
    P = list(prompts("small-gptj")[2][:7])
    dm.eval_seq(2, 0, P)
    dm.seq_copy(0, 2, 7)   # into slot 0
    dm.seq_copy(3, 0, 7)   # from slot 0
    dm.seq_copy(1, 2, 7)
    lg, _ = dm.decode_batch([0, 1, 2, 3], [7] * 4, [9] * 4)
    assert np.isfinite(lg).all()
    for r in range(1, 4):
        assert np.array_equal(bits(lg[r]), bits(lg[0])), r
    toks = [11, 12, 13, 14]
    lg, _ = dm.decode_batch([0, 1, 2, 3], [8] * 4, toks)  # the forks diverge
    for r, t in enumerate(toks):
        alone = dm.eval_seq(4, 0, P + [9, t])
        assert np.array_equal(bits(lg[r]), bits(alone)), r
    assert len({bits(lg[r]).tobytes() for r in range(4)}) == 4
    # a shorter fork: the first 5 rows only, continued from position 5
    dm.seq_copy(5, 1, 5)
    lg, _ = dm.decode_batch([5], [5], [21])
    assert np.array_equal(bits(lg[0]), bits(dm.eval_seq(4, 0, P[:5] + [21])))
    # slot 0 still serves the single-sequence calls
    assert np.array_equal(bits(dm.eval(9, [30])), bits(dm.eval_seq(4, 0, P + [9, 11, 30])))
    dm.close()


def test_seq_copy_argument_errors():
    path, arch_s = model_file("small-gptj")
    L = hip.lib()
    dm = hip.Model.load(path, ARCH[arch_s], n_ctx=64)
    assert L.vsim_model_seq_copy(dm.h, 1, 0, 4) == EINVAL  # one slot until seq_reserve
    dm.seq_reserve(3)
    for dst, src, n in ((1, 1, 4), (0, 0, 4), (3, 0, 4), (0, 3, 4), (-1, 0, 4), (0, -1, 4), (1, 0, 0), (1, 0, -2), (1, 0, 65)):
        assert L.vsim_model_seq_copy(dm.h, dst, src, n) == EINVAL, (dst, src, n)
    assert b"seq_copy" in L.vsim_last_error()
    assert L.vsim_model_seq_copy(dm.h, 1, 0, 64) == 0 and L.vsim_model_seq_copy(dm.h, 0, 2, 1) == 0
    assert L.vsim_model_seq_copy(None, 1, 0, 4) == EINVAL
    dm.sync()
    dm.close()
    st = hip.Model.load(path, ARCH[arch_s], n_ctx=64, layer_begin=0, layer_end=1)
    assert L.vsim_model_seq_copy(st.h, 1, 0, 4) == EINVAL
    st.close()


# ------------------------------------------------------------------ argument errors
def test_decode_batch_sample_argument_errors():
    path, arch_s = model_file("small-gptj")
    L = hip.lib()
    dm = hip.Model.load(path, ARCH[arch_s], n_ctx=64)
    dm.seq_reserve(3)
    s = [hip.Sampler(**p) for p in PARAMS[:3]]
    zero_k = hip.Sampler(**dict(GOLDEN_PARAMS, top_k=0))

    def call(mode, seqs, n_past, toks, samplers, m=dm, nxt_null=False):
        a, b, c = (np.ascontiguousarray(v, np.int32) for v in (seqs, n_past, toks))
        hs = (ctypes.c_void_p * max(len(seqs), 1))(*[None if x is None else x.h for x in samplers])
        nxt = np.zeros(64, np.int32)
        return L.vsim_model_decode_batch_sample(m.h, mode, len(seqs), a.ctypes.data, b.ctypes.data, c.ctypes.data,
                                                hs, None if nxt_null else nxt.ctypes.data)

    E, F = hip.MODE_EXACT, hip.MODE_FAST
    for mode in (E, F):
        assert call(mode, [0, 1, 2], [0, 0, 0], [1, 2, 3], s) == 0
        assert call(mode, [0, 1, 2], [1, 1, 1], [1, 2, 3], [s[0], None, s[2]]) == EINVAL      # a null sampler
        assert b"null sampler" in L.vsim_last_error()
        assert call(mode, [0, 1, 2], [1, 1, 1], [1, 2, 3], [s[0], s[1], s[0]]) == EINVAL      # a sampler twice
        assert b"named twice" in L.vsim_last_error()
        assert call(mode, [0, 1], [1, 1], [1, 2], [s[0], zero_k]) == EINVAL                   # top_k < 1
        assert call(mode, [0, 1, 1], [1, 1, 1], [1, 2, 3], s) == EINVAL                       # decode_batch's own
        assert call(mode, [0, 3], [1, 1], [1, 2], s[:2]) == EINVAL
        assert call(mode, [0, 1], [1, 64], [1, 2], s[:2]) == EINVAL
        assert call(mode, [0, 1], [1, 1], [1, 512], s[:2]) == EINVAL
        assert call(mode, [], [], [], []) == EINVAL
        assert call(mode, [0], [1], [1], s[:1], nxt_null=True) == EINVAL
    for mode in (2, -1, 7):
        assert call(mode, [0], [1], [1], s[:1]) == EINVAL                                     # no such mode
    assert b"mode" in L.vsim_last_error()
    assert L.vsim_model_decode_batch_sample(dm.h, E, 1, None, None, None, None, None) == EINVAL
    # only the two good calls drew: a refused call touches no sampler
    assert [x.stats() for x in s] == [{"device": 2, "host": 0}] * 3
    assert zero_k.stats() == {"device": 0, "host": 0}
    # the exact step refuses a fast-mode model; the fast step serves both
    dm.set_mode(F)
    assert call(E, [0], [1], [1], s[:1]) == EINVAL
    assert b"exact mode" in L.vsim_last_error()
    assert call(F, [0], [1], [1], s[:1]) == 0
    dm.close()
    st = hip.Model.load(path, ARCH[arch_s], n_ctx=64, layer_begin=0, layer_end=1)
    assert call(F, [0], [0], [1], s[:1], m=st) == EINVAL
    st.close()
