"""Weight-only mode (VSIM_MODE_W4A16) through the model executor.  Every kernel of the mode is per
row, so the model contract is bitwise self-consistency: a row's logits do not depend on whether it
came through a prompt, a single-token eval, a scoring window or a batch.  Two-layer synthetic
models of the three architectures at the executor's smallest width (n_embd must be a multiple of
128: E = 128, 4 heads of d = 32, vocabulary 128), n_ctx = 96.

Two numeric checks on the GPT-NeoX quality case of tests/w4a16_ref.py: the device against the h(x)
restatement within REST_TOL (4 x what a legitimate change of summation order moves, measured on the
CPU), and the mode at least QUALITY_FLOOR = 8 times nearer to the ideal forward than exact mode is.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import w4a16_ref as W  # noqa: E402
import oracle_py as O  # noqa: E402
from vsim_amd import hip  # noqa: E402
from vsim_amd import modelgen as mg  # noqa: E402
from vsim_amd.batch import generate_many  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
ARCH = {"gptj": hip.ARCH_GPTJ, "gptneox": hip.ARCH_GPTNEOX, "bloom": hip.ARCH_BLOOM}
CFGS = ["tiny-neox", "tiny-gptj", "tiny-bloom"]
EINVAL = -1
N_CTX = 96


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b, what):
    if not np.array_equal(bits(a), bits(b)):
        bad = np.argwhere(bits(a) != bits(b))
        pytest.fail(f"{what}: {len(bad)} values differ, first {bad[:4].tolist()}: "
                    f"{np.asarray(a)[tuple(bad[0])]!r} against {np.asarray(b)[tuple(bad[0])]!r}")


def load(cfg, tmp_path, seed=11, mode=hip.MODE_W4A16):
    arch_s, hp = mg.CONFIGS[cfg]
    path = str(tmp_path / f"{cfg}.bin")
    mg.write_model(path, arch_s, hp, seed=seed, std=0.05)
    dm = hip.Model.load(path, ARCH[arch_s], n_ctx=N_CTX)
    dm.set_mode(mode)
    return dm, hp, path, arch_s


def tokens_of(hp, n, seed):
    return [int(t) for t in np.random.default_rng(seed).integers(0, hp.n_vocab, n)]


@pytest.fixture
def score_chunks():
    old = hip.score_set_chunk_rows(0)
    yield
    hip.score_set_chunk_rows(old)


@pytest.mark.parametrize("cfg", CFGS)
def test_prompts_and_scoring_equal_single_token_evals(cfg, tmp_path, score_chunks):
    """Prompts of 1, 31, 32, 33 and 65 tokens (both sides of the 32-row chunk seam), and every row of
    a scoring window, against single-token evals -- with the scratch and the caches poisoned first."""
    dm, hp, _, _ = load(cfg, tmp_path)
    dm.debug_poison(66)
    toks = tokens_of(hp, 67, 3)
    single = np.stack([dm.eval(i, [toks[i]]) for i in range(67)])   # row i: the eval that ends at position i
    assert np.isfinite(single).all()
    for n in (1, 31, 32, 33, 65):
        dm.debug_poison(66)
        same(dm.eval(0, toks[:n]), single[n - 1], f"{cfg}: prompt of {n}")
        # the cache rows are those of n single-token evals: the next position sees nothing else
        same(dm.eval(n, [toks[n]]), single[n], f"{cfg}: position {n} after a prompt of {n}")
    # a prompt continued by a prompt across the seam
    dm.debug_poison(66)
    dm.eval(0, toks[:20], want_logits=False)
    same(dm.eval(20, toks[20:66]), single[65], f"{cfg}: 20 + 46")
    for chunk in (0, 7):  # the head's default chunk (65 rows: three launches) and ragged 7-row chunks
        hip.score_set_chunk_rows(chunk)
        dm.debug_poison(66)
        lp, am, lg = dm.score(0, toks[:65], want_logits=True)
        same(lg, single[:65], f"{cfg}: eval_score rows, chunk {chunk}")
        assert np.array_equal(am, single[:65].argmax(axis=1))
        x = single[:65].astype(np.float64)
        ref = x[np.arange(64), toks[1:65]] - (x[:64].max(axis=1) + np.log(np.exp(x[:64] - x[:64].max(axis=1, keepdims=True)).sum(axis=1)))
        assert np.allclose(lp[:64], ref, rtol=0, atol=1e-9) and lp[64] == 0.0
    # the single-token calls: uncaptured general-path steps on slot 0
    n0 = 9
    dm.eval(0, toks[:n0], want_logits=False)
    assert dm.eval_argmax(n0, toks[n0]) == int(single[n0].argmax())
    dm.eval(0, toks[:n0], want_logits=False)
    gen = dm.generate(n0, toks[n0], 5)
    want, t = [], toks[n0]
    dm.eval(0, toks[:n0], want_logits=False)
    for i in range(5):
        t = int(dm.eval(n0 + i, [t]).argmax())
        want.append(t)
    assert list(gen) == want
    dm.close()


class Twins:
    """Slot 2 i advances by decode_batch_w4a16, its twin 2 i + 1 by eval_seq with the model in
    MODE_W4A16; the tokens are teacher-forced from a fixed RNG."""

    def __init__(self, dm, model_mode, seed):
        self.dm, self.mode, self.rng = dm, model_mode, np.random.default_rng(seed)
        dm.set_mode(model_mode)
        self.n_past = {}

    def token(self):
        return int(self.rng.integers(0, self.dm.n_vocab))

    def twin_row(self, slot, n_past, toks):
        self.dm.set_mode(hip.MODE_W4A16)
        lg = self.dm.eval_seq(slot, n_past, toks)
        self.dm.set_mode(self.mode)
        return lg

    def prefill(self, i, n):
        prompt = [self.token() for _ in range(n)]
        same(self.twin_row(2 * i, 0, prompt), self.twin_row(2 * i + 1, 0, prompt), "the pair's prompts")
        self.n_past[i] = n

    def step(self, rows, what, want_logits=True):
        toks = [self.token() for _ in rows]
        lg, nxt = self.dm.decode_batch_w4a16([2 * i for i in rows], [self.n_past[i] for i in rows], toks,
                                             want_logits=want_logits)
        for r, (i, t) in enumerate(zip(rows, toks)):
            want = self.twin_row(2 * i + 1, self.n_past[i], [t])
            if want_logits:
                same(lg[r], want, f"{what}: pair {i} at n_past {self.n_past[i]}")
            assert int(nxt[r]) == int(np.argmax(want)), (what, i)
            self.n_past[i] += 1

    def step_by_eval_seq(self, i, what):
        t = self.token()
        same(self.twin_row(2 * i, self.n_past[i], [t]), self.twin_row(2 * i + 1, self.n_past[i], [t]), what)
        self.n_past[i] += 1


@pytest.mark.parametrize("model_mode", [hip.MODE_W4A16, hip.MODE_EXACT], ids=["model-w4a16", "model-exact"])
@pytest.mark.parametrize("cfg", CFGS)
def test_batched_steps_equal_eval_seq(cfg, model_mode, tmp_path):
    dm, hp, _, _ = load(cfg, tmp_path)
    dm.seq_reserve(8)
    dm.debug_poison(40)
    T = Twins(dm, model_mode, seed=5)
    for i, n in enumerate((1, 3, 33, 9)):
        T.prefill(i, n)
    for k in range(3):  # all four, the row order changing every step
        T.step([(i + k) % 4 for i in range(4)] if k % 2 == 0 else [3, 2, 1, 0], f"{cfg} step {k}")
    for k in range(3, 5):
        T.step([3, 0, 1], f"{cfg} step {k} (without pair 2)")
    T.step([3], "B = 1")
    T.prefill(2, 4)  # a retired pair restarts
    T.step([2, 0, 3], "restarted pair 2")
    T.step([1, 3], "ids only", want_logits=False)
    T.step([1, 3], "after an ids-only step")
    for k in range(4):  # mixed feeding: the batch's slot alternately by the two calls
        if k % 2 == 0:
            T.step_by_eval_seq(0, f"mixed {k}")
        else:
            T.step([0, 2], f"mixed {k}")
    dm.close()


def test_a_full_batch_and_generate_many(tmp_path):
    dm, hp, _, _ = load("tiny-gptj", tmp_path, seed=4)
    dm.seq_reserve(64)
    T = Twins(dm, hip.MODE_W4A16, seed=8)
    for i in range(32):
        T.prefill(i, 1 + i % 5)
    T.step(list(reversed(range(32))), "B = 32")
    T.step(list(range(17)), "B = 17")
    dm.close()
    dm, hp, _, _ = load("tiny-gptj", tmp_path, seed=4)
    prompts = [tokens_of(hp, n, 20 + n) for n in (4, 1, 9, 2, 6, 3, 12)]
    got = generate_many(dm, prompts, 8, n_slots=3, w4a16=True)
    for p, g in zip(prompts, got):
        want, n_past = [int(np.argmax(dm.eval_seq(0, 0, p)))], len(p)
        while len(want) < 8:
            want.append(int(np.argmax(dm.eval_seq(0, n_past, [want[-1]]))))
            n_past += 1
        assert g == want, p
    with pytest.raises(ValueError):
        generate_many(dm, prompts, 2, fast=True, w4a16=True)
    dm.close()


PARAMS = [dict(seed=1, top_k=40, top_p=0.95, temp=0.8, repeat_last_n=64, repeat_penalty=1.3),
          dict(seed=2, top_k=5, top_p=0.5, temp=1.1, repeat_last_n=16, repeat_penalty=1.1),
          dict(seed=3, top_k=64, top_p=1.0, temp=0.7, repeat_last_n=0, repeat_penalty=1.0)]


class Tracked:
    """A Sampler and a host copy of its window, for the twin's vsim_op_topk call."""

    def __init__(self, **p):
        self.params, self.s = p, hip.Sampler(**p)
        self.win = [0] * p["repeat_last_n"]

    def accept(self, t):
        self.s.accept(t)
        self.win = (self.win[1:] + [int(t)]) if self.win else self.win

    def draw(self, val, ids):
        t = self.s.pick(val, ids)
        self.win = (self.win[1:] + [int(t)]) if self.win else self.win
        return t


@pytest.mark.parametrize("model_mode", [hip.MODE_W4A16, hip.MODE_EXACT], ids=["model-w4a16", "model-exact"])
def test_sampled_step_equals_eval_seq_topk_pick(model_mode, tmp_path):
    dm, hp, _, _ = load("tiny-neox", tmp_path, mode=model_mode)
    dm.seq_reserve(6)
    a = [hip.Sampler(**p) for p in PARAMS]   # the batch's samplers, slots 0, 2, 4
    b = [Tracked(**p) for p in PARAMS]       # the twins', slots 1, 3, 5
    n_past, tok = [], []
    for i, n in enumerate((5, 1, 34)):
        pr = tokens_of(hp, n, 40 + i)
        dm.set_mode(hip.MODE_W4A16)
        same(dm.eval_seq(2 * i, 0, pr), dm.eval_seq(2 * i + 1, 0, pr), "prompts")
        dm.set_mode(model_mode)
        for t in pr:
            a[i].accept(t)
            b[i].accept(t)
        n_past.append(n)
        tok.append(pr[-1] % 7 + 3)
    for step in range(5):
        rows = [0, 1, 2] if step % 2 == 0 else [2, 0]
        nxt = dm.decode_batch_sample([2 * i for i in rows], [n_past[i] for i in rows], [tok[i] for i in rows],
                                     [a[i] for i in rows], mode=hip.MODE_W4A16)
        for r, i in enumerate(rows):
            dm.set_mode(hip.MODE_W4A16)
            lg = dm.eval_seq(2 * i + 1, n_past[i], [tok[i]])
            dm.set_mode(model_mode)
            p = b[i].params
            xd = torch.tensor(lg, device=DEV)
            wd = torch.tensor(np.asarray(b[i].win, np.int32), device=DEV) if b[i].win else None
            val = torch.zeros(p["top_k"], dtype=torch.float64, device=DEV)
            ids = torch.zeros(p["top_k"], dtype=torch.int32, device=DEV)
            hip.topk(xd, lg.size, wd, 1.0 / float(np.float32(p["temp"])), float(np.float32(p["repeat_penalty"])),
                     p["top_k"], val, ids)
            torch.cuda.synchronize()
            want = b[i].draw(val.cpu().numpy(), ids.cpu().numpy())
            assert int(nxt[r]) == want, (step, i)
            assert a[i].stats() == b[i].s.stats(), (step, i)
            n_past[i] += 1
            tok[i] = want
    assert all(s.stats()["host"] == 0 for s in a)
    if model_mode == hip.MODE_W4A16:  # eval_sample / generate_sampled: the same step on slot 0
        s1, s2 = hip.Sampler(**PARAMS[0]), Tracked(**PARAMS[0])
        pr = tokens_of(hp, 6, 77)
        dm.eval(0, pr, want_logits=False)
        got = dm.generate_sampled(s1, 6, 5, 4)
        dm.eval_seq(1, 0, pr, want_logits=False)
        t, want = 5, []
        for i in range(4):
            lg = dm.eval_seq(1, 6 + i, [t])
            p = PARAMS[0]
            val = torch.zeros(p["top_k"], dtype=torch.float64, device=DEV)
            ids = torch.zeros(p["top_k"], dtype=torch.int32, device=DEV)
            hip.topk(torch.tensor(lg, device=DEV), lg.size, torch.tensor(np.asarray(s2.win, np.int32), device=DEV),
                     1.0 / float(np.float32(p["temp"])), float(np.float32(p["repeat_penalty"])), p["top_k"], val, ids)
            torch.cuda.synchronize()
            t = s2.draw(val.cpu().numpy(), ids.cpu().numpy())
            want.append(t)
        assert list(got) == want
    dm.close()


@pytest.mark.parametrize("cfg", CFGS)
def test_mode_round_trip_keeps_both_modes_bits(cfg, tmp_path):
    """exact -> w4a16 -> exact: exact-mode logits are the oracle's before and after, the mode's own
    bits the same before and after."""
    dm, hp, path, arch_s = load(cfg, tmp_path, mode=hip.MODE_EXACT)
    om = O.Model.from_device(dm, arch_s, n_ctx=N_CTX)
    toks = tokens_of(hp, 12, 6)
    want = [om.eval(0, toks[:9]), om.eval(9, [toks[9]])]

    def exact_pass(what):
        dm.set_mode(hip.MODE_EXACT)
        same(dm.eval(0, toks[:9]), want[0], f"{cfg}: exact prompt {what}")
        same(dm.eval(9, [toks[9]]), want[1], f"{cfg}: exact step {what}")

    def w4_pass():
        dm.set_mode(hip.MODE_W4A16)
        return np.stack([dm.eval(0, toks[:9]), dm.eval(9, [toks[9]])])

    exact_pass("before")
    first = w4_pass()
    assert not np.array_equal(bits(first[0]), bits(want[0]))   # (another arithmetic)
    exact_pass("after")
    same(w4_pass(), first, f"{cfg}: w4a16 after an exact pass")
    dm.set_mode(hip.MODE_FAST)
    dm.eval(0, toks[:9])
    same(w4_pass(), first, f"{cfg}: w4a16 after a fast pass")
    dm.close()


def test_stage_calls_and_argument_errors(tmp_path):
    dm, hp, path, _ = load("tiny-gptj", tmp_path)
    L = hip.lib()
    tok = torch.zeros(2, dtype=torch.int32, device=DEV)
    for fn, args in ((L.vsim_model_stage_bind, (dm.h, tok.data_ptr(), None, None, tok[1:].data_ptr())),
                     (L.vsim_model_stage_begin, (dm.h, 0)), (L.vsim_model_stage_step, (dm.h,))):
        assert fn(*args) == EINVAL
        assert b"W4A16" in L.vsim_last_error()
    dm.set_mode(hip.MODE_EXACT)   # ... and they work again in another mode
    dm.stage_bind(tok_in=tok.data_ptr(), tok_out=tok[1:].data_ptr())
    dm.stage_begin(0)
    dm.stage_step()
    dm.sync()
    assert L.vsim_model_set_mode(dm.h, 3) == EINVAL and L.vsim_model_set_mode(dm.h, -1) == EINVAL
    dm.seq_reserve(3)

    def call(seqs, n_past, toks, m=dm):
        a, b, c = (np.ascontiguousarray(v, np.int32) for v in (seqs, n_past, toks))
        nxt = np.zeros(64, np.int32)
        return L.vsim_model_decode_batch_w4a16(m.h, len(seqs), a.ctypes.data, b.ctypes.data, c.ctypes.data, None,
                                               nxt.ctypes.data)

    for mode in (hip.MODE_EXACT, hip.MODE_FAST, hip.MODE_W4A16):  # the call names its path
        dm.set_mode(mode)
        assert call([0, 1, 2], [0, 0, 0], [1, 2, 3]) == 0
        assert call([0, 1, 1], [1, 1, 1], [1, 2, 3]) == EINVAL
        assert call([0, 3], [1, 1], [1, 2]) == EINVAL
        assert call([0, 1], [1, N_CTX], [1, 2]) == EINVAL
        assert call([0, 1], [1, 1], [1, hp.n_vocab]) == EINVAL
        assert call([], [], []) == EINVAL
    assert L.vsim_model_decode_batch_w4a16(None, 1, None, None, None, None, None) == EINVAL
    # decode_batch (the exact step) refuses a model in this mode too
    a = np.zeros(1, np.int32)
    assert L.vsim_model_decode_batch(dm.h, 1, a.ctypes.data, a.ctypes.data, a.ctypes.data, None, a.ctypes.data) == EINVAL
    dm.close()
    st = hip.Model.load(path, hip.ARCH_GPTJ, n_ctx=N_CTX, layer_begin=0, layer_end=1)   # a pipeline stage
    assert L.vsim_model_set_mode(st.h, hip.MODE_W4A16) == EINVAL
    assert call([0], [0], [1], st) == EINVAL
    st.close()


def test_cli_mode_w4a16(tmp_path):
    """vsim-hip --mode w4a16: --score prints Model.score's numbers of the mode, and generation with
    top_k 1 the greedy tokens of the mode."""
    import os
    import subprocess
    cli = os.path.join(os.path.dirname(os.path.abspath(hip.__file__)), "_build", "vsim-hip")
    dm, hp, path, _ = load("tiny-neox", tmp_path)
    ids = tokens_of(hp, 20, 13)
    lp, am = dm.score(0, ids)
    first = int(dm.eval(0, ids).argmax())
    want = [first] + [int(t) for t in dm.generate(len(ids), first, 5)]
    dm.set_mode(hip.MODE_EXACT)
    assert not np.array_equal(dm.score(0, ids)[0], lp)   # (the flag matters)
    dm.close()
    r = subprocess.run([cli, "gptneox", "-m", path, "--prompt", " ".join(map(str, ids)), "--score", "--mode", "w4a16",
                        "--n_ctx", str(N_CTX)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rows = [ln.split() for ln in r.stdout.strip().splitlines()[-20:-1]]
    assert [float(x[2]) for x in rows] == [float(v) for v in lp[:19]]  # %.17g round-trips
    assert [int(x[3]) for x in rows] == [int(v) for v in am[:19]]
    r = subprocess.run([cli, "gptneox", "-m", path, "--prompt", " ".join(map(str, ids)), "--mode", "w4a16", "--top_k", "1", "--repeat_penalty", "1.0",
                        "-n", "6", "--n_ctx", str(N_CTX), "-b", "64"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    body = r.stdout.split("<|BEGIN>")[1].split("<END|>")[0].split()
    got = [int(t) for t in body][len(ids):]
    assert got == want[:len(got)] and (len(got) == 6 or got[-1] == 2), (got, want)


def test_restatement_and_quality(tmp_path):
    """Device logits of the quality case (all 24 rows of one scoring window):
    * against the h(x) restatement with fp64 products, RMS within REST_TOL = 4 x REST_ORDER_DIST
      (measured on the CPU, tests/test_w4a16_ref_cpu.py; seed 31: 1.2539e-04, so 5.0157e-04);
    * against the ideal forward (dequantized weights, unrounded activations) at least QUALITY_FLOOR
      = 8 times nearer than exact mode is (the oracle's distance recorded on the CPU: 0.26289)."""
    path, tokens, ideal, rest64 = W.quality_case(str(tmp_path))
    dm = hip.Model.load(path, hip.ARCH_GPTNEOX, n_ctx=N_CTX)
    dm.set_mode(hip.MODE_W4A16)
    _, _, lg = dm.score(0, tokens, want_logits=True)
    d_rest, d_ideal = W.rms(lg, rest64), W.rms(lg, ideal)
    dm.set_mode(hip.MODE_EXACT)
    _, _, lge = dm.score(0, tokens, want_logits=True)
    d_exact = W.rms(lge, ideal)
    dm.close()
    print(f"w4a16 quality case (model seed {W.QUALITY_SEED}): device to restatement {d_rest:.4e} (allowed {W.REST_TOL:.4e}, "
          f"max {np.abs(lg - rest64).max():.3e}); device to ideal {d_ideal:.4e}; exact mode to ideal: device {d_exact:.5f}, "
          f"oracle {W.EXACT_TO_IDEAL:.5f}; ratio {W.EXACT_TO_IDEAL / d_ideal:.1f} (floor {W.QUALITY_FLOOR})")
    assert d_exact == pytest.approx(W.EXACT_TO_IDEAL, rel=1e-6)   # exact mode on the device is the oracle's
    assert d_rest <= W.REST_TOL
    assert W.EXACT_TO_IDEAL / d_ideal >= W.QUALITY_FLOOR
