"""Scoring on the device: k_score_rows (vsim_op_logprob) against the float64 restatement in
score_ref.py, and Model.score (vsim_model_eval_score) against the CPU oracle's logits rows.

* op level: every row's logprob within score_ref's tolerance and the argmax equal, on random
  rows at sizes around the wave / workgroup strides and odd widths (misaligned rows), on crafted
  rows (ties, infinities, NaN, denormals), and bit-equal whatever else shares the launch;
* model, exact mode: every logits row of the scoring eval is the oracle's row for that prefix,
  bit for bit, whatever the head's chunking; the KV cache is left as an eval leaves it;
* model, fast mode: the scores are score_ref's of the call's own logits in every lm_head regime
  (fast mode's own error is the feature's output, printed, not asserted);
* the CLI's --score lines.
"""
import functools
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import oracle_py as O
import score_ref as R
from golden_util import model_path
from vsim_amd import hip, score
from vsim_amd import modelgen as mg

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CLI = os.path.join(ROOT, "vsim_amd", "_build", "vsim-hip")
ARCH = {"gptneox": hip.ARCH_GPTNEOX, "gptj": hip.ARCH_GPTJ, "bloom": hip.ARCH_BLOOM}
DEV = "cuda:0"
EINVAL = -1


# ------------------------------------------------------------------ vsim_op_logprob
def dev_score(x, targets, want_lp=True, want_am=True):
    """One vsim_op_logprob launch over x [R][V] (numpy float32) on the default stream: (logprob
    float64 [R], argmax int32 [R]) as numpy.  The block starts one float past an aligned address,
    so row 0 is 4-byte aligned only, and with an odd V so is every second row after it."""
    R_, V = x.shape
    buf = torch.zeros(R_ * V + 1, dtype=torch.float32, device=DEV)
    buf[1:] = torch.tensor(x.reshape(-1), device=DEV)
    tg = torch.tensor(np.asarray(targets, np.int32), device=DEV) if targets is not None else None
    lp = torch.full((R_,), 123.0, dtype=torch.float64, device=DEV) if want_lp else None
    am = torch.full((R_,), -7, dtype=torch.int32, device=DEV) if want_am else None
    hip.logprob(buf.data_ptr() + 4, V, R_, tg, lp, am)
    torch.cuda.synchronize()
    return (lp.cpu().numpy() if want_lp else None), (am.cpu().numpy() if want_am else None)


def targets_for(g, R_, V):
    """Targets that include 0, V - 1 and -1 among random ids."""
    t = g.integers(0, V, R_).astype(np.int32)
    for i, v in enumerate((V - 1, 0, -1)):
        if i < R_:
            t[(i * 5) % R_] = v
    if R_ == 1:
        t[0] = V - 1
    return t


@pytest.mark.parametrize("V", [1, 63, 64, 65, 1023, 1025, 4099])
@pytest.mark.parametrize("R_", [1, 3, 17])
def test_logprob_matches_the_restatement(V, R_):
    g = np.random.default_rng(1000 * V + R_)
    x = (g.standard_normal((R_, V)) * 2).astype(np.float32)  # N(0, 4)
    t = targets_for(g, R_, V)
    lp, am = dev_score(x, t)
    R.check_rows(x, t, lp, am, (V, R_))
    if R_ == 1:  # the remaining target values on the one row
        for tv in (0, -1):
            lp, am = dev_score(x, [tv])
            R.check_rows(x, [tv], lp, am, (V, tv))


def test_logprob_at_a_vocabulary_size():
    g = np.random.default_rng(50400)
    x = (g.standard_normal((9, 50400)) * 2).astype(np.float32)
    t = targets_for(g, 9, 50400)
    lp, am = dev_score(x, t)
    R.check_rows(x, t, lp, am, "50400")


def crafted_rows(V=1025):
    g = np.random.default_rng(9)
    base = (g.standard_normal(V) * 2).astype(np.float32)
    rows = {}
    rows["all equal"] = np.full(V, -2.5, np.float32)
    r = base.copy(); r[17] = -np.inf
    rows["one -inf"] = r
    r = base.copy(); r[g.permutation(V)[:V - 5]] = -np.inf
    rows["many -inf"] = r
    r = np.full(V, -1e30, np.float32); r[700] = 1e30
    rows["max 1e30"] = r
    rows["denormals"] = (g.integers(1, 1 << 22, V).astype(np.uint32)
                         | (g.integers(0, 2, V).astype(np.uint32) << 31)).view(np.float32)
    r = base.copy(); r[[900, 300, 600]] = np.float32(base.max() + 1)
    rows["duplicated maximum"] = r
    r = base.copy(); r[[800, 200]] = np.nan
    rows["NaN"] = r
    r = base.copy(); r[[640, 64]] = np.inf
    rows["+inf"] = r
    rows["all -inf"] = np.full(V, -np.inf, np.float32)
    r = np.zeros(V, np.float32); r[::2] = -0.0; r[0] = -1.0
    rows["signed zeros"] = r
    return rows


def test_logprob_crafted_rows():
    rows = crafted_rows()
    x = np.stack(list(rows.values()))
    for t in (0, 17, 1024, 300):
        tg = np.full(len(rows), t, np.int32)
        lp, am = dev_score(x, tg)
        for i, name in enumerate(rows):
            R.check_rows(x[i:i + 1], tg[i:i + 1], lp[i:i + 1], am[i:i + 1], (name, t))
    # what the rules say, spelled out once
    lp, am = dev_score(x, np.full(len(rows), 300, np.int32))
    names = list(rows)
    assert am[names.index("duplicated maximum")] == 300 and am[names.index("NaN")] == 200
    assert am[names.index("+inf")] == 64 and am[names.index("signed zeros")] == 1
    for n in ("NaN", "+inf", "all -inf"):
        assert math.isnan(lp[names.index(n)])
    assert lp[names.index("all equal")] == pytest.approx(-math.log(1025), abs=2.0 ** -40)


def test_logprob_rows_do_not_depend_on_the_launch():
    g = np.random.default_rng(11)
    for V in (65, 4099):
        x = (g.standard_normal((17, V)) * 2).astype(np.float32)
        t = g.integers(0, V, 17).astype(np.int32)
        lp, am = dev_score(x, t)
        lp2, am2 = dev_score(x, t)
        assert np.array_equal(lp.view(np.uint64), lp2.view(np.uint64)) and np.array_equal(am, am2)
        for i in (0, 5, 16):
            lp1, am1 = dev_score(x[i:i + 1], t[i:i + 1])
            assert lp1.view(np.uint64)[0] == lp.view(np.uint64)[i] and am1[0] == am[i], (V, i)


def test_logprob_arguments():
    x = np.random.default_rng(12).standard_normal((3, 65)).astype(np.float32)
    lp, _ = dev_score(x, [1, 2, 3], want_am=False)
    _, am = dev_score(x, [1, 2, 3], want_lp=False)
    R.check_rows(x, [1, 2, 3], lp, am, "one output each")
    lp, am = dev_score(x, None)  # no targets: all -1
    assert np.array_equal(lp, np.zeros(3)) and np.array_equal(am, R.score_rows(x, [-1] * 3)[1])
    lp, am = dev_score(x, [65, -2, 1 << 30])  # the caller's bug: treated as "no target", nothing read out of bounds
    assert np.array_equal(lp, np.zeros(3)) and np.array_equal(am, R.score_rows(x, [-1] * 3)[1])
    xd = torch.zeros(8, dtype=torch.float32, device=DEV)
    o = torch.zeros(8, dtype=torch.float64, device=DEV)
    L = hip.lib()
    assert L.vsim_op_logprob(xd.data_ptr(), 0, 1, None, o.data_ptr(), None, None) == EINVAL
    assert L.vsim_op_logprob(xd.data_ptr(), 8, -1, None, o.data_ptr(), None, None) == EINVAL
    assert L.vsim_op_logprob(xd.data_ptr(), 8, 1, None, None, None, None) == EINVAL
    assert L.vsim_op_logprob(xd.data_ptr(), 8, 0, None, o.data_ptr(), None, None) == 0


# ------------------------------------------------------------------ Model.score
@functools.lru_cache(maxsize=None)
def model_file(cfg):
    arch_s, hp = mg.CONFIGS[cfg]
    path = os.path.join(tempfile.mkdtemp(), f"{cfg}.bin")
    mg.write_model(path, arch_s, hp, seed=5, std=0.08)
    return path, arch_s


def text(cfg, n):
    V = mg.CONFIGS[cfg][1].n_vocab
    return [int(v) for v in np.random.default_rng(n).integers(0, V, n)]


@functools.lru_cache(maxsize=None)
def oracle_rows(cfg, n, rows=None):
    """The oracle's logits row for the prefix ending at each position of text(cfg, n) (all
    positions, or `rows`), each evaluated from n_past = 0 on one oracle model; read-only."""
    path, arch_s = model_file(cfg)
    om = O.Model(path, ARCH[arch_s])
    ids = text(cfg, n)
    out = {i: om.eval(0, ids[:i + 1]) for i in (rows if rows is not None else range(n))}
    for v in out.values():
        v.setflags(write=False)
    return out


def load(cfg, mode=hip.MODE_EXACT):
    path, arch_s = model_file(cfg)
    m = hip.Model.load(path, ARCH[arch_s])
    m.set_mode(mode)
    return m


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


@pytest.fixture
def default_chunk():
    yield
    hip.score_set_chunk_rows(0)


@pytest.mark.parametrize("cfg", ["tiny-gptj", "tiny-neox", "tiny-bloom"])
def test_exact_rows_are_the_oracles_whatever_the_chunking(cfg, default_chunk):
    N = 40
    ids = text(cfg, N)
    want = oracle_rows(cfg, N)
    tg = ids[1:] + [-1]
    m = load(cfg)
    got = {}
    for C in (8, 16):  # 5 chunks; 16 + 16 + 8
        assert hip.score_set_chunk_rows(C) in (0, 8)
        lp, am, lg = m.score(0, ids, want_logits=True)
        for i in range(N):
            assert np.array_equal(bits(lg[i]), bits(want[i])), (cfg, C, i)
        R.check_rows(lg, tg, lp, am, (cfg, C))
        assert lp[N - 1] == 0.0  # the default targets end in -1
        got[C] = (lp, am, lg)
    (lp8, am8, lg8), (lp16, am16, lg16) = got[8], got[16]
    assert np.array_equal(bits(lp8), bits(lp16)) and np.array_equal(am8, am16) and np.array_equal(bits(lg8), bits(lg16))
    m.close()


def test_exact_default_chunk_on_a_wider_model():
    cfg, N, rows = "small-gptj", 72, (0, 7, 8, 31, 71)
    ids = text(cfg, N)
    want = oracle_rows(cfg, N, rows)
    m = load(cfg)
    lp, am, lg = m.score(0, ids, want_logits=True)
    for i in rows:
        assert np.array_equal(bits(lg[i]), bits(want[i])), i
    R.check_rows(lg, ids[1:] + [-1], lp, am, cfg)
    lp2, am2 = m.score(0, ids)  # without the logits copy: the same scores
    assert np.array_equal(bits(lp), bits(lp2)) and np.array_equal(am, am2)
    m.close()


def test_exact_windows_chain_and_a_decode_step_follows(default_chunk):
    cfg, N = "tiny-neox", 40
    ids = text(cfg, N)
    hip.score_set_chunk_rows(16)
    m = load(cfg)
    lp, am, lg = m.score(0, ids, want_logits=True)
    # a decode step after the scoring eval == one after a plain eval (then with every unwritten byte NaN)
    step = m.eval(N, [7])
    m2 = load(cfg)
    m2.eval(0, ids)
    assert np.array_equal(bits(step), bits(m2.eval(N, [7])))
    m2.debug_poison(N)
    m2.score(0, ids)
    assert np.array_equal(bits(step), bits(m2.eval(N, [7])))
    # chained: eval of the first 24, then the rest scored at n_past = 24
    m2.debug_poison(N)
    m2.eval(0, ids[:24])
    lpc, amc, lgc = m2.score(24, ids[24:], targets=ids[25:] + [-1], want_logits=True)
    assert np.array_equal(bits(lgc), bits(lg[24:]))
    assert np.array_equal(bits(lpc), bits(lp[24:])) and np.array_equal(amc, am[24:])
    # N == 1: the general path, the oracle's row for the one-token prefix
    lp1, am1, lg1 = m2.score(0, ids[:1], targets=[ids[1]], want_logits=True)
    assert np.array_equal(bits(lg1[0]), bits(oracle_rows(cfg, N)[0]))
    assert bits(lp1)[0] == bits(lp)[0] and am1[0] == am[0]
    m.close()
    m2.close()


def test_score_argument_errors():
    cfg = "tiny-neox"
    path, arch_s = model_file(cfg)
    m = load(cfg)
    V = m.n_vocab
    for tg in ([1, V, 2], [1, -2, 2]):
        with pytest.raises(hip.VsimError, match=r"\(-1\).*target"):
            m.score(0, [1, 2, 3], targets=tg)
    with pytest.raises(hip.VsimError, match=r"\(-1\).*n_ctx"):
        m.score(m.n_ctx - 2, [1, 2, 3])
    m.close()
    s0 = hip.Model.load(path, ARCH[arch_s], layer_begin=0, layer_end=1)
    with pytest.raises(hip.VsimError, match=r"\(-1\).*head"):
        s0.score(0, [1, 2, 3])
    s0.close()


def test_last_stage_scores_from_the_residual():
    cfg, N = "tiny-neox", 12
    path, arch_s = model_file(cfg)
    ids = text(cfg, N)
    whole = load(cfg)
    lp, am, lg = whole.score(0, ids, want_logits=True)
    nl = mg.CONFIGS[cfg][1].n_layer
    s0 = hip.Model.load(path, ARCH[arch_s], layer_begin=0, layer_end=1)
    s1 = hip.Model.load(path, ARCH[arch_s], layer_begin=1, layer_end=nl)
    resid = torch.zeros(N, s0.n_embd, dtype=torch.float32, device=DEV)
    s0.eval(0, ids, resid_out=resid, want_logits=False)
    lps, ams, lgs = s1.score(0, targets=ids[1:] + [-1], resid_in=resid, want_logits=True)
    assert np.array_equal(bits(lgs), bits(lg)) and np.array_equal(bits(lps), bits(lp)) and np.array_equal(ams, am)
    for m in (whole, s0, s1):
        m.close()


FAST = [("tiny-gptj", 40), ("tiny-neox", 40), ("tiny-bloom", 40), ("small-neox", 288)]


@pytest.mark.parametrize("cfg,N", FAST)
def test_fast_scores_are_the_restatement_of_their_own_logits(cfg, N, default_chunk):
    ids = text(cfg, N)
    tg = ids[1:] + [-1]
    me = load(cfg)
    lpe, ame = me.score(0, ids)
    me.close()
    m = load(cfg, hip.MODE_FAST)
    # the default chunk (N = 288: the 256-tile lm_head GEMM, then a 32-row rest on the small-tile
    # one), and 5-row chunks: the quantize + GEMV path below GEMM_MIN_N rows
    for C in (0, 5) if N == 40 else (0,):
        hip.score_set_chunk_rows(C)
        lp, am, lg = m.score(0, ids, want_logits=True)
        assert np.isfinite(lg).all() and np.isfinite(lp).all()
        R.check_rows(lg, tg, lp, am, (cfg, C))
        # for the record (random weights overstate the gap); nothing asserted on it
        print(f"\n{cfg} N={N} chunk={C or 'default'} exact vs fast:", score.agreement(lpe, ame, lp, am))
    m.close()


def test_perplexity_windows_on_the_device():
    """score.perplexity over windows shorter than the text == the same windows scored by hand."""
    cfg = "tiny-gptj"
    ids = text(cfg, 40)
    m = load(cfg)
    r = score.perplexity(m, ids, window=16, stride=8)
    assert r["n_scored"] == 39
    lp, _ = m.score(0, ids[:16])
    assert np.array_equal(bits(r["logprob"][:15]), bits(lp[:15]))
    lp, _ = m.score(0, ids[8:24])  # the second window: 8 context rows, then positions 16..23
    assert np.array_equal(bits(r["logprob"][16:23]), bits(lp[8:15]))
    assert r["ppl"] == pytest.approx(math.exp(-float(np.mean(r["logprob"]))), rel=1e-12)
    m.close()


# ------------------------------------------------------------------ the CLI
def test_cli_score_lines():
    path = model_path("tiny-neox")
    ids = text("tiny-neox", 24)
    m = hip.Model.load(path, hip.ARCH_GPTNEOX)
    lp, am = m.score(0, ids)
    m.close()
    r = subprocess.run([CLI, "gptneox", "-m", path, "--prompt", " ".join(map(str, ids)), "--score"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert "<|BEGIN>" not in r.stdout
    summary = lines[-1]
    assert summary.startswith("score: ")
    rows = [ln.split() for ln in lines[-24:-1]]
    assert [int(x[0]) for x in rows] == list(range(1, 24))
    assert [int(x[1]) for x in rows] == ids[1:]
    assert [float(x[2]) for x in rows] == [float(v) for v in lp[:23]]  # %.17g round-trips
    assert [int(x[3]) for x in rows] == [int(v) for v in am[:23]]
    f = dict(kv.split("=") for kv in summary.split()[1:])
    assert int(f["tokens"]) == 23
    assert float(f["nll"]) == pytest.approx(-float(np.mean(lp[:23])), rel=1e-14)
    assert float(f["ppl"]) == pytest.approx(math.exp(-float(np.mean(lp[:23]))), rel=1e-13)
    assert float(f["top1"]) == pytest.approx(float(np.mean(am[:23] == np.array(ids[1:]))), abs=1e-6)
    # a text longer than the context: windows of n_ctx = 16 tokens, -b 8 the stride -- the lines
    # are score.perplexity's with the same window and stride
    m = hip.Model.load(path, hip.ARCH_GPTNEOX, n_ctx=16)
    want = score.perplexity(m, ids, window=16, stride=8)
    m.close()
    r = subprocess.run([CLI, "gptneox", "-m", path, "--prompt", " ".join(map(str, ids)), "--score", "--n_ctx", "16",
                        "-b", "8"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    rows = [ln.split() for ln in lines[-24:-1]]
    assert [int(x[0]) for x in rows] == list(range(1, 24))
    assert [float(x[2]) for x in rows] == [float(v) for v in want["logprob"]]
    f = dict(kv.split("=") for kv in lines[-1].split()[1:])
    assert float(f["ppl"]) == pytest.approx(want["ppl"], rel=1e-13)
