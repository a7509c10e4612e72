"""The sampler's device stage (k_sample_topk) and the sampled decode step built on it.

* vsim_op_topk against a float64 numpy restatement of the candidate stage of
  sample_top_p_top_k_repeat_penalty (utils.cpp:339-371) -- values as bits, ids exactly --
  on tie-free rows (where the reference's own order is defined) and on rows of ties and
  specials (where the header's rule is: equal values by the lower id);
* Model.eval_sample / generate_sampled against the oracle's loop and the reference's golden
  streams, with the graph on and off, two samplers alternating on one model, the host
  fallback, and the CLI's two sampler paths.
"""
import functools
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import oracle_py as O
from golden_util import e2e, model_path, prompt_ids
from vsim_amd import hip
from vsim_amd import modelgen as mg

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CLI = os.path.join(ROOT, "vsim_amd", "_build", "vsim-hip")
GOLDEN_PARAMS = dict(seed=42, top_k=20, top_p=0.95, temp=0.85, repeat_last_n=64, repeat_penalty=1.3)
CLI_DEFAULTS = dict(seed=42, top_k=40, top_p=0.95, temp=0.8, repeat_last_n=64, repeat_penalty=1.3)
PARAMS = {"golden": GOLDEN_PARAMS, "cli-defaults": CLI_DEFAULTS}
ARCH = {"gptneox": hip.ARCH_GPTNEOX, "gptj": hip.ARCH_GPTJ, "bloom": hip.ARCH_BLOOM}
DEV = "cuda:0"


# ------------------------------------------------------------------ vsim_op_topk
def widen(f):
    """A float parameter passed to a double argument."""
    return float(np.float32(f))


def ref_topk(x, win, temp, penalty, k):
    """(val bits, ids) of the k largest candidates: float64 arithmetic in the reference's order,
    descending by value, equal values by the lower id."""
    scale, pen = 1.0 / widen(temp), widen(penalty)
    c = x.astype(np.float64) * scale
    inwin = np.zeros(x.size, bool)
    w = np.asarray(win, np.int64)
    inwin[w[(w >= 0) & (w < x.size)]] = True
    with np.errstate(invalid="ignore"):
        c = np.where(inwin, np.where(x < 0, c * pen, c / pen), c)
    order = np.lexsort((np.arange(x.size), -c))[:k]
    return c[order].view(np.uint64), order.astype(np.int32)


def dev_topk(xd, n, win, temp, penalty, k):
    """One vsim_op_topk launch on the default stream; returns its device outputs."""
    wd = torch.tensor(np.asarray(win, np.int32), device=DEV) if len(win) else None
    val = torch.zeros(k, dtype=torch.float64, device=DEV)
    ids = torch.full((k,), -1, dtype=torch.int32, device=DEV)
    hip.topk(xd if isinstance(xd, int) else xd.data_ptr(), n, wd, 1.0 / widen(temp), widen(penalty), k, val, ids)
    return val, ids, wd


def check_topk(x, xd, win, temp, penalty, k, what):
    val, ids, _ = dev_topk(xd, x.size, win, temp, penalty, k)
    torch.cuda.synchronize()
    wv, wi = ref_topk(x, win, temp, penalty, k)
    assert np.array_equal(ids.cpu().numpy(), wi), what
    assert np.array_equal(val.cpu().numpy().view(np.uint64), wv), what


@functools.lru_cache(maxsize=None)
def distinct_row(n):
    """A random permutation of n distinct float32 values of both signs."""
    g = np.random.default_rng(n)
    v = ((np.arange(n, dtype=np.float64) - n / 2 + 0.25) * 1e-3).astype(np.float32)
    assert np.unique(v).size == n
    x = g.permutation(v)
    x.setflags(write=False)
    return x


def windows(x, g):
    n = x.size
    r = [int(t) for t in g.integers(0, n, 48)]
    top5 = [int(t) for t in np.argsort(-x.astype(np.float64))[:5]]  # the penalty must reorder the head
    return {"empty": [], "zeros": [0] * 64, "random-dup": r + r[:16], "top5": top5 + top5[:2]}


NK = [(n, k) for n in (1, 20, 128, 257, 4099, 50400, 250880) for k in (1, 20, 40, 64) if k <= n]


@pytest.mark.parametrize("n,k", NK)
def test_topk_matches_numpy(n, k):
    x = distinct_row(n)
    xd = torch.tensor(x, device=DEV)
    g = np.random.default_rng(7 * n + k)
    for wname, win in windows(x, g).items():
        for temp in (0.85, 1.0):
            for pen in (1.0, 1.3):
                wv, _ = ref_topk(x, win, temp, pen, min(n, k + 1))
                assert np.unique(wv).size == wv.size  # tie-free: the reference's own order is what is checked
                check_topk(x, xd, win, temp, pen, k, (wname, temp, pen))


def test_topk_row_offset_by_one_float():
    n = 50400
    x = distinct_row(n)
    buf = torch.zeros(n + 1, dtype=torch.float32, device=DEV)
    buf[1:] = torch.tensor(x, device=DEV)
    assert (buf.data_ptr() + 4) % 16 != 0
    check_topk(x, buf.data_ptr() + 4, [0] * 64, 0.85, 1.3, 40, "offset")


def test_topk_massive_ties_follow_the_id_rule():
    g = np.random.default_rng(3)
    levels = np.array([-3.5, -1.0, -0.0, 0.0, 0.25, 1.0, 2.0, 2.0000002], np.float32)
    for n, k in ((4099, 64), (50400, 40), (257, 20)):
        x = levels[g.integers(0, 8, n)]
        xd = torch.tensor(x, device=DEV)
        for win in ([], list(g.integers(0, n, 64)), list(np.flatnonzero(x == levels[-1])[:40])):
            check_topk(x, xd, win, 0.85, 1.3, k, (n, k, len(win)))


def test_topk_signed_zeros():
    g = np.random.default_rng(4)
    x = np.where(g.integers(0, 2, 257) == 1, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    xd = torch.tensor(x, device=DEV)
    check_topk(x, xd, [], 1.0, 1.0, 20, "zeros")
    check_topk(x, xd, [1, 2, 3, 250], 0.85, 1.3, 20, "zeros, window")


def test_topk_minus_infinity():
    g = np.random.default_rng(6)
    x = g.standard_normal(4099).astype(np.float32)
    x[g.permutation(4099)[:4070]] = -np.inf  # 29 finite values: the -inf entries reach the list
    xd = torch.tensor(x, device=DEV)
    check_topk(x, xd, [], 1.0, 1.0, 64, "-inf")
    check_topk(x, xd, list(g.integers(0, 4099, 64)), 0.85, 1.3, 40, "-inf, window")


@pytest.mark.parametrize("n", [1, 20, 64])
def test_topk_k_equals_n(n):
    x = np.random.default_rng(n).standard_normal(n).astype(np.float32)
    check_topk(x, torch.tensor(x, device=DEV), [0] * 64, 0.85, 1.3, n, n)


def test_topk_back_to_back_launches_share_the_workspace():
    g = np.random.default_rng(8)
    jobs = []
    for i in range(20):
        n = int(g.choice([128, 4099, 50400, 250880, 1500]))
        x = g.standard_normal(n).astype(np.float32) * 3
        win = list(g.integers(0, n, 64))
        k = int(g.choice([1, 20, 40, 64]))
        jobs.append((x, torch.tensor(x, device=DEV), win, k))
    torch.cuda.synchronize()
    outs = [dev_topk(xd, x.size, win, 0.85, 1.3, k) for x, xd, win, k in jobs]  # no synchronize in between
    torch.cuda.synchronize()
    for (x, _, win, k), (val, ids, _) in zip(jobs, outs):
        wv, wi = ref_topk(x, win, 0.85, 1.3, k)
        assert np.array_equal(ids.cpu().numpy(), wi)
        assert np.array_equal(val.cpu().numpy().view(np.uint64), wv)


def test_topk_limits():
    x = torch.zeros(128, dtype=torch.float32, device=DEV)
    val = torch.zeros(128, dtype=torch.float64, device=DEV)
    ids = torch.zeros(128, dtype=torch.int32, device=DEV)
    win = torch.zeros(hip.WINDOW_MAX + 1, dtype=torch.int32, device=DEV)
    for n, k, nw in ((128, 0, 0), (128, hip.TOPK_MAX + 1, 0), (20, 21, 0), (128, 20, hip.WINDOW_MAX + 1), (0, 1, 0)):
        rc = hip.lib().vsim_op_topk(x.data_ptr(), n, win.data_ptr(), nw, 1.0, 1.0, k, val.data_ptr(),
                                    ids.data_ptr(), None)
        assert rc == -1, (n, k, nw)  # VSIM_EINVAL


# ------------------------------------------------------------------ the sampled decode step
@functools.lru_cache(maxsize=None)
def model_file(cfg):
    arch_s, hp = mg.CONFIGS[cfg]
    path = os.path.join(tempfile.mkdtemp(), f"{cfg}.bin")
    mg.write_model(path, arch_s, hp, seed=5, std=0.08)
    return path, arch_s


PROMPT10 = (3, 1, 4, 1, 5, 9, 7, 6, 5, 8)  # 9 + 1: the last chunk is a single token


@functools.lru_cache(maxsize=None)
def oracle_stream(cfg, pname, top_k=None):
    path, arch_s = model_file(cfg)
    p = dict(PARAMS[pname])
    if top_k:
        p["top_k"] = top_k
    return O.Model(path, ARCH[arch_s]).generate(list(PROMPT10), 24, **p)


def device_stream(dm, prompt, params, n_predict=24, n_batch=8):
    """The CLI's loop through the Python API: prompt chunks of n_batch + 1 through eval and
    Sampler.accept, then generate_sampled (a token that follows a multi-token chunk is sampled
    from that eval's logits row on the host).  Returns (ids as the CLI prints them, sampler)."""
    s = hip.Sampler(**params)
    n_predict = min(n_predict, dm.n_ctx - len(prompt))
    chunks = [list(prompt[i:i + n_batch + 1]) for i in range(0, len(prompt), n_batch + 1)]
    out, n_past = [], 0
    for ch in chunks[:-1]:
        for t in ch:
            s.accept(t)
        out += ch
        if ch[-1] == 2:
            return out, s
        dm.eval(n_past, ch, want_logits=False)
        n_past += len(ch)
    last = chunks[-1]
    for t in last:
        s.accept(t)
    out += last
    if last[-1] == 2 or n_predict == 0:
        return out, s
    if len(last) == 1:
        return out + dm.generate_sampled(s, n_past, last[0], n_predict, eos=2), s
    first = s.sample_host(dm.eval(n_past, last))
    out.append(first)
    if first != 2 and n_predict > 1:
        out += dm.generate_sampled(s, n_past + len(last), first, n_predict - 1, eos=2)
    return out, s


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("pname", ["golden", "cli-defaults"])
@pytest.mark.parametrize("cfg", ["tiny-neox", "small-gptj", "tiny-bloom"])
def test_eval_sample_matches_oracle_loop(cfg, pname, graph):
    path, arch_s = model_file(cfg)
    want = oracle_stream(cfg, pname)
    dm = hip.Model.load(path, ARCH[arch_s])
    dm.set_graph(graph)
    got, s = device_stream(dm, PROMPT10, PARAMS[pname])
    assert got == want
    assert s.stats() == {"device": len(want) - len(PROMPT10), "host": 0}
    assert dm.info()["graph"] == graph
    dm.close()


def test_sampled_step_counts_its_launch():
    path, arch_s = model_file("tiny-neox")
    dm = hip.Model.load(path, ARCH[arch_s])
    dm.eval(0, [5])
    base = dm.info()["kernels_per_eval"]
    dm.eval_sample(hip.Sampler(**GOLDEN_PARAMS), 1, 7)
    assert dm.info()["kernels_per_eval"] == base + 1
    dm.close()


def test_two_samplers_alternate_on_one_model():
    """Sampler A decodes at positions 9.., sampler B at 99.. of one model, token by token in
    turn, with the graph on.  A never sees B's positions; B sees A's, so B alone is run with A's
    tokens replayed through plain evals: the same cache contents, one sampler."""
    path, arch_s = model_file("small-gptj")
    pa = dict(seed=42, top_k=20, top_p=0.95, temp=0.85, repeat_last_n=64, repeat_penalty=1.3)
    pb = dict(seed=43, top_k=40, top_p=1.0, temp=1.0, repeat_last_n=8, repeat_penalty=1.0)
    pre = [int(t) for t in np.random.default_rng(12).integers(3, 512, 100)]
    steps = 24

    def start(with_b_prefix):
        dm = hip.Model.load(path, ARCH[arch_s])
        dm.set_graph(True)
        dm.eval(0, pre[:9], want_logits=False)
        if with_b_prefix:
            dm.eval(9, pre[9:99], want_logits=False)
        return dm

    def sampler(p, n_prompt):
        s = hip.Sampler(**p)
        for t in pre[:n_prompt]:
            s.accept(t)
        return s

    dm, sa = start(False), sampler(pa, 10)
    a_alone = dm.generate_sampled(sa, 9, pre[9], steps)
    dm.close()
    a_in = [pre[9]] + a_alone[:-1]  # the token A evaluates at step j

    dm, sb = start(True), sampler(pb, 100)
    b_alone, tb = [], pre[99]
    for j in range(steps):
        dm.eval(9 + j, [a_in[j]], want_logits=False)
        tb = dm.eval_sample(sb, 99 + j, tb)
        b_alone.append(tb)
    dm.close()

    dm, sa, sb = start(True), sampler(pa, 10), sampler(pb, 100)
    a_got, b_got, ta, tb = [], [], pre[9], pre[99]
    for j in range(steps):
        ta = dm.eval_sample(sa, 9 + j, ta)
        tb = dm.eval_sample(sb, 99 + j, tb)
        a_got.append(ta)
        b_got.append(tb)
    dm.close()
    assert a_got == a_alone
    assert b_got == b_alone
    assert a_got != b_got
    assert sa.stats() == {"device": steps, "host": 0} and sb.stats() == {"device": steps, "host": 0}


@pytest.mark.parametrize("name", sorted(e2e()["models"]))
def test_generate_sampled_reproduces_golden_streams(name):
    ent = e2e()["models"][name]
    dm = hip.Model.load(model_path(name), hip.ARCH_GPTNEOX)
    for prompt, toks in ent["sampled"].items():
        got, s = device_stream(dm, prompt_ids(prompt), GOLDEN_PARAMS)
        assert got == toks, prompt
        st = s.stats()
        assert st["device"] >= len(toks) - len(prompt_ids(prompt)) - 1 and st["host"] <= 1
    dm.close()


def test_top_k_past_the_device_limit_falls_back_to_the_host():
    path, arch_s = model_file("small-gptj")
    want = oracle_stream("small-gptj", "golden", top_k=100)
    dm = hip.Model.load(path, ARCH[arch_s])
    got, s = device_stream(dm, PROMPT10, dict(GOLDEN_PARAMS, top_k=100))
    assert got == want
    assert s.stats() == {"device": 0, "host": len(want) - len(PROMPT10)}
    dm.close()


@pytest.mark.parametrize("path_name", ["host", "device"])
def test_cli_sampler_paths_print_the_golden_stream(path_name):
    ent = e2e()["models"]["tiny-neox"]
    for prompt in ("1 2 3 4", "5"):  # the first token follows a 4-token batch / a single-token eval
        toks = ent["sampled"][prompt]
        r = subprocess.run([CLI, "gptneox", "-m", model_path("tiny-neox"), "--prompt", prompt, "--n_predict", "24",
                            "--top_k", "20", "--top_p", "0.95", "--temp", "0.85", "--repeat_last_n", "64",
                            "--repeat_penalty", "1.3", "--seed", "42", "--sampler", path_name],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        got = [int(t) for t in r.stdout.split("<|BEGIN>", 1)[1].split("<END|>", 1)[0].split()]
        assert got == toks, prompt
        lines = r.stdout.strip().splitlines()
        assert lines[-2].startswith("vsim-hip: load ")
        assert lines[-1].startswith(f"vsim-hip: sampler {path_name}: ")
        n_dev = int(lines[-1].split(":")[2].split()[0])
        assert (n_dev > 0) == (path_name == "device")
