"""Weight-only mode's single-token step (enqueue_decode_w4a16) through the model executor: bit for bit
the general path, whichever way it runs.  The step on and off (hip.w4a16_set_step), the hipGraph on
and off, against eval_seq(0, ...) -- which stays on the general path -- for the three tiny configs of
modelgen and a serial-residual GPT-NeoX (E = 128, 4 heads of d = 32, 2 layers, vocabulary 128),
n_ctx = 96, the scratch and the caches poisoned first; the launch budget, the profile's kernel names,
the LayerNorm fallback counters, one wider shape, and the CLI.
"""
import os
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import oracle_py as O  # noqa: E402
from vsim_amd import hip  # noqa: E402
from vsim_amd import modelgen as mg  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
ARCH = {"gptj": hip.ARCH_GPTJ, "gptneox": hip.ARCH_GPTNEOX, "bloom": hip.ARCH_BLOOM}
CONFIGS = dict(mg.CONFIGS)
CONFIGS["tiny-neox-serial"] = ("gptneox", mg.HParams(128, 128, 4, 2, 8, 0))
CONFIGS["wide-neox"] = ("gptneox", mg.HParams(128, 256, 4, 2, 32))        # d = 64
CONFIGS["wide-gptj"] = ("gptj", mg.HParams(128, 256, 4, 2, 16))           # d = 64, n_rot < d
CFGS = ["tiny-neox", "tiny-gptj", "tiny-bloom", "tiny-neox-serial"]
N_CTX = 96
POSITIONS = [0, 1, 31, 32, 33, N_CTX - 1]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b, what):
    if not np.array_equal(bits(a), bits(b)):
        bad = np.argwhere(bits(a) != bits(b))
        pytest.fail(f"{what}: {len(bad)} values differ, first {bad[:4].tolist()}: "
                    f"{np.asarray(a)[tuple(bad[0])]!r} against {np.asarray(b)[tuple(bad[0])]!r}")


def load(cfg, tmp_path, seed=11, mode=hip.MODE_W4A16):
    arch_s, hp = CONFIGS[cfg]
    path = str(tmp_path / f"{cfg}.bin")
    mg.write_model(path, arch_s, hp, seed=seed, std=0.05)
    dm = hip.Model.load(path, ARCH[arch_s], n_ctx=N_CTX)
    dm.set_mode(mode)
    return dm, hp, path, arch_s


def tokens_of(hp, n, seed):
    return [int(t) for t in np.random.default_rng(seed).integers(0, hp.n_vocab, n)]


@pytest.fixture(autouse=True)
def step_switch():
    """Every test starts and ends with the step on."""
    hip.w4a16_set_step(1)
    yield
    hip.w4a16_set_step(1)


def budget(cfg):
    """The issue's launch budget for one eval: the embedding row (+ BLOOM's embedding norm), 7 launches
    per parallel-residual layer or 9 per serial one, 2 for the head."""
    arch_s, hp = CONFIGS[cfg]
    serial = arch_s == "bloom" or (arch_s == "gptneox" and not hp.use_parallel_residual)
    return 1 + (arch_s == "bloom") + hp.n_layer * (9 if serial else 7) + 2


@pytest.mark.parametrize("cfg", CFGS)
def test_step_equals_general_path_at_every_position(cfg, tmp_path):
    dm, hp, _, _ = load(cfg, tmp_path)
    toks = tokens_of(hp, N_CTX + 1, 3)
    dm.debug_poison(N_CTX)
    # the general path's rows: one prompt up to each position, then the single token through eval_seq
    want, after = {}, {}
    for p in POSITIONS:
        if p:
            dm.eval_seq(0, 0, toks[:p], want_logits=False)
        want[p] = dm.eval_seq(0, p, [toks[p]])
        if p + 1 < N_CTX:
            after[p] = dm.eval_seq(0, p + 1, [toks[p + 1]])
    assert all(np.isfinite(v).all() for v in want.values())
    counts = {}
    for step in (1, 0):
        for graph in (True, False):
            hip.w4a16_set_step(step)
            dm.set_graph(graph)
            for p in POSITIONS:
                dm.debug_poison(N_CTX)
                if p:
                    dm.eval_seq(0, 0, toks[:p], want_logits=False)
                same(dm.eval(p, [toks[p]]), want[p], f"{cfg}: step {step} graph {graph} position {p}")
                counts[step] = dm.info()["kernels_per_eval"]
                if p + 1 < N_CTX:   # the cache row this step wrote, read by the general path and by the step
                    same(dm.eval_seq(0, p + 1, [toks[p + 1]]), after[p], f"{cfg}: general path after step {step} at {p}")
                    same(dm.eval(p + 1, [toks[p + 1]]), after[p], f"{cfg}: step {step} graph {graph} after itself at {p}")
    print(f"{cfg}: kernels per eval: step {counts[1]} (budget {budget(cfg)}), general path {counts[0]}")
    assert counts[1] <= budget(cfg) and counts[1] < counts[0]
    dm.close()


@pytest.mark.parametrize("cfg", CFGS)
def test_argmax_generate_and_sampling(cfg, tmp_path):
    dm, hp, _, _ = load(cfg, tmp_path)
    toks = tokens_of(hp, 12, 5)
    n0 = 9
    # the loop of general-path evals
    dm.eval_seq(0, 0, toks[:n0], want_logits=False)
    want, t = [], toks[n0]
    for i in range(20):
        t = int(dm.eval_seq(0, n0 + i, [t]).argmax())
        want.append(t)
    p = dict(seed=5, top_k=7, top_p=0.9, temp=0.7, repeat_last_n=8, repeat_penalty=1.2)

    def twin_sampled(n):
        """eval_seq + vsim_op_topk + pick, the window kept here."""
        s, win = hip.Sampler(**p), [0] * p["repeat_last_n"]
        dm.eval_seq(0, 0, toks[:n0], want_logits=False)
        t, out = toks[n0], []
        for i in range(n):
            lg = dm.eval_seq(0, n0 + i, [t])
            val = torch.zeros(p["top_k"], dtype=torch.float64, device=DEV)
            ids = torch.zeros(p["top_k"], dtype=torch.int32, device=DEV)
            hip.topk(torch.tensor(lg, device=DEV), lg.size, torch.tensor(np.asarray(win, np.int32), device=DEV),
                     1.0 / float(np.float32(p["temp"])), float(np.float32(p["repeat_penalty"])), p["top_k"], val, ids)
            torch.cuda.synchronize()
            t = s.pick(val.cpu().numpy(), ids.cpu().numpy())
            win = win[1:] + [int(t)]
            out.append(t)
        return out

    want_s = twin_sampled(6)
    for step in (1, 0):
        for graph in (True, False):
            hip.w4a16_set_step(step)
            dm.set_graph(graph)
            what = f"{cfg}: step {step} graph {graph}"
            dm.eval_seq(0, 0, toks[:n0], want_logits=False)
            assert dm.eval_argmax(n0, toks[n0]) == want[0], what
            dm.eval_seq(0, 0, toks[:n0], want_logits=False)
            assert list(dm.generate(n0, toks[n0], 20)) == want, what
            dm.eval_seq(0, 0, toks[:n0], want_logits=False)
            assert list(dm.generate_sampled(hip.Sampler(**p), n0, toks[n0], 6)) == want_s, what
            s1 = hip.Sampler(**p)
            dm.eval_seq(0, 0, toks[:n0], want_logits=False)
            assert dm.eval_sample(s1, n0, toks[n0]) == want_s[0], what
    dm.close()


@pytest.mark.parametrize("cfg", ["tiny-neox", "tiny-gptj", "tiny-bloom"])
def test_mode_switches_with_graphs_on(cfg, tmp_path):
    """exact -> w4a16 -> fast -> w4a16 with graphs on: the mode's bits unchanged, exact mode the oracle's."""
    dm, hp, path, arch_s = load(cfg, tmp_path, mode=hip.MODE_EXACT)
    dm.set_graph(True)
    om = O.Model.from_device(dm, arch_s, n_ctx=N_CTX)
    toks = tokens_of(hp, 12, 6)
    want = [om.eval(0, toks[:9]), om.eval(9, [toks[9]])]

    def exact_pass(what):
        dm.set_mode(hip.MODE_EXACT)
        same(dm.eval(0, toks[:9]), want[0], f"{cfg}: exact prompt {what}")
        same(dm.eval(9, [toks[9]]), want[1], f"{cfg}: exact step {what}")

    def w4_pass():
        dm.set_mode(hip.MODE_W4A16)
        dm.eval(0, toks[:9], want_logits=False)
        return np.stack([dm.eval(9, [toks[9]]), dm.eval(10, [toks[10]])])

    exact_pass("before")
    first = w4_pass()
    dm.eval_seq(0, 0, toks[:9], want_logits=False)
    same(first, np.stack([dm.eval_seq(0, 9, [toks[9]]), dm.eval_seq(0, 10, [toks[10]])]), f"{cfg}: the general path")
    dm.set_mode(hip.MODE_FAST)
    dm.eval(0, toks[:9])
    dm.eval(9, [toks[9]])
    same(w4_pass(), first, f"{cfg}: w4a16 after a fast pass")
    exact_pass("after")
    same(w4_pass(), first, f"{cfg}: w4a16 after an exact pass")
    dm.close()


@pytest.mark.parametrize("cfg", ["tiny-neox", "tiny-bloom"])
def test_profile_names_and_switch(cfg, tmp_path):
    dm, hp, _, _ = load(cfg, tmp_path)
    toks = tokens_of(hp, 6, 8)
    new, old = {"k_gemv_w4a16", "k_w4a16_ln", "k_w4a16_gelu"}, {"k_gemm_w4a16_rows"}

    def names(step):
        hip.w4a16_set_step(step)
        dm.set_graph(True)     # profiling forces the eager form
        dm.set_profile(True)
        for i in range(3):
            dm.eval(i, [toks[i]])
        dm.eval_argmax(3, toks[3])
        out = " | ".join(k["name"] for k in dm.profile_kernels())
        dm.set_profile(False)
        return out

    on, off = names(1), names(0)
    assert all(n in on for n in new) and not any(n in on for n in old), on
    assert all(n in off for n in old) and not any(n in off for n in new), off
    dm.close()


def test_norm_fallbacks_move_identically(tmp_path):
    """The same tokens through the step and through the general path: vsim_norm_fallbacks moves by the
    same amounts (k_w4a16_ln counts as k_norm_exact does)."""
    dm, hp, _, _ = load("tiny-neox", tmp_path, seed=23)
    toks = tokens_of(hp, 40, 9)
    deltas = []
    for step in (1, 0):
        hip.w4a16_set_step(step)
        dm.sync()
        c0 = hip.norm_fallbacks()
        for i, t in enumerate(toks):
            dm.eval(i, [t], want_logits=False)
        dm.sync()
        c1 = hip.norm_fallbacks()
        deltas.append((c1[0] - c0[0], c1[1] - c0[1]))
    print(f"norm fallbacks over {len(toks)} tokens: step {deltas[0]}, general path {deltas[1]}")
    assert deltas[0] == deltas[1]
    dm.close()


@pytest.mark.parametrize("cfg", ["wide-neox", "wide-gptj"])
def test_wider_shapes(cfg, tmp_path):
    """E = 256 with d = 64, and GPT-J rotating fewer dimensions than the head has."""
    dm, hp, _, _ = load(cfg, tmp_path)
    toks = tokens_of(hp, 40, 4)
    dm.set_graph(True)
    dm.debug_poison(N_CTX)
    dm.eval_seq(0, 0, toks[:33], want_logits=False)
    want = [dm.eval_seq(0, 33 + i, [toks[33 + i]]) for i in range(3)]
    dm.debug_poison(N_CTX)
    dm.eval_seq(0, 0, toks[:33], want_logits=False)
    for i in range(3):
        same(dm.eval(33 + i, [toks[33 + i]]), want[i], f"{cfg}: position {33 + i}")
    assert dm.info()["kernels_per_eval"] <= budget(cfg)
    dm.close()


def test_cli_generates_through_the_step(tmp_path):
    """vsim-hip --mode w4a16 --top_k 1, with the graph and with --no-graph: the tokens of Model.generate
    with the step switched off (the CLI has no switch of its own)."""
    cli = os.path.join(os.path.dirname(os.path.abspath(hip.__file__)), "_build", "vsim-hip")
    dm, hp, path, _ = load("tiny-neox", tmp_path)
    ids = tokens_of(hp, 20, 13)
    hip.w4a16_set_step(0)
    first = int(dm.eval(0, ids).argmax())
    want = [first] + [int(t) for t in dm.generate(len(ids), first, 5)]
    dm.close()
    for extra in ([], ["--no-graph"]):
        r = subprocess.run([cli, "gptneox", "-m", path, "--prompt", " ".join(map(str, ids)), "--mode", "w4a16", "--top_k", "1",
                            "--repeat_penalty", "1.0", "-n", "6", "--n_ctx", str(N_CTX), "-b", "64"] + extra,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        body = r.stdout.split("<|BEGIN>")[1].split("<END|>")[0].split()
        got = [int(t) for t in body][len(ids):]
        assert got == want[:len(got)] and (len(got) == 6 or got[-1] == 2), (extra, got, want)
