"""Per-node parity of the graph executor (vsim_graph_compute_rc, vsim_amd/csrc/graph.cpp and
graph.hip) with the reference's own ggml_graph_compute, run on the same graph object in the
same process by oracle/_ref/graph_cases (oracle/graph_cases.c, `make -C oracle graphcases`).

Each case builds a small graph with the ggml API alone -- permutes, padded views, cache views,
both rope styles, the Q4_0 and F32 products, the mirror lifecycle, refused nodes, a two-layer
GPT-J-style composite -- computes it with the reference, restores memory, computes it on the
device and compares every checked tensor bit for bit; there is no tolerance anywhere.  The
driver prints one CHECK line per tensor and exits 0 only if every one has mismatches=0 (and,
for a refusal, VSIM_EINVAL naming the op, host memory byte-identical, the computes counter
unchanged and a valid graph passing right after).

Two live runs of the reference's eval loop on the executor (oracle/_ref/vsim-graph) against the
reference binary close the model-level gaps: the serial-residual GPT-NeoX, whose decode steps
stay on the per-node path by design, and prompt batches on a cache four batches deep.
"""
import os
import re
import subprocess

import pytest

from golden_util import e2e, model_path
from vsim_amd import modelgen as mg

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CASES_BIN = os.path.join(ROOT, "oracle", "_ref", "graph_cases")
GRAPH = os.path.join(ROOT, "oracle", "_ref", "vsim-graph")
REFBIN = os.path.join(ROOT, "oracle", "_ref", "vsim-ref")

# The driver's cases, in its --list order: a case dropped from the driver fails test_case_list.
CASES = [
    "dup_perm_0213", "cpy_perm_1023", "cpy_perm_2013", "cpy_cache_view",
    "add_padded_view", "mul_padded_view", "add_transposed_src1", "addmul_3d",
    "repeat_rows", "repeat_cols", "repeat_both",
    "scale_leaf", "scale_node_scalar",
    "mask_only", "mask_past8", "mask_past0", "mask_one_row", "mask_one_col", "mask_300_cols", "mask_equal_row",
    "norm_32x1", "norm_32x5", "norm_96x1", "norm_96x5", "norm_1000x1", "norm_1000x5",
    "gelu_1000", "get_rows_1", "get_rows_9",
    "mmq_1_32_1", "mmq_33_64_2", "mmq_130_96_9", "mmq_gather_rows", "mmq_small_then_large",
    "kq_cache_view", "kq_4d", "kqv", "kqv_2_keys", "kqv_4d",
    "rope_d8_p0", "rope_d8_p3", "rope_d32_p0", "rope_d32_p3", "rope_mode1",
    "neox_rope_d8_p0", "neox_rope_d8_p3", "neox_rope_d32_p0", "neox_rope_d32_p3", "neox_rope_mode1",
    "rope_regrow", "neox_rope_regrow", "rope_two_dims",
    "life_two_arenas", "life_leaf_reshaped", "life_reset", "life_sync_view",
    "refuse_alibi", "refuse_silu", "refuse_cpy_strided_dst", "refuse_cpy_f16", "refuse_get_rows_f32",
    "gptj_two_layers",
]
REFUSALS = [c for c in CASES if c.startswith("refuse_")]
# The transposed F32 product sums per-thread partials (ggml.c:4535-4581, 4469-4493), so these
# results depend on the thread count in their last bits.  kqv_2_keys does not: with two keys
# both groupings are the one add x0 + x1.  Nor does gptj_two_layers at 1 vs 4: its KQV rows are
# re-quantized to Q4_0 for the output projection, which absorbs the last-bit differences.
THREAD_GROUPED = ["kqv", "kqv_4d"]
# The device groups by cgraph->n_threads only in that product; every other kernel is the same at
# any thread count, so those cases run once.  0 threads: the reference takes 8 (ggml.c:8246).
THREADS = {"kqv": (1, 2, 4, 7, 0), "kqv_2_keys": (1, 7), "kqv_4d": (1, 4), "gptj_two_layers": (1, 4),
           "kq_cache_view": (1, 4)}

CHECK = re.compile(r"^CHECK (\S+) (\S+) elems=(\d+) mismatches=(\d+) first=(-?\d+) ref=([0-9a-f]{8}) got=([0-9a-f]{8})$")


def cases_bin():
    if not os.path.exists(CASES_BIN):
        pytest.skip("oracle/_ref/graph_cases not built (make -C oracle ref graphcases, needs /root/reference)")
    return CASES_BIN


def run_case(name, threads, *extra):
    r = subprocess.run([cases_bin(), name, "--threads", str(threads), *extra], capture_output=True, text=True,
                       timeout=120)
    print(r.stdout, end="")
    return r


def check_lines(out):
    """{tensor: (elems, mismatches)} of a run's CHECK lines; every line must parse"""
    got = {}
    for ln in out.splitlines():
        if ln.startswith("CHECK"):
            m = CHECK.match(ln)
            assert m, ln
            got[m.group(2)] = (int(m.group(3)), int(m.group(4)))
    return got


def test_case_list():
    r = subprocess.run([cases_bin(), "--list"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.split() == CASES


@pytest.mark.parametrize("name,threads", [(c, t) for c in CASES for t in THREADS.get(c, (1,))])
def test_graph_node_case(name, threads):
    r = run_case(name, threads)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    checks = check_lines(r.stdout)
    assert checks and all(m == 0 and n > 0 for n, m in checks.values()), r.stdout
    if name in REFUSALS:
        assert re.search(r"^REFUSE \S+ rc=-1 named=1 untouched=1 computes_same=1 ", r.stdout, re.M), r.stdout
        assert "after" in checks
    if name == "scale_node_scalar":
        # bit-equal ("out" compared) or refused in the dry pass with host memory untouched
        assert "out" in checks or ("untouched=1" in r.stdout and "parameter must be a leaf" in r.stdout), r.stdout
    if name == "gptj_two_layers":
        assert "FASTPATH gptj_two_layers fast_evals=0 plans=0" in r.stdout
        assert set(checks) == {f"{s}.{t}" for s in ("batch", "token") for t in ("logits", "memory_k", "memory_v")}


# ---------------------------------------------------------------------- live runs
def run_cli(exe, args, threads, env=None):
    if not os.path.exists(exe):
        pytest.skip(f"{os.path.relpath(exe, ROOT)} not built (make -C oracle ref graphdrop, needs /root/reference)")
    r = subprocess.run([exe, "gptneox", *args, "--threads", str(threads)], capture_output=True, text=True,
                       timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout, r.stderr


def logits_rows(out):
    return [ln.split()[1:] for ln in out.splitlines() if ln.startswith("logits:")]


def stats(err):
    m = re.search(r"(\d+) computes, (\d+) on the decode fast path, (\d+) fast-path plans", err)
    assert m, err[-1000:]
    return tuple(int(v) for v in m.groups())


def live(path, prompt, threads):
    """(the executor's logits rows, the reference's, the executor's stats) of a prompt eval:
    --return_logits prints a row per prompt token and ends the run after the prompt"""
    args = ["-m", path, "--prompt", prompt, "--return_logits", "--n_predict", "6", "--top_k", "1"]
    ref, _ = run_cli(REFBIN, args, threads)
    out, err = run_cli(GRAPH, args, threads, env=dict(os.environ, VSIM_GRAPH_STATS="1"))
    return logits_rows(out), logits_rows(ref), stats(err)


def tokens(out):
    body = out.split("<|BEGIN>", 1)[1].split("<END|>", 1)[0]
    return [int(t) for t in re.sub(r"use_parallel_residual == \d+", " ", body).split()]


@pytest.mark.parametrize("threads", [1, 4])
def test_serial_residual_neox_runs_per_node(tmp_path, threads):
    """use_parallel_residual = 0 (vsim.cpp:626-658): no graph matches the fused step, so the
    prompt batches and every decode step run node by node.  The reference's CLI prints logits
    only with --return_logits, which ends the run after the prompt; the decode steps are
    therefore a second, greedy run whose token stream (the argmax of every step's logits, each
    step fed by the one before) must be the reference's."""
    ent = e2e()["models"]["small-neox"]
    arch, hp = mg.CONFIGS["small-neox"]
    hp = mg.HParams(hp.n_vocab, hp.n_embd, hp.n_head, hp.n_layer, hp.n_rot, use_parallel_residual=0)
    path = str(tmp_path / "small-neox-serial.bin")
    mg.write_model(path, arch, hp, seed=ent["seed"], std=ent["std"])
    prompt = "50 12 2 0 7 99 100 3 3 4 5 6"
    got, ref, (computes, fast_evals, plans) = live(path, prompt, threads)
    assert (computes, fast_evals, plans) == (1 + 2, 0, 0)  # the warm-up eval, batches of 9 and 3
    assert len(got) == len(ref) >= 1
    assert got == ref
    greedy = ["-m", path, "--prompt", prompt, "--n_predict", "6", "--top_k", "1", "--top_p", "1.0", "--temp", "1.0",
              "--repeat_penalty", "1.0", "--seed", "42"]
    want = tokens(run_cli(REFBIN, greedy, threads)[0])
    out, err = run_cli(GRAPH, greedy, threads, env=dict(os.environ, VSIM_GRAPH_STATS="1"))
    n_gen = len(want) - len(prompt.split())
    assert n_gen >= 3 and tokens(out) == want
    # every sample but the last is evaluated, each as a graph of its own
    assert stats(err) == (1 + 2 + n_gen - 1, 0, 0)


def test_prompt_batches_on_a_deep_cache():
    """40 prompt tokens in batches of 9 (vsim.cpp:862-876): five prompt graphs, four of them on
    a non-empty cache (n_past 9, 18, 27, 36)."""
    prompt = " ".join(str((37 * i + 11) % 512) for i in range(40))
    got, ref, (computes, fast_evals, plans) = live(model_path("small-neox"), prompt, 4)
    assert (computes, fast_evals) == (1 + 5, 0)  # the warm-up eval and the five batches, per node
    assert len(got) == len(ref) >= 1
    assert got == ref
