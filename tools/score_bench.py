"""Scoring one 2,048-token window on the GPU: Model.score against the token-by-token method.

Model: the GPT-J-6B shape (28 layers, E = 4096, n_vocab = 50400), Model.create + randomize,
n_ctx = 2048.  Per mode (fast, exact), in one process:

  score     Model.score of the whole window (vsim_model_eval_score: one prompt pass, the head over
            all rows in chunks, k_score_rows): wall clock around the call, which ends in a stream
            synchronize; median of --runs runs after a warm-up, reserve(2048) first.
  stepwise  the only method without it: eval of the first token, then 2,047 single-token evals
            with the logits row copied out and log-sum-exp + argmax on the host (numpy, double).
            Median of --step-runs runs.
  kernels   per-kernel device time of one profiled score call (set_profile: an event pair per
            launch), to see what k_score_rows costs beside the lm_head product.

and the exact-vs-fast agreement of the two score results.  The weights are random: see the note
the output ends with.

    python tools/score_bench.py --out profiles/score_bench.txt
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
from vsim_amd import hip, score  # noqa: E402
from vsim_amd import modelgen as mg  # noqa: E402


def stepwise(m, ids):
    """log P(ids[i + 1] | ids[..i]) and the greedy id for every i, one decode step per token."""
    lp, am = np.zeros(len(ids) - 1), np.zeros(len(ids) - 1, np.int32)
    for i in range(len(ids) - 1):
        x = m.eval(i, [ids[i]]).astype(np.float64)
        mx = x.max()
        lp[i] = x[ids[i + 1]] - (mx + np.log(np.exp(x - mx).sum()))
        am[i] = int(np.argmax(x))
    return lp, am


def wall(fn):
    t = time.perf_counter()
    r = fn()
    return time.perf_counter() - t, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="-")
    ap.add_argument("--config", default="gpt-j-6B")
    ap.add_argument("--layers", type=int, default=0, help="fewer layers than the config's (rehearsals)")
    ap.add_argument("--window", type=int, default=2048)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--step-runs", type=int, default=3)
    ap.add_argument("--rev", default="", help="the commit the tree stands on (default: git rev-parse)")
    a = ap.parse_args()
    if hip.lib().vsim_device_count() < 1:
        raise SystemExit("score_bench: no GPU (these are measurements; there is no CPU stand-in)")
    import torch
    out = sys.stdout if a.out == "-" else open(a.out, "w")
    arch_s, hp = mg.CONFIGS[a.config]
    L, N = a.layers or hp.n_layer, a.window
    arch = {"gptneox": hip.ARCH_GPTNEOX, "gptj": hip.ARCH_GPTJ, "bloom": hip.ARCH_BLOOM}[arch_s]
    m = hip.Model.create(arch, dict(n_vocab=hp.n_vocab, n_embd=hp.n_embd, n_head=hp.n_head, n_layer=L, n_rot=hp.n_rot,
                                    use_parallel_residual=1), n_ctx=N)
    m.randomize(seed=1234, std=0.02)
    ids = [(7919 * i + 11) % hp.n_vocab for i in range(N)]
    head = a.rev
    try:
        head = head or subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True,
                              text=True).stdout.strip()
    except OSError:
        head = ""
    gpu = torch.cuda.get_device_name(0) or torch.cuda.get_device_properties(0).gcnArchName
    print(f"# score_bench: {a.config} shape, {L} layers, random weights (std 0.02), one window of {N} tokens, "
          f"n_ctx {N}; {gpu}; tree at {head or 'unknown'} + this change", file=out)
    print(f"# wall-clock ms around calls that end in a stream synchronize; score: median of {a.runs} after a warm-up; "
          f"stepwise: median of {a.step_runs}", file=out)
    res = {}
    for name, mode in (("fast", hip.MODE_FAST), ("exact", hip.MODE_EXACT)):
        m.set_mode(mode)
        m.reserve(N)
        m.score(0, ids)  # warm-up: the scoring scratch, every kernel of the path
        ts = [wall(lambda: m.score(0, ids)) for _ in range(a.runs)]
        t_score = statistics.median(t for t, _ in ts)
        lp, am = ts[-1][1]
        m.eval(0, ids[:1])  # warm-up of the decode step (graph capture)
        tw = [wall(lambda: stepwise(m, ids)) for _ in range(a.step_runs)]
        t_step = statistics.median(t for t, _ in tw)
        slp, sam = tw[-1][1]
        res[name] = (lp, am)
        print(f"\n[{name}] Model.score: {t_score * 1e3:9.1f} ms  (runs: {' '.join(f'{t * 1e3:.1f}' for t, _ in ts)})", file=out)
        print(f"[{name}] stepwise   : {t_step * 1e3:9.1f} ms  (runs: {' '.join(f'{t * 1e3:.1f}' for t, _ in tw)})", file=out)
        print(f"[{name}] ratio stepwise / score: {t_step / t_score:.1f}x", file=out)
        print(f"[{name}] score vs stepwise over the {N - 1} scored positions (informative): "
              f"{score.agreement(lp[:N - 1], am[:N - 1], slp, sam)}", file=out)
        m.set_profile(True)
        m.score(0, ids)
        ks = m.profile_kernels()
        m.set_profile(False)
        tot = sum(k["ms"] for k in ks)
        print(f"[{name}] device time per kernel of one profiled Model.score ({tot:.2f} ms in {sum(k['launches'] for k in ks)} "
              f"launches):", file=out)
        for k in sorted(ks, key=lambda k: -k["ms"]):
            print(f"    {k['name']:<44} {k['ms']:9.3f} ms {100 * k['ms'] / tot:6.2f}% {k['launches']:6d} launches", file=out)
        by = {k["name"]: k["ms"] for k in ks}
        if by.get("lm_head (score)"):
            print(f"[{name}] k_score_rows / lm_head (score) = {by['k_score_rows'] / by['lm_head (score)']:.3f}", file=out)
        out.flush()
    ag = score.agreement(res["exact"][0][:N - 1], res["exact"][1][:N - 1], res["fast"][0][:N - 1], res["fast"][1][:N - 1])
    nll = {k: -float(np.mean(v[0][:N - 1])) for k, v in res.items()}
    print(f"\nexact vs fast on this window: {ag}", file=out)
    print(f"nll exact {nll['exact']:.6f} (ppl {np.exp(nll['exact']):.1f}), fast {nll['fast']:.6f} (ppl {np.exp(nll['fast']):.1f}); "
          f"ln(n_vocab) = {np.log(hp.n_vocab):.6f}", file=out)
    print("note: these are random weights.  Their logits are nearly flat and their activations have no structure the "
          "quantizer can lean on, so the exact-vs-fast gap above overstates what a trained checkpoint shows (DESIGN.md "
          "2.2); it is here to show the tool at work.  A real checkpoint's number is the user's to produce: "
          "vsim-hip --score --mode exact|fast.", file=out)
    m.close()
    if out is not sys.stdout:
        out.close()
        print(open(a.out).read())


if __name__ == "__main__":
    main()
