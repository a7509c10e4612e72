#!/usr/bin/env python3
"""Aggregate decode rate of vsim_model_decode_batch against the single-stream greedy loop.

A model of a benchmark config's shape with random weights, exact mode.  For each batch size B the
B sequences sit in slots 0..B-1; positions [0, pos0) are run and discarded (they fill the caches
and warm every kernel up), then the steps at positions pos0 .. pos1-1 are timed: a host clock
round calls that each end in a stream synchronize, only the greedy ids leaving the device, each
row's id fed back as its next token.  vsim_batch_set_gemm 2 (k_gemm_exact_rows at every B) and 0
(the GEMV jobs) alternate inside every repeat; the figure of a (B, setting) is the median over the repeats.

The baseline is vsim_model_generate over the same positions -- what a user with B sequences gets
today by running them in turn -- measured in the same job, from this library and, with
--baseline-lib, from another build of the library (the parent commit's) in a child process.

  python tools/batch_bench.py --out profiles/batch_decode_bench.txt --baseline-lib PATH --tree "1b11083 + this change"
  python tools/batch_bench.py --one-step 16        # for a profiler run: warm-up, then one B = 16 step
"""
import argparse
import ctypes
import json
import os
import socket
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

from vsim_amd import modelgen as mg  # noqa: E402

ARCH = {"gptneox": 0, "gptj": 1, "bloom": 2}


def hparams(cfg, layers):
    arch_s, hp = mg.CONFIGS[cfg]
    return arch_s, dict(n_vocab=hp.n_vocab, n_embd=hp.n_embd, n_head=hp.n_head, n_layer=layers or hp.n_layer,
                        n_rot=hp.n_rot, use_parallel_residual=hp.use_parallel_residual)


def baseline_child(a):
    """vsim_model_generate on the library at a.lib, through plain ctypes (an older build has none
    of the batch symbols, so vsim_amd.hip cannot bind it): prints one JSON line."""
    L = ctypes.CDLL(a.lib, mode=ctypes.RTLD_GLOBAL)
    arch_s, hp = hparams(a.config, a.layers)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    hpc = (ctypes.c_int32 * 6)(hp["n_vocab"], hp["n_embd"], hp["n_head"], hp["n_layer"], hp["n_rot"],
                               hp["use_parallel_residual"])
    L.vsim_model_create.argtypes = [ci, vp, ci, ci, ci, ci, ctypes.POINTER(vp)]
    L.vsim_model_randomize.argtypes = [vp, ctypes.c_uint64, ctypes.c_float]
    L.vsim_model_set_mode.argtypes = [vp, ci]
    L.vsim_model_set_graph.argtypes = [vp, ci]
    L.vsim_model_eval.argtypes = [vp, ci, vp, ci, vp, vp, vp]
    L.vsim_model_generate.argtypes = [vp, ci, ctypes.c_int32, ci, vp]
    L.vsim_model_free.argtypes = [vp]
    L.vsim_last_error.restype = ctypes.c_char_p
    h = vp()

    def ck(rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed ({rc}): {L.vsim_last_error().decode(errors='replace')}")

    ck(L.vsim_model_create(ARCH[arch_s], hpc, a.n_ctx, 0, 0, -1, ctypes.byref(h)), "create")
    ck(L.vsim_model_randomize(h, 1, 0.02), "randomize")
    ck(L.vsim_model_set_mode(h, 0), "set_mode")
    ck(L.vsim_model_set_graph(h, 1), "set_graph")
    prompt = np.arange(1, a.pos0 + 1, dtype=np.int32)
    ck(L.vsim_model_eval(h, 0, prompt.ctypes.data, a.pos0, None, None, None), "eval")
    n = a.pos1 - a.pos0
    out = np.zeros(n, np.int32)
    runs = []
    for r in range(a.repeats + 1):  # the first captures the graph and is discarded
        t0 = time.perf_counter()
        ck(L.vsim_model_generate(h, a.pos0, 7, n, out.ctypes.data), "generate")
        runs.append(n / (time.perf_counter() - t0))
    L.vsim_model_free(h)
    print(json.dumps({"tok_s": statistics.median(runs[1:]), "runs": runs[1:]}))


def run_baseline(a, lib):
    cmd = [sys.executable, os.path.abspath(__file__), "--baseline-child", "--lib", lib, "--config", a.config,
           "--layers", str(a.layers), "--n-ctx", str(a.n_ctx), "--pos0", str(a.pos0), "--pos1", str(a.pos1),
           "--repeats", str(a.repeats)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(f"baseline run on {lib} failed:\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def timed_steps(dm, B, pos0, pos1, timed=True):
    """Positions [0, pos1) of B sequences in slots 0..B-1; returns the seconds of [pos0, pos1)."""
    seqs = list(range(B))
    tok = [3 + b for b in range(B)]
    t0 = 0.0
    for p in range(pos1):
        if p == pos0:
            t0 = time.perf_counter()
        _, nxt = dm.decode_batch(seqs, [p] * B, tok, want_logits=False)
        tok = [int(t) for t in nxt]
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="gpt-j-6B")
    ap.add_argument("--layers", type=int, default=0, help="0: the config's own depth")
    ap.add_argument("--n-ctx", type=int, default=512)
    ap.add_argument("--bs", default="1,2,4,8,16,32")
    ap.add_argument("--pos0", type=int, default=10)
    ap.add_argument("--pos1", type=int, default=138)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--baseline-lib", default="", help="another build of libvsim_hip.so (the parent commit's)")
    ap.add_argument("--tree", default="?", help="what the tree is, for the header line")
    ap.add_argument("--out", default="")
    ap.add_argument("--one-step", type=int, default=0, help="warm-up, then one step of this B (profiler runs)")
    ap.add_argument("--baseline-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--lib", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.baseline_child:
        return baseline_child(a)

    from vsim_amd import hip
    arch_s, hp = hparams(a.config, a.layers)
    bs = [int(b) for b in a.bs.split(",")]
    dm = hip.Model.create(ARCH[arch_s], hp, n_ctx=a.n_ctx)
    dm.randomize(seed=1, std=0.02)
    dm.set_mode(hip.MODE_EXACT)
    dm.seq_reserve(max(bs + [a.one_step, 1]))
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    if a.one_step:
        B = a.one_step
        timed_steps(dm, B, 0, a.pos0)  # fills positions [0, pos0) and loads the kernels
        dm.decode_batch(list(range(B)), [a.pos0] * B, [5] * B, want_logits=False)
        dm.close()
        return
    import torch
    box = f"{socket.gethostname()} {torch.cuda.get_device_properties(0).gcnArchName}"
    n = a.pos1 - a.pos0
    say(f"# batch_bench: {a.config} shape, {hp['n_layer']} layers, random weights (std 0.02), exact mode, "
        f"n_ctx {a.n_ctx}; box {box}; tree at {a.tree}")
    say(f"# aggregate tok/s of decode_batch over positions {a.pos0}..{a.pos1 - 1} ({n} steps, ids only, positions "
        f"0..{a.pos0 - 1} discarded as warm-up), wall clock round calls that end in a stream synchronize; "
        f"median of {a.repeats} repeats, the two product paths alternating inside each repeat")
    res = {}
    for B in bs:
        runs = {2: [], 0: []}
        for r in range(a.repeats):
            for g in ((2, 0) if r % 2 == 0 else (0, 2)):
                hip.batch_set_gemm(g)
                runs[g].append(B * n / timed_steps(dm, B, a.pos0, a.pos1))
        res[B] = {g: statistics.median(v) for g, v in runs.items()}
        say(f"B {B:2d}: k_gemm_exact_rows {res[B][2]:9.1f} tok/s   GEMV jobs {res[B][0]:9.1f} tok/s   "
            f"rows/jobs {res[B][2] / res[B][0]:5.2f}   (runs {' '.join(f'{v:.0f}' for v in runs[2])} | "
            f"{' '.join(f'{v:.0f}' for v in runs[0])})")
    hip.batch_set_gemm(2)
    # where the time of one B = 16 step goes (event pairs round every launch; its own pass)
    if 16 in bs:
        timed_steps(dm, 16, 0, a.pos0)
        dm.set_profile(True)
        dm.decode_batch(list(range(16)), [a.pos0] * 16, [5] * 16, want_logits=False)
        ks = dm.profile_kernels()
        dm.set_profile(False)
        tot = sum(k["ms"] for k in ks)
        say(f"device time per kernel of one profiled B = 16 step at position {a.pos0} ({tot:.3f} ms, "
            f"{sum(k['launches'] for k in ks)} profiled launches):")
        for k in sorted(ks, key=lambda k: -k["ms"]):
            say(f"    {k['name']:<40s} {k['ms']:9.3f} ms  {100 * k['ms'] / tot:6.2f}%  {k['launches']:5d} launches")
        # k_gemm_exact_rows against its fp32 VALU bound: 2 lane-ops per weight and activation row
        # (gemm_exact.hip's accounting), 256 CUs x 4 SIMDs x 16 lanes at 2.4 GHz
        w = sum(k["bytes"] for k in ks if k["name"].startswith("k_gemm_exact_rows") or k["name"].startswith("lm_head"))
        ms = sum(k["ms"] for k in ks if k["name"].startswith("k_gemm_exact_rows") or k["name"].startswith("lm_head"))
        if ms > 0:
            ops = w / 0.625 * 16 * 2
            bound_ms = ops / (256 * 4 * 16 * 2.4e9) * 1e3
            say(f"    products: {w / 0.625 / 1e9:.3f} G weights x 16 rows x 2 lane-ops = {ops / 1e9:.1f} G lane-ops; "
                f"VALU bound {bound_ms:.3f} ms; measured {ms:.3f} ms: {100 * bound_ms / ms:.1f}% of the bound's rate")
    dm.close()
    base = {}
    base["this library"] = run_baseline(a, hip.LIB_PATH)
    if a.baseline_lib:
        base["parent commit"] = run_baseline(a, a.baseline_lib)
    for k, v in base.items():
        say(f"single stream, vsim_model_generate (hipGraph on), {k}: {v['tok_s']:.1f} tok/s "
            f"(runs {' '.join(f'{x:.1f}' for x in v['runs'])})")
    ref = base.get("parent commit", base["this library"])["tok_s"]
    first = {g: next((B for B in bs if res[B][g] > 1.05 * ref), None) for g in (2, 0)}
    say(f"smallest B whose aggregate rate exceeds the single-stream baseline by more than 5 %: "
        f"k_gemm_exact_rows {first[2]}, GEMV jobs {first[0]}")
    for B in (16, 32):
        if B in res:
            say(f"ratio to the baseline at B = {B}: k_gemm_exact_rows {res[B][2] / ref:.2f}x, GEMV jobs {res[B][0] / ref:.2f}x")
    say("k_gemm_exact_rows vs GEMV jobs by more than 5 %: " +
        ", ".join(f"B {B}: {'yes' if res[B][2] > 1.05 * res[B][0] else 'no'}" for B in bs))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
