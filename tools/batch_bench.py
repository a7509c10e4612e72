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

--mode fast measures vsim_model_decode_batch_fast instead (vsim_batch_set_fast_gemm 2, k_gemm_fast_rows
at every B, against 0, one k_gemv_fast launch per row), with two baselines from --baseline-lib in child
processes: that library's exact vsim_model_decode_batch at the same B, and its fast-mode
vsim_model_generate; then one profiled B = 32 step.

  python tools/batch_bench.py --mode fast --out profiles/batch_fast_bench.txt --baseline-lib PATH --tree "..."

--sample measures vsim_model_decode_batch_sample in both modes (one sampler per row: top_k 20, top_p
0.95, temp 0.85, repeat_last_n 64, repeat_penalty 1.3, seeds 1..B) against the greedy step of the same
library and against what the parent commit offers for sampled batches: its decode_batch /
decode_batch_fast with the [B][n_vocab] logits copied out and vsim_sampler_sample_host per row, run
from --baseline-lib in a child process.

  python tools/batch_bench.py --sample --out profiles/batch_sample_bench.txt --baseline-lib PATH --tree "..."

--mode w4a16 measures vsim_model_decode_batch_w4a16 (weight-only products: Q4_0 weights, fp16
activation rows) beside decode_batch_fast and decode_batch of --baseline-lib in child processes, then
one profiled B = 32 step with the product's weight bytes per second, then one Model.score window of
--score-tokens tokens (default 2048; 0: none) in the new mode, in fast and in exact mode.

  python tools/batch_bench.py --mode w4a16 --bs 1,4,8,16,32 --out profiles/w4a16_bench.txt --baseline-lib PATH --tree "..."
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
    ck(L.vsim_model_set_mode(h, 1 if a.child_mode == "fast" else 0), "set_mode")
    ck(L.vsim_model_set_graph(h, 1), "set_graph")
    if a.child_kind == "batch":
        return baseline_child_batch(a, L, h, ck)
    if a.child_kind == "sample":
        return baseline_child_sample(a, L, h, ck)
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


def baseline_child_batch(a, L, h, ck):
    """vsim_model_decode_batch (exact mode) of the library at a.lib for every B of a.bs, timed as
    timed_steps does: prints one JSON line {B: {"tok_s", "runs"}}."""
    vp, ci = ctypes.c_void_p, ctypes.c_int
    L.vsim_model_seq_reserve.argtypes = [vp, ci]
    L.vsim_model_decode_batch.argtypes = [vp, ci, vp, vp, vp, vp, vp]
    step = L.vsim_model_decode_batch
    if a.child_mode == "fast":  # (the model is in fast mode: the fast step)
        step = L.vsim_model_decode_batch_fast
        step.argtypes = [vp, ci, vp, vp, vp, vp, vp]
    if a.child_mode == "w4a16":  # (the weight-only step, whatever the model's mode)
        step = L.vsim_model_decode_batch_w4a16
        step.argtypes = [vp, ci, vp, vp, vp, vp, vp]
    bs = [int(b) for b in a.bs.split(",")]
    ck(L.vsim_model_seq_reserve(h, max(bs)), "seq_reserve")
    n, res = a.pos1 - a.pos0, {}
    for B in bs:
        seqs, nxt, runs = np.arange(B, dtype=np.int32), np.zeros(B, np.int32), []
        for r in range(a.repeats):
            tok, t0 = np.arange(3, 3 + B, dtype=np.int32), 0.0
            for p in range(a.pos1):
                if p == a.pos0:
                    t0 = time.perf_counter()
                npst = np.full(B, p, np.int32)
                ck(step(h, B, seqs.ctypes.data, npst.ctypes.data, tok.ctypes.data, None, nxt.ctypes.data), "decode_batch")
                tok = nxt.copy()
            runs.append(B * n / (time.perf_counter() - t0))
        res[B] = {"tok_s": statistics.median(runs), "runs": runs}
    L.vsim_model_free(h)
    print(json.dumps(res))


SAMPLE_PARAMS = dict(top_k=20, top_p=0.95, temp=0.85, repeat_last_n=64, repeat_penalty=1.3)  # interface.py's


def baseline_child_sample(a, L, h, ck):
    """Sampled batches as the library at a.lib allows them without a sampled batched step: its
    decode_batch (exact) and decode_batch_fast with all B logits rows copied to the host, then
    vsim_sampler_sample_host per row.  Prints one JSON line {mode: {B: {"tok_s", "runs"}}}."""
    vp, ci = ctypes.c_void_p, ctypes.c_int
    L.vsim_model_seq_reserve.argtypes = [vp, ci]
    for f in (L.vsim_model_decode_batch, L.vsim_model_decode_batch_fast):
        f.argtypes = [vp, ci, vp, vp, vp, vp, vp]
    L.vsim_sampler_create.argtypes = [vp, ctypes.POINTER(vp)]
    L.vsim_sampler_sample_host.argtypes = [vp, vp, ci, vp]
    L.vsim_sampler_free.argtypes = [vp]
    bs = [int(b) for b in a.bs.split(",")]
    ck(L.vsim_model_seq_reserve(h, max(bs)), "seq_reserve")
    _, hp = hparams(a.config, a.layers)
    V, n, res = hp["n_vocab"], a.pos1 - a.pos0, {}

    class SP(ctypes.Structure):
        _fields_ = [("seed", ctypes.c_int32), ("top_k", ctypes.c_int32), ("repeat_last_n", ctypes.c_int32),
                    ("top_p", ctypes.c_float), ("temp", ctypes.c_float), ("repeat_penalty", ctypes.c_float)]

    for mode, step in (("exact", L.vsim_model_decode_batch), ("fast", L.vsim_model_decode_batch_fast)):
        res[mode] = {}
        for B in bs:
            seqs, lg, runs = np.arange(B, dtype=np.int32), np.zeros((B, V), np.float32), []
            for r in range(a.repeats):
                sm = []
                for b in range(B):
                    p, s = SP(1 + b, 20, 64, 0.95, 0.85, 1.3), vp()
                    ck(L.vsim_sampler_create(ctypes.byref(p), ctypes.byref(s)), "sampler_create")
                    sm.append(s)
                tok, t0, t = np.arange(3, 3 + B, dtype=np.int32), 0.0, ctypes.c_int32()
                for p in range(a.pos1):
                    if p == a.pos0:
                        t0 = time.perf_counter()
                    npst = np.full(B, p, np.int32)
                    ck(step(h, B, seqs.ctypes.data, npst.ctypes.data, tok.ctypes.data, lg.ctypes.data, None), "decode_batch")
                    for b in range(B):
                        ck(L.vsim_sampler_sample_host(sm[b], lg[b].ctypes.data, V, ctypes.byref(t)), "sample_host")
                        tok[b] = t.value
                runs.append(B * n / (time.perf_counter() - t0))
                for s in sm:
                    L.vsim_sampler_free(s)
            res[mode][B] = {"tok_s": statistics.median(runs), "runs": runs}
    L.vsim_model_free(h)
    print(json.dumps(res))


def timed_sample_steps(dm, hip, B, pos0, pos1, fast):
    """timed_steps through decode_batch_sample, a fresh sampler per row."""
    sm = [hip.Sampler(seed=1 + b, **SAMPLE_PARAMS) for b in range(B)]
    seqs, tok, t0 = list(range(B)), [3 + b for b in range(B)], 0.0
    for p in range(pos1):
        if p == pos0:
            t0 = time.perf_counter()
        tok = [int(t) for t in dm.decode_batch_sample(seqs, [p] * B, tok, sm, fast=fast)]
    dt = time.perf_counter() - t0
    assert all(s.stats() == {"device": pos1, "host": 0} for s in sm)
    return dt


def main_sample(a):
    """--sample: the sampled step against the greedy step and the parent's logits-out + host sampler."""
    from vsim_amd import hip
    import torch
    arch_s, hp = hparams(a.config, a.layers)
    bs = [int(b) for b in a.bs.split(",")]
    dm = hip.Model.create(ARCH[arch_s], hp, n_ctx=a.n_ctx)
    dm.randomize(seed=1, std=0.02)
    dm.set_mode(hip.MODE_EXACT)  # (decode_batch_fast and the fast sampled step serve a model in either mode)
    dm.seq_reserve(max(bs))
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    box = f"{socket.gethostname()} {torch.cuda.get_device_properties(0).gcnArchName}"
    n = a.pos1 - a.pos0
    say(f"# batch_bench --sample: {a.config} shape, {hp['n_layer']} layers, random weights (std 0.02), n_ctx {a.n_ctx}; "
        f"box {box}; tree at {a.tree}")
    say(f"# aggregate tok/s over positions {a.pos0}..{a.pos1 - 1} ({n} steps, positions 0..{a.pos0 - 1} discarded as warm-up), "
        f"wall clock round calls that end in a stream synchronize; median of {a.repeats} repeats, sampled and greedy "
        f"alternating inside each repeat; samplers: {SAMPLE_PARAMS}, seed 1 + row")
    res = {}
    for mode, fast in (("exact", False), ("fast", True)):
        res[mode] = {}
        for B in bs:
            runs = {"sampled": [], "greedy": []}
            for r in range(a.repeats):
                for v in (("sampled", "greedy") if r % 2 == 0 else ("greedy", "sampled")):
                    dt = timed_sample_steps(dm, hip, B, a.pos0, a.pos1, fast) if v == "sampled" else \
                        timed_steps(dm, B, a.pos0, a.pos1, fast=fast)
                    runs[v].append(B * n / dt)
            res[mode][B] = {v: statistics.median(x) for v, x in runs.items()}
            r_ = res[mode][B]
            say(f"{mode:5s} B {B:2d}: decode_batch_sample {r_['sampled']:9.1f} tok/s   greedy step {r_['greedy']:9.1f} tok/s   "
                f"sampled/greedy {r_['sampled'] / r_['greedy']:5.3f}   step {1e3 * B / r_['sampled']:7.3f} ms against "
                f"{1e3 * B / r_['greedy']:7.3f} ms   (runs {' '.join(f'{v:.0f}' for v in runs['sampled'])} | "
                f"{' '.join(f'{v:.0f}' for v in runs['greedy'])})")
    dm.close()
    lib = a.baseline_lib or hip.LIB_PATH
    who = "parent commit" if a.baseline_lib else "this library"
    base = run_baseline(a, lib, "sample")
    ok = True
    for mode in ("exact", "fast"):
        for B in bs:
            b_ = base[mode][str(B)]
            ratio = res[mode][B]["sampled"] / b_["tok_s"]
            if B >= 4 and ratio <= 1.0:
                ok = False
            say(f"{mode:5s} B {B:2d}: logits out + sample_host per row, {who}: {b_['tok_s']:9.1f} tok/s (step "
                f"{1e3 * B / b_['tok_s']:7.3f} ms)   decode_batch_sample / that {ratio:5.2f}   "
                f"(runs {' '.join(f'{x:.0f}' for x in b_['runs'])})")
    for mode in ("exact", "fast"):
        if 32 in res[mode]:
            r_, b_ = res[mode][32], base[mode]["32"]
            say(f"{mode} B = 32: sampling costs {1e3 * 32 / r_['sampled'] - 1e3 * 32 / r_['greedy']:+.3f} ms per step over the "
                f"greedy step; the host sampler path costs {1e3 * 32 / b_['tok_s'] - 1e3 * 32 / r_['greedy']:+.3f} ms over it")
    say(f"decode_batch_sample faster than logits out + sample_host at every B >= 4, both modes: {'yes' if ok else 'NO'}")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def run_baseline(a, lib, kind="generate", mode="exact"):
    cmd = [sys.executable, os.path.abspath(__file__), "--baseline-child", "--lib", lib, "--config", a.config,
           "--layers", str(a.layers), "--n-ctx", str(a.n_ctx), "--pos0", str(a.pos0), "--pos1", str(a.pos1),
           "--repeats", str(a.repeats), "--child-kind", kind, "--child-mode", mode, "--bs", a.bs]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError(f"baseline run on {lib} failed:\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def timed_steps(dm, B, pos0, pos1, timed=True, fast=False, w4a16=False):
    """Positions [0, pos1) of B sequences in slots 0..B-1; returns the seconds of [pos0, pos1)."""
    seqs = list(range(B))
    tok = [3 + b for b in range(B)]
    t0 = 0.0
    step = dm.decode_batch_w4a16 if w4a16 else dm.decode_batch_fast if fast else dm.decode_batch
    for p in range(pos1):
        if p == pos0:
            t0 = time.perf_counter()
        _, nxt = step(seqs, [p] * B, tok, want_logits=False)
        tok = [int(t) for t in nxt]
    return time.perf_counter() - t0


def main_fast(a):
    """--mode fast: decode_batch_fast under both product paths, the parent library's exact batch and
    fast single stream, and where one B = 32 step's time goes."""
    from vsim_amd import hip
    import torch
    arch_s, hp = hparams(a.config, a.layers)
    bs = [int(b) for b in a.bs.split(",")]
    dm = hip.Model.create(ARCH[arch_s], hp, n_ctx=a.n_ctx)
    dm.randomize(seed=1, std=0.02)
    dm.set_mode(hip.MODE_FAST)
    dm.seq_reserve(max(bs + [32]))
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    box = f"{socket.gethostname()} {torch.cuda.get_device_properties(0).gcnArchName}"
    n = a.pos1 - a.pos0
    say(f"# batch_bench --mode fast: {a.config} shape, {hp['n_layer']} layers, random weights (std 0.02), "
        f"n_ctx {a.n_ctx}; box {box}; tree at {a.tree}")
    say(f"# aggregate tok/s of decode_batch_fast over positions {a.pos0}..{a.pos1 - 1} ({n} steps, ids only, "
        f"positions 0..{a.pos0 - 1} discarded as warm-up), wall clock round calls that end in a stream synchronize; "
        f"median of {a.repeats} repeats, the two product paths alternating inside each repeat")
    res = {}
    for B in bs:
        runs = {2: [], 0: []}
        for r in range(a.repeats):
            for g in ((2, 0) if r % 2 == 0 else (0, 2)):
                hip.batch_set_fast_gemm(g)
                runs[g].append(B * n / timed_steps(dm, B, a.pos0, a.pos1, fast=True))
        res[B] = {g: statistics.median(v) for g, v in runs.items()}
        say(f"B {B:2d}: k_gemm_fast_rows {res[B][2]:9.1f} tok/s   k_gemv_fast per row {res[B][0]:9.1f} tok/s   "
            f"rows/per-row {res[B][2] / res[B][0]:5.2f}   (runs {' '.join(f'{v:.0f}' for v in runs[2])} | "
            f"{' '.join(f'{v:.0f}' for v in runs[0])})")
    hip.batch_set_fast_gemm(2)
    # where the time of one B = 32 step goes (event pairs round every launch; its own pass)
    timed_steps(dm, 32, 0, a.pos0, fast=True)
    dm.set_profile(True)
    dm.decode_batch_fast(list(range(32)), [a.pos0] * 32, [5] * 32, want_logits=False)
    ks = dm.profile_kernels()
    dm.set_profile(False)
    tot = sum(k["ms"] for k in ks)
    say(f"device time per kernel of one profiled B = 32 step at position {a.pos0} ({tot:.3f} ms, "
        f"{sum(k['launches'] for k in ks)} profiled launches of {dm.info()['kernels_per_eval']} in the step; "
        f"the unprofiled ones are the LayerNorm, quantize, GELU, join and embedding kernels):")
    for k in sorted(ks, key=lambda k: -k["ms"]):
        say(f"    {k['name']:<40s} {k['ms']:9.3f} ms  {100 * k['ms'] / tot:6.2f}%  {k['launches']:5d} launches")
    prod = [k for k in ks if k["name"].startswith("k_gemm_fast_rows") or k["name"].startswith("lm_head")]
    w, ms = sum(k["bytes"] for k in prod), sum(k["ms"] for k in prod)
    if ms > 0:
        say(f"    products: {w / 1e9:.3f} GB of weights in {ms:.3f} ms: {w / ms / 1e9:.2f} TB/s")
    step_ms = 32e3 / res[32][2] if 32 in res else 0.0
    if step_ms:
        say(f"    wall clock of a B = 32 step (above): {step_ms:.3f} ms; profiled device time {tot:.3f} ms; the rest "
            f"({step_ms - tot:.3f} ms) is the unprofiled kernels, launch gaps (no hipGraph) and the host round trip")
    dm.close()
    lib = a.baseline_lib or hip.LIB_PATH
    who = "parent commit" if a.baseline_lib else "this library"
    eb = {int(k): v for k, v in run_baseline(a, lib, "batch", "exact").items()}
    fs = run_baseline(a, lib, "generate", "fast")
    for B in bs:
        say(f"exact vsim_model_decode_batch, {who}, B {B:2d}: {eb[B]['tok_s']:9.1f} tok/s   fast/exact "
            f"{res[B][2] / eb[B]['tok_s']:5.2f}   (runs {' '.join(f'{x:.0f}' for x in eb[B]['runs'])})")
    say(f"fast single stream, vsim_model_generate (hipGraph on), {who}: {fs['tok_s']:.1f} tok/s "
        f"(runs {' '.join(f'{x:.1f}' for x in fs['runs'])})")
    say("k_gemm_fast_rows vs k_gemv_fast per row by more than 5 %: " +
        ", ".join(f"B {B}: {'yes' if res[B][2] > 1.05 * res[B][0] else 'no'}" for B in bs))
    first = next((B for B in bs if res[B][2] > 1.05 * fs["tok_s"]), None)
    say(f"smallest B whose aggregate rate exceeds the fast single stream by more than 5 %: {first}")
    if 32 in res:
        say(f"B = 32 condition: k_gemm_fast_rows {res[32][2]:.1f} tok/s against per-row {res[32][0]:.1f} "
            f"({res[32][2] / res[32][0]:.2f}x) and the exact batch {eb[32]['tok_s']:.1f} ({res[32][2] / eb[32]['tok_s']:.2f}x): "
            f"{'holds' if res[32][2] > 1.05 * max(res[32][0], eb[32]['tok_s']) else 'FAILS'}")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def main_w4a16(a):
    """--mode w4a16: decode_batch_w4a16 beside the baseline library's fast and exact batched steps,
    where one B = 32 step's time goes, and one scoring window in the three modes."""
    from vsim_amd import hip
    import torch
    arch_s, hp = hparams(a.config, a.layers)
    bs = [int(b) for b in a.bs.split(",")]
    n_ctx = a.n_ctx
    dm = hip.Model.create(ARCH[arch_s], hp, n_ctx=n_ctx)
    dm.randomize(seed=1, std=0.02)
    dm.set_mode(hip.MODE_W4A16)
    dm.seq_reserve(max(bs + [32]))
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    box = f"{socket.gethostname()} {torch.cuda.get_device_properties(0).gcnArchName}"
    n = a.pos1 - a.pos0
    say(f"# batch_bench --mode w4a16: {a.config} shape, {hp['n_layer']} layers, random weights (std 0.02), "
        f"n_ctx {n_ctx}; box {box}; tree at {a.tree}")
    say(f"# aggregate tok/s of decode_batch_w4a16 over positions {a.pos0}..{a.pos1 - 1} ({n} steps, ids only, "
        f"positions 0..{a.pos0 - 1} discarded as warm-up), wall clock round calls that end in a stream synchronize; "
        f"median of {a.repeats} repeats")
    res = {}
    if a.attn == "both":
        return main_w4a16_attn(a, dm, hip, bs, n, say, lines)
    hip.w4a16_set_attn(1 if a.attn == "f16" else 0)
    say(f"# the mode's attention (vsim_w4a16_set_attn): {a.attn}")
    for B in bs:
        runs = [B * n / timed_steps(dm, B, a.pos0, a.pos1, w4a16=True) for _ in range(a.repeats)]
        res[B] = statistics.median(runs)
        say(f"B {B:2d}: decode_batch_w4a16 {res[B]:9.1f} tok/s   (runs {' '.join(f'{v:.0f}' for v in runs)})")
    timed_steps(dm, 32, 0, a.pos0, w4a16=True)
    dm.set_profile(True)
    dm.decode_batch_w4a16(list(range(32)), [a.pos0] * 32, [5] * 32, want_logits=False)
    ks = dm.profile_kernels()
    dm.set_profile(False)
    tot = sum(k["ms"] for k in ks)
    say(f"device time per kernel of one profiled B = 32 step at position {a.pos0} ({tot:.3f} ms, "
        f"{sum(k['launches'] for k in ks)} profiled launches of {dm.info()['kernels_per_eval']} in the step):")
    for k in sorted(ks, key=lambda k: -k["ms"]):
        say(f"    {k['name']:<40s} {k['ms']:9.3f} ms  {100 * k['ms'] / tot:6.2f}%  {k['launches']:5d} launches")
    prod = [k for k in ks if k["name"].startswith("k_gemm_w4a16_rows") or k["name"].startswith("lm_head")]
    w, ms = sum(k["bytes"] for k in prod), sum(k["ms"] for k in prod)
    if ms > 0:
        say(f"    products: {w / 1e9:.3f} GB of weights in {ms:.3f} ms: {w / ms / 1e9:.2f} TB/s of weight bytes at B = 32")
    if 32 in res:
        say(f"    wall clock of a B = 32 step (above): {32e3 / res[32]:.3f} ms; profiled device time {tot:.3f} ms")
    dm.close()
    if a.score_tokens:  # (a model of its own: one slot at the window's length)
        dm = hip.Model.create(ARCH[arch_s], hp, n_ctx=a.score_tokens)
        dm.randomize(seed=1, std=0.02)
        toks = [int(t) for t in np.random.default_rng(1).integers(0, hp["n_vocab"], a.score_tokens)]
        for name, mode in (("w4a16", hip.MODE_W4A16), ("fast", hip.MODE_FAST), ("exact", hip.MODE_EXACT)):
            dm.set_mode(mode)
            dm.reserve(a.score_tokens)
            dm.score(0, toks[:64])  # (loads the kernels)
            t0 = time.perf_counter()
            lp, _ = dm.score(0, toks)
            dt = time.perf_counter() - t0
            say(f"Model.score, one window of {a.score_tokens} tokens, {name:5s}: {dt:8.3f} s  ({a.score_tokens / dt:8.1f} tok/s, "
                f"mean logprob {float(np.mean(lp[:-1])):.4f})")
        dm.close()
    lib = a.baseline_lib or hip.LIB_PATH
    who = "parent commit" if a.baseline_lib else "this library"
    fb = {int(k): v for k, v in run_baseline(a, lib, "batch", "fast").items()}
    eb = {int(k): v for k, v in run_baseline(a, lib, "batch", "exact").items()}
    for B in bs:
        say(f"{who}, B {B:2d}: decode_batch_fast {fb[B]['tok_s']:9.1f} tok/s   decode_batch {eb[B]['tok_s']:9.1f} tok/s   "
            f"w4a16/fast {res[B] / fb[B]['tok_s']:5.2f}   w4a16/exact {res[B] / eb[B]['tok_s']:5.2f}")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def main_w4a16_attn(a, dm, hip, bs, n, say, lines):
    """--mode w4a16 --attn both: decode_batch_w4a16 with the attention switch at 1 (k_attn_w4a16_rows)
    and at 0 (k_attn_decode_batch), the parent library's step, and the attention kernel's time in one
    profiled step of each setting."""
    res = {}
    for sw, name in ((1, "attn f16  "), (0, "attn exact")):
        hip.w4a16_set_attn(sw)
        for B in bs:
            timed_steps(dm, B, a.pos0, a.pos1, w4a16=True)  # (a warm pass)
            runs = [B * n / timed_steps(dm, B, a.pos0, a.pos1, w4a16=True) for _ in range(a.repeats)]
            res[sw, B] = statistics.median(runs)
            say(f"B {B:2d}, {name}: decode_batch_w4a16 {res[sw, B]:9.1f} tok/s   (runs {' '.join(f'{v:.0f}' for v in runs)})")
    for sw in (1, 0):
        hip.w4a16_set_attn(sw)
        for B in bs:
            timed_steps(dm, B, 0, a.pos0, w4a16=True)
            dm.set_profile(True)
            dm.decode_batch_w4a16(list(range(B)), [a.pos0] * B, [5] * B, want_logits=False)
            ks = dm.profile_kernels()
            dm.set_profile(False)
            tot = sum(k["ms"] for k in ks)
            at = [k for k in ks if k["name"].startswith("k_attn")]
            say(f"one profiled step, B {B:2d}, position {a.pos0}, switch {sw}: " +
                ", ".join(f"{k['name']} {k['ms']:.3f} ms in {k['launches']} launches" for k in at) + f"; all kernels {tot:.3f} ms")
    hip.w4a16_set_attn(0)
    dm.close()
    if a.baseline_lib:
        pb = {int(k): v for k, v in run_baseline(a, a.baseline_lib, "batch", "w4a16").items()}
        for B in bs:
            say(f"parent commit, B {B:2d}: decode_batch_w4a16 {pb[B]['tok_s']:9.1f} tok/s   "
                f"(runs {' '.join(f'{v:.0f}' for v in pb[B]['runs'])})   f16 / parent {res[1, B] / pb[B]['tok_s']:5.2f}   "
                f"exact / parent {res[0, B] / pb[B]['tok_s']:5.2f}")
    if a.out:
        with open(a.out, "a" if a.append else "w") as f:
            f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="exact", choices=["exact", "fast", "w4a16"])
    ap.add_argument("--attn", default="exact", choices=["exact", "f16", "both"],
                    help="--mode w4a16: the mode's attention (vsim_w4a16_set_attn); both: the two settings side by side")
    ap.add_argument("--append", action="store_true", help="--attn both: add to --out instead of replacing it")
    ap.add_argument("--score-tokens", type=int, default=2048, help="--mode w4a16: the scoring window (0: none)")
    ap.add_argument("--sample", action="store_true", help="the sampled step, both modes (see the module text)")
    ap.add_argument("--child-kind", default="generate", help=argparse.SUPPRESS)
    ap.add_argument("--child-mode", default="exact", help=argparse.SUPPRESS)
    ap.add_argument("--config", default="gpt-j-6B")
    ap.add_argument("--layers", type=int, default=0, help="0: the config's own depth")
    ap.add_argument("--n-ctx", type=int, default=512)
    ap.add_argument("--bs", default="", help="default 1,2,4,8,16,32 (--mode fast: 1,2,4,8,12,16,24,32)")
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
    a.bs = a.bs or ("1,4,8,16,32" if a.sample else "1,2,4,8,12,16,24,32" if a.mode == "fast" else "1,2,4,8,16,32")
    if a.baseline_child:
        return baseline_child(a)
    if a.sample:
        return main_sample(a)
    if a.mode == "fast":
        return main_fast(a)
    if a.mode == "w4a16":
        return main_w4a16(a)

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
