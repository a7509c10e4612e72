#!/usr/bin/env python3
"""Single-stream decode rate of weight-only mode (VSIM_MODE_W4A16): its fused single-token step under
hipGraph against the general path it replaced.

A model of a benchmark config's shape with random weights.  Positions [0, pos0) are evaluated as a
prompt and discarded, then vsim_model_generate runs the steps at positions pos0 .. pos1-1: a host
clock round one call that ends in a stream synchronize, only the ids leaving the device.  The first
call of every setting (it captures the graph and loads the kernels) is discarded; the figure is the
median over the repeats.  Measured in one job:

  * this library, the step on, hipGraph on (what a user gets) and off;
  * this library, the step switched off (vsim_w4a16_set_step 0): the general path, one host round trip
    per token;
  * with --baseline-lib, another build of the library (the parent commit's) in a child process, which
    knows no switch and runs its general path;
  * beside them, for context: decode_batch_w4a16 at B = 1 and a fast-mode single stream;
  * one profiled step's per-kernel list, with the weight bytes per second of k_gemv_w4a16.

  python tools/w4a16_step_bench.py --out profiles/w4a16_step_bench.txt --baseline-lib PATH --tree "369093a + this change"
  python tools/w4a16_step_bench.py --config pythia-12b --out profiles/w4a16_step_bench.txt --append --baseline-lib PATH --tree "..."
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
MODES = {"exact": 0, "fast": 1, "w4a16": 2}


def hparams(cfg, layers):
    arch_s, hp = mg.CONFIGS[cfg]
    return arch_s, dict(n_vocab=hp.n_vocab, n_embd=hp.n_embd, n_head=hp.n_head, n_layer=layers or hp.n_layer,
                        n_rot=hp.n_rot, use_parallel_residual=hp.use_parallel_residual)


def child(a):
    """vsim_model_generate on the library at a.lib through plain ctypes (an older build has none of the
    new symbols, so vsim_amd.hip cannot bind it): prints one JSON line."""
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
    ck(L.vsim_model_set_mode(h, MODES[a.child_mode]), "set_mode")
    ck(L.vsim_model_set_graph(h, 1), "set_graph")
    prompt = np.arange(1, a.pos0 + 1, dtype=np.int32)
    ck(L.vsim_model_eval(h, 0, prompt.ctypes.data, a.pos0, None, None, None), "eval")
    n = a.pos1 - a.pos0
    out = np.zeros(n, np.int32)
    runs = []
    for r in range(a.repeats + 1):  # the first loads the kernels (and captures a graph where there is one)
        t0 = time.perf_counter()
        ck(L.vsim_model_generate(h, a.pos0, 7, n, out.ctypes.data), "generate")
        runs.append(n / (time.perf_counter() - t0))
    L.vsim_model_free(h)
    print(json.dumps({"tok_s": statistics.median(runs[1:]), "runs": runs[1:], "ids": [int(t) for t in out[:8]]}))


def run_child(a, lib, mode):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--lib", lib, "--child-mode", mode, "--config", a.config,
           "--layers", str(a.layers), "--n-ctx", str(a.n_ctx), "--pos0", str(a.pos0), "--pos1", str(a.pos1),
           "--repeats", str(a.repeats)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError(f"baseline child failed: {r.stdout[-1000:]}{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def attn_section(a, dm, hip, generate_rate, prompt, say, lines):
    """--attn both: the captured step with the attention switch at 1 (k_attn_w4a16_rows) and at 0
    (k_attn_decode_batch), the parent library, and the attention kernel's time in one profiled step."""
    res = {}
    for sw, name in ((1, "attn f16  "), (0, "attn exact")):
        hip.w4a16_set_attn(sw)
        res[sw] = generate_rate(hip.MODE_W4A16, 1, True)
        t, runs, ids, nk = res[sw]
        say(f"this library, {name}, step on, hipGraph on {t:8.1f} tok/s  ({1e3 / t:6.3f} ms per step, {nk} launches; "
            f"runs {' '.join(f'{v:.1f}' for v in runs)}; first ids {ids})")
    for sw in (1, 0):
        hip.w4a16_set_attn(sw)
        dm.eval(0, prompt, want_logits=False)
        dm.set_profile(True)
        dm.eval_argmax(a.pos0, 7)
        ks = dm.profile_kernels()
        dm.set_profile(False)
        tot = sum(k["ms"] for k in ks)
        say(f"one profiled step at position {a.pos0}, switch {sw}: " +
            ", ".join(f"{k['name']} {k['ms']:.3f} ms in {k['launches']} launches" for k in ks if k["name"].startswith("k_attn")) +
            f"; all kernels {tot:.3f} ms")
    hip.w4a16_set_attn(0)
    dm.close()
    if a.baseline_lib:
        base = run_child(a, a.baseline_lib, "w4a16")
        say(f"parent commit, w4a16                     {base['tok_s']:8.1f} tok/s  (runs {' '.join(f'{v:.1f}' for v in base['runs'])}; "
            f"first ids {base['ids']}; same ids as switch 0: {'yes' if base['ids'] == res[0][2] else 'NO'})")
        say(f"attn f16 / parent {res[1][0] / base['tok_s']:.3f}x   attn exact / parent {res[0][0] / base['tok_s']:.3f}x")
    if a.out:
        with open(a.out, "a" if a.append else "w") as f:
            f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="gpt-j-6B")
    ap.add_argument("--layers", type=int, default=0, help="0: the config's own depth")
    ap.add_argument("--n-ctx", type=int, default=512)
    ap.add_argument("--pos0", type=int, default=10)
    ap.add_argument("--pos1", type=int, default=138)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--baseline-lib", default="", help="another build of libvsim_hip.so (the parent commit's)")
    ap.add_argument("--tree", default="?", help="what the tree is, for the header line")
    ap.add_argument("--out", default="")
    ap.add_argument("--append", action="store_true", help="add to --out instead of replacing it (a second config)")
    ap.add_argument("--attn", default="exact", choices=["exact", "f16", "both"],
                    help="the mode's attention (vsim_w4a16_set_attn); both: the two settings and the parent side by side")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--child-mode", default="w4a16", help=argparse.SUPPRESS)
    ap.add_argument("--lib", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)

    import torch
    from vsim_amd import hip
    arch_s, hp = hparams(a.config, a.layers)
    n = a.pos1 - a.pos0
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    box = f"{socket.gethostname()} {torch.cuda.get_device_properties(0).gcnArchName}"
    say(f"# w4a16_step_bench: {a.config} shape, {hp['n_layer']} layers, random weights (std 0.02), n_ctx {a.n_ctx}; "
        f"box {box}; tree at {a.tree}")
    say(f"# single-stream tok/s of vsim_model_generate over positions {a.pos0}..{a.pos1 - 1} ({n} steps, ids only, "
        f"positions 0..{a.pos0 - 1} a discarded prompt), wall clock round one call that ends in a stream synchronize; "
        f"median of {a.repeats} repeats after one discarded call")
    dm = hip.Model.create(ARCH[arch_s], hp, n_ctx=a.n_ctx)
    dm.randomize(seed=1, std=0.02)
    prompt = list(range(1, a.pos0 + 1))

    def generate_rate(mode, step, graph):
        hip.w4a16_set_step(step)
        dm.set_mode(mode)
        dm.set_graph(graph)
        dm.eval(0, prompt, want_logits=False)
        runs, ids = [], None
        for r in range(a.repeats + 1):
            t0 = time.perf_counter()
            ids = dm.generate(a.pos0, 7, n)
            runs.append(n / (time.perf_counter() - t0))
        return statistics.median(runs[1:]), runs[1:], [int(t) for t in ids[:8]], dm.info()["kernels_per_eval"]

    if a.attn == "both":
        return attn_section(a, dm, hip, generate_rate, prompt, say, lines)
    hip.w4a16_set_attn(1 if a.attn == "f16" else 0)
    say(f"# the mode's attention (vsim_w4a16_set_attn): {a.attn}")
    res = {}
    for name, mode, step, graph in (("step on, hipGraph on", hip.MODE_W4A16, 1, True),
                                    ("step on, hipGraph off", hip.MODE_W4A16, 1, False),
                                    ("step off (general path)", hip.MODE_W4A16, 0, True),
                                    ("fast mode, hipGraph on", hip.MODE_FAST, 1, True)):
        res[name] = generate_rate(mode, step, graph)
        t, runs, ids, nk = res[name]
        say(f"this library, {name:<24s} {t:8.1f} tok/s  ({1e3 / t:6.3f} ms per step, {nk} launches; "
            f"runs {' '.join(f'{v:.1f}' for v in runs)}; first ids {ids})")
    on, off = res["step on, hipGraph on"], res["step off (general path)"]
    say(f"same ids with the step on and off: {'yes' if on[2] == off[2] == res['step on, hipGraph off'][2] else 'NO'}")
    # decode_batch_w4a16 at B = 1: the batched step's rate for one sequence
    hip.w4a16_set_step(1)
    dm.set_mode(hip.MODE_W4A16)
    dm.eval(0, prompt, want_logits=False)
    runs = []
    for r in range(a.repeats + 1):
        tok, t0 = 7, time.perf_counter()
        for p in range(a.pos0, a.pos1):
            _, nxt = dm.decode_batch_w4a16([0], [p], [tok], want_logits=False)
            tok = int(nxt[0])
        runs.append(n / (time.perf_counter() - t0))
    say(f"this library, decode_batch_w4a16 at B = 1 {statistics.median(runs[1:]):8.1f} tok/s  "
        f"(runs {' '.join(f'{v:.1f}' for v in runs[1:])})")
    # where one step's device time goes (event pairs round every launch: the eager form)
    dm.eval(0, prompt, want_logits=False)
    dm.set_profile(True)
    dm.eval_argmax(a.pos0, 7)
    ks = dm.profile_kernels()
    dm.set_profile(False)
    tot = sum(k["ms"] for k in ks)
    say(f"device time per kernel of one profiled step at position {a.pos0} ({tot:.3f} ms, "
        f"{sum(k['launches'] for k in ks)} profiled launches of {dm.info()['kernels_per_eval']} in the step):")
    for k in sorted(ks, key=lambda k: -k["ms"]):
        rate = f"  {k['bytes'] / k['ms'] / 1e9:6.2f} TB/s of weight bytes" if k["name"].startswith("k_gemv_w4a16") and k["ms"] > 0 else ""
        say(f"    {k['name']:<40s} {k['ms']:9.3f} ms  {100 * k['ms'] / tot:6.2f}%  {k['launches']:5d} launches{rate}")
    prod = [k for k in ks if k["name"].startswith("k_gemv_w4a16")]
    w, ms = sum(k["bytes"] for k in prod), sum(k["ms"] for k in prod)
    if ms > 0:
        say(f"    k_gemv_w4a16: {w / 1e9:.3f} GB of weights in {ms:.3f} ms: {w / ms / 1e9:.2f} TB/s of weight bytes")
    say(f"    wall clock of a step under hipGraph (above): {1e3 / on[0]:.3f} ms; profiled device time {tot:.3f} ms")
    dm.close()
    say(f"step on / step off, this library: {on[0] / off[0]:.2f}x")
    if a.baseline_lib:
        base = run_child(a, a.baseline_lib, "w4a16")
        say(f"parent commit, w4a16 (general path)    {base['tok_s']:8.1f} tok/s  (runs {' '.join(f'{v:.1f}' for v in base['runs'])}; "
            f"first ids {base['ids']}; same ids: {'yes' if base['ids'] == on[2] else 'NO'})")
        say(f"step on / parent commit: {on[0] / base['tok_s']:.2f}x")
    if a.out:
        with open(a.out, "a" if a.append else "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
