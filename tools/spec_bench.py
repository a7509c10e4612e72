#!/usr/bin/env python3
"""Runs of tokens per slot (vsim_model_decode_runs) and greedy speculative decoding, measured.

A model of a benchmark config's shape with random weights, n_ctx 2048.  One prompt is evaluated
into slot 1 and forked into the other slots (finite cache rows everywhere a step reads).  Every
figure is a host clock round calls that end in a stream synchronize, ids only; the first call of a
setting is discarded and the figure is the median of the repeats.  In one job:

  (a) step time of decode_runs at one run of 1 / 2 / 4 / 8 / 16 / 32 rows in the three modes, against
      decode_batch* at that many distinct slots and against the fused single-token step
      (Model.generate), at positions 10.. and near 1,900;
  (b) generate_speculative tok/s in weight-only mode with ReplayDrafter at acceptance 0 / 0.5 / 0.8 /
      1.0 (each drafted place right with that probability) and k = 3 / 7 / 15, against Model.generate
      of this library and, with --baseline-lib, of another build (the parent commit's) in a child process;
  (c) self-speculation: fast-mode drafts of the same model object, weight-only verify, with the
      acceptance observed.  Random weights: that acceptance says nothing about real text.

  python tools/spec_bench.py --out profiles/spec_bench.txt --baseline-lib PATH --tree "50a601e + this change"
  python tools/spec_bench.py --config pythia-12b --out profiles/spec_bench.txt --append --baseline-lib PATH --tree "..."
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
ROWS = (1, 2, 4, 8, 16, 32)


def hparams(cfg, layers):
    arch_s, hp = mg.CONFIGS[cfg]
    return arch_s, dict(n_vocab=hp.n_vocab, n_embd=hp.n_embd, n_head=hp.n_head, n_layer=layers or hp.n_layer,
                        n_rot=hp.n_rot, use_parallel_residual=hp.use_parallel_residual)


def child(a):
    """vsim_model_generate in weight-only mode on the library at a.lib through plain ctypes (an older
    build has none of the new symbols): prints one JSON line."""
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
    h = vp()
    assert L.vsim_model_create(ARCH[arch_s], hpc, a.n_ctx, 0, 0, -1, ctypes.byref(h)) == 0
    assert L.vsim_model_randomize(h, 1, 0.02) == 0
    assert L.vsim_model_set_mode(h, 2) == 0
    assert L.vsim_model_set_graph(h, 1) == 0
    prompt = np.arange(1, a.pos0 + 1, dtype=np.int32)
    assert L.vsim_model_eval(h, 0, prompt.ctypes.data, a.pos0, None, None, None) == 0
    out = np.zeros(a.n_predict, np.int32)
    runs = []
    for r in range(a.repeats + 1):
        t0 = time.perf_counter()
        assert L.vsim_model_generate(h, a.pos0, 7, a.n_predict, out.ctypes.data) == 0
        runs.append(a.n_predict / (time.perf_counter() - t0))
    L.vsim_model_free(h)
    print(json.dumps({"tok_s": statistics.median(runs[1:]), "ids": [int(t) for t in out]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="gpt-j-6B")
    ap.add_argument("--layers", type=int, default=0, help="0: the config's own depth")
    ap.add_argument("--n-ctx", type=int, default=2048)
    ap.add_argument("--pos0", type=int, default=10)
    ap.add_argument("--pos-late", type=int, default=1900)
    ap.add_argument("--n-predict", type=int, default=96)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--baseline-lib", default="", help="another build of libvsim_hip.so (the parent commit's)")
    ap.add_argument("--tree", default="?", help="what the tree is, for the header line")
    ap.add_argument("--out", default="")
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--lib", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)

    import torch
    from vsim_amd import hip
    from vsim_amd.spec import ModelDrafter, ReplayDrafter, generate_speculative
    arch_s, hp = hparams(a.config, a.layers)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    written = [0]

    def flush():  # (after every section, so a job that is cut short leaves what it measured)
        if a.out and written[0] < len(lines):
            with open(a.out, "a" if a.append or written[0] else "w") as f:
                f.write("\n".join(lines[written[0]:]) + "\n")
            written[0] = len(lines)

    box = f"{socket.gethostname()} {torch.cuda.get_device_properties(0).gcnArchName}"
    say(f"# spec_bench: {a.config} shape, {hp['n_layer']} layers, random weights (std 0.02), n_ctx {a.n_ctx}; box {box}; "
        f"tree at {a.tree}")
    say(f"# host clock round calls that end in a stream synchronize, ids only; median of {a.repeats} after one discarded call")
    dm = hip.Model.create(ARCH[arch_s], hp, n_ctx=a.n_ctx)
    dm.randomize(seed=1, std=0.02)
    dm.seq_reserve(34)
    dm.set_graph(True)
    dm.set_mode(hip.MODE_W4A16)
    late = a.pos_late
    fill = [1 + i % 1000 for i in range(late + 33)]
    dm.eval_seq(1, 0, fill, want_logits=False)
    for s in [0] + list(range(2, 34)):
        dm.seq_copy(s, 1, len(fill))

    def med(fn):
        ts = []
        for r in range(a.repeats + 1):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts[1:])

    modes = (("exact", hip.MODE_EXACT, "decode_batch"), ("fast", hip.MODE_FAST, "decode_batch_fast"),
             ("w4a16", hip.MODE_W4A16, "decode_batch_w4a16"))
    say("(a) step time, ms: decode_runs at one run of n rows on one slot | decode_batch* at n distinct slots | their ratio")
    single = {}
    for mname, mode, batch_name in modes:
        dm.set_mode(mode)
        for pos in (a.pos0, late):
            single[mname, pos] = med(lambda: dm.generate(pos, 7, 16)) / 16
            cells = []
            for n in ROWS:
                toks = [7 + i for i in range(n)]
                tr = med(lambda: dm.decode_runs([1], [pos], [toks], mode, want_logits=False))
                tb = med(lambda: getattr(dm, batch_name)(list(range(1, n + 1)), [pos] * n, toks, want_logits=False))
                cells.append(f"n={n}: {tr:7.3f} | {tb:7.3f} | {tr / tb:5.3f}")
                if mname == "w4a16":
                    single[mname, pos, n] = tr
            say(f"  {mname:<5s} position {pos:4d}: fused single-token step {single[mname, pos]:6.3f} ms per token;  " + ";  ".join(cells))
    for pos in (a.pos0, late):
        s1 = single["w4a16", pos]
        say(f"  w4a16 position {pos}: break-even accepted tokens per verify step (run step / single step): " +
            ", ".join(f"n={n}: {single['w4a16', pos, n] / s1:.2f}" for n in ROWS))
    flush()

    # (b) the loop, weight-only mode
    dm.set_mode(hip.MODE_W4A16)
    prompt = list(range(1, a.pos0 + 2))   # pos0 + 1 tokens: the first verify step runs at pos0
    dm.eval(0, prompt[:-1], want_logits=False)
    stream = [int(t) for t in dm.generate(a.pos0, prompt[-1], a.n_predict)]
    gen = a.n_predict / (med(lambda: dm.generate(a.pos0, prompt[-1], a.n_predict)) / 1e3)
    say(f"(b) generate_speculative, w4a16, {a.n_predict} tokens from position {a.pos0}; Model.generate of this library: {gen:.1f} tok/s")
    base = None
    if a.baseline_lib:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--lib", a.baseline_lib, "--config", a.config, "--layers",
               str(a.layers), "--n-ctx", str(a.n_ctx), "--pos0", str(a.pos0), "--n-predict", str(a.n_predict), "--repeats",
               str(a.repeats)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise RuntimeError(f"baseline child failed: {r.stdout[-500:]}{r.stderr[-1500:]}")
        base = json.loads(r.stdout.strip().splitlines()[-1])
        # the child's prompt is 1..pos0 and its first token 7; compare rates, not ids
        say(f"    parent commit's Model.generate (w4a16, child process): {base['tok_s']:.1f} tok/s")
    ref = base["tok_s"] if base else gen
    for p in (0.0, 0.5, 0.8, 1.0):
        rng = np.random.default_rng(7)
        wrong = frozenset(i for i in range(a.n_predict) if rng.random() >= p)
        cells = []
        for k in (3, 7, 15):
            res = {}

            def go():
                res["r"] = generate_speculative(dm, prompt, a.n_predict, ReplayDrafter(stream, wrong=wrong,
                                                                                       n_vocab=hp["n_vocab"]), k=k, slot=1)
            ms = med(go)
            ids, st = res["r"]
            ok = "same ids" if ids == stream else "IDS DIFFER"
            cells.append(f"k={k}: {a.n_predict / ms * 1e3:7.1f} tok/s ({a.n_predict / ms * 1e3 / ref:4.2f}x, {st['steps']} steps, "
                         f"{st['accepted']}/{st['drafted']} accepted, {ok})")
        say(f"    acceptance {p:3.1f}: " + ";  ".join(cells))
    flush()

    # (c) self-speculation
    say("(c) self-speculation: fast-mode drafts of the same model object on slot 0, w4a16 verify on slot 1 "
        "(random weights: this acceptance says nothing about real text)")
    for k in (3, 7):
        res = {}

        def go():
            res["r"] = generate_speculative(dm, prompt, a.n_predict, ModelDrafter(dm, mode=hip.MODE_FAST, back=hip.MODE_W4A16),
                                            k=k, slot=1)
        ms = med(go)
        ids, st = res["r"]
        say(f"    k={k}: {a.n_predict / ms * 1e3:7.1f} tok/s ({a.n_predict / ms * 1e3 / ref:4.2f}x), {st['steps']} steps, "
            f"{st['accepted']}/{st['drafted']} drafted tokens accepted ({st['accepted'] / max(st['drafted'], 1):.2f}), "
            f"{'same ids' if ids == stream else 'IDS DIFFER'}")
    dm.close()
    flush()


if __name__ == "__main__":
    main()
