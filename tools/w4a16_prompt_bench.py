#!/usr/bin/env python3
"""Prompt rate of weight-only mode (VSIM_MODE_W4A16): k_gemm_w4a16_tile, one launch per product,
against k_gemm_w4a16_rows on chunks of 32 rows (vsim_w4a16_set_tile_gemm 0, and the parent commit).

A model of a benchmark config's shape with random weights.  Every figure is a wall clock round one
call that ends in a stream synchronize; a warm call first, then the median of --repeats.  In one job:

  * Model.eval of an N-token prompt (default 2,048): this library with the switch at 1 and at 0, and
    with --baseline-lib another build of the library (the parent commit's) in a child process, which
    knows no switch; a hash of the logits from each;
  * one N-token Model.score window, the same three;
  * prompt evals at N = 33 .. 512 with the switch at 2 against 0: the source of W4A16_TILE_MIN_N
    (product_plan.hpp);
  * the product alone through the two op entries at n = 2,048 on three shapes;
  * one profiled eval's per-kernel list (profiled once; profiled times are not compared with the
    un-profiled ones above).

  python tools/w4a16_prompt_bench.py --out profiles/w4a16_prompt_bench.txt --baseline-lib PATH --tree "55af294 + this change"
  python tools/w4a16_prompt_bench.py --config pythia-12b --out profiles/w4a16_prompt_bench.txt --append --baseline-lib PATH --tree "..."
"""
import argparse
import ctypes
import hashlib
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
MODE_W4A16 = 2
THRESHOLD_NS = (33, 64, 96, 128, 256, 512)
OP_SHAPES = ((4096, 4096), (16384, 4096), (4096, 16384))


def hparams(cfg, layers):
    arch_s, hp = mg.CONFIGS[cfg]
    return arch_s, dict(n_vocab=hp.n_vocab, n_embd=hp.n_embd, n_head=hp.n_head, n_layer=layers or hp.n_layer,
                        n_rot=hp.n_rot, use_parallel_residual=hp.use_parallel_residual)


def tokens_of(n, n_vocab):
    return (np.arange(n, dtype=np.int64) * 7919 % n_vocab).astype(np.int32)


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def timed(call, repeats):
    """A warm call, then `repeats` timed ones: (median s, runs, the last result)."""
    out = call()
    runs = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = call()
        runs.append(time.perf_counter() - t0)
    return statistics.median(runs), runs, out


def child(a):
    """The prompt eval and the score window on the library at a.lib through plain ctypes (an older
    build has none of the new symbols, so vsim_amd.hip cannot bind it): prints one JSON line."""
    L = ctypes.CDLL(a.lib, mode=ctypes.RTLD_GLOBAL)
    arch_s, hp = hparams(a.config, a.layers)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    hpc = (ctypes.c_int32 * 6)(hp["n_vocab"], hp["n_embd"], hp["n_head"], hp["n_layer"], hp["n_rot"],
                               hp["use_parallel_residual"])
    L.vsim_model_create.argtypes = [ci, vp, ci, ci, ci, ci, ctypes.POINTER(vp)]
    L.vsim_model_randomize.argtypes = [vp, ctypes.c_uint64, ctypes.c_float]
    L.vsim_model_set_mode.argtypes = [vp, ci]
    L.vsim_model_eval.argtypes = [vp, ci, vp, ci, vp, vp, vp]
    L.vsim_model_eval_score.argtypes = [vp, ci, vp, ci, vp, vp, vp, vp, vp]
    L.vsim_model_free.argtypes = [vp]
    L.vsim_last_error.restype = ctypes.c_char_p
    h = vp()

    def ck(rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed ({rc}): {L.vsim_last_error().decode(errors='replace')}")

    ck(L.vsim_model_create(ARCH[arch_s], hpc, a.n_ctx, 0, 0, -1, ctypes.byref(h)), "create")
    ck(L.vsim_model_randomize(h, 1, 0.02), "randomize")
    ck(L.vsim_model_set_mode(h, MODE_W4A16), "set_mode")
    N = a.n
    tok = tokens_of(N, hp["n_vocab"])
    tgt = np.concatenate([tok[1:], np.array([-1], np.int32)])
    lg = np.zeros(hp["n_vocab"], np.float32)
    lp, am = np.zeros(N, np.float64), np.zeros(N, np.int32)

    def ev():
        ck(L.vsim_model_eval(h, 0, tok.ctypes.data, N, None, None, lg.ctypes.data), "eval")
        return lg.copy()

    def sc():
        ck(L.vsim_model_eval_score(h, 0, tok.ctypes.data, N, None, tgt.ctypes.data, lp.ctypes.data, am.ctypes.data, None),
           "eval_score")
        return lp.copy()

    e_med, e_runs, e_out = timed(ev, a.repeats)
    s_med, s_runs, s_out = timed(sc, a.repeats)
    L.vsim_model_free(h)
    print(json.dumps({"eval": e_med, "eval_runs": e_runs, "eval_hash": digest(e_out), "score": s_med, "score_runs": s_runs,
                      "score_hash": digest(s_out)}))


def run_child(a, lib):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--lib", lib, "--config", a.config, "--layers", str(a.layers),
           "--n-ctx", str(a.n_ctx), "--n", str(a.n), "--repeats", str(a.repeats)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError(f"baseline child failed: {r.stdout[-1000:]}{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def op_bench(say, hip, torch, repeats):
    """The product alone at n = 2,048 through the two op entries (the rows entry in 64 calls of 32 rows)."""
    n = 2048
    say(f"the product alone at n = {n} (random Q4_0 weight and operand; 5 products per timed call; median of {repeats} after a warm call):")
    rng = np.random.default_rng(3)
    for M, K in OP_SHAPES:
        w = torch.from_numpy(rng.integers(0, 256, hip.q4_bytes(M, K), dtype=np.uint8)).cuda()
        # scales: small finite floats instead of random bytes
        nblk = ((M + 31) // 32) * 32 * (K // 32)
        w[nblk * 16:] = torch.from_numpy((rng.standard_normal(nblk).astype(np.float32) * np.float32(0.01)).view(np.uint8)).cuda()
        x = torch.from_numpy(rng.standard_normal((n, K)).astype(np.float32)).cuda()
        x16 = torch.zeros(n * K, dtype=torch.float16, device="cuda")
        e = torch.zeros(n, dtype=torch.int32, device="cuda")
        for r0 in range(0, n, 32):
            hip.w4a16_rows(x[r0:r0 + 32], K, 32, x16[r0 * K:], e[r0:])
        ya = torch.zeros(n * M, dtype=torch.float32, device="cuda")
        yb = torch.zeros(n * M, dtype=torch.float32, device="cuda")

        def tile():
            for _ in range(5):
                hip.q4_gemm_w4a16_tile(w, M, K, x16, e, n, None, ya)
            torch.cuda.synchronize()

        def rows():
            for _ in range(5):
                for r0 in range(0, n, 32):
                    hip.q4_gemm_w4a16_rows(w, M, K, x16[r0 * K:], e[r0:], 32, None, yb[r0 * M:])
            torch.cuda.synchronize()

        t_tile = timed(tile, repeats)[0] / 5
        t_rows = timed(rows, repeats)[0] / 5
        eq = bool(torch.equal(ya.view(torch.int32), yb.view(torch.int32)))
        flop = 2.0 * M * K * n
        say(f"    M = {M:5d} K = {K:5d}: tile {t_tile * 1e6:9.1f} us ({flop / t_tile / 1e12:6.1f} TFLOP/s)   "
            f"chunked rows {t_rows * 1e6:9.1f} us ({flop / t_rows / 1e12:6.1f} TFLOP/s)   rows / tile {t_rows / t_tile:5.2f}x   "
            f"same bits: {'yes' if eq else 'NO'}")
        del w, x, x16, e, ya, yb


def attn_section(a, dm, hip, tok, N, say):
    """--attn both: the prompt eval and the score window with the attention switch at 1
    (k_attn_w4a16_tile) and at 0 (the exact path's KQ, softmax and KQV), the parent library, and the
    attention's share of one profiled eval at each setting.  The exact path's three attention kernels
    carry no profile name: their time is the profiled eval's wall clock less its named kernels."""
    res = {}
    for sw in (1, 0):
        hip.w4a16_set_attn(sw)
        e_med, e_runs, e_out = timed(lambda: dm.eval(0, tok), a.repeats)
        s_med, s_runs, s_out = timed(lambda: dm.score(0, tok)[0], a.repeats)
        res[sw] = dict(eval=e_med, eval_runs=e_runs, eval_hash=digest(e_out), score=s_med, score_runs=s_runs,
                       score_hash=digest(s_out))
    names = {1: "this library, attn f16  (switch 1)", 0: "this library, attn exact (switch 0)"}
    if a.baseline_lib:
        res["parent"] = run_child(a, a.baseline_lib)
        names["parent"] = "parent commit                     "
    for what, label in (("eval", f"Model.eval of a {N}-token prompt"), ("score", f"one {N}-token Model.score window")):
        say(f"{label}:")
        for k in (1, 0, "parent"):
            if k in res:
                r = res[k]
                say(f"    {names[k]} {r[what] * 1e3:9.2f} ms  (runs {' '.join(f'{v * 1e3:.2f}' for v in r[what + '_runs'])}; "
                    f"hash {r[what + '_hash']})")
        if "parent" in res:
            say(f"    switch 0's hash equals the parent's: {'yes' if res[0][what + '_hash'] == res['parent'][what + '_hash'] else 'NO'}")
            slow, fast = max(res[1][what + "_runs"]), min(res["parent"][what + "_runs"])
            say(f"    parent / switch 1: {res['parent'][what] / res[1][what]:.2f}x (medians); slowest switch-1 run {slow * 1e3:.2f} ms "
                f"against fastest parent run {fast * 1e3:.2f} ms: {'faster' if slow < fast else 'NOT faster'}")
        say(f"    switch 0 / switch 1: {res[0][what] / res[1][what]:.2f}x")
    for sw in (1, 0):
        hip.w4a16_set_attn(sw)
        dm.eval(0, tok, want_logits=False)
        dm.set_profile(True)
        t0 = time.perf_counter()
        dm.eval(0, tok, want_logits=False)
        wall = (time.perf_counter() - t0) * 1e3
        ks = dm.profile_kernels()
        dm.set_profile(False)
        tot = sum(k["ms"] for k in ks)
        if sw:
            at = sum(k["ms"] for k in ks if k["name"].startswith("k_attn_w4a16"))
            say(f"one profiled {N}-token eval, switch 1: {tot:.2f} ms of named kernels, k_kv_f16 + k_attn_w4a16_tile {at:.3f} ms "
                f"({100 * at / tot:.2f} % of them; {at / max(1, sum(k['launches'] for k in ks if k['name'].startswith('k_attn_w4a16'))):.3f} ms per layer); "
                f"wall clock of the profiled call {wall:.2f} ms")
        else:
            say(f"one profiled {N}-token eval, switch 0: {tot:.2f} ms of named kernels, wall clock of the profiled call {wall:.2f} ms: "
                f"{wall - tot:.2f} ms ({100 * (wall - tot) / wall:.1f} %) outside them -- k_kq, k_attn_softmax, k_kqv and the RoPE / cache write")
        for k in sorted(ks, key=lambda k: -k["ms"]):
            say(f"    {k['name']:<40s} {k['ms']:9.3f} ms  {100 * k['ms'] / tot:6.2f}%  {k['launches']:5d} launches")
    hip.w4a16_set_attn(0)
    dm.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="gpt-j-6B")
    ap.add_argument("--layers", type=int, default=0, help="0: the config's own depth")
    ap.add_argument("--n-ctx", type=int, default=2048)
    ap.add_argument("--n", type=int, default=2048, help="tokens of the prompt and of the score window")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--baseline-lib", default="", help="another build of libvsim_hip.so (the parent commit's)")
    ap.add_argument("--tree", default="?", help="what the tree is, for the header line")
    ap.add_argument("--no-ops", action="store_true", help="skip the op-entry section (a second config)")
    ap.add_argument("--out", default="")
    ap.add_argument("--append", action="store_true", help="add to --out instead of replacing it (a second config)")
    ap.add_argument("--attn", default="exact", choices=["exact", "f16", "both"],
                    help="the mode's attention (vsim_w4a16_set_attn); both: the two settings and the parent side by side")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--lib", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)

    import torch
    from vsim_amd import hip
    arch_s, hp = hparams(a.config, a.layers)
    N = a.n
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def flush():
        if a.out:
            with open(a.out, "a" if a.append or flush.done else "w") as f:
                f.write("\n".join(lines[flush.done:]) + "\n")
            flush.done = len(lines)
    flush.done = 0

    box = f"{socket.gethostname()} {torch.cuda.get_device_properties(0).gcnArchName}"
    say(f"# w4a16_prompt_bench: {a.config} shape, {hp['n_layer']} layers, random weights (std 0.02), n_ctx {a.n_ctx}; "
        f"box {box}; tree at {a.tree}")
    say(f"# wall clock round one call that ends in a stream synchronize; a warm call, then the median of {a.repeats}; "
        f"W4A16_TILE_MIN_N = {hip.W4A16_TILE_MIN_N}")
    dm = hip.Model.create(ARCH[arch_s], hp, n_ctx=a.n_ctx)
    dm.randomize(seed=1, std=0.02)
    dm.set_mode(hip.MODE_W4A16)
    tok = [int(t) for t in tokens_of(N, hp["n_vocab"])]

    if a.attn == "both":
        attn_section(a, dm, hip, tok, N, say)
        return flush()
    hip.w4a16_set_attn(1 if a.attn == "f16" else 0)
    say(f"# the mode's attention (vsim_w4a16_set_attn): {a.attn}")
    res = {}
    for sw in (1, 0):
        hip.w4a16_set_tile_gemm(sw)
        e_med, e_runs, e_out = timed(lambda: dm.eval(0, tok), a.repeats)
        s_med, s_runs, s_out = timed(lambda: dm.score(0, tok)[0], a.repeats)
        res[sw] = dict(eval=e_med, eval_runs=e_runs, eval_hash=digest(e_out), score=s_med, score_runs=s_runs,
                       score_hash=digest(s_out))
    names = {1: "this library, switch 1 (tile)   ", 0: "this library, switch 0 (chunks) "}
    if a.baseline_lib:
        res["parent"] = run_child(a, a.baseline_lib)
        names["parent"] = "parent commit (chunks)          "
    for what, label in (("eval", f"Model.eval of a {N}-token prompt"), ("score", f"one {N}-token Model.score window")):
        say(f"{label}:")
        for k in (1, 0, "parent"):
            if k in res:
                r = res[k]
                say(f"    {names[k]} {r[what] * 1e3:9.2f} ms  (runs {' '.join(f'{v * 1e3:.2f}' for v in r[what + '_runs'])}; "
                    f"hash {r[what + '_hash']})")
        hashes = {res[k][what + "_hash"] for k in res}
        say(f"    same hash from all: {'yes' if len(hashes) == 1 else 'NO'}")
        if "parent" in res:
            slow, fast = max(res[1][what + "_runs"]), min(res["parent"][what + "_runs"])
            say(f"    parent / switch 1: {res['parent'][what] / res[1][what]:.2f}x (medians); slowest switch-1 run {slow * 1e3:.2f} ms "
                f"against fastest parent run {fast * 1e3:.2f} ms: {'faster' if slow < fast else 'NOT faster'}")
        say(f"    switch 0 / switch 1: {res[0][what] / res[1][what]:.2f}x")
    flush()

    say("prompt evals, the switch at 2 (tile at every N) against 0 (chunks), for W4A16_TILE_MIN_N:")
    for n in THRESHOLD_NS:
        t = {}
        for sw in (2, 0):
            hip.w4a16_set_tile_gemm(sw)
            t[sw] = timed(lambda: dm.eval(0, tok[:n]), a.repeats)
        say(f"    N = {n:4d}: tile {t[2][0] * 1e3:8.3f} ms   chunks {t[0][0] * 1e3:8.3f} ms   chunks / tile {t[0][0] / t[2][0]:5.2f}x   "
            f"same bits: {'yes' if np.array_equal(t[2][2].view(np.uint32), t[0][2].view(np.uint32)) else 'NO'}")
    flush()

    # where a prompt's device time goes now (event pairs round every launch; profiled once)
    hip.w4a16_set_tile_gemm(1)
    dm.eval(0, tok, want_logits=False)
    dm.set_profile(True)
    dm.eval(0, tok, want_logits=False)
    ks = dm.profile_kernels()
    dm.set_profile(False)
    tot = sum(k["ms"] for k in ks)
    say(f"device time per kernel of one profiled {N}-token eval, switch 1 ({tot:.2f} ms in {sum(k['launches'] for k in ks)} "
        f"profiled launches; not comparable with the un-profiled wall clocks above):")
    for k in sorted(ks, key=lambda k: -k["ms"]):
        say(f"    {k['name']:<40s} {k['ms']:9.3f} ms  {100 * k['ms'] / tot:6.2f}%  {k['launches']:5d} launches")
    dm.close()
    flush()
    if not a.no_ops:
        op_bench(say, hip, torch, a.repeats)
        flush()


if __name__ == "__main__":
    main()
