#!/usr/bin/env python3
"""k_sample_topk_rows against one k_sample_topk launch per row, on the same rows and parameters.

B logits rows of n random values (N(0, 3)), every row with interface.py's sampler settings (k 20,
temperature 0.85, penalty 1.3) and a window of 64 ids of its own.  After a warm-up, `iters` rounds
of: one vsim_op_topk_rows launch, then B vsim_op_topk launches, on one stream.

  python tools/sample_rows_bench.py --n 50400                 # event timing, every --wg setting
  rocprofv3 --kernel-trace --stats ... -- python tools/sample_rows_bench.py --n 50400 --wg 0 --plain
                                                              # (--plain: no events, the trace times the kernels)
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

from vsim_amd import hip  # noqa: E402

DEV = "cuda:0"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=50400)
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--wg", default="0,64,32,16,8,4,2", help="vsim_topk_rows_set_wg settings to time (0: the default rule)")
    ap.add_argument("--plain", action="store_true", help="no event timing: for a run under the profiler")
    a = ap.parse_args()
    n, B = a.n, a.B
    g = np.random.default_rng(1)
    x = torch.tensor((g.standard_normal((B, n)) * 3).astype(np.float32), device=DEV)
    pa = np.zeros(B, hip.TOPK_PARAMS_DTYPE)
    wins = g.integers(0, n, (B, 64)).astype(np.int32)
    for b in range(B):
        pa[b]["scale"], pa[b]["penalty"], pa[b]["k"], pa[b]["nw"] = 1.0 / float(np.float32(0.85)), float(np.float32(1.3)), 20, 64
        pa[b]["win"][:64] = wins[b]
    pd = torch.tensor(pa.view(np.uint8).reshape(-1), device=DEV)
    out = torch.zeros(B * hip.TOPK_OUT_DTYPE.itemsize, dtype=torch.uint8, device=DEV)
    wd = torch.tensor(wins, device=DEV)
    val = torch.zeros((B, 20), dtype=torch.float64, device=DEV)
    ids = torch.zeros((B, 20), dtype=torch.int32, device=DEV)

    def rows():
        hip.topk_rows(x, n, n, B, pd, out)

    def serial():
        for b in range(B):
            hip.topk(x[b], n, wd[b], pa[b]["scale"], pa[b]["penalty"], 20, val[b], ids[b])

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ts = []
        for _ in range(a.iters):
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        return statistics.median(ts)

    settings = [int(w) for w in a.wg.split(",")]
    for _ in range(3):
        rows()
        serial()
    torch.cuda.synchronize()
    o = out.cpu().numpy().view(hip.TOPK_OUT_DTYPE)
    assert np.array_equal(o["id"][:, :20], ids.cpu().numpy()) and np.array_equal(o["val"][:, :20], val.cpu().numpy())
    if a.plain:
        hip.topk_rows_set_wg(settings[0])
        for _ in range(a.iters):
            rows()
            serial()
        torch.cuda.synchronize()
        return
    t_serial = timed(serial)
    print(f"n {n}, B {B}, median of {a.iters}, stream events round the launches (launch gaps of the serial case included)")
    print(f"  {B} x k_sample_topk            {t_serial:9.1f} us")
    for w in settings:
        hip.topk_rows_set_wg(w)
        t = timed(rows)
        print(f"  k_sample_topk_rows, wg {w:2d}      {t:9.1f} us   serial / rows {t_serial / t:5.2f}")
    hip.topk_rows_set_wg(0)


if __name__ == "__main__":
    main()
