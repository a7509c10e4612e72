"""Measurements of the model quantizer on the GPU.

  kernel  k_quantize_w (vsim_op_q4_quantize_w) at 50400 x 4096 and 4096 x 16384, F16 and F32
          sources, W4T32 and AoS outputs: bytes read plus bytes written per second from device
          events, beside a device-to-device copy that moves the same number of bytes, timed in
          the same process in alternation.  The copy is the ceiling; the ratio is the result.
  load    a 2-layer GPT-J-width model (E = 4096, full vocabulary) written by modelgen at ftype 1:
          Model.load(quantize=True), vsim_quantize_file on the device and on the host, and the
          plain load of the resulting Q4_0 file, all from the page cache.  Informative only.

    python tools/quantize_bench.py kernel --out profiles/quantize_w_kernel.txt
    python tools/quantize_bench.py load --out profiles/quantize_load.txt [--dir /tmp]
"""
import argparse
import dataclasses
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
from vsim_amd import hip  # noqa: E402
from vsim_amd import modelgen as mg  # noqa: E402


def kernel(out):
    import torch
    dev = "cuda"
    print(f"# k_quantize_w against a device-to-device copy of the same bytes ({torch.cuda.get_device_name(0)})", file=out)
    print("# GB/s = (bytes read + bytes written) / time; median of 7 rounds of 20 launches, alternating", file=out)
    print(f"{'rows':>6} {'k':>6} {'src':>4} {'out':>6} {'MB moved':>9} {'kernel us':>10} {'kernel GB/s':>12} "
          f"{'copy us':>9} {'copy GB/s':>10} {'ratio':>6}", file=out)
    for rows, k in ((50400, 4096), (4096, 16384)):
        for st, dt, name in ((hip.SRC_F16, torch.float16, "f16"), (hip.SRC_F32, torch.float32, "f32")):
            x = (torch.randn((rows, k), device=dev, dtype=torch.float32) * 0.02).to(dt)
            w = torch.empty(hip.q4_bytes(rows, k), dtype=torch.uint8, device=dev)
            a = torch.empty(rows * k // 32 * 20, dtype=torch.uint8, device=dev)
            moved = x.numel() * x.element_size() + rows * k // 32 * 20
            cs = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
            cd = torch.empty_like(cs)
            for target in ("w4t32", "aos"):
                def run_kernel():
                    if target == "w4t32":
                        hip.quantize_w(x, st, rows, k, w=w, w_rows=rows)
                    else:
                        hip.quantize_w(x, st, rows, k, aos=a)

                def timed(fn, n=20):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(n):
                        fn()
                    e1.record()
                    e1.synchronize()
                    return e0.elapsed_time(e1) * 1e3 / n  # us per launch

                for _ in range(3):
                    run_kernel()
                    cd.copy_(cs)
                torch.cuda.synchronize()
                tk, tc = [], []
                for _ in range(7):
                    tk.append(timed(run_kernel))
                    tc.append(timed(lambda: cd.copy_(cs)))
                k_us, c_us = statistics.median(tk), statistics.median(tc)
                print(f"{rows:>6} {k:>6} {name:>4} {target:>6} {moved / 1e6:>9.1f} {k_us:>10.1f} {moved / k_us / 1e3:>12.1f} "
                      f"{c_us:>9.1f} {2 * cs.numel() / c_us / 1e3:>10.1f} {c_us / k_us:>6.2f}", file=out)
                out.flush()


def load(out, workdir):
    arch_s, hp = "gptj", dataclasses.replace(mg.HParams(50400, 4096, 16, 2, 64), ftype=1)
    src, q_dev, q_host = (os.path.join(workdir, n) for n in ("bench-f16.bin", "bench-q4-dev.bin", "bench-q4-host.bin"))
    t0 = time.time()
    mg.write_model(src, arch_s, hp, seed=1, std=0.02)
    print(f"# 2-layer GPT-J-width model (E = 4096, n_vocab = 50400) at ftype 1: {os.path.getsize(src) / 1e6:.0f} MB "
          f"(written in {time.time() - t0:.1f} s); wall-clock seconds, files in the page cache", file=out)
    open(src, "rb").read()

    def wall(fn):
        t = time.time()
        r = fn()
        return time.time() - t, r

    for rep in range(2):
        t, m = wall(lambda: hip.Model.load(src, hip.ARCH_GPTJ, n_ctx=64, quantize=True))
        m.close()
        print(f"Model.load(quantize=True) of the F16 file, run {rep}:        {t:8.3f} s", file=out)
    for rep in range(2):
        t, _ = wall(lambda: hip.quantize_file(src, q_dev, hip.ARCH_GPTJ, device=0))
        print(f"vsim_quantize_file on the device, run {rep}:                 {t:8.3f} s", file=out)
    t, _ = wall(lambda: hip.quantize_file(src, q_host, hip.ARCH_GPTJ, device=-1))
    print(f"vsim_quantize_file on the host (one thread):              {t:8.3f} s", file=out)
    same = open(q_dev, "rb").read() == open(q_host, "rb").read()
    print(f"device and host outputs identical: {same} ({os.path.getsize(q_dev) / 1e6:.0f} MB)", file=out)
    for rep in range(2):
        t, m = wall(lambda: hip.Model.load(q_dev, hip.ARCH_GPTJ, n_ctx=64))
        m.close()
        print(f"plain Model.load of the Q4_0 file, run {rep}:                {t:8.3f} s", file=out)
    for p in (src, q_dev, q_host):
        os.remove(p)
    if not same:
        raise SystemExit("device and host outputs differ")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernel", "load"])
    ap.add_argument("--out", default="-")
    ap.add_argument("--dir", default=None)
    a = ap.parse_args()
    if hip.lib().vsim_device_count() < 1:
        raise SystemExit("quantize_bench: no GPU (these are measurements; there is no CPU stand-in)")
    out = sys.stdout if a.out == "-" else open(a.out, "w")
    if a.what == "kernel":
        kernel(out)
    else:
        with tempfile.TemporaryDirectory(dir=a.dir) as d:
            load(out, d)
    if out is not sys.stdout:
        out.close()
        print(open(a.out).read())


if __name__ == "__main__":
    main()
