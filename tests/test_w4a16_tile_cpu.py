"""k_gemm_w4a16_tile on the CPU.

* tests/w4a16_tile_cases.py's inputs have teeth: on the rows the GPU test feeds the kernel at K = 544
  and 1,056, each of three wrong kernels (contiguous strands, a pairwise tree over the partials, an
  fma with two roundings) changes bits in at least one output of every finite row that can tell
  them apart, over the four weights that meet the row.  A row whose operand is non-zero in one
  block only (families 3 and 13: one 1e30 outlier among values that scale to zero, one non-zero
  last element) is a single term, on which every order and every rounding agrees by construction;
  all-zero rows give zero; the row of f32 subnormals gives f32 subnormals, which the final scaling
  rounds once more.  Those are asserted to be exactly those families.
* product_plan (vsim_amd/csrc/product_plan.hpp, compiled alone) with the prompt's switch.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import w4a16_ref as W
import w4a16_tile_cases as C

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HEADER = os.path.join(ROOT, "vsim_amd", "csrc", "product_plan.hpp")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_fma32_is_one_rounding():
    """Against exact rational arithmetic on values chosen to sit near ties of the fp32 result."""
    from fractions import Fraction
    rng = np.random.default_rng(5)
    a = rng.standard_normal(4000).astype(np.float32)
    b = rng.standard_normal(4000).astype(np.float32)
    c = (-(a.astype(np.float64) * b.astype(np.float64)) * (1 + rng.integers(-3, 4, 4000) * 2.0 ** -24)).astype(np.float32)
    c[::2] = rng.standard_normal(2000).astype(np.float32) * 64
    got = C.fma32(a, b, c)
    for i in range(0, 4000, 7):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo, hi = np.nextafter(got[i], np.float32(-np.inf)), np.nextafter(got[i], np.float32(np.inf))
        d = abs(Fraction(float(got[i])) - exact)
        assert d <= abs(Fraction(float(lo)) - exact) and d <= abs(Fraction(float(hi)) - exact), i
    two = (a * b).astype(np.float32) + c
    assert (bits(two) != bits(got)).any()


@functools.lru_cache(maxsize=None)
def emulated(M, K):
    aos, b, wd, wq, x, h, e = C.case(M, K)
    dots = C.block_dots(wq, h)
    return x, h, e, C.emulate(wd, dots, e), {v: C.emulate(wd, dots, e, wrong=v) for v in C.VARIANTS}


@pytest.mark.parametrize("K", [544, 1056])
def test_every_wrong_variant_bites_every_row(K):
    nb = K // 32
    runs = [emulated(M, K) for M in C.MS]      # the same 300 rows against the four weights
    x, h, e = runs[0][:3]
    assert all(np.array_equal(r[0].view(np.uint32), x.view(np.uint32)) for r in runs)
    good = np.concatenate([r[3] for r in runs], axis=1)
    wrong = {v: np.concatenate([r[4][v] for r in runs], axis=1) for v in C.VARIANTS}
    blocks_used = (h.reshape(C.N_ROWS, nb, 32) != 0).any(axis=2).sum(axis=1)
    bad = set(C.bad_rows())
    assert len(bad) == 24 and len({j % 16 for j in bad if C.family_of(j) == 8}) == 8   # another place in every tile
    exempt = C.ONE_BLOCK_FAMILIES + C.ZERO_FAMILIES + (C.SUBNORMAL_FAMILY,)
    for j in range(C.N_ROWS):
        fam = C.family_of(j)
        if j in bad:
            assert e[j] == W.NONFINITE and (bits(good[j]) == W.QNAN_BITS).all()
            continue
        assert np.isfinite(good[j]).all()
        if blocks_used[j] <= 1:                      # a single term: nothing to tell apart
            assert fam in C.ONE_BLOCK_FAMILIES + C.ZERO_FAMILIES, (j, fam)
            for v in C.VARIANTS:
                assert np.array_equal(bits(wrong[v][j]), bits(good[j])), (j, v)
            continue
        if (np.abs(good[j]) < 2.0 ** -126).all():    # subnormal outputs: rounded once more by the scaling
            assert fam == C.SUBNORMAL_FAMILY, (j, fam)
            continue
        assert fam not in exempt, (j, fam)
        for v in C.VARIANTS:
            assert (bits(wrong[v][j]) != bits(good[j])).any(), f"K={K}: {v} does not bite row {j} (family {fam})"


def test_emulation_within_the_bound_of_the_fp64_product():
    """The restatement itself is an instance of the formula: inside w4a16_ref's derived bound."""
    M, K = 40, 544
    aos, b, wd, wq, x, h, e = C.case(M, K)
    y = C.emulate(wd, C.block_dots(wq, h), e, b)
    y64, tol = W.product64(wd, wq, h, e, b)
    ok = [j for j in range(C.N_ROWS) if e[j] != W.NONFINITE]
    assert W.bound_ratio(y[ok], y64[ok], tol[ok]) <= 1.0


# ------------------------------------------------------------------ the plan
PROGRAM = r"""
#include "%s"
#include <cstdio>
#include <initializer_list>
using namespace vsim;
static void show(const char *label, BatchKind kind, int mode, int N, bool x16, int sw) {
  ProductQuery q;
  q.kind = kind;
  q.mode = mode;
  q.N = N;
  q.M = 512;
  q.K = 512;
  q.x16 = x16;
  q.w4a16_tile = sw;
  const ProductPlan p = product_plan(q);
  printf("%%s N=%%d sw=%%d | %%d|%%d|%%d|%%s|%%d|%%d|%%d|%%s\n", label, N, sw, (int)p.kernel, p.launches, p.kernels,
         p.name ? p.name : "-", p.passes, (int)p.w4a16, (int)p.w4a16_tile, p.error ? p.error : "-");
}
int main() {
  static_assert(W4A16_TILE_MIN_N > 32, "every N <= 32 keeps the chunked launches");
  static_assert(W4A16_TILE_ROWS >= 64, "TN");
  printf("min_n %%d rows %%d default %%d\n", W4A16_TILE_MIN_N, W4A16_TILE_ROWS, ProductQuery{}.w4a16_tile);
  const int T = W4A16_TILE_MIN_N;
  for (BatchKind kind : {BatchKind::PROMPT, BatchKind::PROMPT_SLOT}) {
    const char *l = kind == BatchKind::PROMPT ? "prompt" : "slot";
    for (int N : {1, 32, 33, T - 1, T, T + 1, 300, 2048}) show(l, kind, VSIM_MODE_W4A16, N, false, 0);
    for (int N : {1, 32, 33, T - 1, T, T + 1, 300, 2048}) show(l, kind, VSIM_MODE_W4A16, N, false, 1);
    for (int N : {1, 33, 2048}) show(l, kind, VSIM_MODE_W4A16, N, false, 2);
    show(l, kind, VSIM_MODE_W4A16, 300, true, 2);
  }
  for (int sw : {0, 1, 2}) {
    for (int N : {1, 17, 32}) show("rows", BatchKind::ROWS_W4A16, VSIM_MODE_W4A16, N, false, sw);
    show("rows", BatchKind::ROWS_W4A16, VSIM_MODE_EXACT, 4, false, sw);
  }
  int old = w4a16_set_tile_gemm(0);
  printf("switch %%d", old);
  old = w4a16_set_tile_gemm(2); printf(" %%d", old);
  old = w4a16_set_tile_gemm(7); printf(" %%d", old);
  old = w4a16_set_tile_gemm(-1); printf(" %%d", old);
  printf(" %%d\n", w4a16_tile_gemm());
  return 0;
}
"""

LEFT = "weight-only mode: a product left the f32 rows"
NAME_ROWS, NAME_TILE = "k_gemm_w4a16_rows", "k_gemm_w4a16_tile"


def chunks(label, N, sw):
    c = -(-N // 32)
    return f"{label} N={N} sw={sw} | 0|{c}|{c}|{NAME_ROWS}|{c}|1|0|-"


def tile(label, N, sw, rows):
    return f"{label} N={N} sw={sw} | 0|1|1|{NAME_TILE}|{-(-N // rows)}|1|1|-"


def test_product_plan_with_the_prompt_switch(tmp_path):
    src, exe = tmp_path / "plan.cpp", tmp_path / "plan"
    src.write_text(PROGRAM % HEADER)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-o", str(exe), str(src)], check=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    head = got[0].split()
    T, rows, default = int(head[1]), int(head[3]), int(head[5])
    assert T > 32 and rows >= 64 and default == 1
    from vsim_amd import hip
    assert hip.W4A16_TILE_MIN_N == T   # (the Python side's copy, for the model test)
    want = []
    for l in ("prompt", "slot"):
        ns = [1, 32, 33, T - 1, T, T + 1, 300, 2048]
        want += [chunks(l, N, 0) for N in ns]                                          # switch 0: today's chunks
        want += [tile(l, N, 1, rows) if N >= T else chunks(l, N, 1) for N in ns]       # switch 1: from the threshold on
        want += [tile(l, N, 2, rows) for N in (1, 33, 2048)]                           # switch 2: at every N
        want.append(f"{l} N=300 sw=2 | 0|0|0|-|1|0|0|{LEFT}")                          # the error, unchanged
    for sw in (0, 1, 2):                                                               # the batched step: untouched
        want += [chunks("rows", N, sw) for N in (1, 17, 32)]
        want.append(f"rows N=4 sw={sw} | 0|0|0|-|1|0|0|{LEFT}")
    want.append("switch 1 0 2 1 1")
    assert got[1:] == want
