"""product_plan (vsim_amd/csrc/product_plan.hpp): which kernel runs a Q4_0 product, from values alone.

A stand-alone program that includes only that header (no HIP) is compiled with g++ and prints the
plan for a grid of inputs; the expected table below is written out from the thresholds in the tree:
GEMM_MIN_N = 8 and G2_MIN_N = 256 rows (fast-mode fp16 GEMMs), EXACT_GEMV_MAX_N = 32 rows in jobs
of 4 (exact prompt), BATCH_GEMM_MIN_N = 12 and BATCH_FAST_GEMM_MIN_N = 4 rows (the batched steps'
switches at their default, 1), VSIM_BATCH_MAX = 32 rows.
"""
import os
import subprocess

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HEADER = os.path.join(ROOT, "vsim_amd", "csrc", "product_plan.hpp")

PROGRAM = r"""
#include "%s"
#include <cstdio>
#include <initializer_list>
using namespace vsim;
static const char *kname(ProductKernel k) {
  switch (k) {
    case ProductKernel::NONE: return "none";
    case ProductKernel::GEMM_F16_256: return "k_gemm_f16_256";
    case ProductKernel::GEMM_F16: return "k_gemm_f16";
    case ProductKernel::GEMM_EXACT: return "k_gemm_exact";
    case ProductKernel::GEMM_EXACT_ROWS: return "k_gemm_exact_rows";
    case ProductKernel::GEMM_FAST_ROWS: return "k_gemm_fast_rows";
    case ProductKernel::GEMV_CHAIN: return "gemv_chain";
    case ProductKernel::GEMV_FAST: return "k_gemv_fast";
  }
  return "?";
}
static void show(const char *label, BatchKind kind, int mode, int N, int K, bool x16, bool gelu, bool epi, int sw) {
  ProductQuery q;
  q.kind = kind;
  q.mode = mode;
  q.N = N;
  q.M = 512;
  q.K = K;
  q.x16 = x16;
  q.gelu = gelu;
  q.epi = epi;
  q.gemm = q.fast_gemm = sw;
  const ProductPlan p = product_plan(q);
  printf("%%s N=%%d K=%%d x16=%%d gelu=%%d epi=%%d sw=%%d | %%s|%%d|%%d|%%s|%%d|%%d|%%d|%%s\n", label, N, K, x16, gelu, epi, sw,
         kname(p.kernel), p.launches, p.kernels, p.name ? p.name : "-", p.passes, p.gelu, p.fused, p.error ? p.error : "-");
}
int main() {
  // a prompt batch carries the fp16 operand exactly when PromptBatch says so: fast mode from GEMM_MIN_N rows on
  for (int N : {1, 7, 8, 255, 256}) show("fast-prompt", BatchKind::PROMPT, VSIM_MODE_FAST, N, 512, f16_gemm_rows(VSIM_MODE_FAST, N), false, false, 1);
  show("fast-prompt", BatchKind::PROMPT, VSIM_MODE_FAST, 256, 512, true, true, false, 1);
  show("fast-prompt", BatchKind::PROMPT_SLOT, VSIM_MODE_FAST, 256, 512, true, false, true, 1);
  show("fast-prompt", BatchKind::PROMPT, VSIM_MODE_FAST, 256, 544, true, false, true, 1);
  show("fast-prompt", BatchKind::PROMPT, VSIM_MODE_FAST, 256, 544, true, true, false, 1);
  // (launch_q4_gemv's fast-mode products: Q4 rows at every N)
  for (int N : {7, 8, 256}) show("fast-q4rows", BatchKind::PROMPT, VSIM_MODE_FAST, N, 512, false, false, false, 1);
  for (int N : {1, 4, 5, 32, 33}) show("exact-prompt", BatchKind::PROMPT, VSIM_MODE_EXACT, N, 512, false, false, false, 1);
  for (int sw : {0, 1, 2})
    for (int N : {1, 11, 12, 32}) show("exact-rows", BatchKind::ROWS_EXACT, VSIM_MODE_EXACT, N, 512, false, false, false, sw);
  for (int sw : {0, 1, 2})
    for (int N : {1, 3, 4, 32}) show("fast-rows", BatchKind::ROWS_FAST, VSIM_MODE_FAST, N, 512, false, false, false, sw);
  show("fast-rows", BatchKind::ROWS_FAST, VSIM_MODE_FAST, 4, 512, true, false, false, 2);
  show("fast-rows", BatchKind::ROWS_FAST, VSIM_MODE_FAST, 33, 512, false, false, false, 2);
  return 0;
}
"""

GENERAL1, GENERAL = "gemv (general path)", "gemv (prompt rows)"
LEFT = "fast batched step: a product left the Q4 rows"

# label, N, K, x16, gelu asked, epi asked, switch -> kernel, launches, kernels counted, profile name,
# passes over the weight (algorithmic bytes), GELU epilogue runs, an epilogue runs, error
EXPECTED = [
    # fast prompt: the decode GEMV per row below 8 rows (one kernel counted, whatever the launches),
    # the fp16 GEMM from 8, its 256-wide tiles from 256 rows where K % 64 == 0
    ("fast-prompt", 1, 512, 0, 0, 0, 1, "k_gemv_fast", 1, 1, GENERAL1, 1, 0, 0, "-"),
    ("fast-prompt", 7, 512, 0, 0, 0, 1, "k_gemv_fast", 7, 1, GENERAL, 1, 0, 0, "-"),
    ("fast-prompt", 8, 512, 1, 0, 0, 1, "k_gemm_f16", 1, 1, "k_gemm_f16 (prompt)", 1, 0, 0, "-"),
    ("fast-prompt", 255, 512, 1, 0, 0, 1, "k_gemm_f16", 1, 1, "k_gemm_f16 (prompt)", 1, 0, 0, "-"),
    ("fast-prompt", 256, 512, 1, 0, 0, 1, "k_gemm_f16_256", 1, 1, "k_gemm_f16_256 (prompt)", 1, 0, 0, "-"),
    ("fast-prompt", 256, 512, 1, 1, 0, 1, "k_gemm_f16_256", 1, 1, "k_gemm_f16_256 (prompt)", 1, 1, 1, "-"),
    ("fast-prompt", 256, 512, 1, 0, 1, 1, "k_gemm_f16_256", 1, 1, "k_gemm_f16_256 (prompt)", 1, 0, 1, "-"),
    ("fast-prompt", 256, 544, 1, 0, 1, 1, "k_gemm_f16", 1, 1, "k_gemm_f16 (prompt)", 1, 0, 0, "-"),
    ("fast-prompt", 256, 544, 1, 1, 0, 1, "k_gemm_f16", 1, 1, "k_gemm_f16 (prompt)", 1, 0, 0, "-"),
    ("fast-q4rows", 7, 512, 0, 0, 0, 1, "k_gemv_fast", 7, 1, GENERAL, 1, 0, 0, "-"),
    ("fast-q4rows", 8, 512, 0, 0, 0, 1, "k_gemm_f16", 1, 1, GENERAL, 1, 0, 0, "-"),
    ("fast-q4rows", 256, 512, 0, 0, 0, 1, "k_gemm_f16", 1, 1, GENERAL, 1, 0, 0, "-"),
    # exact prompt: the chain GEMV in jobs of 4 up to 32 rows, k_gemm_exact beyond
    ("exact-prompt", 1, 512, 0, 0, 0, 1, "gemv_chain", 1, 1, GENERAL1, 1, 0, 0, "-"),
    ("exact-prompt", 4, 512, 0, 0, 0, 1, "gemv_chain", 1, 1, GENERAL, 1, 0, 0, "-"),
    ("exact-prompt", 5, 512, 0, 0, 0, 1, "gemv_chain", 2, 1, GENERAL, 1, 0, 0, "-"),
    ("exact-prompt", 32, 512, 0, 0, 0, 1, "gemv_chain", 8, 1, GENERAL, 1, 0, 0, "-"),
    ("exact-prompt", 33, 512, 0, 0, 0, 1, "k_gemm_exact", 1, 1, GENERAL, 1, 0, 0, "-"),
    # exact rows: switch 0 the prompt's GEMV jobs, 1 k_gemm_exact_rows from 12 rows, 2 always
    ("exact-rows", 1, 512, 0, 0, 0, 0, "gemv_chain", 1, 1, GENERAL1, 1, 0, 0, "-"),
    ("exact-rows", 11, 512, 0, 0, 0, 0, "gemv_chain", 3, 1, GENERAL, 1, 0, 0, "-"),
    ("exact-rows", 12, 512, 0, 0, 0, 0, "gemv_chain", 3, 1, GENERAL, 1, 0, 0, "-"),
    ("exact-rows", 32, 512, 0, 0, 0, 0, "gemv_chain", 8, 1, GENERAL, 1, 0, 0, "-"),
    ("exact-rows", 1, 512, 0, 0, 0, 1, "gemv_chain", 1, 1, GENERAL1, 1, 0, 0, "-"),
    ("exact-rows", 11, 512, 0, 0, 0, 1, "gemv_chain", 3, 1, GENERAL, 1, 0, 0, "-"),
    ("exact-rows", 12, 512, 0, 0, 0, 1, "k_gemm_exact_rows", 1, 1, "k_gemm_exact_rows (batch)", 1, 0, 0, "-"),
    ("exact-rows", 32, 512, 0, 0, 0, 1, "k_gemm_exact_rows", 1, 1, "k_gemm_exact_rows (batch)", 1, 0, 0, "-"),
    ("exact-rows", 1, 512, 0, 0, 0, 2, "k_gemm_exact_rows", 1, 1, "k_gemm_exact_rows (batch)", 1, 0, 0, "-"),
    ("exact-rows", 11, 512, 0, 0, 0, 2, "k_gemm_exact_rows", 1, 1, "k_gemm_exact_rows (batch)", 1, 0, 0, "-"),
    ("exact-rows", 12, 512, 0, 0, 0, 2, "k_gemm_exact_rows", 1, 1, "k_gemm_exact_rows (batch)", 1, 0, 0, "-"),
    ("exact-rows", 32, 512, 0, 0, 0, 2, "k_gemm_exact_rows", 1, 1, "k_gemm_exact_rows (batch)", 1, 0, 0, "-"),
    # fast rows: switch 0 one k_gemv_fast launch per row (N launches, N kernels counted, N passes
    # over the weight), 1 k_gemm_fast_rows from 4 rows, 2 always
    ("fast-rows", 1, 512, 0, 0, 0, 0, "k_gemv_fast", 1, 1, "k_gemv_fast (batch, per row)", 1, 0, 0, "-"),
    ("fast-rows", 3, 512, 0, 0, 0, 0, "k_gemv_fast", 3, 3, "k_gemv_fast (batch, per row)", 3, 0, 0, "-"),
    ("fast-rows", 4, 512, 0, 0, 0, 0, "k_gemv_fast", 4, 4, "k_gemv_fast (batch, per row)", 4, 0, 0, "-"),
    ("fast-rows", 32, 512, 0, 0, 0, 0, "k_gemv_fast", 32, 32, "k_gemv_fast (batch, per row)", 32, 0, 0, "-"),
    ("fast-rows", 1, 512, 0, 0, 0, 1, "k_gemv_fast", 1, 1, "k_gemv_fast (batch, per row)", 1, 0, 0, "-"),
    ("fast-rows", 3, 512, 0, 0, 0, 1, "k_gemv_fast", 3, 3, "k_gemv_fast (batch, per row)", 3, 0, 0, "-"),
    ("fast-rows", 4, 512, 0, 0, 0, 1, "k_gemm_fast_rows", 1, 1, "k_gemm_fast_rows (batch)", 1, 0, 0, "-"),
    ("fast-rows", 32, 512, 0, 0, 0, 1, "k_gemm_fast_rows", 1, 1, "k_gemm_fast_rows (batch)", 1, 0, 0, "-"),
    ("fast-rows", 1, 512, 0, 0, 0, 2, "k_gemm_fast_rows", 1, 1, "k_gemm_fast_rows (batch)", 1, 0, 0, "-"),
    ("fast-rows", 3, 512, 0, 0, 0, 2, "k_gemm_fast_rows", 1, 1, "k_gemm_fast_rows (batch)", 1, 0, 0, "-"),
    ("fast-rows", 4, 512, 0, 0, 0, 2, "k_gemm_fast_rows", 1, 1, "k_gemm_fast_rows (batch)", 1, 0, 0, "-"),
    ("fast-rows", 32, 512, 0, 0, 0, 2, "k_gemm_fast_rows", 1, 1, "k_gemm_fast_rows (batch)", 1, 0, 0, "-"),
    # a fast rows batch whose product has an fp16 operand, or more than 32 rows: the executor's error
    ("fast-rows", 4, 512, 1, 0, 0, 2, "none", 0, 0, "-", 1, 0, 0, LEFT),
    ("fast-rows", 33, 512, 0, 0, 0, 2, "none", 0, 0, "-", 1, 0, 0, LEFT),
]


def test_product_plan_table(tmp_path):
    src, exe = tmp_path / "plan.cpp", tmp_path / "plan"
    src.write_text(PROGRAM % HEADER)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-o", str(exe), str(src)], check=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    want = ["%s N=%d K=%d x16=%d gelu=%d epi=%d sw=%d | %s|%d|%d|%s|%d|%d|%d|%s" % row for row in EXPECTED]
    assert got == want
