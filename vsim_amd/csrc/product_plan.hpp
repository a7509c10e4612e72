// vsim_amd/csrc/product_plan.hpp — which kernel runs a product of a Q4_0 weight with N activation rows.
//
// The one place where that is decided: product_plan answers from values alone (the kind of batch,
// the products' mode, the shape, what operand the rows are, the epilogue asked for, the two
// process-wide switches), and the executor (PromptBatch::mm, run_layer), launch_q4_gemv and
// launch_gemm_fast_rows all act on its answer.  Host code without a HIP header: tests/test_product_plan_cpu.py
// compiles it alone.
#pragma once

#include <atomic>

#include "../../include/vsim_hip.h"

namespace vsim {

// What a batch of N rows on its way through the layers and the head is (BatchDesc, model.cpp)
enum class BatchKind {
  PROMPT,       // N tokens of one sequence at n_past, on the model's own cache (eval, eval_score)
  PROMPT_SLOT,  // the same on a named sequence slot's cache (eval_seq)
  ROWS_EXACT,   // one token each of N sequences, exact products (decode_batch)
  ROWS_FAST,    // the same with fast products, the Q4 rows kept at every N (decode_batch_fast)
  ROWS_W4A16,   // the same with weight-only products on the f32 rows (decode_batch_w4a16)
};
inline bool is_rows(BatchKind k) {
  return k == BatchKind::ROWS_EXACT || k == BatchKind::ROWS_FAST || k == BatchKind::ROWS_W4A16;
}

// Fast-mode products from this many rows on run on the fp16 MFMA GEMM (gemm_f16.hip); a prompt
// batch then carries its activations as the GEMM's fp16 operand (scratch pf_x16)
constexpr int GEMM_MIN_N = 8;
// ... and from this many rows on, with K % 64 == 0, on its 256 x 256-tile form, which has the
// GELU-quantize and the G2Epi epilogues
constexpr int G2_MIN_N = 256;
// Exact products of up to this many rows run as decode GEMVs, 4 rows (jobs) per launch: the
// register-tiled chain GEMM's 128-token tiles cost the same for 5 tokens as for 128 (r04 rocprof:
// 1.09 ms per GPT-J GEMM for a 5-token prompt)
constexpr int EXACT_GEMV_MAX_N = 32;
constexpr int GEMV_JOBS = 4;
// from this many rows on a batched step's exact products run on k_gemm_exact_rows by default: below it
// the GEMV jobs are faster (profiles/batch_decode_bench.txt)
constexpr int BATCH_GEMM_MIN_N = 12;
// from this many rows on the products of a fast batched step run on k_gemm_fast_rows by default: the
// smallest measured B at which it beats the per-row launches by more than 5 % at both measured
// shapes (profiles/batch_fast_bench.txt: GPT-J-6B 1.07x at B = 2, 1.58x at 4;
// batch_fast_bench_pythia12b.txt: 0.78x at B = 2, 1.18x at 4)
constexpr int BATCH_FAST_GEMM_MIN_N = 4;
// from this many rows on the products of a weight-only prompt batch run on k_gemm_w4a16_tile by
// default, in one launch, instead of k_gemm_w4a16_rows on chunks of VSIM_BATCH_MAX rows: the smallest
// measured N of {33, 64, 96, 128, 256} at which a prompt eval on it beats the chunked one by more
// than 5 % at both measured shapes (profiles/w4a16_prompt_bench.txt: GPT-J-6B 1.07x at N = 33, 1.14x
// at 64, 1.49x at 96, 1.77x at 128, 2.35x at 256; pythia-12b 1.48x, 1.59x, 1.76x, 1.84x, 2.52x)
constexpr int W4A16_TILE_MIN_N = 33;
// ... and the activation rows of one of its workgroups: the weight streams once per this many rows
constexpr int W4A16_TILE_ROWS = 64;

// The process-wide switches (0: the GEMV path, 1: the rows GEMM from its threshold on, 2: always;
// another value selects 1; the weight-only prompt's: 0: the chunked rows kernel, 1: the tile kernel
// from its threshold on, 2: always).  The setters return the old setting.
inline std::atomic<int> g_batch_gemm{1};       // vsim_batch_set_gemm
inline std::atomic<int> g_batch_fast_gemm{1};  // vsim_batch_set_fast_gemm
inline std::atomic<int> g_w4a16_tile_gemm{1};  // vsim_w4a16_set_tile_gemm
inline int batch_set_gemm(int v) { return g_batch_gemm.exchange(v < 0 || v > 2 ? 1 : v); }
inline int batch_set_fast_gemm(int v) { return g_batch_fast_gemm.exchange(v < 0 || v > 2 ? 1 : v); }
inline int w4a16_set_tile_gemm(int v) { return g_w4a16_tile_gemm.exchange(v < 0 || v > 2 ? 1 : v); }
inline int batch_gemm() { return g_batch_gemm.load(); }
inline int batch_fast_gemm() { return g_batch_fast_gemm.load(); }
inline int w4a16_tile_gemm() { return g_w4a16_tile_gemm.load(); }

// The two row-count thresholds of the fp16 GEMMs, each compared here and nowhere else:
// fast-mode rows that go to the fp16 GEMM, and an fp16 operand that goes to its 256-wide tiles
inline bool f16_gemm_rows(int mode, int N) { return mode == VSIM_MODE_FAST && N >= GEMM_MIN_N; }
inline bool wide_gemm(bool x16, int N, int K) { return x16 && N >= G2_MIN_N && K % 64 == 0; }

enum class ProductKernel {
  NONE,             // no kernel takes it (ProductPlan::error)
  GEMM_F16_256,     // k_gemm_f16_256: launch_gemm_q4_256
  GEMM_F16,         // k_gemm_f16: launch_gemm_f16x (fp16 operand) or launch_gemm_q4_f16 (Q4 rows)
  GEMM_EXACT,       // k_gemm_exact: launch_gemm_exact
  GEMM_EXACT_ROWS,  // k_gemm_exact_rows: launch_gemm_exact_rows
  GEMM_FAST_ROWS,   // k_gemm_fast_rows: launch_gemm_fast_rows
  GEMV_CHAIN,       // the exact chain GEMV, GEMV_JOBS rows per launch: launch_gemv_rows
  GEMV_FAST,        // k_gemv_fast, one launch per row: launch_gemv_rows
};
// (Weight-only mode's k_gemm_w4a16_rows is ProductPlan::w4a16, not an enumerator here:
// tests/test_product_plan_cpu.py compiles a switch over this enum without a default under -Werror, so
// the enum cannot grow while that file stays as it is.)

struct ProductQuery {
  BatchKind kind = BatchKind::PROMPT;
  int mode = VSIM_MODE_EXACT;
  int N = 1, M = 0, K = 0;
  bool x16 = false;   // the rows are the GEMM's fp16 operand (else Q4 rows and their factors)
  bool gelu = false;  // asked for: bias + GELU + quantize of the product into the next fp16 operand
  bool epi = false;   // asked for: a G2Epi epilogue (RoPE, residual join, fp16 copies)
  int gemm = 1, fast_gemm = 1;  // the switches' settings (batch_gemm(), batch_fast_gemm())
  int w4a16_tile = 1;           // ... and w4a16_tile_gemm()
};

struct ProductPlan {
  ProductKernel kernel = ProductKernel::NONE;
  int launches = 0;            // kernel launches the product makes
  int kernels = 0;             // ... and how many of them kernels_per_eval counts (see below)
  const char *name = nullptr;  // the profile's name of the product
  int passes = 1;              // algorithmic bytes: this many passes over the weight
  bool gelu = false;           // the GELU-quantize epilogue runs (only k_gemm_f16_256 has it: M % 32 == 0)
  bool fused = false;          // that or the G2Epi epilogue runs
  // weight-only mode: k_gemm_w4a16_rows (launch_gemm_w4a16_rows) runs the product on the rows' fp16
  // operand, one launch per chunk of VSIM_BATCH_MAX rows; `kernel` stays NONE
  bool w4a16 = false;
  const char *error = nullptr;
  // ... or, with w4a16 set too, k_gemm_w4a16_tile (launch_gemm_w4a16_tile) in one launch: the same bits
  bool w4a16_tile = false;
};

// kernels_per_eval is not consistent about launches: a product on the GEMV paths of the general
// dispatch (GEMV_CHAIN, or GEMV_FAST below GEMM_MIN_N rows of a prompt) counts as one kernel
// however many launches carry its rows, while the fast batched step's per-row fallback counts
// its N.  Both figures are pinned by tests; kept as they are.
inline ProductPlan product_plan(const ProductQuery &q) {
  using PK = ProductKernel;
  ProductPlan p;
  auto is = [&](PK k, int launches, int kernels, const char *name) {
    p.kernel = k;
    p.launches = launches;
    p.kernels = kernels;
    p.name = name;
  };
  if (q.mode == VSIM_MODE_W4A16 || q.kind == BatchKind::ROWS_W4A16) {
    // weight-only mode: the per-row kernel on consecutive chunks of VSIM_BATCH_MAX rows (a chunked
    // weight pass: chunking cannot change a row's bits), or for a prompt batch, by the switch, the
    // tile kernel that gives every row the same bits in one launch
    const int chunks = (q.N + VSIM_BATCH_MAX - 1) / VSIM_BATCH_MAX;
    const bool prompt = q.kind == BatchKind::PROMPT || q.kind == BatchKind::PROMPT_SLOT;
    if (q.x16 || q.gelu || q.epi || q.mode != VSIM_MODE_W4A16) {
      p.error = "weight-only mode: a product left the f32 rows";
    } else if (prompt && (q.w4a16_tile == 2 || (q.w4a16_tile == 1 && q.N >= W4A16_TILE_MIN_N))) {
      is(PK::NONE, 1, 1, "k_gemm_w4a16_tile");
      p.w4a16 = p.w4a16_tile = true;
      p.passes = (q.N + W4A16_TILE_ROWS - 1) / W4A16_TILE_ROWS;
    } else {
      is(PK::NONE, chunks, chunks, "k_gemm_w4a16_rows");
      p.w4a16 = true;
      p.passes = chunks;
    }
  } else if (q.kind == BatchKind::ROWS_FAST) {
    // k_gemv_fast's value of every row, in one pass of the weight for all rows or as one launch
    // per row: the same bits
    if (q.x16 || q.N > VSIM_BATCH_MAX) {
      p.error = "fast batched step: a product left the Q4 rows";
    } else if (q.fast_gemm == 2 || (q.fast_gemm == 1 && q.N >= BATCH_FAST_GEMM_MIN_N)) {
      is(PK::GEMM_FAST_ROWS, 1, 1, "k_gemm_fast_rows (batch)");
    } else {
      is(PK::GEMV_FAST, q.N, q.N, "k_gemv_fast (batch, per row)");
      p.passes = q.N;
    }
  } else if (wide_gemm(q.x16, q.N, q.K)) {
    // long prompt: the 256-wide-tile GEMM, the Q4_0 weight dequantized to fp16 in LDS
    is(PK::GEMM_F16_256, 1, 1, "k_gemm_f16_256 (prompt)");
    p.gelu = q.gelu && q.M % 32 == 0;
    p.fused = p.gelu || q.epi;
  } else if (q.x16) {
    is(PK::GEMM_F16, 1, 1, "k_gemm_f16 (prompt)");
  } else {
    // Q4 rows.  The profile calls the general dispatch's products by their row count alone.
    const char *general = q.N > 1 ? "gemv (prompt rows)" : "gemv (general path)";
    const bool exact = q.mode == VSIM_MODE_EXACT;
    if (q.kind == BatchKind::ROWS_EXACT && exact && q.N <= VSIM_BATCH_MAX &&
        (q.gemm == 2 || (q.gemm == 1 && q.N >= BATCH_GEMM_MIN_N)))
      // batched decode step: every weight block dequantized once for all the rows
      is(PK::GEMM_EXACT_ROWS, 1, 1, "k_gemm_exact_rows (batch)");
    else if (f16_gemm_rows(q.mode, q.N))
      is(PK::GEMM_F16, 1, 1, general);
    else if (exact && q.N > EXACT_GEMV_MAX_N)
      is(PK::GEMM_EXACT, 1, 1, general);
    else if (exact)
      is(PK::GEMV_CHAIN, (q.N + GEMV_JOBS - 1) / GEMV_JOBS, 1, general);
    else
      is(PK::GEMV_FAST, q.N, 1, general);
  }
  return p;
}

}  // namespace vsim
