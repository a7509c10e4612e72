// vsim_amd/csrc/model.cpp — device-resident model executor (layer 3 of vsim_hip.h).
//
// One eval = the reference's gptneox_eval graph (vsim.cpp:470-747) or the GPT-J graph
// built from the same ggml ops, executed as a fixed sequence of HIP kernels on one
// stream.  Weights (Q4 SoA), LayerNorm/bias vectors, the F32 KV cache
// ([layer][n_ctx][E], vsim.cpp:349-366) and all activations stay in HBM; per eval the
// host sends the token ids and receives one logits row (vsim.cpp:736-737).
// A pipeline stage owns layers [l0, l1); stages exchange the residual inpL ([N][E] f32).
//
// What the host side keeps is described once each: what distinguishes the three graphs
// (GraphDesc: the one prompt layer, run_layer, the head and the decode steps branch on it), the
// operands of a prompt product (Product), what kind of batch runs the layers (BatchDesc) and which
// kernel then runs a product (product_plan.hpp: PromptBatch::mm switches on its answer), the tensors of an
// architecture (arch_table: plan_slots and bind_pointers walk it), the scratch buffers (scratch_table:
// allocated, freed and poisoned from it), the five single-token step graphs (StepGraph
// step[5], captured by decode_graph) and what a step of each kind enqueues (enqueue_step:
// the captured and the eager form are the same call).  LAUNCH brackets a profiled launch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <map>
#include <string>
#include <vector>

#include "common.hpp"
#include "decode_jobs.hpp"
#include "fast.hpp"
#include "sampler.hpp"
#include "../../include/vsim_hip.h"

using namespace vsim;

namespace {

enum Kind { KQ4 = 0, KF32 = 1 };

struct Slot {
  void *ptr;
  int kind;
  int rows, k;  // Q4: rows x k ; F32: k elements (rows = 1)
  int layer;    // -1 for global tensors
  bool loaded;
};

struct LayerW {
  // (BLOOM: wq/wk/wv are the three row blocks of the fused query_key_value tensor, each
  // repacked on its own; bq/bk/bv point into its one bias vector)
  void *wq = nullptr, *wk = nullptr, *wv = nullptr, *wo = nullptr, *wfc = nullptr, *wproj = nullptr;
  float *ln1_w = nullptr, *ln1_b = nullptr, *ln2_w = nullptr, *ln2_b = nullptr;
  float *bq = nullptr, *bk = nullptr, *bv = nullptr, *bo = nullptr, *bfc = nullptr, *bproj = nullptr;
};

// The single-token step, captured once per kind and mode as a hipGraph (decode_graph):
//   STEP_LOGITS  vsim_model_eval: uploads, the decode kernels, the logits copy-out
//   STEP_ARGMAX  the greedy variant: device argmax, 4-byte copy-out instead of the logits
//   STEP_GEN     the device-resident greedy loop (vsim_model_generate): no uploads, no copy-out;
//                the argmax kernel feeds tok_dev / npast_dev and records into hist_dev[n_ctx]
//   STEP_STAGE   the pipeline stage step (vsim_model_stage_*) between the bound device buffers,
//                ending by advancing n_past on the device
//   STEP_SAMPLE  the sampled variant (vsim_model_eval_sample): the sampler's parameter block and
//                window are uploaded too, k_sample_topk follows the decode kernels, and the
//                candidates (TopkOut, 768 bytes) are copied out instead of the logits
enum StepKind { STEP_LOGITS = 0, STEP_ARGMAX = 1, STEP_GEN = 2, STEP_STAGE = 3, STEP_SAMPLE = 4 };
struct StepGraph {
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  int mode = -1;    // the mode it was captured in (-1: recapture on next use)
  int kernels = 0;  // kernels in one replay
};

// What distinguishes the three graphs, filled once from arch and use_parallel_residual
// (model_create_impl); the prompt layer, the head and the decode steps branch on these alone.
enum Rotary { ROT_NONE, ROT_NEOX, ROT_GPTJ };  // none (BLOOM), rotate-half, interleaved pairs
// The MLP's input and the layer's output: parallel (x + attn + ff, the MLP beside the attention);
// serial adding to the old row (GPT-NeoX with use_parallel_residual = 0: the MLP reads
// LN(x + attn), the layer ends x + attn + ff all the same, vsim.cpp:626-658); serial keeping the
// joined row (BLOOM: inpFF = x + attn is the residual, the layer ends inpFF + ff)
enum Residual { RES_PARALLEL, RES_SERIAL_OLD, RES_SERIAL_JOINED };
struct GraphDesc {
  Rotary rotary = ROT_NEOX;
  bool qkvo_bias = true;   // Q, K, V and the out-projection carry biases
  bool alibi = false;      // the softmax adds the head slopes' bias
  bool two_norms = true;   // a LayerNorm of its own for the MLP (false: the input norm feeds both)
  Residual residual = RES_PARALLEL;
  bool emb_norm = false;   // LayerNorm on the embedding rows
  bool lmh_bias = false;   // bias on the lm_head
};

// What a batched decode step (vsim_model_decode_batch) uploads besides the tokens, in one copy:
// each row's slot cache bases and its position
struct BatchWords {
  float *kc[VSIM_BATCH_MAX], *vc[VSIM_BATCH_MAX];
  int32_t npast[VSIM_BATCH_MAX];
};

}  // namespace

struct vsim_model {
  int arch = VSIM_ARCH_GPTNEOX;
  GraphDesc gd;
  unsigned *err_dev = nullptr, *err_host = nullptr;  // this model's bounded-wait timeouts (spin_check)
  unsigned err_seen = 0;
  vsim_hparams hp{};
  int n_ctx = 512, device = 0, l0 = 0, l1 = 0;
  bool first = true, last = true;
  int mode = VSIM_MODE_EXACT;
  bool graph_enabled = false;
  hipStream_t stream = nullptr;

  uint8_t *warena = nullptr;  // all weights of this stage
  size_t wbytes = 0;
  std::map<std::string, Slot> slots;
  std::vector<LayerW> layers;
  void *wte = nullptr, *lmh = nullptr;
  float *lnf_w = nullptr, *lnf_b = nullptr, *lmh_b = nullptr;
  float *emb_w = nullptr, *emb_b = nullptr;  // BLOOM word_embeddings_layernorm
  float *alibi = nullptr;                    // BLOOM: device head slopes [n_head]

  float *kcache = nullptr, *vcache = nullptr;
  // sequence slots 1.. (vsim_model_seq_reserve), each [layers][n_ctx][E] like kcache / vcache,
  // which are slot 0
  std::vector<float *> kslot, vslot;
  double2 *rope_cs = nullptr;

  // scratch, sized for n_max tokens
  int n_max = 0;
  float *inpL = nullptr, *cur1 = nullptr, *cur2 = nullptr, *Qb = nullptr, *Kb = nullptr, *Vb = nullptr;
  float *attn_in = nullptr, *attn = nullptr, *ff = nullptr, *fch = nullptr, *kq = nullptr, *logits = nullptr;
  uint8_t *xq1 = nullptr, *xq2 = nullptr, *xq3 = nullptr;
  float *xd1 = nullptr, *xd2 = nullptr, *xd3 = nullptr;
  int32_t *tok_dev = nullptr;
  int32_t *tok_host = nullptr;  // pinned
  float *logit_host = nullptr;  // pinned
  BatchWords *bw_host = nullptr, *bw_dev = nullptr;  // the batched step's per-row words (pinned, device)
  // weight-only mode's single-token step: slot 0's cache bases {kcache, vcache} on the device, the
  // one-row AttnRows of its k_attn_decode_batch (written when the scratch is allocated)
  float **w4_kv = nullptr;
  unsigned w4_gen = 0;  // vsim_w4a16_set_step's count of changes when the step graphs were last checked
  int kernels_last = 0;

  // fused single-token decode step (layer.hip) and its graphs
  uint8_t *xqa = nullptr;     // attention output, quantized
  float *xda = nullptr;
  float *inpL2 = nullptr;     // second residual buffer (the join alternates between the two)
  float *resid_final = nullptr;  // where the last fused step left the stage's residual
  int *npast_dev = nullptr, *npast_host = nullptr;
  StepGraph step[5];  // by StepKind
  int *am_dev = nullptr, *am_host = nullptr;  // the greedy steps' token
  unsigned long long *am_ws = nullptr;  // the argmax's key and workgroup count (zero between launches)
  int *hist_dev = nullptr;              // STEP_GEN's record [n_ctx]
  // STEP_SAMPLE: the sampler's parameter block (pinned, device), the candidates (device, pinned)
  // and k_sample_topk's workspace (its counter zero between launches)
  TopkParams *sp_host = nullptr, *sp_dev = nullptr;
  TopkOut *so_dev = nullptr, *so_host = nullptr;
  void *tk_ws = nullptr;
  // pipeline stage step (vsim_model_stage_*): device buffers the caller binds (the token in
  // on the first stage, the residual in / out between stages, the greedy token out on the
  // last) and the host's count of enqueued steps (n_ctx bound)
  const int32_t *st_tok_in = nullptr;
  const float *st_resid_in = nullptr;
  float *st_resid_out = nullptr;
  int32_t *st_tok_out = nullptr;
  int st_npast = -1;
  unsigned *tail_done = nullptr;  // the fast decode step's per-head counters (fast_decode.hip)
  // the layer tail's hand-off block (TailSync, TailLn) and its views (decode_jobs.hpp: tail_ws_bytes,
  // tail_ws_carve, null with it); zeroed at allocation (tag 0 never matches)
  void *tail_ws = nullptr;
  TailWs tw;
  // fast-mode decode step (fast_decode.hip): fc_out split-K partial rows and attention
  // chunk partials (both consumed by the layer's k_fast_oproj_join)
  float *fast_ffp = nullptr, *fast_part = nullptr;
  void *pf_scratch = nullptr;  // fast prefill: fp16 K / V^T copies (attn_prefill.hip)
  void *pf_x16 = nullptr;      // fast prefill: fp16 GEMM operands, [n_max][E] then [n_max][4E]
  size_t pf_bytes = 0;
  // scoring (vsim_model_eval_score), allocated on the first scoring call (ensure_score_scratch):
  // one head chunk's logits [score_rows][n_vocab], the targets (pinned, device) and the results
  // (device, pinned: n_max doubles, then n_max ints)
  int score_rows = 0;
  float *score_x = nullptr;
  int32_t *score_tgt = nullptr, *score_tgt_host = nullptr;
  void *score_out = nullptr, *score_out_host = nullptr;
  // the sampled batched step (vsim_model_decode_batch_sample), allocated with them: a parameter
  // block per row (pinned, device), the rows' candidates (device, pinned) and k_sample_topk_rows'
  // workspace (every row's counter zero between launches)
  TopkParams *bs_par_host = nullptr, *bs_par_dev = nullptr;
  TopkOut *bs_out_dev = nullptr, *bs_out_host = nullptr;
  void *bs_ws = nullptr;

  // graph executor's fast path (graph.cpp): weights and KV cache borrowed from its device
  // mirrors (not freed here), the KQV key grouping of the caller's thread count and the
  // scale the graph carries (0: computed from the hparams)
  bool borrowed = false;
  int kqv_nth = 1;
  float attn_scale = 0.0f;

  // F32 / F16 sources on their way to Q4_0 (vsim_model_set_tensor_src, the quantizing loader): two
  // pinned host buffers and their device twins of `cap` bytes each, the copy stream, and per buffer
  // the events "copied to the device" and "quantized"; allocated on first use (quant_reserve)
  struct QuantStage {
    void *host[2] = {nullptr, nullptr}, *dev[2] = {nullptr, nullptr};
    size_t cap = 0;
    hipStream_t copy = nullptr;
    hipEvent_t copied[2] = {nullptr, nullptr}, done[2] = {nullptr, nullptr};
  } qstage;

  // Per-kernel profiling (bench.py's live roofline): with profiling on, the decode step runs
  // eagerly and an event pair brackets every launch, tagged with the kernel's name and the
  // algorithmic bytes it moves (Q4_0 weights at 0.625 B/weight, KV rows, activations).
  struct ProfRec {
    size_t ev;
    std::string kind;
    double bytes;
  };
  struct ProfKind {
    std::string name;
    double ms = 0.0, bytes = 0.0;
    long n = 0;
  };
  bool profile = false;
  int prof_npast = 0;  // n_past of the step being enqueued (host copy, for the KV byte counts)
  std::vector<hipEvent_t> prof_events;
  std::vector<ProfRec> prof_pending;
  size_t prof_used = 0;
  std::vector<ProfKind> prof_kinds;
};

namespace {

int E_(const vsim_model *m) { return m->hp.n_embd; }

// the caches of sequence slot s (0: the model's own)
float *slot_k(const vsim_model *m, int s) { return s == 0 ? m->kcache : m->kslot[s - 1]; }
float *slot_v(const vsim_model *m, int s) { return s == 0 ? m->vcache : m->vslot[s - 1]; }

// ---------------------------------------------------------------- scratch
// Every scratch allocation for n tokens, in allocation order: where the pointer lives, its
// bytes (0: not allocated at this n), and how it is allocated and treated.
// pinned host memory; zero-filled; NaN-filled by debug_poison; scoring's (0 bytes until score_rows is set)
enum { S_PINNED = 1, S_ZERO = 2, S_POISON = 4, S_SCORE = 8 };
struct ScratchBuf {
  void **p;
  size_t bytes;
  int flags;
};

std::vector<ScratchBuf> scratch_table(vsim_model *m, size_t n) {
  const size_t E = E_(m), F = 4 * E, V = m->hp.n_vocab, H = m->hp.n_head, f = sizeof(float);
  const size_t d = E / H, nch = fast_nchunk(m->n_ctx);
  // counters of the fused layer kernels at [0], [64], [128] (separate 256-byte lines)
  // (k_layer_exact: one set per layer, [il - l0][256], zeroed by a memset node per token)
  const size_t ncnt = (size_t)std::max(1, m->l1 - m->l0) * 256;
  std::vector<ScratchBuf> t;
  auto add = [&](auto **p, size_t bytes, int flags = 0) { t.push_back({(void **)p, bytes, flags}); };
  auto q4 = [&](size_t k) { return n * k / QK * QBYTES; };  // n activation rows of k values, Q4_0
  for (float **p : {&m->inpL, &m->cur1, &m->cur2, &m->Qb, &m->Kb, &m->Vb, &m->attn_in, &m->attn, &m->ff})
    add(p, n * E * f, S_POISON);
  add(&m->fch, n * F * f, S_POISON);
  add(&m->kq, n * H * m->n_ctx * f, S_POISON);
  add(&m->logits, V * f, S_POISON);
  add(&m->xq1, q4(E), S_POISON);
  add(&m->xq2, q4(E), S_POISON);
  add(&m->xq3, q4(F), S_POISON);
  add(&m->xd1, n * E * f, S_POISON);
  add(&m->xd2, n * E * f, S_POISON);
  add(&m->xd3, n * F * f, S_POISON);
  add(&m->tok_dev, n * sizeof(int32_t));
  add(&m->tok_host, n * sizeof(int32_t), S_PINNED);
  add(&m->logit_host, V * f, S_PINNED);
  add(&m->bw_host, sizeof(BatchWords), S_PINNED);
  add(&m->bw_dev, sizeof(BatchWords));
  add(&m->w4_kv, 2 * sizeof(float *));
  add(&m->xqa, q4(E), S_POISON);
  add(&m->xda, n * E * f, S_POISON);
  add(&m->inpL2, E * f, S_POISON);
  add(&m->npast_dev, sizeof(int));
  add(&m->npast_host, sizeof(int), S_PINNED);
  add(&m->am_dev, sizeof(int));
  add(&m->am_ws, 2 * sizeof(unsigned long long), S_ZERO);
  add(&m->am_host, sizeof(int), S_PINNED);
  add(&m->hist_dev, (size_t)m->n_ctx * sizeof(int));
  add(&m->sp_host, sizeof(TopkParams), S_PINNED);
  add(&m->sp_dev, sizeof(TopkParams));
  add(&m->so_dev, sizeof(TopkOut));
  add(&m->so_host, sizeof(TopkOut), S_PINNED);
  add(&m->tk_ws, TOPK_WS_BYTES, S_ZERO);
  add(&m->tail_done, ncnt * sizeof(unsigned), S_ZERO);
  add(&m->tail_ws, tail_ws_bytes(E), S_ZERO);  // one allocation, its views in m->tw
  add(&m->fast_ffp, 8 * E * f);
  add(&m->pf_x16, n >= (size_t)GEMM_MIN_N ? n * (E + F) * sizeof(uint16_t) : 0, S_POISON);
  add(&m->fast_part, H * nch * (d + 2) * f, S_ZERO);  // finite stale values
  const size_t sn = m->score_rows ? n : 0, so = sizeof(double) + sizeof(int32_t);
  add(&m->score_x, (size_t)m->score_rows * V * f, S_POISON | S_SCORE);
  add(&m->score_tgt, sn * sizeof(int32_t), S_SCORE);
  add(&m->score_tgt_host, sn * sizeof(int32_t), S_PINNED | S_SCORE);
  add(&m->score_out, sn * so, S_SCORE);
  add(&m->score_out_host, sn * so, S_PINNED | S_SCORE);
  const size_t bs = m->score_rows ? VSIM_BATCH_MAX : 0;
  add(&m->bs_par_host, bs * sizeof(TopkParams), S_PINNED | S_SCORE);
  add(&m->bs_par_dev, bs * sizeof(TopkParams), S_SCORE);
  add(&m->bs_out_dev, bs * sizeof(TopkOut), S_SCORE);
  add(&m->bs_out_host, bs * sizeof(TopkOut), S_PINNED | S_SCORE);
  add(&m->bs_ws, bs * TOPK_WS_BYTES, S_ZERO | S_SCORE);
  return t;
}

void drop(StepGraph &g) {
  if (g.exec) (void)hipGraphExecDestroy(g.exec);
  if (g.graph) (void)hipGraphDestroy(g.graph);
  g = StepGraph{};
}

void free_scratch(vsim_model *m) {
  for (StepGraph &g : m->step) drop(g);  // they hold the scratch addresses
  for (const ScratchBuf &b : scratch_table(m, m->n_max)) {
    if (*b.p) (void)(b.flags & S_PINNED ? hipHostFree(*b.p) : hipFree(*b.p));
    *b.p = nullptr;
  }
  m->tw = tail_ws_carve(m->tail_ws, E_(m));
  if (m->pf_scratch) (void)hipFree(m->pf_scratch);
  m->pf_scratch = nullptr;
  m->pf_bytes = 0;
  m->st_npast = -1;  // the device n_past went with npast_dev: stage_step needs a new stage_begin
  m->n_max = 0;
}

int ensure_scratch(vsim_model *m, int N) {
  if (N <= m->n_max) return VSIM_OK;
  VSIM_HIP(hipStreamSynchronize(m->stream));
  free_scratch(m);
  const int n = N < 16 ? 16 : N;
  for (const ScratchBuf &b : scratch_table(m, n)) {
    if (!b.bytes) continue;
    if (b.flags & S_PINNED)
      VSIM_HIP(hipHostMalloc(b.p, b.bytes, hipHostMallocDefault));
    else
      VSIM_HIP(hipMalloc(b.p, b.bytes));
    if (b.flags & S_ZERO) VSIM_HIP(hipMemset(*b.p, 0, b.bytes));
  }
  m->tw = tail_ws_carve(m->tail_ws, E_(m));
  float *const kv[2] = {m->kcache, m->vcache};
  VSIM_HIP(hipMemcpy(m->w4_kv, kv, sizeof(kv), hipMemcpyHostToDevice));
  m->n_max = n;
  return VSIM_OK;
}

// Scoring's buffers for head chunks of `rows` rows, allocated on the first scoring call (and
// again when a larger chunk is asked for); from then on they follow the scratch's size like
// every other entry of the table.  After ensure_scratch.
int ensure_score_scratch(vsim_model *m, int rows) {
  if (rows <= m->score_rows) return VSIM_OK;
  VSIM_HIP(hipStreamSynchronize(m->stream));
  auto release = [&] {
    for (const ScratchBuf &b : scratch_table(m, m->n_max)) {
      if (!(b.flags & S_SCORE) || !*b.p) continue;
      (void)(b.flags & S_PINNED ? hipHostFree(*b.p) : hipFree(*b.p));
      *b.p = nullptr;
    }
  };
  release();
  m->score_rows = rows;
  for (const ScratchBuf &b : scratch_table(m, m->n_max)) {
    if (!(b.flags & S_SCORE) || !b.bytes) continue;
    const hipError_t e = b.flags & S_PINNED ? hipHostMalloc(b.p, b.bytes, hipHostMallocDefault) : hipMalloc(b.p, b.bytes);
    if (e != hipSuccess || ((b.flags & S_ZERO) && hipMemset(*b.p, 0, b.bytes) != hipSuccess)) {
      if (e != hipSuccess) *b.p = nullptr;
      release();
      m->score_rows = 0;
      return hip_fail(e != hipSuccess ? e : hipErrorUnknown, "score scratch");
    }
  }
  return VSIM_OK;
}

// fast prefill's fp16 K / V^T copies, allocated on first need (prompt evals are never
// graph-captured: allocating there is safe)
int ensure_pf_scratch(vsim_model *m) {
  if (m->pf_scratch) return VSIM_OK;
  m->pf_bytes = attn_prefill_scratch(E_(m), m->n_ctx);
  VSIM_HIP(hipMalloc(&m->pf_scratch, m->pf_bytes));
  return VSIM_OK;
}

// ---------------------------------------------------------------- tensors
// One row per tensor of an architecture: where its device pointer lives (a LayerW member, or
// a model member for the globals), its ggml-file name (globals) or the suffix after the layer
// prefix, and its shape -- Q4: rows x k; F32: k elements.  A global belongs to the first or the
// last stage.
enum Dim { D_E, D_4E, D_V, D_3E };
struct TensorRow {
  const char *name;
  Dim rows, k;
  void *LayerW::*lq;  // exactly one of the four targets is set: layer / global, Q4 / F32
  float *LayerW::*lf;
  void *vsim_model::*gq;
  float *vsim_model::*gf;
  bool first;
  int kind() const { return lq || gq ? KQ4 : KF32; }
};
TensorRow row(void *LayerW::*p, const char *n, Dim rows, Dim k) { return {n, rows, k, p, nullptr, nullptr, nullptr, false}; }
TensorRow row(float *LayerW::*p, const char *n, Dim k) { return {n, D_E, k, nullptr, p, nullptr, nullptr, false}; }
TensorRow row(void *vsim_model::*p, const char *n, Dim rows, Dim k, bool first) {
  return {n, rows, k, nullptr, nullptr, p, nullptr, first};
}
TensorRow row(float *vsim_model::*p, const char *n, Dim k, bool first) {
  return {n, D_E, k, nullptr, nullptr, nullptr, p, first};
}

struct ArchTable {
  const char *layer_prefix;  // + layer index + "." + the row's suffix
  std::vector<TensorRow> globals, layer;
};

const ArchTable &arch_table(int arch) {
  using M = vsim_model;
  using L = LayerW;
  const bool FIRST = true, LAST = false;
  static const ArchTable neox = {
      "gpt_neox.layers.",
      {row(&M::wte, "gpt_neox.embed_in.weight", D_V, D_E, FIRST),
       row(&M::lnf_w, "gpt_neox.final_layer_norm.weight", D_E, LAST),
       row(&M::lnf_b, "gpt_neox.final_layer_norm.bias", D_E, LAST),
       row(&M::lmh, "embed_out.weight", D_V, D_E, LAST)},
      {row(&L::ln1_w, "input_layernorm.weight", D_E),
       row(&L::ln1_b, "input_layernorm.bias", D_E),
       row(&L::ln2_w, "post_attention_layernorm.weight", D_E),
       row(&L::ln2_b, "post_attention_layernorm.bias", D_E),
       row(&L::wq, "attention.query.weight", D_E, D_E),
       row(&L::bq, "attention.query.bias", D_E),
       row(&L::wk, "attention.key.weight", D_E, D_E),
       row(&L::bk, "attention.key.bias", D_E),
       row(&L::wv, "attention.value.weight", D_E, D_E),
       row(&L::bv, "attention.value.bias", D_E),
       row(&L::wo, "attention.dense.weight", D_E, D_E),
       row(&L::bo, "attention.dense.bias", D_E),
       row(&L::wfc, "mlp.dense_h_to_4h.weight", D_4E, D_E),
       row(&L::bfc, "mlp.dense_h_to_4h.bias", D_4E),
       row(&L::wproj, "mlp.dense_4h_to_h.weight", D_E, D_4E),
       row(&L::bproj, "mlp.dense_4h_to_h.bias", D_E)}};
  static const ArchTable bloom = {  // convert_bloom_to_ggml.py:22-34 names
      "layers.",
      {row(&M::wte, "tok_embeddings.weight", D_V, D_E, FIRST),
       row(&M::emb_w, "norm.weight", D_E, FIRST),
       row(&M::emb_b, "norm.bias", D_E, FIRST),
       row(&M::lnf_w, "output_norm.weight", D_E, LAST),
       row(&M::lnf_b, "output_norm.bias", D_E, LAST),
       row(&M::lmh, "output.weight", D_V, D_E, LAST)},
      {row(&L::ln1_w, "attention_norm.weight", D_E),
       row(&L::ln1_b, "attention_norm.bias", D_E),
       row(&L::wq, "attention.query_key_value.weight/q", D_E, D_E),  // the file tensor's row blocks
       row(&L::wk, "attention.query_key_value.weight/k", D_E, D_E),
       row(&L::wv, "attention.query_key_value.weight/v", D_E, D_E),
       row(&L::bq, "attention.query_key_value.bias", D_3E),  // bk, bv: views into it (bind_pointers)
       row(&L::wo, "attention.wo.weight", D_E, D_E),
       row(&L::bo, "attention.wo.bias", D_E),
       row(&L::ln2_w, "ffn_norm.weight", D_E),
       row(&L::ln2_b, "ffn_norm.bias", D_E),
       row(&L::wfc, "feed_forward.w1.weight", D_4E, D_E),
       row(&L::bfc, "feed_forward.w1.bias", D_4E),
       row(&L::wproj, "feed_forward.w2.weight", D_E, D_4E),
       row(&L::bproj, "feed_forward.w2.bias", D_E)}};
  static const ArchTable gptj = {
      "transformer.h.",
      {row(&M::wte, "transformer.wte.weight", D_V, D_E, FIRST),
       row(&M::lnf_w, "transformer.ln_f.weight", D_E, LAST),
       row(&M::lnf_b, "transformer.ln_f.bias", D_E, LAST),
       row(&M::lmh, "lm_head.weight", D_V, D_E, LAST),
       row(&M::lmh_b, "lm_head.bias", D_V, LAST)},
      {row(&L::ln1_w, "ln_1.weight", D_E),
       row(&L::ln1_b, "ln_1.bias", D_E),
       row(&L::wq, "attn.q_proj.weight", D_E, D_E),
       row(&L::wk, "attn.k_proj.weight", D_E, D_E),
       row(&L::wv, "attn.v_proj.weight", D_E, D_E),
       row(&L::wo, "attn.out_proj.weight", D_E, D_E),
       row(&L::wfc, "mlp.fc_in.weight", D_4E, D_E),
       row(&L::bfc, "mlp.fc_in.bias", D_4E),
       row(&L::wproj, "mlp.fc_out.weight", D_E, D_4E),
       row(&L::bproj, "mlp.fc_out.bias", D_E)}};
  return arch == VSIM_ARCH_GPTNEOX ? neox : arch == VSIM_ARCH_BLOOM ? bloom : gptj;
}

// fn(ggml name, row, layer or -1) for every tensor this stage owns: the first stage's globals,
// the last stage's, then layer by layer
template <class Fn>
void for_each_tensor(const vsim_model *m, Fn fn) {
  const ArchTable &t = arch_table(m->arch);
  for (const TensorRow &r : t.globals)
    if (r.first ? m->first : m->last) fn(std::string(r.name), r, -1);
  for (int i = m->l0; i < m->l1; ++i) {
    const std::string p = t.layer_prefix + std::to_string(i) + ".";
    for (const TensorRow &r : t.layer) fn(p + r.name, r, i);
  }
}

// Register every tensor this stage owns, with its ggml-file name and shape.
void plan_slots(vsim_model *m, std::vector<std::pair<std::string, Slot>> &out) {
  const int E = m->hp.n_embd;
  auto dim = [&](Dim d) { return d == D_E ? E : d == D_4E ? 4 * E : d == D_3E ? 3 * E : m->hp.n_vocab; };
  for_each_tensor(m, [&](const std::string &n, const TensorRow &r, int layer) {
    out.push_back({n, Slot{nullptr, r.kind(), r.kind() == KQ4 ? dim(r.rows) : 1, dim(r.k), layer, false}});
  });
}

// bytes of the tensor in the ggml file (AoS blocks) and on the device (W4T32, padded)
size_t slot_bytes(const Slot &s) {
  return s.kind == KQ4 ? (size_t)s.rows * s.k / QK * QBYTES : (size_t)s.k * sizeof(float);
}
size_t slot_dev_bytes(const Slot &s) { return s.kind == KQ4 ? w4_bytes(s.rows, s.k) : (size_t)s.k * sizeof(float); }

void bind_pointers(vsim_model *m) {
  m->layers.assign(m->l1 - m->l0, LayerW{});
  for_each_tensor(m, [&](const std::string &n, const TensorRow &r, int layer) {
    auto it = m->slots.find(n);
    void *p = it == m->slots.end() ? nullptr : it->second.ptr;
    if (r.gq) m->*r.gq = p;
    if (r.gf) m->*r.gf = (float *)p;
    if (r.lq) m->layers[layer - m->l0].*r.lq = p;
    if (r.lf) m->layers[layer - m->l0].*r.lf = (float *)p;
  });
  if (m->arch == VSIM_ARCH_BLOOM)  // q | k | v of the one query_key_value bias vector
    for (LayerW &L : m->layers) {
      L.bk = L.bq + m->hp.n_embd;
      L.bv = L.bq + 2 * m->hp.n_embd;
    }
}

// BLOOM's fused query_key_value weight: one file tensor, three [E][E] row blocks q | k | v,
// each a slot of its own (name + QKV_PARTS[i])
const char *const QKV_PARTS[3] = {"/q", "/k", "/v"};
bool is_fused_qkv(const vsim_model *m, const std::string &n) {
  const std::string suf = "attention.query_key_value.weight";
  return m->arch == VSIM_ARCH_BLOOM && n.size() >= suf.size() && n.compare(n.size() - suf.size(), suf.size(), suf) == 0;
}

#define RC(x)                    \
  do {                           \
    int rc_ = (x);               \
    if (rc_) return rc_;         \
  } while (0)

// part(slot name, byte offset, bytes) for each of a fused tensor's row blocks: the caller's
// nbytes in thirds.  `who` prefixes the error message.
template <class Fn>
int for_qkv_parts(const std::string &n, size_t nbytes, const char *who, Fn part) {
  if (nbytes % 3 != 0) { set_error(std::string(who) + ": fused qkv size"); return VSIM_EINVAL; }
  for (int i = 0; i < 3; ++i) RC(part((n + QKV_PARTS[i]).c_str(), i * (nbytes / 3), nbytes / 3));
  return VSIM_OK;
}

// Bounded cross-workgroup waits that gave up (k_layer_tail, the barrier-free chain GEMV, the
// stream-K finisher) count into the model's own device word (m->err_dev: every launch this model
// enqueues gets it through ErrScope, so another model's or a standalone op's timeout never fails
// this one).  spin_read enqueues its copy to pinned host memory ahead of the call's stream sync;
// spin_check, after that sync, fails the call with VSIM_ESPIN when it grew: some tile went on
// with incomplete data, so the results are not the reference's.
struct ErrScope {
  unsigned *old;
  explicit ErrScope(vsim_model *m) : old(set_spin_error_target(m->err_dev)) {}
  ~ErrScope() { set_spin_error_target(old); }
};
int spin_read(vsim_model *m) {
  VSIM_HIP(hipMemcpyAsync(m->err_host, m->err_dev, sizeof(unsigned), hipMemcpyDeviceToHost, m->stream));
  return VSIM_OK;
}
int spin_check(vsim_model *m) {
  const unsigned n = *(volatile unsigned *)m->err_host;
  if (n > m->err_seen) {
    const unsigned grew = n - m->err_seen;
    m->err_seen = n;
    add_model_spin_timeouts(grew);
    // a workgroup that gave up may have left the argmax workspace mid-update: zero it again
    (void)hipMemsetAsync(m->am_ws, 0, 2 * sizeof(unsigned long long), m->stream);
    (void)hipMemsetAsync(m->tk_ws, 0, sizeof(unsigned), m->stream);
    (void)hipStreamSynchronize(m->stream);
    set_error("a bounded cross-workgroup wait gave up " + std::to_string(grew) +
              " time(s) in this call (device " + std::to_string(m->device) + "): results not valid");
    return VSIM_ESPIN;
  }
  return VSIM_OK;
}

// Profiling brackets (eager launches only): prof_begin records the start event and returns
// its slot (-1 when profiling is off); prof_end records the end and tags the pair.
long prof_begin(vsim_model *m) {
  if (!m->profile) return -1;
  if (m->prof_used + 2 > m->prof_events.size()) {
    hipEvent_t a, b;
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return -1;
    m->prof_events.push_back(a);
    m->prof_events.push_back(b);
  }
  const size_t i = m->prof_used;
  m->prof_used += 2;
  (void)hipEventRecord(m->prof_events[i], m->stream);
  return (long)i;
}
void prof_end(vsim_model *m, long ev, const std::string &kind, double bytes) {
  if (ev < 0) return;
  (void)hipEventRecord(m->prof_events[ev + 1], m->stream);
  m->prof_pending.push_back({(size_t)ev, kind, bytes});
}
// after the stream synchronised: fold the pending pairs into the per-kernel totals
int prof_collect(vsim_model *m) {
  for (const auto &r : m->prof_pending) {
    float ms = 0.0f;
    VSIM_HIP(hipEventElapsedTime(&ms, m->prof_events[r.ev], m->prof_events[r.ev + 1]));
    size_t k = 0;
    while (k < m->prof_kinds.size() && m->prof_kinds[k].name != r.kind) ++k;
    if (k == m->prof_kinds.size()) {
      m->prof_kinds.emplace_back();
      m->prof_kinds.back().name = r.kind;
    }
    m->prof_kinds[k].ms += ms;
    m->prof_kinds[k].bytes += r.bytes;
    m->prof_kinds[k].n += 1;
  }
  m->prof_pending.clear();
  m->prof_used = 0;
  return VSIM_OK;
}

// One launch between its profiling brackets, counted into nk.  A macro so that the name (some
// are built as std::string) and the bytes are evaluated only when profiling is on.
#define LAUNCH(m, nk, call, name, bytes)                   \
  do {                                                     \
    const long ev_ = prof_begin(m);                        \
    RC(call);                                              \
    if (ev_ >= 0) prof_end(m, ev_, name, bytes);           \
    ++nk;                                                  \
  } while (0)

double w4_algo_bytes(const W4 &w) { return (double)w.rows * w.k / QK * QBYTES; }

// The heads of one decode step's layer (attn.hpp) on this layer's Q / K / V rows in Qb / Kb / Vb:
// the attention output leaves quantized in the row(s) o, every head over nsplit workgroups.  The
// cache and the position come with attn_job: the layer's and the device position of the single-token
// step; null for a rows batch, whose rows each have their own (AttnRows).
AttnDesc decode_attn_desc(const vsim_model *m, const DevTables &tab, const ActRow &o, int nsplit) {
  const GraphDesc &G = m->gd;
  const int E = m->hp.n_embd, H = m->hp.n_head;
  return AttnDesc{.d = E / H, .H = H, .n_rot = G.rotary == ROT_NONE ? 0 : m->hp.n_rot,
                  .style = G.rotary == ROT_GPTJ ? 1 : 0, .n_ctx = m->n_ctx, .nsplit = nsplit, .kqv_nth = m->kqv_nth,
                  .scale = m->attn_scale != 0.0f ? m->attn_scale : default_attn_scale(E, H),
                  .alibi = G.alibi ? m->alibi : nullptr, .q = m->Qb, .k = m->Kb, .v = m->Vb, .cs = m->rope_cs,
                  .etab = tab.exp_f16, .o = o};
}

// One product of a Q4_0 weight with the batch's activation rows (PromptBatch::mm).  Every operand
// defaults to absent; a call site names what it sets (designated initializers, in this order).
struct Product {
  W4 w{};                     // the weight, [M = w.rows][K = w.k]
  const float *x = nullptr;   // the rows as f32 ...
  uint8_t *xq = nullptr;      // ... and as Q4 activations with their factors xd:
  float *xd = nullptr;
  bool quantize = false;      // made from x by this call, or left there by an earlier one
  const float *bias = nullptr;
  float *y = nullptr;
  // fast-mode prompt batches: the rows are already the GEMM's fp16 operand (launch_act_quant_f16,
  // launch_norm_f16q), and x / xq / xd go unused
  const void *x16 = nullptr;
  // fc_in of a long prompt: bias gq_bias + GELU + quantize of the product straight into the next
  // GEMM's fp16 operand gq, in the GEMM's epilogue
  void *gq = nullptr;
  const float *gq_bias = nullptr;
  const G2Epi *epi = nullptr;  // RoPE or the residual join in the long prompt GEMM's epilogue
  const char *what = nullptr;  // the profile's name for the product instead of the kernel's
  bool fused = false;          // out: the GELU-quantize or the G2Epi epilogue ran
};

// What a batch of N rows on its way through the layers and the head is, said once by the caller
// (designated initializers, in this order) and read by enqueue_prompt, run_layer and run_head.
struct BatchDesc {
  BatchKind kind = BatchKind::PROMPT;
  int N = 1;
  int n_past = 0;  // the prompt kinds' position (a rows batch has one per row, in `rows`)
  // the prompt kinds' KV cache ([layers][n_ctx][E] each): the model's own or a sequence slot's
  float *kcache = nullptr, *vcache = nullptr;
  // the rows kinds' per-row slot cache bases and positions, on the device
  const BatchWords *rows = nullptr;
  // The products' mode: the model's for a prompt; the call's for a rows batch (decode_batch is
  // exact, decode_batch_fast fast, whatever the model's mode)
  int mode = VSIM_MODE_EXACT;
  const char *who = "";  // prefixes the error messages
  // a rows batch of vsim_model_decode_runs: rows may share a cache (at distinct positions), so the
  // attention is k_kv_rows + the heads without their cache writes instead of the one launch
  bool runs = false;
};

// A batch on its way through the layers and the head, counting its launches into nk.  What
// follows from the descriptor is derived here (pf) and in product_plan (the products' kernels).
struct PromptBatch {
  vsim_model *m;
  const BatchDesc &D;
  const int N;
  int &nk;
  // fast-mode prompt batch: every activation goes once from f32 to the GEMM's fp16 operand
  // (quantize_row_q4_0 values, k_act_quant_f16; the GELU folded into fc_out's), in the model's
  // scratch pf_x16: xa [N][E] norm outputs, then xb [N][F] attention / GELU outputs.  A rows
  // batch keeps the Q4 rows at every N.
  bool pf;
  void *xa, *xb;
  PromptBatch(vsim_model *m_, const BatchDesc &D_, int &nk_)
      : m(m_), D(D_), N(D_.N), nk(nk_), pf(!is_rows(D_.kind) && f16_gemm_rows(D_.mode, D_.N) && m_->pf_x16),
        xa(pf ? m_->pf_x16 : nullptr), xb(pf ? (void *)((uint16_t *)m_->pf_x16 + (size_t)N * E_(m_)) : nullptr) {}

  int act16(const float *x, int K, void *x16, const float *gbias, bool gelu) {
    if (!pf) return VSIM_OK;
    ++nk;
    return launch_act_quant_f16(x, K, N, gbias, gelu, x16, m->stream);
  }
  // LayerNorm + affine (vsim.cpp:526-533); fast-mode batch: straight to the GEMM's fp16 operand
  int norm(const float *x, float *y, const float *w, const float *b, void *x16) {
    ++nk;
    return pf ? launch_norm_f16q(x, x16, E_(m), N, w, b, m->stream) : launch_norm(x, y, E_(m), N, w, b, m->stream);
  }
  // Quantize the activation (unless it is an fp16 operand already) and run the product on the
  // kernel product_plan names.
  int mm(Product &P) {
    const int M = P.w.rows, K = P.w.k;
    hipStream_t s = m->stream;
    const ProductPlan pl = product_plan({.kind = D.kind, .mode = D.mode, .N = N, .M = M, .K = K, .x16 = P.x16 != nullptr,
                                         .gelu = P.gq && P.gq_bias, .epi = P.epi != nullptr, .gemm = batch_gemm(),
                                         .fast_gemm = batch_fast_gemm(), .w4a16_tile = w4a16_tile_gemm()});
    P.fused = pl.fused;
    if (pl.error) { set_error(pl.error); return VSIM_EINVAL; }
    // Weight-only mode never quantizes: the rows' fp16 operand (launch_w4a16_rows) takes the place
    // of the Q4 rows in P.xq / P.xd (w4a16_operand), made and shared under the same `quantize` flag
    const W4a16Operand o = w4a16_operand({{P.xq}, P.xd});
    if (P.quantize && pl.w4a16) {
      LAUNCH(m, nk, launch_w4a16_rows(P.x, K, N, o.h, o.e, s), "k_w4a16_rows", (double)N * K * 6);
    } else if (P.quantize && !P.x16) {
      RC(launch_q4_quantize(P.x, K, N, P.xq, P.xd, s));
      ++nk;
    }
    const long ev = prof_begin(m);
    if (pl.w4a16_tile) RC(launch_gemm_w4a16_tile(P.w, o.h, o.e, N, P.bias, P.y, s));
    else if (pl.w4a16) RC(launch_gemm_w4a16_rows(P.w, o.h, o.e, N, P.bias, P.y, s));
    switch (pl.kernel) {
      case ProductKernel::GEMM_F16_256:
        RC(launch_gemm_q4_256(P.w, P.x16, N, pl.gelu ? P.gq_bias : P.bias, P.y, s, pl.gelu ? P.gq : nullptr,
                              pl.gelu ? nullptr : P.epi));
        break;
      case ProductKernel::GEMM_F16:
        RC(P.x16 ? launch_gemm_f16x(P.w, P.x16, N, P.bias, P.y, s) : launch_gemm_q4_f16(P.w, P.xq, N, P.bias, P.y, s));
        break;
      case ProductKernel::GEMM_EXACT: RC(launch_gemm_exact(P.w, P.xd, N, P.bias, P.y, s)); break;
      case ProductKernel::GEMM_EXACT_ROWS: RC(launch_gemm_exact_rows(P.w, P.xd, N, P.bias, P.y, s)); break;
      // (launch_gemm_fast_rows asks the same plan of the same switch: vsim_op_q4_gemm_fast_rows' contract)
      case ProductKernel::GEMM_FAST_ROWS: RC(launch_gemm_fast_rows(P.w, P.xq, N, P.bias, P.y, s)); break;
      case ProductKernel::GEMV_CHAIN: RC(launch_gemv_rows(P.w, P.xq, P.xd, N, GEMV_JOBS, P.bias, P.y, D.mode, s)); break;
      case ProductKernel::GEMV_FAST: RC(launch_gemv_rows(P.w, P.xq, P.xd, N, 1, P.bias, P.y, D.mode, s)); break;
      case ProductKernel::NONE: break;
    }
    if (ev >= 0) prof_end(m, ev, P.what ? P.what : pl.name, w4_algo_bytes(P.w) * pl.passes);
    nk += pl.kernels;
    return VSIM_OK;
  }
};

// One layer of a prompt batch, for all three graphs: LN -> Q/K/V (+bias) -> KV write (+ RoPE) ->
// KQ -> scale (-> ALiBi) -> mask -> softmax -> KQV -> out-projection (+bias) -> the MLP's input ->
// fc_in (+bias) -> GELU -> fc_out (+bias) -> residual join (GPT-NeoX: vsim.cpp:526-695; BLOOM:
// oracle eval_bloom, inpFF = attn + inpL -> LN -> w1 -> GELU -> w2 -> inpL = ff + inpFF).  What
// differs between them is GraphDesc's.
bool w4a16_attn16(const vsim_model *m);  // (below, with the mode's switches)

int run_layer(PromptBatch &B, int il) {
  vsim_model *m = B.m;
  const GraphDesc &G = m->gd;
  const LayerW &L = m->layers[il - m->l0];
  const BatchDesc &D = B.D;
  const bool rows = is_rows(D.kind), w4a16 = D.mode == VSIM_MODE_W4A16;
  const int N = D.N, n_past = D.n_past, E = m->hp.n_embd, H = m->hp.n_head, d = E / H, F = 4 * E;
  int &nk = B.nk;
  hipStream_t s = m->stream;
  RC(B.norm(m->inpL, m->cur1, L.ln1_w, L.ln1_b, B.xa));
  const size_t loff = (size_t)(il - m->l0) * m->n_ctx * E;
  float *kc = rows ? nullptr : D.kcache + loff, *vc = rows ? nullptr : D.vcache + loff;
  // long GPT-J prompt: RoPE and the KV-cache write (vsim.cpp:553-580) in the Q/K/V GEMMs'
  // epilogues -- K and V straight into their cache rows -- instead of a pass of their own
  const bool g2 = wide_gemm(B.pf, N, E);  // (the layer's products: K = E, or 4 E for fc_out)
  const bool rope_epi = g2 && G.rotary == ROT_GPTJ;
  G2Epi er;
  er.cs = m->rope_cs;
  er.d = d;
  er.n_rot = m->hp.n_rot;
  er.p0 = n_past;
  float *kout = rope_epi ? kc + (size_t)n_past * E : m->Kb, *vout = rope_epi ? vc + (size_t)n_past * E : m->Vb;
  // ... and the new keys' fp16 copies for the prompt attention (K rows, V^T columns), which
  // then converts only the cached keys before them.  (ALiBi lives in the softmax kernel only:
  // BLOOM keeps the KQ / softmax / KQV kernels in both modes.)
  const bool attn16 = !rows && !G.alibi && D.mode == VSIM_MODE_FAST && N >= 8 && attn_prefill_supported(d) && E % 64 == 0;
  // weight-only mode's fp16 attention (attn_w4a16.hip, vsim_w4a16_set_attn): every path of the model
  // at every N, the prompt kinds on the tile form, the rows kind on the single-query form
  const bool wattn = w4a16 && w4a16_attn16(m);
  if (attn16 || (wattn && !rows)) RC(ensure_pf_scratch(m));
  const bool kv16_epi = rope_epi && attn16;
  G2Epi ek = er, ev;
  if (kv16_epi) {
    ek.h16 = attn_prefill_k16(m->pf_scratch, E, n_past + N);
    ev.h16 = attn_prefill_vt16(m->pf_scratch, E, n_past + N);
    ev.h16_t = 1;
    ev.h16_ld = attn_prefill_ldt(n_past + N);
    ev.p0 = n_past;
  }
  // Q, K, V (+ bias, vsim.cpp:540-547) on the input norm's rows, which Q's call quantizes for all
  // three; a long GPT-J prompt's Q and K (both RoPE epilogues, no bias) as one launch of both
  // tile grids
  Product q{.w = w4_view(L.wq, E, E), .x = m->cur1, .xq = m->xq1, .xd = m->xd1, .quantize = true,
            .bias = G.qkvo_bias ? L.bq : nullptr, .y = m->Qb, .x16 = B.xa, .epi = rope_epi ? &er : nullptr};
  Product k{.w = w4_view(L.wk, E, E), .xq = m->xq1, .xd = m->xd1, .bias = G.qkvo_bias ? L.bk : nullptr, .y = kout,
            .x16 = B.xa, .epi = rope_epi ? &ek : nullptr};
  Product v{.w = w4_view(L.wv, E, E), .xq = m->xq1, .xd = m->xd1, .bias = G.qkvo_bias ? L.bv : nullptr, .y = vout,
            .x16 = B.xa, .epi = kv16_epi ? &ev : nullptr};
  if (rope_epi && gemm_pair_enabled(E, E)) {
    LAUNCH(m, nk, launch_gemm_q4_256_pair(q.w, k.w, B.xa, N, m->Qb, kout, er, ek, s), "k_gemm_f16_256 (prompt)",
           2.0 * E * E / QK * QBYTES);
  } else {
    RC(B.mm(q));
    RC(B.mm(k));
  }
  RC(B.mm(v));
  const float scale = default_attn_scale(E, H);
  if (rows) {
    // batched decode step: RoPE, the cache write, KQ, softmax, KQV and the out-projection's
    // activation quantize of every row in one launch, each row on its own cache at its own
    // position (attn.hpp, the single-token step's head); Q4 rows in launch_q4_quantize's layout
    DevTables tab;
    RC(tables_get(&tab));
    AttnJob A = attn_job(decode_attn_desc(m, tab, ActRow{q4_rows(m->xq2, E, N), m->xd2}, 1), nullptr, nullptr, nullptr);
    if (w4a16) A.out = m->attn_in;  // the out-projection's operand is made from the f32 row
    const AttnRows R{D.rows->kc, D.rows->vc, loff, D.rows->npast};
    if (D.runs) {
      if (wattn)
        LAUNCH(m, nk, launch_attn_w4a16_runs(A, R, N, s), "k_kv_rows + k_attn_w4a16_runs", 0.0);
      else
        LAUNCH(m, nk, launch_attn_decode_runs(A, R, N, m->n_ctx, s), "k_kv_rows + k_attn_decode_runs", 0.0);
      ++nk;  // (two launches)
    } else if (wattn) {
      LAUNCH(m, nk, launch_attn_w4a16_rows(A, R, N, s), "k_attn_w4a16_rows", 0.0);
    } else {
      LAUNCH(m, nk, launch_attn_decode_batch(A, R, N, m->n_ctx, s), "k_attn_decode_batch", 0.0);
    }
  } else if (!rope_epi) {
    RC(launch_rope_kv_write(G.rotary == ROT_GPTJ ? 1 : 0, m->Qb, m->Kb, m->Vb, kc, vc, d, H, N, n_past,
                            G.rotary == ROT_NONE ? 0 : m->hp.n_rot, m->rope_cs, s));
    ++nk;
  }
  // attention (vsim.cpp:583-616)
  const int nkv = n_past + N;
  // (head dim 256: the attention writes the out-projection's fp16 operand itself)
  const bool attn_q16 = attn16 && B.pf && attn_prefill_quantizes(d);
  if (rows) {
    // (done above, the out-projection's Q4 rows included)
  } else if (attn16) {
    // fast-mode prompt: one-pass fp16 MFMA attention (attn_prefill.hip)
    RC(launch_attn_prefill_f16(m->Qb, kc, vc, d, H, N, n_past, scale, m->attn_in, s, m->pf_scratch, m->pf_bytes,
                               kv16_epi, attn_q16 ? B.xb : nullptr));
    nk += 2;
  } else if (wattn) {
    LAUNCH(m, nk, launch_attn_w4a16_tile(m->Qb, kc, vc, d, H, N, n_past, scale, m->attn_in, s, m->pf_scratch, m->pf_bytes),
           "k_attn_w4a16_tile", 2.0 * nkv * E * sizeof(float));
    ++nk;  // (k_kv_f16 before it)
  } else {
    RC(launch_kq(kc, E, m->Qb, E, d, H, nkv, N, m->kq, s, n_past)); ++nk;
    RC(launch_attn_softmax(m->kq, nkv, N, H, n_past, scale, s, G.alibi ? m->alibi : nullptr, w4a16)); ++nk;
    RC(launch_kqv(vc, E, m->kq, d, H, nkv, N, m->attn_in, 1, s, n_past)); ++nk;
  }
  if (!attn_q16) RC(B.act16(m->attn_in, E, B.xb, nullptr, false));
  Product o{.w = w4_view(L.wo, E, E), .x = m->attn_in, .xq = m->xq2, .xd = m->xd2, .quantize = !rows || w4a16,
            .bias = G.qkvo_bias ? L.bo : nullptr, .y = m->attn, .x16 = B.xb};
  RC(B.mm(o));
  // fc_in (its bias goes with the GELU) reads the input norm's quantized row again, or the MLP's
  // own norm: of x (parallel), or of x + attn, joined in cur2 (vsim.cpp:631-649) and normalized in
  // place -- unless the joined row is the residual and stays there (BLOOM: the norm goes to cur1)
  const bool serial = G.residual != RES_PARALLEL, keep_joined = G.residual == RES_SERIAL_JOINED;
  Product fi{.w = w4_view(L.wfc, F, E), .xq = m->xq1, .xd = m->xd1, .y = m->fch, .x16 = B.xa, .gq = B.xb,
             .gq_bias = L.bfc};
  if (G.two_norms) {
    if (serial) {
      VSIM_HIP(hipMemcpyAsync(m->cur2, m->attn, sizeof(float) * N * E, hipMemcpyDeviceToDevice, s));
      RC(launch_add_bias(m->cur2, m->inpL, N * E, 1, s)); ++nk;  // cur + inpL elementwise
    }
    float *ny = keep_joined ? m->cur1 : m->cur2;
    RC(B.norm(serial ? m->cur2 : m->inpL, ny, L.ln2_w, L.ln2_b, B.xa));
    fi.x = ny;
    fi.xq = m->xq2;
    fi.xd = m->xd2;
    fi.quantize = true;
  }
  RC(B.mm(fi));
  if (B.pf) {
    if (!fi.fused) RC(B.act16(m->fch, F, B.xb, L.bfc, true));  // bias + GELU + quantize, one pass
  } else {
    RC(launch_gelu(m->fch, m->fch, N * F, L.bfc, F, s)); ++nk;
  }
  // fc_out; a long prompt joins the residual in its epilogue (vsim.cpp:694-695 or 657), except
  // BLOOM's, whose residual is cur2
  G2Epi ej;
  ej.res = m->inpL;
  ej.res_a = serial ? nullptr : m->attn;
  const bool join_epi = g2 && !keep_joined;
  Product fo{.w = w4_view(L.wproj, E, F), .x = m->fch, .xq = m->xq3, .xd = m->xd3, .quantize = true, .bias = L.bproj,
             .y = join_epi ? m->inpL : m->ff, .x16 = B.xb, .epi = join_epi ? &ej : nullptr};
  RC(B.mm(fo));
  if (fo.fused != join_epi) {
    set_error("prompt layer: residual epilogue not taken");
    return VSIM_EINVAL;
  }
  if (keep_joined) {  // inpL = ff + inpFF
    VSIM_HIP(hipMemcpyAsync(m->inpL, m->cur2, sizeof(float) * N * E, hipMemcpyDeviceToDevice, s));
    RC(launch_add_bias(m->inpL, m->ff, N * E, 1, s)); ++nk;
  } else if (!join_epi) {
    RC(launch_add_residual(m->inpL, m->attn, m->ff, N * E, serial ? 1 : 0, s));
    ++nk;
  }
  return VSIM_OK;
}

// Fast-mode single-token step (fast_decode.hip): 3 launches per layer.  Same buffers and
// the same replayable form as enqueue_decode (token and n_past from device memory).
// Shapes the fast step handles: head dim a multiple of 32 up to 256, rotary pairs inside one
// 32-row tile (GPT-J pairs; GPT-NeoX rotate-half with n_rot <= 32), n_embd <= 8192.
// The launches' arguments come from decode_jobs.hpp (fast_gemv, fast_tail_job, fast_oproj_job).
bool fast_decode_ok(const vsim_model *m) {
  const int E = m->hp.n_embd, H = m->hp.n_head, d = E / H;
  const int nch = fast_nchunk(m->n_ctx);
  return d % 32 == 0 && d <= 256 && E <= 8192 && E % 128 == 0 &&
         m->gd.residual == RES_PARALLEL && (m->gd.rotary == ROT_GPTJ || m->hp.n_rot <= 32) && 2 * H * nch <= 4096 &&
         nch <= FD_MAXCH;  // (launch_fast_tail's limit: a longer context takes the exact step)
}

int enqueue_decode_fast(vsim_model *m, int &nk) {
  const int E = m->hp.n_embd, H = m->hp.n_head, d = E / H, F = 4 * E, V = m->hp.n_vocab;
  const GraphDesc &G = m->gd;
  hipStream_t s = m->stream;
  DevTables tab;
  RC(tables_get(&tab));
  // the Q4 rows of the step: fc_in's GELU output, the attention output (the norms' stay in LDS)
  const Q4Rows x3 = q4_rows(m->xq3, F), xa = q4_rows(m->xqa, E);
  if (m->first) {
    RC(launch_get_rows(m->wte, E, V, m->tok_dev, 1, m->inpL, s));
    ++nk;
  }
  const int sf = fast_sf(E);
  const FastPos pos{m->npast_dev, m->rope_cs, d, m->hp.n_rot, G.rotary == ROT_GPTJ ? 1 : 0};
  const double kv_bytes = 2.0 * ((double)m->prof_npast + 1) * E * sizeof(float);
  float *R[2] = {m->inpL, m->inpL2};
  int cur = 0;
  for (int il = m->l0; il < m->l1; ++il) {
    const LayerW &L = m->layers[il - m->l0];
    const size_t loff = (size_t)(il - m->l0) * m->n_ctx * E;
    // LayerNorm(s) -> Q4 activations in the GEMV's prologue (GPT-J: one LayerNorm feeds
    // attention and MLP), then {fc_in -> GELU -> quantize, Q, K, V}
    const float *bq = G.qkvo_bias ? L.bq : nullptr, *bk = G.qkvo_bias ? L.bk : nullptr,
                *bv = G.qkvo_bias ? L.bv : nullptr, *bo = G.qkvo_bias ? L.bo : nullptr;
    float *kc = m->kcache + loff, *vc = m->vcache + loff;
    const NormRow n1{L.ln1_w, L.ln1_b}, n2{L.ln2_w, L.ln2_b};
    const FastJob jobs[4] = {fast_job(L.wfc, F, E, L.bfc, nullptr, FE_GELU_Q, 1),
                             fast_job(L.wq, E, E, bq, m->Qb, FE_ROPE_Q, 0), fast_job(L.wk, E, E, bk, kc, FE_ROPE_K, 0),
                             fast_job(L.wv, E, E, bv, vc, FE_V, 0)};
    const FastAct act{.lnx = R[cur], .n = {n1, G.two_norms ? n2 : n1}};
    // (clears K2's per-head counters, tail_done[4h])
    const FastGemv P = fast_gemv(act, jobs, 4, tab.gelu_f16, x3, pos, m->tail_done, 4 * H);
    LAUNCH(m, nk, launch_fast_gemv(P, E, s), "k_fast_gemv (fc_in, Q, K, V)",
           w4_algo_bytes(P.j[0].w) + 3 * w4_algo_bytes(P.j[1].w));
    // fc_out split over K | attention chunks, the last of a head merging them
    const FastTail T = fast_tail_job(
        w4_view(L.wproj, E, F), x3, m->fast_ffp, sf,
        FastAttn{.q = m->Qb, .kc = kc, .vc = vc, .npast = m->npast_dev, .d = d, .H = H, .nchunk = fast_nchunk(m->n_ctx),
                 .scale = default_attn_scale(E, H), .part = m->fast_part, .hcnt = m->tail_done, .o = xa});
    LAUNCH(m, nk, launch_fast_tail(T, s), "k_fast_tail (fc_out + attention)", w4_algo_bytes(T.wf) + kv_bytes);
    // out-projection + residual join into the other buffer
    const FastOproj O = fast_oproj_job(w4_view(L.wo, E, E), xa, bo, m->fast_ffp, sf, L.bproj, R[cur], R[cur ^ 1]);
    LAUNCH(m, nk, launch_fast_oproj_join(O, s), "k_fast_oproj_join", w4_algo_bytes(O.w));
    cur ^= 1;
  }
  if (m->last) {
    const NormRow nf{m->lnf_w, m->lnf_b};
    const FastJob head = fast_job(m->lmh, V, E, G.lmh_bias ? m->lmh_b : nullptr, m->logits, FE_STORE, 0);
    const FastAct act{.lnx = R[cur], .n = {nf, nf}};
    const FastGemv P = fast_gemv(act, &head, 1, nullptr, Q4Rows{}, FastPos{}, nullptr, 0);
    LAUNCH(m, nk, launch_fast_gemv(P, E, s), "k_fast_gemv (lm_head)", w4_algo_bytes(P.j[0].w));
  }
  m->resid_final = R[cur];
  return VSIM_OK;
}

// Exact mode: the single-token decode step as fused launches per layer (layer.hip,
// gemv_chain.hip).  Reads the token from tok_dev and n_past from npast_dev, so the enqueued
// sequence is replayable (hipGraph).
//   1. k_ln_quant: (join of the previous layer +) input LayerNorm (+ post_attention
//      LayerNorm for GPT-NeoX), quantized -- since r06 only for the first layer of the step
//      (or when the previous tail could not run it, TailLn)
//   2. k_gemv_solo: {fc_in (+ bias, GELU, requantize), Q, K, V}
//   3. k_layer_tail: fc_out beside the attention heads and the out-projection, then the join
//      and the next layer's LayerNorm(s) (or the final norm) quantized (TailLn; without it the
//      biases join in the next step 1)
// fc_out's K = 4E chain (vsim.cpp:680-690) is the layer's longest dependency, so the
// attention branch fills the CUs beside it instead of running before it.
// Serial-residual graphs (BLOOM; GPT-NeoX with use_parallel_residual = 0, vsim.cpp:626-658)
// feed the MLP from the attention's residual, so nothing runs beside fc_out; 6 launches:
//   1. k_ln_quant (join of the previous layer's MLP output +) input LayerNorm
//   2. GEMV {Q, K, V} (+ bias)
//   3. k_layer_tail without fc_out: the heads (BLOOM: ALiBi) and the out-projection
//   4. k_ln_quant: attn + bias + x joined, post-attention LayerNorm (BLOOM keeps the joined
//      row as the residual, inpFF; GPT-NeoX's serial graph adds the MLP to the old one)
//   5. GEMV fc_in (+ bias, GELU, requantize)       6. GEMV fc_out
// What one enqueue of that step carries from launch to launch, and its recurring launches (their
// jobs from decode_jobs.hpp).
struct DecodeStep {
  vsim_model *m;
  int &nk;
  const DevTables tab;
  hipStream_t s;
  const int E, F;
  // the Q4 rows of the step: norm 1's, norm 2's, fc_in's GELU output, the attention output
  const ActRow x1, x2, x3, xa;
  // The residual join of layer l (inpL += attn + ff, vsim.cpp:694-695) runs inside layer
  // l+1's LayerNorm kernel (or the final norm); the joined row goes to the other of the two
  // residual buffers, so both norm workgroups of GPT-NeoX can read the old one.
  float *R[2];
  int cur = 0;
  LnJoin pend;           // the join the last layer left to the next norm (jout null: none)
  bool ln_done = false;  // the last layer's tail ran the next norm(s) (TailLn)
  bool tail, lnt_ok;
  int nsplit = 1;
  // algorithmic bytes of the profiled launches: KV rows read (P + 1) and
  // written by the attention, rows of E floats read / written by the LayerNorm step
  const double kv_bytes;

  DecodeStep(vsim_model *m_, int &nk_, const DevTables &tab_)
      : m(m_), nk(nk_), tab(tab_), s(m_->stream), E(m_->hp.n_embd), F(4 * E),
        x1{q4_rows(m->xq1, E), m->xd1}, x2{q4_rows(m->xq2, E), m->xd2}, x3{q4_rows(m->xq3, F), m->xd3},
        xa{q4_rows(m->xqa, E), m->xda}, R{m->inpL, m->inpL2},
        kv_bytes(2.0 * ((double)m->prof_npast + 1) * E * sizeof(float)) {
    const int d = E / m->hp.n_head;
    const bool serial = m->gd.residual != RES_PARALLEL;
    // the attention heads fuse into k_layer_tail while their LDS (scores over n_ctx) fits it
    tail = m->mode == VSIM_MODE_EXACT && (size_t)attn_lds_floats(d, m->n_ctx) * sizeof(float) <= 75264;
    // the next layer's LayerNorm inside the tail (TailLn; parallel-residual graphs: the tail is
    // where both branches of the layer end)
    lnt_ok = tail && !serial && m->l1 <= 255 && tail_ln_ok(E);
    // each head over two workgroups (its KQV columns halved; the scores computed by both) in the
    // parallel-residual fused tail, where it was measured: r05, 248-token GPT-J lines 608.9 / 612.5
    // vs 606.9 / 610.8 tok/s unsplit, 602.6 / 601.3 at four (profiles/r05_tail_variants_ab.txt).
    // The largest split <= ATT_SPLIT whose column parts are whole 32-blocks; the serial graphs'
    // heads and the standalone k_attn_decode stay one workgroup per head.  (A/B builds:
    // tools/build_variant.sh NAME model.cpp 's/ATT_SPLIT = 2/ATT_SPLIT = 1/'.)
    constexpr int ATT_SPLIT = 2;
    for (int sp = tail && !serial ? ATT_SPLIT : 1; sp > 1; --sp)
      if (d % sp == 0 && (d / sp) % QK == 0) {
        nsplit = sp;
        break;
      }
  }

  // reads: the row (+ the four join vectors), each norm's affine; writes: the joined row, each
  // norm's factors xd (E floats) and Q4 row (0.625 B per value)
  double ln_bytes(int nnorm, bool join) const {
    return 4.0 * E * (1 + (join ? 5 : 0) + 3 * nnorm) + 0.625 * E * nnorm;
  }
  const LnJoin *pending() const { return pend.jout ? &pend : nullptr; }
  // layer l ends with its branches unjoined: a (+ ab) and m->ff (+ fb) join x into the other buffer
  void leave_join(const float *a, const float *ab, const float *fb) { pend = LnJoin{a, ab, m->ff, fb, R[cur ^ 1]}; }

  // k_ln_quant: (join +) one or two norms of the residual row, quantized; a join that stores moves
  // the residual to the other buffer.  first: the step's first norm advances the epoch (the tails' tags)
  int ln_quant(const NormRow &n1, const NormRow *n2, const LnJoin *join, bool first) {
    const LnQuantPair P = ln_quant_jobs(R[cur], n1, n2, join, tail && first ? m->tw.ep : nullptr);
    LAUNCH(m, nk, launch_ln_quant(P.j1, P.second(), E, s), "k_ln_quant", ln_bytes(n2 ? 2 : 1, join != nullptr));
    if (join && join->jout) cur ^= 1;
    return VSIM_OK;
  }
  // (exact_kernel: the exact kernel's name as the profile has always had it for this product,
  // where it does not ask gemv_chain_solo)
  int gemv(const GemvBatch &Bt, const char *what, double bytes, const char *exact_kernel = nullptr) {
    if (!exact_kernel) exact_kernel = gemv_chain_solo(Bt) ? "k_gemv_solo" : "k_gemv_chain32";
    LAUNCH(m, nk, launch_gemv_epi(Bt, m->mode, s),
           std::string(m->mode != VSIM_MODE_EXACT ? "k_gemv_fast_epi" : exact_kernel) + " (" + what + ")", bytes);
    return VSIM_OK;
  }
  // attention for the new token (attn.hpp) on layer il's cache: inside k_layer_tail beside the
  // products f and o (and the next norms N), or alone
  AttnJob attn(int il) const {
    const size_t loff = (size_t)(il - m->l0) * m->n_ctx * E;
    return attn_job(decode_attn_desc(m, tab, xa, nsplit), m->kcache + loff, m->vcache + loff, m->npast_dev);
  }
  int layer_tail(const GemvBatch &f, const GemvBatch &o, int il, const TailLn *N, const char *name, double w_bytes) {
    LAUNCH(m, nk, launch_layer_tail(f, o, attn(il), TailSync{m->tw.hflag, m->tw.ep, il}, m->n_ctx, s, N), name,
           w_bytes + kv_bytes + (N ? ln_bytes(N->w2 ? 2 : 1, true) : 0.0));
    return VSIM_OK;
  }
  int attn_decode(int il) {
    LAUNCH(m, nk, launch_attn_decode(attn(il), m->n_ctx, s), "k_attn_decode", kv_bytes);
    return VSIM_OK;
  }

  // One serial-residual layer (steps 1-6 above)
  int layer_serial(int il) {
    const LayerW &L = m->layers[il - m->l0];
    // 1. (join +) input LayerNorm + quantize
    RC(ln_quant(NormRow{L.ln1_w, L.ln1_b, x1}, nullptr, pending(), il == m->l0));
    // 2. Q, K, V (+ bias; BLOOM: the fused query_key_value's row blocks)
    const GemvBatch B = gemv_batch({gemv_job(L.wq, E, E, x1, L.bq, m->Qb), gemv_job(L.wk, E, E, x1, L.bk, m->Kb),
                                    gemv_job(L.wv, E, E, x1, L.bv, m->Vb)});
    RC(gemv(B, "Q, K, V", 3 * w4_algo_bytes(B.j[0].w)));
    // 3. heads + out-projection (its bias joins in step 4)
    const GemvBatch Bo = gemv_batch({gemv_job(L.wo, E, E, xa, nullptr, m->attn)});
    if (tail) {
      RC(layer_tail(GemvBatch{}, Bo, il, nullptr, "k_layer_tail (attention + out-proj)", w4_algo_bytes(Bo.j[0].w)));
    } else {
      RC(attn_decode(il));
      RC(gemv(Bo, "out-proj", w4_algo_bytes(Bo.j[0].w)));
    }
    // 4. inpFF = (attn + b_o) + x, post-attention LayerNorm + quantize
    const LnJoin j4{m->attn, L.bo, nullptr, nullptr, m->gd.residual == RES_SERIAL_JOINED ? R[cur ^ 1] : nullptr};
    RC(ln_quant(NormRow{L.ln2_w, L.ln2_b, x2}, nullptr, &j4, false));
    // 5. fc_in (+ bias, GELU, requantize)   6. fc_out (its bias joins in the next step 1)
    GemvBatch Bi = gemv_batch({gemv_job(L.wfc, F, E, x2, L.bfc, nullptr)});
    gelu_quant_into(Bi.j[0], tab.gelu_f16, x3);
    RC(gemv(Bi, "fc_in", w4_algo_bytes(Bi.j[0].w)));
    const GemvBatch Bf = gemv_batch({gemv_job(L.wproj, E, F, x3, nullptr, m->ff)});
    RC(gemv(Bf, "fc_out", w4_algo_bytes(Bf.j[0].w)));
    leave_join(nullptr, nullptr, L.bproj);
    return VSIM_OK;
  }

  // One parallel-residual layer (steps 1-3 above)
  int layer_parallel(int il) {
    const GraphDesc &G = m->gd;
    const LayerW &L = m->layers[il - m->l0];
    // 1. (join +) LayerNorm(s) + quantize, unless the previous layer's tail ran them (TailLn)
    if (!ln_done) {
      const NormRow n1{L.ln1_w, L.ln1_b, x1}, n2{L.ln2_w, L.ln2_b, x2};
      RC(ln_quant(n1, G.two_norms ? &n2 : nullptr, pending(), il == m->l0));
    }
    ln_done = false;
    // 2. {fc_in (+bias, GELU, requantize), Q, K, V}
    GemvBatch B = gemv_batch({gemv_job(L.wfc, F, E, G.two_norms ? x2 : x1, L.bfc, nullptr),
                              gemv_job(L.wq, E, E, x1, G.qkvo_bias ? L.bq : nullptr, m->Qb),
                              gemv_job(L.wk, E, E, x1, G.qkvo_bias ? L.bk : nullptr, m->Kb),
                              gemv_job(L.wv, E, E, x1, G.qkvo_bias ? L.bv : nullptr, m->Vb)});
    gelu_quant_into(B.j[0], tab.gelu_f16, x3);
    RC(gemv(B, "fc_in, Q, K, V", w4_algo_bytes(B.j[0].w) + 3 * w4_algo_bytes(B.j[1].w), "k_gemv_solo"));
    // 3. attention for the new token (attn.hpp), fc_out and the out-projection
    GemvBatch Bf = gemv_batch({gemv_job(L.wproj, E, F, x3, nullptr, m->ff)});
    const GemvBatch Bo = gemv_batch({gemv_job(L.wo, E, E, xa, nullptr, m->attn)});
    const double w_bytes = w4_algo_bytes(Bf.j[0].w) + w4_algo_bytes(Bo.j[0].w);
    const float *ab = G.qkvo_bias ? L.bo : nullptr;
    // the next LayerNorm inside this tail: every layer but a non-last stage's last one
    if (lnt_ok && (il + 1 < m->l1 || m->last)) {
      NormRow n1{m->lnf_w, m->lnf_b, x1}, n2;  // the final norm, for the lm_head
      const bool next = il + 1 < m->l1;          // or the next layer's input norm(s)
      if (next) {
        const LayerW &Ln = m->layers[il + 1 - m->l0];
        n1 = NormRow{Ln.ln1_w, Ln.ln1_b, x1};
        n2 = NormRow{Ln.ln2_w, Ln.ln2_b, x2};
      }
      const TailLn N = tail_ln_job(R[cur], R[cur ^ 1], ab, L.bproj, n1, next && G.two_norms ? &n2 : nullptr, m->tw,
                                   dev_stats(), il);
      RC(layer_tail(Bf, Bo, il, &N, "k_layer_tail (fc_out + attention + out-proj + join + LayerNorm)", w_bytes));
      cur ^= 1;
      ln_done = true;
      pend = LnJoin{};
      return VSIM_OK;
    }
    if (tail) {
      RC(layer_tail(Bf, Bo, il, nullptr, "k_layer_tail (fc_out + attention + out-proj)", w_bytes));
    } else {
      RC(attn_decode(il));
      Bf.j[Bf.nj++] = Bo.j[0];
      RC(gemv(Bf, "fc_out, out-proj", w_bytes, "k_gemv_chain32"));
    }
    leave_join(m->attn, ab, L.bproj);
    return VSIM_OK;
  }

  // The stage's end: the final norm (unless the last tail ran it) and the lm_head, or on a non-last
  // stage the join the last layer left
  int head() {
    if (m->last) {
      if (!ln_done) RC(ln_quant(NormRow{m->lnf_w, m->lnf_b, x1}, nullptr, pending(), false));
      const GemvBatch B = gemv_batch(
          {gemv_job(m->lmh, m->hp.n_vocab, E, x1, m->gd.lmh_bias ? m->lmh_b : nullptr, m->logits)});
      RC(gemv(B, "lm_head", w4_algo_bytes(B.j[0].w), "k_gemv_solo"));
    } else if (const LnJoin *j = pending()) {
      RC(launch_residual_join(R[cur], j->ja, j->jab, j->jf, j->jfb, j->jout, E, s));
      ++nk;
      cur ^= 1;
    }
    m->resid_final = R[cur];
    return VSIM_OK;
  }
};

// Weight-only mode's single-token step (w4a16_decode.hip), in enqueue_decode's replayable form: the
// position comes from npast_dev.  Every launch gives the bits of the general path's kernels on the
// same row (run_layer at N = 1), so the logits and the cache rows are eval_seq's.  Per layer:
//   parallel residual (GPT-J, GPT-NeoX), 7 launches:
//     1. k_w4a16_ln       the input norm (+ GPT-NeoX's post-attention norm of the same row) -> operands
//     2. k_gemv_w4a16     {Q, K, V, fc_in}
//     3. k_attn_decode_batch at one row: RoPE, the cache write, KQ, softmax, KQV -> the f32 row
//     4. k_w4a16_rows     the attention row's operand (its maximum runs across the heads)
//     5. k_gemv_w4a16     {out-projection}
//     6. k_w4a16_gelu     fc_in's row + bias -> GELU -> operand
//     7. k_gemv_w4a16     {fc_out}, joining inpL = inpL + (attn + ff) in place
//   serial residual (GPT-NeoX with use_parallel_residual = 0, BLOOM), 9 launches: 1 with one norm, 2
//     without fc_in, 3, 4, 5 joining cur2 = attn + inpL, then k_w4a16_ln of cur2 with the
//     post-attention norm, k_gemv_w4a16 {fc_in}, 6, and 7 joining ff + inpL (BLOOM: + cur2) into inpL.
//   head, 2 launches: k_w4a16_ln with the final norm, k_gemv_w4a16 {lm_head (+ GPT-J's bias)}.
// Process-wide switch (vsim_w4a16_set_step) and the shapes the step takes: k_attn_decode_batch's
// (head dim a multiple of 32 up to 256, its LDS row for n_ctx scores) and k_w4a16_ln's row in LDS.
std::atomic<int> g_w4a16_step{1};
std::atomic<unsigned> g_w4a16_gen{0};  // changes of the switch: a model drops its step graphs after one

bool w4a16_step_ok(const vsim_model *m) {
  const int E = m->hp.n_embd, d = E / m->hp.n_head;
  return d % 32 == 0 && d <= 256 && (size_t)E * 4 <= 64 * 1024 &&
         (size_t)attn_lds_floats(d, m->n_ctx) * sizeof(float) <= 160 * 1024;
}
// weight-only mode on the general path for its single-token calls too (switched off, or a shape
// the step does not take): uncaptured, one host round trip per token
bool w4a16_general(const vsim_model *m) {
  return m->mode == VSIM_MODE_W4A16 && !(g_w4a16_step.load() && w4a16_step_ok(m));
}
// Process-wide switch of the mode's attention (vsim_w4a16_set_attn): 0 the exact path's kernels, 1
// the fp16 MFMA attention of attn_w4a16.hip on the graphs and shapes it takes.  One answer per model
// for all of its paths -- prompt, slot, rows batch, single-token step -- so that none mixes the two.
std::atomic<int> g_w4a16_attn{0};
bool w4a16_attn16(const vsim_model *m) {
  const int E = m->hp.n_embd, d = E / m->hp.n_head;
  return m->mode == VSIM_MODE_W4A16 && g_w4a16_attn.load() && !m->gd.alibi && attn_w4a16_supported(d, E);
}

int enqueue_decode_w4a16(vsim_model *m, int &nk) {
  const int E = m->hp.n_embd, F = 4 * E, V = m->hp.n_vocab;
  const GraphDesc &G = m->gd;
  hipStream_t s = m->stream;
  DevTables tab;
  RC(tables_get(&tab));
  // the row operands in the exact step's rows (as the general path's products use the same buffers);
  // the attention's Q4 row goes where the f32 row's operand follows it
  const ActRow ra{q4_rows(m->xqa, E), m->xda};
  const W4a16Operand x1 = w4a16_operand({{m->xq1}, m->xd1}), x2 = w4a16_operand({{m->xq2}, m->xd2}),
                     x3 = w4a16_operand({{m->xq3}, m->xd3}), xa = w4a16_operand(ra);
  const bool serial = G.residual != RES_PARALLEL, keep_joined = G.residual == RES_SERIAL_JOINED;
  const double kv_bytes = 2.0 * ((double)m->prof_npast + 1) * E * sizeof(float);
  auto ln = [&](const float *x, const NormRow &n1, const W4a16Operand &o1, const NormRow *n2 = nullptr,
                const W4a16Operand &o2 = {}) {
    LAUNCH(m, nk, launch_w4a16_ln(w4a16_ln_job(x, E, n1, o1, n2, o2), s), "k_w4a16_ln",
           4.0 * E * (n2 ? 5 : 3) + 2.0 * E * (n2 ? 2 : 1));
    return VSIM_OK;
  };
  auto gemv = [&](std::initializer_list<W4a16GemvJob> jobs, const char *what) {
    double bytes = 0.0;
    for (const W4a16GemvJob &j : jobs) bytes += w4_algo_bytes(j.w);
    LAUNCH(m, nk, launch_w4a16_gemv(w4a16_gemv(jobs), s), std::string("k_gemv_w4a16 (") + what + ")", bytes);
    return VSIM_OK;
  };
  for (int il = m->l0; il < m->l1; ++il) {
    const LayerW &L = m->layers[il - m->l0];
    const size_t loff = (size_t)(il - m->l0) * m->n_ctx * E;
    const float *bq = G.qkvo_bias ? L.bq : nullptr, *bk = G.qkvo_bias ? L.bk : nullptr,
                *bv = G.qkvo_bias ? L.bv : nullptr, *bo = G.qkvo_bias ? L.bo : nullptr;
    const bool two_here = G.two_norms && !serial;  // both norms read the same row
    const NormRow n1{L.ln1_w, L.ln1_b}, n2{L.ln2_w, L.ln2_b};
    RC(ln(m->inpL, n1, x1, two_here ? &n2 : nullptr, x2));
    const W4a16GemvJob q = w4a16_gemv_job(L.wq, E, E, x1, bq, m->Qb), k = w4a16_gemv_job(L.wk, E, E, x1, bk, m->Kb),
                       v = w4a16_gemv_job(L.wv, E, E, x1, bv, m->Vb);
    // fc_in's bias goes with the GELU
    if (serial)
      RC(gemv({q, k, v}, "Q, K, V"));
    else
      RC(gemv({q, k, v, w4a16_gemv_job(L.wfc, F, E, two_here ? x2 : x1, nullptr, m->fch)}, "Q, K, V, fc_in"));
    AttnJob A = attn_job(decode_attn_desc(m, tab, ra, 1), nullptr, nullptr, nullptr);
    A.out = m->attn_in;
    const AttnRows R{m->w4_kv, m->w4_kv + 1, loff, m->npast_dev};
    if (w4a16_attn16(m))
      LAUNCH(m, nk, launch_attn_w4a16_rows(A, R, 1, s), "k_attn_w4a16_rows", kv_bytes);
    else
      LAUNCH(m, nk, launch_attn_decode_batch(A, R, 1, m->n_ctx, s), "k_attn_decode_batch", kv_bytes);
    LAUNCH(m, nk, launch_w4a16_rows(m->attn_in, E, 1, xa.h, xa.e, s), "k_w4a16_rows", (double)E * 6);
    if (serial) {
      // cur2 = attn + inpL, the MLP's input (BLOOM: and the residual)
      RC(gemv({w4a16_gemv_job(L.wo, E, E, xa, bo, m->cur2, m->inpL)}, "out-proj"));
      RC(ln(m->cur2, n2, x2));
      RC(gemv({w4a16_gemv_job(L.wfc, F, E, x2, nullptr, m->fch)}, "fc_in"));
    } else {
      RC(gemv({w4a16_gemv_job(L.wo, E, E, xa, bo, m->attn)}, "out-proj"));
    }
    LAUNCH(m, nk, launch_w4a16_gelu(m->fch, L.bfc, F, x3.h, x3.e, nullptr, s), "k_w4a16_gelu", (double)F * 10);
    // the layer's join in fc_out's epilogue (k_add_residual's orders; BLOOM: ff + the joined row)
    RC(gemv({w4a16_gemv_job(L.wproj, E, F, x3, L.bproj, m->inpL, keep_joined ? m->cur2 : m->inpL,
                            serial ? nullptr : m->attn)},
            "fc_out"));
  }
  RC(ln(m->inpL, NormRow{m->lnf_w, m->lnf_b}, x1));
  RC(gemv({w4a16_gemv_job(m->lmh, V, E, x1, G.lmh_bias ? m->lmh_b : nullptr, m->logits)}, "lm_head"));
  m->resid_final = m->inpL;
  return VSIM_OK;
}

int enqueue_decode(vsim_model *m, int &nk) {
  if (m->mode == VSIM_MODE_FAST && fast_decode_ok(m)) return enqueue_decode_fast(m, nk);
  const int E = m->hp.n_embd, V = m->hp.n_vocab;
  hipStream_t s = m->stream;
  DevTables tab;
  RC(tables_get(&tab));
  if (m->first && m->gd.emb_norm) {  // word embeddings + word_embeddings_layernorm
    RC(launch_get_rows(m->wte, E, V, m->tok_dev, 1, m->cur1, s));
    RC(launch_norm(m->cur1, m->inpL, E, 1, m->emb_w, m->emb_b, s));
    nk += 2;
  } else if (m->first) {
    RC(launch_get_rows(m->wte, E, V, m->tok_dev, 1, m->inpL, s));
    ++nk;
  }
  if (m->mode == VSIM_MODE_W4A16) return enqueue_decode_w4a16(m, nk);  // (a whole model: set_mode)
  DecodeStep S(m, nk, tab);
  for (int il = m->l0; il < m->l1; ++il)
    RC(m->gd.residual != RES_PARALLEL ? S.layer_serial(il) : S.layer_parallel(il));
  return S.head();
}

thread_local std::string t_err;

}  // namespace

namespace vsim {
void set_error(const std::string &msg) { t_err = msg; }
int hip_fail(hipError_t e, const char *what) {
  t_err = std::string(what) + ": " + hipGetErrorString(e);
  return VSIM_EHIP;
}
}  // namespace vsim

extern "C" {

const char *vsim_last_error(void) { return t_err.c_str(); }

int vsim_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

size_t vsim_q4_bytes(int rows, int k) { return w4_bytes(rows, k); }

}  // extern "C"

namespace vsim {
// vsim_model_create, or (borrow != null) a whole-model GPT-NeoX / GPT-J executor whose weight
// slots point at device buffers the caller owns (ggml tensor name -> W4T32 / F32 device
// pointer, every slot must be there) and whose KV cache is kc / vc ([layer][n_ctx][E] f32):
// the graph executor's fast path, graph.cpp.
int model_create_impl(int arch, const vsim_hparams *hp, int n_ctx, int device, int layer_begin, int layer_end,
                      const std::map<std::string, void *> *borrow, float *kc, float *vc, vsim_model **out) {
  if (!hp || !out) { set_error("model_create: null argument"); return VSIM_EINVAL; }
  if (arch != VSIM_ARCH_GPTNEOX && arch != VSIM_ARCH_GPTJ && arch != VSIM_ARCH_BLOOM) {
    set_error("model_create: unknown arch");
    return VSIM_EINVAL;
  }
  if (hp->n_embd % hp->n_head || hp->n_embd % 128 || hp->n_rot > hp->n_embd / hp->n_head || hp->n_rot % 2 ||
      n_ctx <= 0) {
    set_error("model_create: unsupported hparams (n_embd % 128, n_rot <= head dim, even n_rot)");
    return VSIM_EINVAL;
  }
  if (layer_end < 0) layer_end = hp->n_layer;
  if (layer_begin < 0 || layer_begin >= layer_end || layer_end > hp->n_layer) {
    set_error("model_create: bad layer range");
    return VSIM_EINVAL;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device >= ndev) { set_error("model_create: no such device"); return VSIM_ENODEV; }
  VSIM_HIP(hipSetDevice(device));
  auto *m = new vsim_model();
  m->arch = arch;
  m->hp = *hp;
  m->n_ctx = n_ctx;
  m->device = device;
  m->l0 = layer_begin;
  m->l1 = layer_end;
  m->first = layer_begin == 0;
  m->last = layer_end == hp->n_layer;
  const bool gptj = arch == VSIM_ARCH_GPTJ, bloom = arch == VSIM_ARCH_BLOOM;
  GraphDesc &G = m->gd;
  G.rotary = bloom ? ROT_NONE : gptj ? ROT_GPTJ : ROT_NEOX;
  G.qkvo_bias = !gptj;
  G.alibi = G.emb_norm = bloom;
  G.two_norms = !gptj;
  G.residual = bloom ? RES_SERIAL_JOINED : gptj || hp->use_parallel_residual ? RES_PARALLEL : RES_SERIAL_OLD;
  G.lmh_bias = gptj;
  auto fail = [&](int rc) { vsim_model_free(m); return rc; };
  if (hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking) != hipSuccess)
    return fail(hip_fail(hipErrorUnknown, "stream"));
  std::vector<std::pair<std::string, Slot>> plan;
  plan_slots(m, plan);
  if (borrow) {
    if (arch == VSIM_ARCH_BLOOM || !kc || !vc) { set_error("model_create: borrowed weights: GPT-NeoX / GPT-J only"); return fail(VSIM_EINVAL); }
    for (auto &ps : plan) {
      auto it = borrow->find(ps.first);
      if (it == borrow->end() || !it->second) {
        set_error("model_create: borrowed weights: no device buffer for " + ps.first);
        return fail(VSIM_EINVAL);
      }
      ps.second.ptr = it->second;
      ps.second.loaded = true;
      m->slots[ps.first] = ps.second;
    }
    m->borrowed = true;
    m->kcache = kc;
    m->vcache = vc;
    bind_pointers(m);
  }
  size_t tot = 0;
  for (auto &ps : plan) tot += (slot_dev_bytes(ps.second) + 255) & ~(size_t)255;
  const size_t E = hp->n_embd, nl = layer_end - layer_begin;
  if (!borrow) {
    // + FD_PAD: the fast GEMV streams whole 16-block batches and zeroes the scales of slots past
    // a wave's range, so it may read up to 8 KB past a tensor (fast_decode.hip TileStream)
    if (hipMalloc((void **)&m->warena, tot + FD_PAD) != hipSuccess) { set_error("model_create: weight alloc failed"); return fail(VSIM_ENOMEM); }
    m->wbytes = tot;
    size_t off = 0;
    for (auto &ps : plan) {
      ps.second.ptr = m->warena + off;
      off += (slot_dev_bytes(ps.second) + 255) & ~(size_t)255;
      m->slots[ps.first] = ps.second;
    }
    bind_pointers(m);
    if (hipMalloc((void **)&m->kcache, nl * n_ctx * E * sizeof(float)) != hipSuccess ||
        hipMalloc((void **)&m->vcache, nl * n_ctx * E * sizeof(float)) != hipSuccess) {
      set_error("model_create: KV cache alloc failed");
      return fail(VSIM_ENOMEM);
    }
    (void)hipMemset(m->kcache, 0, nl * n_ctx * E * sizeof(float));
    (void)hipMemset(m->vcache, 0, nl * n_ctx * E * sizeof(float));
  } else {
    m->wbytes = tot;
  }
  const int half = hp->n_rot / 2 > 0 ? hp->n_rot / 2 : 1;
  std::vector<double2> cs((size_t)n_ctx * half);
  if (hp->n_rot > 0) rope_table_host(cs.data(), n_ctx, hp->n_rot);
  if (hipMalloc((void **)&m->rope_cs, cs.size() * sizeof(double2)) != hipSuccess) return fail(VSIM_ENOMEM);
  if (hipMemcpy(m->rope_cs, cs.data(), cs.size() * sizeof(double2), hipMemcpyHostToDevice) != hipSuccess)
    return fail(hip_fail(hipErrorUnknown, "rope table upload"));
  if (arch == VSIM_ARCH_BLOOM) {
    m->hp.n_rot = 0;
    m->hp.use_parallel_residual = 0;
    std::vector<float> sl(hp->n_head);
    alibi_slopes_host(sl.data(), hp->n_head);
    if (hipMalloc((void **)&m->alibi, sl.size() * sizeof(float)) != hipSuccess) return fail(VSIM_ENOMEM);
    if (hipMemcpy(m->alibi, sl.data(), sl.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
      return fail(hip_fail(hipErrorUnknown, "alibi slopes upload"));
  }
  DevTables t;
  if (int rc = tables_get(&t)) return fail(rc);
  if (hipMalloc((void **)&m->err_dev, sizeof(unsigned)) != hipSuccess || hipMemset(m->err_dev, 0, sizeof(unsigned)) != hipSuccess ||
      hipHostMalloc((void **)&m->err_host, sizeof(unsigned), hipHostMallocDefault) != hipSuccess)
    return fail(VSIM_ENOMEM);
  *m->err_host = 0;
  if (int rc = ensure_scratch(m, 16)) return fail(rc);
  *out = m;
  return VSIM_OK;
}

// The borrowed model's per-call settings: the reference pool's KQV grouping (cgraph->n_threads)
// and the graph's own attention scale; a change drops the captured decode graphs.
}  // namespace vsim

// ---------------------------------------------------------------- F32 / F16 sources -> Q4_0
namespace {

std::atomic<int> g_quant_chunk_rows{0};             // vsim_quantize_set_chunk_rows (0: default)
constexpr size_t QUANT_CHUNK_BYTES = (size_t)64 << 20;  // default source bytes per staging chunk

int quant_chunk_rows(int k, size_t esz) {
  long long c = g_quant_chunk_rows.load();
  if (c <= 0) c = (long long)(QUANT_CHUNK_BYTES / ((size_t)k * esz));
  c = (c + T32 - 1) / T32 * T32;
  return (int)std::max<long long>(T32, std::min<long long>(c, 1 << 30));
}

void quant_release(vsim_model *m) {
  vsim_model::QuantStage &q = m->qstage;
  for (int b = 0; b < 2; ++b) {
    if (q.host[b]) (void)hipHostFree(q.host[b]);
    if (q.dev[b]) (void)hipFree(q.dev[b]);
    if (q.copied[b]) (void)hipEventDestroy(q.copied[b]);
    if (q.done[b]) (void)hipEventDestroy(q.done[b]);
  }
  if (q.copy) (void)hipStreamDestroy(q.copy);
  q = vsim_model::QuantStage();
}

int quant_reserve(vsim_model *m, size_t bytes) {
  vsim_model::QuantStage &q = m->qstage;
  if (!q.copy) {
    VSIM_HIP(hipStreamCreateWithFlags(&q.copy, hipStreamNonBlocking));
    for (int b = 0; b < 2; ++b) {
      VSIM_HIP(hipEventCreateWithFlags(&q.copied[b], hipEventDisableTiming));
      VSIM_HIP(hipEventCreateWithFlags(&q.done[b], hipEventDisableTiming));
    }
  }
  if (bytes <= q.cap) return VSIM_OK;
  for (int b = 0; b < 2; ++b) {
    if (q.host[b]) (void)hipHostFree(q.host[b]);
    if (q.dev[b]) (void)hipFree(q.dev[b]);
    q.host[b] = q.dev[b] = nullptr;
  }
  q.cap = 0;
  for (int b = 0; b < 2; ++b) {
    VSIM_HIP(hipHostMalloc(&q.host[b], bytes, hipHostMallocDefault));
    VSIM_HIP(hipMalloc(&q.dev[b], bytes));
  }
  q.cap = bytes;
  return VSIM_OK;
}

// Quantize a [s.rows][s.k] matrix of src_type into the Q4_0 slot s.  `next(dst, n)` delivers the
// next n source bytes (rows in order) into pinned memory and returns false when the source ends
// early (-> QUANT_SHORT).  Chunk i goes host[i & 1] -> dev[i & 1] on the copy stream, then
// k_quantize_w on the model's stream: the copy of chunk i + 1 overlaps the kernel of chunk i, and
// a buffer pair is reused only after its copy (host side) and its kernel (device side) finished.
constexpr int QUANT_SHORT = 1;
template <typename Next>
int quantize_into_slot(vsim_model *m, Slot &s, int src_type, Next next) {
  const size_t esz = src_type == VSIM_SRC_F16 ? 2 : 4, row_bytes = (size_t)s.k * esz;
  const int chunk = std::min(quant_chunk_rows(s.k, esz), (s.rows + T32 - 1) / T32 * T32);
  RC(quant_reserve(m, (size_t)chunk * row_bytes));
  vsim_model::QuantStage &q = m->qstage;
  int rc = VSIM_OK, i = 0;
  auto hip = [&](hipError_t e, const char *what) {
    if (e != hipSuccess && rc == VSIM_OK) rc = hip_fail(e, what);
    return e == hipSuccess;
  };
  for (int r0 = 0; r0 < s.rows && rc == VSIM_OK; r0 += chunk, ++i) {
    const int b = i & 1, n = std::min(chunk, s.rows - r0);
    if (i >= 2) {
      if (!hip(hipEventSynchronize(q.copied[b]), "quantize: wait for the staging copy")) break;
      if (!hip(hipStreamWaitEvent(q.copy, q.done[b], 0), "quantize: order the staging copy")) break;
    }
    if (!next(q.host[b], (size_t)n * row_bytes)) { rc = QUANT_SHORT; break; }
    if (!hip(hipMemcpyAsync(q.dev[b], q.host[b], (size_t)n * row_bytes, hipMemcpyHostToDevice, q.copy),
             "quantize: upload"))
      break;
    if (!hip(hipEventRecord(q.copied[b], q.copy), "quantize: record")) break;
    if (!hip(hipStreamWaitEvent(m->stream, q.copied[b], 0), "quantize: order the kernel")) break;
    rc = launch_quantize_w(q.dev[b], src_type, n, s.k, s.ptr, s.rows, r0, nullptr, nullptr, m->stream);
    if (rc != VSIM_OK) break;
    if (!hip(hipEventRecord(q.done[b], m->stream), "quantize: record")) break;
  }
  // nothing of this call stays in flight, whatever happened
  const hipError_t e1 = hipStreamSynchronize(q.copy), e2 = hipStreamSynchronize(m->stream);
  hip(e1, "quantize: copy stream");
  hip(e2, "quantize: kernel stream");
  if (rc == VSIM_OK) s.loaded = true;
  return rc;
}

}  // namespace

namespace vsim {
int model_set_attn(vsim_model *m, int kqv_nth, float scale) {
  if (kqv_nth < 1) kqv_nth = 1;
  if (m->kqv_nth == kqv_nth && m->attn_scale == scale) return VSIM_OK;
  VSIM_HIP(hipStreamSynchronize(m->stream));
  m->kqv_nth = kqv_nth;
  m->attn_scale = scale;
  for (StepGraph &g : m->step) g.mode = -1;  // recapture on next use
  return VSIM_OK;
}
}  // namespace vsim

extern "C" {

int vsim_model_create(int arch, const vsim_hparams *hp, int n_ctx, int device, int layer_begin, int layer_end,
                      vsim_model **out) {
  return model_create_impl(arch, hp, n_ctx, device, layer_begin, layer_end, nullptr, nullptr, nullptr, out);
}

void vsim_model_free(vsim_model *m) {
  if (!m) return;
  (void)hipSetDevice(m->device);
  if (m->stream) (void)hipStreamSynchronize(m->stream);
  if (m->alibi) (void)hipFree(m->alibi);
  quant_release(m);
  free_scratch(m);
  if (m->warena) (void)hipFree(m->warena);
  if (m->kcache && !m->borrowed) (void)hipFree(m->kcache);
  if (m->vcache && !m->borrowed) (void)hipFree(m->vcache);
  for (float *p : m->kslot) (void)hipFree(p);
  for (float *p : m->vslot) (void)hipFree(p);
  if (m->rope_cs) (void)hipFree(m->rope_cs);
  if (m->err_dev) (void)hipFree(m->err_dev);
  if (m->err_host) (void)hipHostFree(m->err_host);
  if (m->stream) (void)gemm_release_stream(m->stream);  // the prompt GEMM's stream-K workspace
  if (m->stream) (void)hipStreamDestroy(m->stream);
  for (hipEvent_t e : m->prof_events) (void)hipEventDestroy(e);
  delete m;
}

int vsim_model_set_tensor(vsim_model *m, const char *name, const void *host, size_t nbytes) {
  if (m->borrowed) { set_error("set_tensor: the weights belong to the graph executor"); return VSIM_EINVAL; }
  if (const std::string n(name); is_fused_qkv(m, n))  // the three row blocks, q | k | v
    return for_qkv_parts(n, nbytes, "set_tensor", [&](const char *part, size_t off, size_t nb) {
      return vsim_model_set_tensor(m, part, (const uint8_t *)host + off, nb);
    });
  auto it = m->slots.find(name);
  if (it == m->slots.end()) { set_error(std::string("set_tensor: unknown tensor ") + name); return VSIM_EINVAL; }
  Slot &s = it->second;
  if (nbytes != slot_bytes(s)) { set_error(std::string("set_tensor: wrong size for ") + name); return VSIM_EINVAL; }
  VSIM_HIP(hipSetDevice(m->device));
  if (s.kind == KF32) {
    VSIM_HIP(hipMemcpy(s.ptr, host, nbytes, hipMemcpyHostToDevice));
  } else {
    void *stage = nullptr;
    VSIM_HIP(hipMalloc(&stage, nbytes));
    hipError_t e = hipMemcpy(stage, host, nbytes, hipMemcpyHostToDevice);
    int rc = e == hipSuccess ? launch_q4_repack(stage, s.ptr, s.rows, s.k, m->stream) : hip_fail(e, "upload");
    if (rc == 0) rc = hipStreamSynchronize(m->stream) == hipSuccess ? 0 : VSIM_EHIP;
    (void)hipFree(stage);
    if (rc) return rc;
  }
  s.loaded = true;
  return VSIM_OK;
}

int vsim_model_get_tensor(vsim_model *m, const char *name, void *host, size_t nbytes) {
  if (!m || !name || !host) { set_error("get_tensor: null argument"); return VSIM_EINVAL; }
  if (const std::string n(name); is_fused_qkv(m, n))  // the three row blocks back to back
    return for_qkv_parts(n, nbytes, "get_tensor", [&](const char *part, size_t off, size_t nb) {
      return vsim_model_get_tensor(m, part, (uint8_t *)host + off, nb);
    });
  auto it = m->slots.find(name);
  if (it == m->slots.end()) { set_error(std::string("get_tensor: unknown tensor ") + name); return VSIM_EINVAL; }
  const Slot &s = it->second;
  if (nbytes != slot_bytes(s)) { set_error(std::string("get_tensor: wrong size for ") + name); return VSIM_EINVAL; }
  VSIM_HIP(hipSetDevice(m->device));
  VSIM_HIP(hipStreamSynchronize(m->stream));
  if (s.kind == KF32) {
    VSIM_HIP(hipMemcpy(host, s.ptr, nbytes, hipMemcpyDeviceToHost));
    return VSIM_OK;
  }
  void *stage = nullptr;
  VSIM_HIP(hipMalloc(&stage, nbytes));
  int rc = launch_q4_unpack(s.ptr, stage, s.rows, s.k, m->stream);
  if (rc == 0 && hipStreamSynchronize(m->stream) != hipSuccess) rc = hip_fail(hipErrorUnknown, "unpack");
  if (rc == 0 && hipMemcpy(host, stage, nbytes, hipMemcpyDeviceToHost) != hipSuccess) rc = hip_fail(hipErrorUnknown, "download");
  (void)hipFree(stage);
  return rc;
}

int vsim_model_randomize(vsim_model *m, uint64_t seed, float stddev) {
  if (m->borrowed) { set_error("randomize: the weights belong to the graph executor"); return VSIM_EINVAL; }
  VSIM_HIP(hipSetDevice(m->device));
  uint64_t id = 0;
  for (auto &kv : m->slots) {
    Slot &s = kv.second;
    const uint64_t sd = seed * 0x9E3779B97F4A7C15ull + (++id) * 0xD1B54A32D192ED03ull;
    const bool gain = kv.first.find("norm.weight") != std::string::npos || kv.first.find("ln_") != std::string::npos
                          ? kv.first.find(".weight") != std::string::npos
                          : false;
    if (s.kind == KQ4)
      RC(launch_randn_q4(s.ptr, s.rows, s.k, sd, stddev, m->stream));
    else
      RC(launch_randn_f32((float *)s.ptr, s.k, sd, stddev, gain ? 1.0f : 0.0f, m->stream));
    s.loaded = true;
  }
  VSIM_HIP(hipStreamSynchronize(m->stream));
  return VSIM_OK;
}

// The ggml model file (vsim.cpp:108-458; convert_gptj_to_ggml.py; convert_bloom_to_ggml.py):
// header, vocab, then tensor records {n_dims, name_len, ftype, ne[n_dims], name, data} to EOF.
// Checked as gptneox_model_load checks them (vsim.cpp:398-438): every header field read, every
// record's name known, its element count and its shape those of the tensor the graph expects
// (ne[0] = the inner dimension K, ne[1] = rows), its type the expected one, no tensor missing.
// F32 / F16 weight files (f16 = 0 / 1, vsim.cpp:179-190) take the reference's F32 / F16 mul_mat,
// which is not this library's path: they are refused with that reason.
// With VSIM_LOAD_QUANTIZE (vsim_model_load_file_ex) the converters' F32 / F16 files load too: a
// 2-D record whose slot is a Q4_0 matrix may have ftype 0 or 1 and streams through the staging
// buffers into k_quantize_w (quantize_into_slot); every check and message is the plain loader's.
static int load_file_impl(const char *path, int arch, int n_ctx, int device, int layer_begin, int layer_end, int flags,
                          vsim_model **out) {
  if (!path || !out) { set_error("load: null argument"); return VSIM_EINVAL; }
  const bool qz = (flags & VSIM_LOAD_QUANTIZE) != 0;
  std::ifstream f(path, std::ios::binary);
  if (!f) { set_error(std::string("load: cannot open ") + path); return VSIM_EFILE; }
  auto rd = [&](void *p, size_t n) { f.read((char *)p, n); return (size_t)f.gcount() == n; };
  auto bad = [](const std::string &why) { set_error("load: " + why); return VSIM_EFILE; };
  uint32_t magic = 0;
  if (!rd(&magic, 4) || magic != 0x67676d6c) return bad("bad magic");
  vsim_hparams hp{};
  int32_t ftype = 0;
  bool ok = rd(&hp.n_vocab, 4) && rd(&hp.n_embd, 4);
  if (arch == VSIM_ARCH_BLOOM) {  // convert_bloom_to_ggml.py:79-85: ..., multiple_of, n_head, n_layer, ftype
    int32_t n_mult = 0;
    ok = ok && rd(&n_mult, 4) && rd(&hp.n_head, 4) && rd(&hp.n_layer, 4);
    hp.n_rot = 0;
  } else {
    ok = ok && rd(&hp.n_head, 4) && rd(&hp.n_layer, 4) && rd(&hp.n_rot, 4);
  }
  hp.use_parallel_residual = arch == VSIM_ARCH_BLOOM ? 0 : 1;
  if (arch == VSIM_ARCH_GPTNEOX) ok = ok && rd(&hp.use_parallel_residual, 4);
  ok = ok && rd(&ftype, 4);
  if (!ok) return bad("truncated header");
  if (hp.n_vocab <= 0 || hp.n_embd <= 0 || hp.n_head <= 0 || hp.n_layer <= 0 || hp.n_rot < 0)
    return bad("header values out of range");
  if (!qz && (ftype == 0 || ftype == 1))
    return bad("F32 / F16 weight files take the reference's F32 / F16 mul_mat (vsim.cpp:179-190); this library "
               "runs the Q4_0 path: quantize the file to Q4_0 (f16 == 2) first");
  if (ftype != 2 && !(qz && (ftype == 0 || ftype == 1))) return bad("only Q4_0 (f16 == 2) files are supported");
  int32_t nv = hp.n_vocab;
  if (arch == VSIM_ARCH_GPTJ && !rd(&nv, 4)) return bad("truncated vocab count");
  if (nv < 0 || nv > (1 << 24)) return bad("vocab count out of range");
  for (int i = 0; i < nv; ++i) {
    uint32_t len = 0;
    if (!rd(&len, 4) || len > (1u << 20)) return bad("truncated or corrupt vocab");
    f.seekg(len, std::ios::cur);
    if (!f) return bad("truncated vocab");
  }
  vsim_model *m = nullptr;
  if (layer_end < 0) layer_end = hp.n_layer;
  RC(vsim_model_create(arch, &hp, n_ctx, device, layer_begin, layer_end, &m));
  std::map<std::string, Slot> full;  // every tensor of the whole model (all stages)
  {
    vsim_model whole;
    whole.arch = arch;
    whole.hp = hp;
    whole.l0 = 0;
    whole.l1 = hp.n_layer;
    std::vector<std::pair<std::string, Slot>> plan;
    plan_slots(&whole, plan);
    for (auto &ps : plan) full[ps.first] = ps.second;
  }
  auto fail_load = [&](const std::string &why) {
    vsim_model_free(m);
    return bad(why);
  };
  std::vector<char> buf;
  while (true) {
    int32_t nd = 0, ln = 0, ft = 0;
    if (!rd(&nd, 4)) break;  // end of file between records
    if (!rd(&ln, 4) || !rd(&ft, 4)) return fail_load("truncated tensor record");
    if (nd < 1 || nd > 2 || ln < 1 || ln > 512) return fail_load("corrupt tensor record (n_dims / name length)");
    int32_t dims[2] = {1, 1};
    size_t ne = 1;
    for (int i = 0; i < nd; ++i) {
      if (!rd(&dims[i], 4) || dims[i] <= 0) return fail_load("corrupt tensor dimensions");
      ne *= (size_t)dims[i];
    }
    std::string name(ln, 0);
    if (!rd(&name[0], ln)) return fail_load("truncated tensor name");
    if (ft != 0 && ft != 2 && !(qz && ft == 1)) return fail_load("unsupported tensor type in " + name);
    if (ft == 2 && dims[0] % QK) return fail_load("Q4_0 tensor " + name + " with ne[0] not a multiple of 32");
    const size_t nbytes = ft == 0 ? ne * 4 : ft == 1 ? ne * 2 : ne / QK * QBYTES;
    // the tensor as the whole model's graph expects it (BLOOM's fused query_key_value: the
    // slot of its first row block, three times the rows)
    const bool fused = full.find(name) == full.end() && full.find(name + "/q") != full.end();
    auto fit = full.find(fused ? name + "/q" : name);
    if (fit == full.end()) return fail_load("unknown tensor " + name);
    const Slot &sl = fit->second;
    // a Q4_0 matrix arrives as Q4_0, or, when quantizing, as the F32 / F16 matrix it is made from
    const bool from_src = qz && sl.kind == KQ4 && nd == 2 && ft != 2;
    if (!from_src && (sl.kind == KQ4) != (ft == 2)) return fail_load("type mismatch " + name);
    const int want_rows = sl.kind == KQ4 ? sl.rows * (fused ? 3 : 1) : 1;
    if (dims[0] != sl.k || (nd == 2 ? dims[1] : 1) != want_rows) {
      char msg[256];
      snprintf(msg, sizeof msg, "tensor %s has the wrong shape in the model file: got [%d, %d], expected [%d, %d]",
               name.c_str(), dims[0], nd == 2 ? dims[1] : 1, sl.k, want_rows);
      return fail_load(msg);
    }
    if (m->slots.find(fused ? name + "/q" : name) == m->slots.end()) {  // another pipeline stage's tensor
      f.seekg(nbytes, std::ios::cur);
      if (!f) return fail_load("truncated tensor " + name);
      continue;
    }
    if (from_src) {  // the record's rows stream into the slot (BLOOM's fused one: q | k | v in turn)
      if (hipSetDevice(m->device) != hipSuccess) return fail_load("cannot select the device");
      for (int part = 0; part < (fused ? 3 : 1); ++part) {
        Slot &dst = m->slots.find(fused ? name + QKV_PARTS[part] : name)->second;
        const int rc = quantize_into_slot(m, dst, ft == 1 ? VSIM_SRC_F16 : VSIM_SRC_F32,
                                          [&](void *p, size_t n) { return rd(p, n); });
        if (rc == QUANT_SHORT) return fail_load("truncated tensor " + name);
        if (rc) {
          vsim_model_free(m);
          return rc;
        }
      }
      continue;
    }
    buf.resize(nbytes);
    if (!rd(buf.data(), nbytes)) return fail_load("truncated tensor " + name);
    if (int rc = vsim_model_set_tensor(m, name.c_str(), buf.data(), nbytes)) {
      vsim_model_free(m);
      return rc;
    }
  }
  for (auto &kv : m->slots)
    if (!kv.second.loaded) return fail_load("tensor missing from file: " + kv.first);
  quant_release(m);  // the staging buffers are not needed once the file is in
  *out = m;
  return VSIM_OK;
}

int vsim_model_load_file(const char *path, int arch, int n_ctx, int device, int layer_begin, int layer_end,
                         vsim_model **out) {
  return load_file_impl(path, arch, n_ctx, device, layer_begin, layer_end, 0, out);
}

int vsim_model_load_file_ex(const char *path, int arch, int n_ctx, int device, int layer_begin, int layer_end,
                            int flags, vsim_model **out) {
  if (flags & ~VSIM_LOAD_QUANTIZE) { set_error("load: unknown flag"); return VSIM_EINVAL; }
  return load_file_impl(path, arch, n_ctx, device, layer_begin, layer_end, flags, out);
}

int vsim_quantize_set_chunk_rows(int rows) { return g_quant_chunk_rows.exchange(rows > 0 ? rows : 0); }

int vsim_model_set_tensor_src(vsim_model *m, const char *name, const void *host, size_t nbytes, int src_type) {
  if (!m || !name || !host) { set_error("set_tensor_src: null argument"); return VSIM_EINVAL; }
  if (src_type != VSIM_SRC_F32 && src_type != VSIM_SRC_F16) {
    set_error("set_tensor_src: src_type must be VSIM_SRC_F32 or VSIM_SRC_F16");
    return VSIM_EINVAL;
  }
  if (m->borrowed) { set_error("set_tensor_src: the weights belong to the graph executor"); return VSIM_EINVAL; }
  if (const std::string n(name); is_fused_qkv(m, n))  // the three row blocks, q | k | v
    return for_qkv_parts(n, nbytes, "set_tensor_src", [&](const char *part, size_t off, size_t nb) {
      return vsim_model_set_tensor_src(m, part, (const uint8_t *)host + off, nb, src_type);
    });
  auto it = m->slots.find(name);
  if (it == m->slots.end()) { set_error(std::string("set_tensor_src: unknown tensor ") + name); return VSIM_EINVAL; }
  Slot &s = it->second;
  if (s.kind == KF32) {  // 1-D tensors stay F32: the existing path
    if (src_type != VSIM_SRC_F32) {
      set_error(std::string("set_tensor_src: ") + name + " is an F32 vector");
      return VSIM_EINVAL;
    }
    return vsim_model_set_tensor(m, name, host, nbytes);
  }
  if (nbytes != (size_t)s.rows * s.k * (src_type == VSIM_SRC_F16 ? 2 : 4)) {
    set_error(std::string("set_tensor_src: wrong size for ") + name);
    return VSIM_EINVAL;
  }
  VSIM_HIP(hipSetDevice(m->device));
  const uint8_t *src = (const uint8_t *)host;
  return quantize_into_slot(m, s, src_type, [&](void *p, size_t n) {
    memcpy(p, src, n);
    src += n;
    return true;
  });
}

int vsim_model_set_mode(vsim_model *m, int mode) {
  if (mode != VSIM_MODE_EXACT && mode != VSIM_MODE_FAST && mode != VSIM_MODE_W4A16) {
    set_error("set_mode: bad mode");
    return VSIM_EINVAL;
  }
  if (mode == VSIM_MODE_W4A16 && (!m->first || !m->last || m->borrowed)) {
    set_error("set_mode: VSIM_MODE_W4A16 needs a whole model");
    return VSIM_EINVAL;
  }
  // A context of more than FD_MAXCH chunks is beyond the fast decode step's merge
  // (launch_fast_tail refuses it): such a model runs in exact mode throughout
  m->mode = mode == VSIM_MODE_FAST && fast_nchunk(m->n_ctx) > FD_MAXCH ? VSIM_MODE_EXACT : mode;
  return VSIM_OK;
}

int vsim_w4a16_set_attn(int v) {
  const int on = v == 1 ? 1 : 0, old = g_w4a16_attn.exchange(on);
  if (old != on) ++g_w4a16_gen;
  return old;
}

int vsim_w4a16_set_step(int enable) {
  const int on = enable ? 1 : 0, old = g_w4a16_step.exchange(on);
  if (old != on) ++g_w4a16_gen;
  return old;
}

int vsim_model_set_graph(vsim_model *m, int enable) {
  m->graph_enabled = enable != 0;
  return VSIM_OK;
}

int vsim_model_hparams(const vsim_model *m, vsim_hparams *hp, int *n_ctx, int *lb, int *le) {
  if (hp) *hp = m->hp;
  if (n_ctx) *n_ctx = m->n_ctx;
  if (lb) *lb = m->l0;
  if (le) *le = m->l1;
  return VSIM_OK;
}

void *vsim_model_stream(vsim_model *m) { return (void *)m->stream; }
const float *vsim_model_logits_dev(vsim_model *m) { return m->logits; }

int vsim_model_info(vsim_model *m, int *kernels_per_eval, int *graph_enabled, size_t *weight_bytes) {
  if (kernels_per_eval) *kernels_per_eval = m->kernels_last;
  if (graph_enabled) *graph_enabled = m->graph_enabled ? 1 : 0;
  if (weight_bytes) *weight_bytes = m->wbytes;
  return VSIM_OK;
}

}  // extern "C"

namespace {

// token (first stage) and n_past from their pinned host words
int upload_step(vsim_model *m) {
  if (m->first)
    VSIM_HIP(hipMemcpyAsync(m->tok_dev, m->tok_host, sizeof(int32_t), hipMemcpyHostToDevice, m->stream));
  VSIM_HIP(hipMemcpyAsync(m->npast_dev, m->npast_host, sizeof(int), hipMemcpyHostToDevice, m->stream));
  return VSIM_OK;
}

__global__ void k_npast_advance(int *npast) { npast[0] += 1; }

// The whole single-token step of a kind, as decode_graph captures it and the eager paths run it:
//   STEP_LOGITS  uploads, the decode kernels, then the logits to their pinned host row (last
//                stage, when wanted) or the residual to resid_out (other stages, when given)
//   STEP_ARGMAX  uploads, the decode kernels, the device argmax and its 4-byte copy-out
//   STEP_GEN     no uploads, no copy-out: the argmax feeds the next step (launch_argmax_gen)
//   STEP_STAGE   from the bound device buffers: token (first stage) or residual (other stages)
//                in, this stage's layers, then the residual out (non-last stages) or the device
//                argmax into the bound token word (last stage), then n_past + 1 on the device
//   STEP_SAMPLE  uploads (the sampler's block too), the decode kernels, k_sample_topk reading its
//                k, window, scale and penalty from that block, and the candidates' copy-out
int enqueue_step(vsim_model *m, StepKind kind, int &nk, bool want_logits = true, float *resid_out = nullptr) {
  hipStream_t s = m->stream;
  const int E = m->hp.n_embd, V = m->hp.n_vocab;
  if (kind == STEP_STAGE && m->first)
    VSIM_HIP(hipMemcpyAsync(m->tok_dev, m->st_tok_in, sizeof(int32_t), hipMemcpyDeviceToDevice, s));
  else if (kind == STEP_STAGE)
    VSIM_HIP(hipMemcpyAsync(m->inpL, m->st_resid_in, sizeof(float) * E, hipMemcpyDeviceToDevice, s));
  else if (kind != STEP_GEN)
    RC(upload_step(m));
  if (kind == STEP_SAMPLE)
    VSIM_HIP(hipMemcpyAsync(m->sp_dev, m->sp_host, sizeof(TopkParams), hipMemcpyHostToDevice, s));
  RC(enqueue_decode(m, nk));
  switch (kind) {
    case STEP_LOGITS:
      if (m->last && want_logits)
        VSIM_HIP(hipMemcpyAsync(m->logit_host, m->logits, sizeof(float) * V, hipMemcpyDeviceToHost, s));
      else if (!m->last && resid_out)
        VSIM_HIP(hipMemcpyAsync(resid_out, m->resid_final, sizeof(float) * E, hipMemcpyDeviceToDevice, s));
      break;
    case STEP_ARGMAX:
      RC(launch_argmax(m->logits, V, m->am_dev, m->am_ws, s));
      ++nk;
      VSIM_HIP(hipMemcpyAsync(m->am_host, m->am_dev, sizeof(int), hipMemcpyDeviceToHost, s));
      break;
    case STEP_GEN:
      RC(launch_argmax_gen(m->logits, V, m->am_dev, m->am_ws, m->tok_dev, m->npast_dev, m->hist_dev, s));
      ++nk;
      break;
    case STEP_SAMPLE:
      LAUNCH(m, nk,
             launch_topk(m->logits, V, m->sp_dev, nullptr, 0, 0.0, 0.0, 0, m->so_dev->val, m->so_dev->id, m->tk_ws, s),
             "k_sample_topk", (double)V * sizeof(float));
      VSIM_HIP(hipMemcpyAsync(m->so_host, m->so_dev, sizeof(TopkOut), hipMemcpyDeviceToHost, s));
      break;
    case STEP_STAGE:
      if (m->last) {
        RC(launch_argmax(m->logits, V, m->st_tok_out, m->am_ws, s));
        ++nk;
      } else {
        VSIM_HIP(hipMemcpyAsync(m->st_resid_out, m->resid_final, sizeof(float) * E, hipMemcpyDeviceToDevice, s));
      }
      hipLaunchKernelGGL(k_npast_advance, dim3(1), dim3(1), 0, s, m->npast_dev);
      VSIM_HIP(hipGetLastError());
      ++nk;
      break;
  }
  return VSIM_OK;
}

// Capture (once per kind and mode) the whole step as a hipGraph.
int decode_graph(vsim_model *m, StepKind kind) {
  StepGraph &g = m->step[kind];
  if (const unsigned gen = g_w4a16_gen.load(); gen != m->w4_gen) {  // vsim_w4a16_set_step since the last look
    for (StepGraph &o : m->step) drop(o);
    m->w4_gen = gen;
  }
  if (g.exec && g.mode == m->mode) return VSIM_OK;
  drop(g);
  if (w4a16_attn16(m)) RC(attn_w4a16_prepare());  // (kernel attributes: not inside a capture)
  VSIM_HIP(hipStreamBeginCapture(m->stream, hipStreamCaptureModeThreadLocal));
  int nk = 0;
  const int rc = enqueue_step(m, kind, nk);
  hipGraph_t captured = nullptr;
  const hipError_t ce = hipStreamEndCapture(m->stream, &captured);
  if (rc) {
    if (captured) (void)hipGraphDestroy(captured);
    return rc;
  }
  if (ce != hipSuccess) return hip_fail(ce, "hipStreamEndCapture");
  g.graph = captured;
  VSIM_HIP(hipGraphInstantiate(&g.exec, g.graph, nullptr, nullptr, 0));
  g.mode = m->mode;
  g.kernels = nk;
  return VSIM_OK;
}

// One step of a kind: its graph replayed (the token / n_past uploads are nodes of the graph:
// they read the pinned host words when the graph runs), or enqueued eagerly.  Profiling needs
// the eager form (an event pair around every launch).  nk: the step's kernels, either way.
int run_step(vsim_model *m, StepKind kind, bool graph, int &nk, bool want_logits = true, float *resid_out = nullptr) {
  if (!graph || m->profile) return enqueue_step(m, kind, nk, want_logits, resid_out);
  RC(decode_graph(m, kind));
  VSIM_HIP(hipGraphLaunch(m->step[kind].exec, m->stream));
  nk = m->step[kind].kernels;
  return VSIM_OK;
}

// The general path up to the head for the batch D describes (prompt batches; scoring at every N;
// the batched decode steps): the embedding of its D.N `tokens` (first stage) or the residual from
// resid_in, then this stage's layers; the rows' residual ends in inpL.
int enqueue_prompt(vsim_model *m, const BatchDesc &D, const int32_t *tokens, const float *resid_in, int &nk) {
  const int E = m->hp.n_embd, V = m->hp.n_vocab, N = D.N;
  hipStream_t s = m->stream;
  if (m->first) {
    if (!tokens) { set_error(std::string(D.who) + ": first stage needs tokens"); return VSIM_EINVAL; }
    for (int i = 0; i < N; ++i) {
      if (tokens[i] < 0 || tokens[i] >= V) { set_error(std::string(D.who) + ": token id out of range"); return VSIM_EINVAL; }
      m->tok_host[i] = tokens[i];
    }
    VSIM_HIP(hipMemcpyAsync(m->tok_dev, m->tok_host, N * sizeof(int32_t), hipMemcpyHostToDevice, s));
    if (m->gd.emb_norm) {  // word embeddings + word_embeddings_layernorm
      RC(launch_get_rows(m->wte, E, V, m->tok_dev, N, m->cur1, s));
      RC(launch_norm(m->cur1, m->inpL, E, N, m->emb_w, m->emb_b, s));
      nk += 2;
    } else {
      RC(launch_get_rows(m->wte, E, V, m->tok_dev, N, m->inpL, s));
      ++nk;
    }
  } else {
    if (!resid_in) { set_error(std::string(D.who) + ": non-first stage needs resid_in"); return VSIM_EINVAL; }
    VSIM_HIP(hipMemcpyAsync(m->inpL, resid_in, sizeof(float) * N * E, hipMemcpyDeviceToDevice, s));
  }
  PromptBatch B(m, D, nk);
  for (int il = m->l0; il < m->l1; ++il) RC(run_layer(B, il));
  return VSIM_OK;
}

// The head for the D.N rows of the residual from x: the final LayerNorm and the lm_head product
// (+ GPT-J's bias) into out ([D.N][n_vocab]), profiled as `what`.  The batch's kind, mode and row
// count pick the product as for any other (product_plan): exact mode the row-exact GEMV / GEMM
// (rows independent of their neighbours); a fast-mode prompt the fp16 MFMA GEMM on
// launch_norm_f16q's operand from GEMM_MIN_N rows, else quantize + GEMV; a batched step its rows'.
int run_head(vsim_model *m, const BatchDesc &D, const float *x, float *out, const char *what, int &nk) {
  PromptBatch B(m, D, nk);
  RC(B.norm(x, m->cur1, m->lnf_w, m->lnf_b, B.xa));
  Product P{.w = w4_view(m->lmh, m->hp.n_vocab, E_(m)), .x = m->cur1, .xq = m->xq1, .xd = m->xd1, .quantize = true,
            .bias = m->gd.lmh_bias ? m->lmh_b : nullptr, .y = out, .x16 = B.xa, .what = what};
  return B.mm(P);
}

// The head of the prompt kinds' last row, which alone leaves an eval (vsim.cpp:736-737; rows are
// independent): one row, so the f32 norm and the GEMV in both modes
int run_last_row_head(vsim_model *m, const BatchDesc &D, int &nk) {
  const BatchDesc one{.kind = D.kind, .N = 1, .mode = D.mode, .who = D.who};
  return run_head(m, one, m->inpL + (size_t)(D.N - 1) * E_(m), m->logits, nullptr, nk);
}

// A single-token step on the general path on slot 0, uncaptured: what the whole-model single-token
// calls (eval_argmax, generate, eval_sample) run in weight-only mode without its step (w4a16_general).
// The logits row ends in m->logits.
int enqueue_single_general(vsim_model *m, const char *who, int n_past, int32_t token, int &nk) {
  const BatchDesc D{.kind = BatchKind::PROMPT, .N = 1, .n_past = n_past, .kcache = m->kcache, .vcache = m->vcache,
                    .mode = m->mode, .who = who};
  RC(enqueue_prompt(m, D, &token, nullptr, nk));
  return run_last_row_head(m, D, nk);
}

// Can the device make this sampler's candidates (k_sample_topk's limits)?  Otherwise: the logits
// and the reference's host code.
bool sampler_on_device(const vsim_sampler *sm, int V) {
  return !(sm->top_k > VSIM_TOPK_MAX || sm->top_k > V || sm->win.size() > (size_t)VSIM_WINDOW_MAX || !(sm->temp > 0.0) ||
           !(sm->repeat_penalty > 0.0));
}
// The sampler's parameter block; for one whose row takes the host path, one candidate of an
// empty window, which nobody reads
void fill_topk_params(TopkParams *pb, const vsim_sampler *sm, bool on_dev) {
  pb->scale = on_dev ? 1.0 / sm->temp : 1.0;
  pb->penalty = on_dev ? sm->repeat_penalty : 1.0;
  pb->k = on_dev ? sm->top_k : 1;
  pb->nw = on_dev ? (int32_t)sm->win.size() : 0;
  if (pb->nw) memcpy(pb->win, sm->win.data(), sizeof(int32_t) * sm->win.size());
}

// The end of a call that waits for its work: the bounded waits' word read back, the stream
// drained, the call failed if a wait gave up; then nk recorded as the call's kernels and the
// profile's event pairs folded in.
int finish_call(vsim_model *m, int nk) {
  RC(spin_read(m));
  VSIM_HIP(hipStreamSynchronize(m->stream));
  RC(spin_check(m));
  m->kernels_last = nk;
  if (m->profile) RC(prof_collect(m));
  return VSIM_OK;
}

// The opening of the whole-model single-token calls (`who`: eval_argmax, generate, eval_sample)
// for `steps` steps from n_past (steps_name: how the range message spells it): the checks, the
// device and the scratch, then the token and n_past into their pinned host words.  Zero steps
// end after the range check: there is nothing to set up.
int begin_single(vsim_model *m, const char *who, int n_past, int steps, const char *steps_name, int32_t token) {
  const std::string w(who);
  if (!m->first || !m->last) {
    set_error(w + ": needs a whole-model stage with the single-token decode path");
    return VSIM_EINVAL;
  }
  if (n_past < 0 || n_past + steps > m->n_ctx) {
    set_error(w + ": n_past + " + steps_name + " exceeds n_ctx");
    return VSIM_EINVAL;
  }
  if (steps == 0) return VSIM_OK;
  VSIM_HIP(hipSetDevice(m->device));
  RC(ensure_scratch(m, 1));
  if (token < 0 || token >= m->hp.n_vocab) { set_error(w + ": token id out of range"); return VSIM_EINVAL; }
  m->tok_host[0] = token;
  m->npast_host[0] = n_past;
  m->prof_npast = n_past;
  m->st_npast = -1;  // the step sets the device n_past: a stage step needs a new stage_begin
  return VSIM_OK;
}

std::atomic<int> g_score_chunk_rows{0};  // vsim_score_set_chunk_rows (0: default)
constexpr size_t SCORE_SCRATCH_BYTES = (size_t)64 << 20;
constexpr int SCORE_MIN_ROWS = 8, SCORE_MAX_ROWS = 256;

// rows per head chunk of a scoring eval: the [C][n_vocab] f32 scratch at or below 64 MiB, at
// least 8 rows (the fp16 GEMM's minimum), at most 256 (one tile column of the long-prompt GEMM)
int score_chunk_rows(const vsim_model *m) {
  const int c = g_score_chunk_rows.load();
  if (c > 0) return std::min(c, SCORE_MAX_ROWS);
  const size_t fit = SCORE_SCRATCH_BYTES / ((size_t)m->hp.n_vocab * sizeof(float));
  return (int)std::max<size_t>(SCORE_MIN_ROWS, std::min<size_t>(fit, SCORE_MAX_ROWS));
}

}  // namespace

extern "C" {

int vsim_model_eval_argmax(vsim_model *m, int n_past, int32_t token, int32_t *next_token) {
  if (!m || !next_token) { set_error("eval_argmax: null argument"); return VSIM_EINVAL; }
  RC(begin_single(m, "eval_argmax", n_past, 1, "1", token));
  const ErrScope es(m);
  int nk = 0;
  if (w4a16_general(m)) {
    RC(enqueue_single_general(m, "eval_argmax", n_past, token, nk));
    RC(launch_argmax(m->logits, m->hp.n_vocab, m->am_dev, m->am_ws, m->stream));
    ++nk;
    VSIM_HIP(hipMemcpyAsync(m->am_host, m->am_dev, sizeof(int), hipMemcpyDeviceToHost, m->stream));
  } else {
    RC(run_step(m, STEP_ARGMAX, m->graph_enabled, nk));
  }
  RC(finish_call(m, nk));
  *next_token = m->am_host[0];
  return VSIM_OK;
}

int vsim_model_generate(vsim_model *m, int n_past, int32_t token, int n_steps, int32_t *tokens_out) {
  if (!m || !tokens_out || n_steps < 0) { set_error("generate: bad argument"); return VSIM_EINVAL; }
  RC(begin_single(m, "generate", n_past, n_steps, "n_steps", token));
  if (n_steps == 0) return VSIM_OK;
  const ErrScope es(m);
  if (w4a16_general(m)) {  // one general-path step and one host round trip per token
    for (int i = 0; i < n_steps; ++i) {
      int nk = 0;
      RC(enqueue_single_general(m, "generate", n_past + i, token, nk));
      RC(launch_argmax(m->logits, m->hp.n_vocab, m->am_dev, m->am_ws, m->stream));
      ++nk;
      VSIM_HIP(hipMemcpyAsync(m->am_host, m->am_dev, sizeof(int), hipMemcpyDeviceToHost, m->stream));
      RC(finish_call(m, nk));
      token = tokens_out[i] = m->am_host[0];
    }
    return VSIM_OK;
  }
  RC(upload_step(m));
  int nk = 0;  // kernels of one decode step (argmax included)
  for (int i = 0; i < n_steps; ++i) {
    nk = 0;
    m->prof_npast = n_past + i;
    RC(run_step(m, STEP_GEN, m->graph_enabled, nk));
  }
  VSIM_HIP(hipMemcpyAsync(tokens_out, m->hist_dev + n_past, sizeof(int32_t) * n_steps, hipMemcpyDeviceToHost,
                          m->stream));
  return finish_call(m, nk);
}

int vsim_model_eval_sample(vsim_model *m, vsim_sampler *sm, int n_past, int32_t token, int32_t *next_token) {
  if (!m || !sm || !next_token) { set_error("eval_sample: null argument"); return VSIM_EINVAL; }
  RC(begin_single(m, "eval_sample", n_past, 1, "1", token));
  const int V = m->hp.n_vocab;
  if (!sampler_on_device(sm, V)) {  // the logits step and the reference's host code
    std::vector<float> lg((size_t)V);
    RC(vsim_model_eval(m, n_past, &token, 1, nullptr, nullptr, lg.data()));
    return vsim_sampler_sample_host(sm, lg.data(), V, next_token);
  }
  if (sm->top_k < 1) { set_error("eval_sample: top_k < 1"); return VSIM_EINVAL; }
  const ErrScope es(m);
  fill_topk_params(m->sp_host, sm, true);
  int nk = 0;
  if (w4a16_general(m)) {
    hipStream_t s = m->stream;
    VSIM_HIP(hipMemcpyAsync(m->sp_dev, m->sp_host, sizeof(TopkParams), hipMemcpyHostToDevice, s));
    RC(enqueue_single_general(m, "eval_sample", n_past, token, nk));
    LAUNCH(m, nk, launch_topk(m->logits, V, m->sp_dev, nullptr, 0, 0.0, 0.0, 0, m->so_dev->val, m->so_dev->id, m->tk_ws, s),
           "k_sample_topk", (double)V * sizeof(float));
    VSIM_HIP(hipMemcpyAsync(m->so_host, m->so_dev, sizeof(TopkOut), hipMemcpyDeviceToHost, s));
  } else {
    RC(run_step(m, STEP_SAMPLE, m->graph_enabled, nk));
  }
  RC(finish_call(m, nk));
  return vsim_sampler_pick(sm, m->so_host->val, m->so_host->id, sm->top_k, next_token);
}

int vsim_model_generate_sampled(vsim_model *m, vsim_sampler *sm, int n_past, int32_t token, int n_steps, int32_t eos,
                                int32_t *tokens_out, int *n_out) {
  if (!m || !sm || !tokens_out || !n_out || n_steps < 0) { set_error("generate_sampled: bad argument"); return VSIM_EINVAL; }
  *n_out = 0;
  if (n_past < 0 || n_past + n_steps > m->n_ctx) {
    set_error("generate_sampled: n_past + n_steps exceeds n_ctx");
    return VSIM_EINVAL;
  }
  for (int i = 0; i < n_steps; ++i) {
    int32_t nxt = 0;
    RC(vsim_model_eval_sample(m, sm, n_past + i, token, &nxt));
    tokens_out[(*n_out)++] = nxt;
    if (nxt == eos) break;
    token = nxt;
  }
  return VSIM_OK;
}

int vsim_model_reserve(vsim_model *m, int n_tokens) {
  if (!m) { set_error("reserve: null model"); return VSIM_EINVAL; }
  if (n_tokens <= 0 || n_tokens > m->n_ctx) { set_error("reserve: n_tokens must be in 1..n_ctx"); return VSIM_EINVAL; }
  VSIM_HIP(hipSetDevice(m->device));
  RC(ensure_scratch(m, n_tokens));
  const int E = E_(m), d = E / m->hp.n_head;
  if (n_tokens >= 8 && attn_prefill_supported(d) && E % 64 == 0) {
    RC(ensure_pf_scratch(m));
    RC(attn_prefill_prepare());
  }
  if (wide_gemm(true, n_tokens, E)) RC(gemm_reserve_stream(m->stream));
  VSIM_HIP(hipStreamSynchronize(m->stream));
  return VSIM_OK;
}

int vsim_model_eval(vsim_model *m, int n_past, const int32_t *tokens, int N, const float *resid_in, float *resid_out,
                    float *logits) {
  if (!m) { set_error("eval: null model"); return VSIM_EINVAL; }
  if (N <= 0 || n_past < 0 || n_past + N > m->n_ctx) { set_error("eval: n_past + N exceeds n_ctx"); return VSIM_EINVAL; }
  m->st_npast = -1;  // an eval sets the device n_past: a stage step needs a new stage_begin
  VSIM_HIP(hipSetDevice(m->device));
  const ErrScope es(m);
  RC(ensure_scratch(m, N));
  const int E = m->hp.n_embd, V = m->hp.n_vocab;
  hipStream_t s = m->stream;
  int nk = 0;
  if (N == 1 && !w4a16_general(m)) {  // every graph has a single-token step (the serial-residual ones with 6 launches per layer)
    if (m->first) {
      if (!tokens) { set_error("eval: first stage needs tokens"); return VSIM_EINVAL; }
      if (tokens[0] < 0 || tokens[0] >= V) { set_error("eval: token id out of range"); return VSIM_EINVAL; }
      m->tok_host[0] = tokens[0];
    } else {
      if (!resid_in) { set_error("eval: non-first stage needs resid_in"); return VSIM_EINVAL; }
      VSIM_HIP(hipMemcpyAsync(m->inpL, resid_in, sizeof(float) * E, hipMemcpyDeviceToDevice, s));
    }
    m->npast_host[0] = n_past;
    m->prof_npast = n_past;
    // (the graph is the whole model's step: a partial stage, with its residual in and out, runs eagerly)
    RC(run_step(m, STEP_LOGITS, m->graph_enabled && m->first && m->last, nk, logits != nullptr, resid_out));
  } else {
    // general path: prompt batches (N > 1), and weight-only mode's evals without its step
    const BatchDesc D{.kind = BatchKind::PROMPT, .N = N, .n_past = n_past, .kcache = m->kcache, .vcache = m->vcache,
                      .mode = m->mode, .who = "eval"};
    RC(enqueue_prompt(m, D, tokens, resid_in, nk));
    if (m->last) {
      RC(run_last_row_head(m, D, nk));
      if (logits) VSIM_HIP(hipMemcpyAsync(m->logit_host, m->logits, sizeof(float) * V, hipMemcpyDeviceToHost, s));
    } else if (resid_out) {
      VSIM_HIP(hipMemcpyAsync(resid_out, m->inpL, sizeof(float) * N * E, hipMemcpyDeviceToDevice, s));
    }
  }
  RC(finish_call(m, nk));
  if (m->last && logits) memcpy(logits, m->logit_host, sizeof(float) * V);
  return VSIM_OK;
}

int vsim_model_seq_reserve(vsim_model *m, int n_seq) {
  if (!m) { set_error("seq_reserve: null model"); return VSIM_EINVAL; }
  if (m->borrowed || !m->first || !m->last) {
    set_error("seq_reserve: needs a whole model that owns its KV cache");
    return VSIM_EINVAL;
  }
  const int have = 1 + (int)m->kslot.size();
  if (n_seq < have) { set_error("seq_reserve: the slots cannot shrink (have " + std::to_string(have) + ")"); return VSIM_EINVAL; }
  if (n_seq == have) return VSIM_OK;
  VSIM_HIP(hipSetDevice(m->device));
  const size_t bytes = (size_t)(m->l1 - m->l0) * m->n_ctx * E_(m) * sizeof(float);
  std::vector<float *> nk, nv;  // the new slots, handed over only when all of them exist
  auto undo = [&] {
    for (float *p : nk) (void)hipFree(p);
    for (float *p : nv) (void)hipFree(p);
  };
  for (int i = have; i < n_seq; ++i) {
    float *k = nullptr, *v = nullptr;
    if (hipMalloc((void **)&k, bytes) != hipSuccess) k = nullptr;
    if (k && hipMalloc((void **)&v, bytes) != hipSuccess) v = nullptr;
    if (!k || !v) {
      (void)hipGetLastError();  // the allocation's error stays with this call
      if (k) (void)hipFree(k);
      undo();
      set_error("seq_reserve: KV cache alloc failed for slot " + std::to_string(i));
      return VSIM_ENOMEM;
    }
    nk.push_back(k);
    nv.push_back(v);
    if (hipMemsetAsync(k, 0, bytes, m->stream) != hipSuccess || hipMemsetAsync(v, 0, bytes, m->stream) != hipSuccess) {
      undo();
      return hip_fail(hipErrorUnknown, "seq_reserve: clearing a slot");
    }
  }
  if (hipStreamSynchronize(m->stream) != hipSuccess) {
    undo();
    return hip_fail(hipErrorUnknown, "seq_reserve: clearing the slots");
  }
  m->kslot.insert(m->kslot.end(), nk.begin(), nk.end());
  m->vslot.insert(m->vslot.end(), nv.begin(), nv.end());
  return VSIM_OK;
}

int vsim_model_eval_seq(vsim_model *m, int seq, int n_past, const int32_t *tokens, int N, float *logits) {
  if (!m) { set_error("eval_seq: null model"); return VSIM_EINVAL; }
  if (!m->first || !m->last) { set_error("eval_seq: needs a whole model"); return VSIM_EINVAL; }
  if (seq < 0 || seq > (int)m->kslot.size()) { set_error("eval_seq: slot outside the reserve (seq_reserve)"); return VSIM_EINVAL; }
  if (N <= 0 || n_past < 0 || n_past + N > m->n_ctx) { set_error("eval_seq: n_past + N exceeds n_ctx"); return VSIM_EINVAL; }
  m->st_npast = -1;  // as an eval: a stage step needs a new stage_begin
  VSIM_HIP(hipSetDevice(m->device));
  const ErrScope es(m);
  RC(ensure_scratch(m, N));
  const int V = m->hp.n_vocab;
  int nk = 0;
  const BatchDesc D{.kind = BatchKind::PROMPT_SLOT, .N = N, .n_past = n_past, .kcache = slot_k(m, seq),
                    .vcache = slot_v(m, seq), .mode = m->mode, .who = "eval_seq"};
  RC(enqueue_prompt(m, D, tokens, nullptr, nk));
  RC(run_last_row_head(m, D, nk));
  if (logits) VSIM_HIP(hipMemcpyAsync(m->logit_host, m->logits, sizeof(float) * V, hipMemcpyDeviceToHost, m->stream));
  RC(finish_call(m, nk));
  if (logits) memcpy(logits, m->logit_host, sizeof(float) * V);
  return VSIM_OK;
}

namespace {
// One batched decode step with the products in `mode` (vsim_model_decode_batch: exact, on a model in
// exact mode; vsim_model_decode_batch_fast: fast, vsim_model_decode_batch_w4a16: weight-only, whatever
// the model's mode)
// -- or, with samplers, the sampled step (vsim_model_decode_batch_sample): next[b] drawn by samplers[b]
int decode_rows_impl(vsim_model *m, int mode, int B, const int32_t *seq, const int32_t *n_past, const int32_t *tokens,
                     float *logits, int32_t *next, vsim_sampler *const *samplers, bool runs);

int decode_batch_impl(vsim_model *m, int mode, int B, const int32_t *seq, const int32_t *n_past,
                      const int32_t *tokens, float *logits, int32_t *next, vsim_sampler *const *samplers = nullptr) {
  if (!m || !seq || !n_past || !tokens) { set_error("decode_batch: null argument"); return VSIM_EINVAL; }
  if (!m->first || !m->last) { set_error("decode_batch: needs a whole model"); return VSIM_EINVAL; }
  if (mode == VSIM_MODE_EXACT && m->mode != VSIM_MODE_EXACT) {
    set_error("decode_batch: exact mode only (a fast-mode batch is vsim_model_decode_batch_fast's)");
    return VSIM_EINVAL;
  }
  if (B < 1 || B > VSIM_BATCH_MAX) { set_error("decode_batch: B must be in 1..32"); return VSIM_EINVAL; }
  const int V = m->hp.n_vocab, nslot = 1 + (int)m->kslot.size();
  uint64_t used = 0;  // (VSIM_BATCH_MAX rows name at most that many distinct slots; slots >= 64 compared pairwise)
  for (int b = 0; b < B; ++b) {
    if (seq[b] < 0 || seq[b] >= nslot) { set_error("decode_batch: slot outside the reserve (seq_reserve)"); return VSIM_EINVAL; }
    bool dup = seq[b] < 64 && ((used >> seq[b]) & 1);
    for (int a = 0; a < b && !dup; ++a) dup = seq[a] == seq[b];
    if (dup) { set_error("decode_batch: a slot is named twice"); return VSIM_EINVAL; }
    if (seq[b] < 64) used |= (uint64_t)1 << seq[b];
    if (n_past[b] < 0 || n_past[b] >= m->n_ctx) { set_error("decode_batch: n_past outside [0, n_ctx)"); return VSIM_EINVAL; }
    if (tokens[b] < 0 || tokens[b] >= V) { set_error("decode_batch: token id out of range"); return VSIM_EINVAL; }
  }
  return decode_rows_impl(m, mode, B, seq, n_past, tokens, logits, next, samplers, false);
}

// The checked step: row b on slot seq[b] at n_past[b].  runs: the rows of vsim_model_decode_runs,
// where consecutive rows may name one slot at consecutive positions.
int decode_rows_impl(vsim_model *m, int mode, int B, const int32_t *seq, const int32_t *n_past, const int32_t *tokens,
                     float *logits, int32_t *next, vsim_sampler *const *samplers, bool runs) {
  const int V = m->hp.n_vocab;
  // the sampled step: which rows' candidates the device makes (the others: sample_host on the row's logits)
  bool on_dev[VSIM_BATCH_MAX] = {};
  bool any_dev = false;
  for (int b = 0; samplers && b < B; ++b) {
    const vsim_sampler *sm = samplers[b];
    if (!sm) { set_error("decode_batch_sample: null sampler"); return VSIM_EINVAL; }
    for (int a = 0; a < b; ++a)
      if (samplers[a] == sm) { set_error("decode_batch_sample: a sampler is named twice"); return VSIM_EINVAL; }
    if (sm->top_k < 1) { set_error("decode_batch_sample: top_k < 1"); return VSIM_EINVAL; }
    on_dev[b] = sampler_on_device(sm, V);
    any_dev |= on_dev[b];
  }
  m->st_npast = -1;  // as an eval: a stage step needs a new stage_begin
  VSIM_HIP(hipSetDevice(m->device));
  const ErrScope es(m);
  RC(ensure_scratch(m, B));
  RC(ensure_score_scratch(m, B));  // the head's [B][n_vocab] rows and the greedy ids: scoring's buffers
  hipStream_t s = m->stream;
  for (int b = 0; b < B; ++b) {
    m->bw_host->kc[b] = slot_k(m, seq[b]);
    m->bw_host->vc[b] = slot_v(m, seq[b]);
    m->bw_host->npast[b] = n_past[b];
  }
  VSIM_HIP(hipMemcpyAsync(m->bw_dev, m->bw_host, sizeof(BatchWords), hipMemcpyHostToDevice, s));
  int nk = 0;
  const BatchKind kind = mode == VSIM_MODE_EXACT  ? BatchKind::ROWS_EXACT
                         : mode == VSIM_MODE_FAST ? BatchKind::ROWS_FAST
                                                  : BatchKind::ROWS_W4A16;
  const BatchDesc D{.kind = kind, .N = B, .rows = m->bw_dev, .mode = mode, .who = runs ? "decode_runs" : "decode_batch",
                    .runs = runs};
  RC(enqueue_prompt(m, D, tokens, nullptr, nk));
  RC(run_head(m, D, m->inpL, m->score_x, "lm_head (batch)", nk));
  int32_t *am_dev = (int32_t *)m->score_out;
  if (samplers) {
    // the rows' parameter blocks (only the B in use travel), one launch for all rows, the B lists back
    for (int b = 0; b < B; ++b) fill_topk_params(m->bs_par_host + b, samplers[b], on_dev[b]);
    if (any_dev) {
      VSIM_HIP(hipMemcpyAsync(m->bs_par_dev, m->bs_par_host, sizeof(TopkParams) * B, hipMemcpyHostToDevice, s));
      LAUNCH(m, nk, launch_topk_rows(m->score_x, V, V, B, m->bs_par_dev, m->bs_out_dev, m->bs_ws, s),
             "k_sample_topk_rows", (double)B * V * sizeof(float));
      VSIM_HIP(hipMemcpyAsync(m->bs_out_host, m->bs_out_dev, sizeof(TopkOut) * B, hipMemcpyDeviceToHost, s));
    }
    std::vector<std::vector<float>> host_rows((size_t)B);
    for (int b = 0; b < B; ++b) {
      if (on_dev[b]) continue;
      host_rows[b].resize((size_t)V);
      VSIM_HIP(hipMemcpyAsync(host_rows[b].data(), m->score_x + (size_t)b * V, sizeof(float) * V, hipMemcpyDeviceToHost, s));
    }
    RC(finish_call(m, nk));
    for (int b = 0; b < B; ++b) {
      if (on_dev[b])
        RC(vsim_sampler_pick(samplers[b], m->bs_out_host[b].val, m->bs_out_host[b].id, samplers[b]->top_k, &next[b]));
      else
        RC(vsim_sampler_sample_host(samplers[b], host_rows[b].data(), V, &next[b]));
    }
    return VSIM_OK;
  }
  if (next) {
    LAUNCH(m, nk, launch_score_rows(m->score_x, V, B, nullptr, nullptr, am_dev, s), "k_score_rows",
           (double)B * V * sizeof(float));
    VSIM_HIP(hipMemcpyAsync(m->score_out_host, am_dev, sizeof(int32_t) * B, hipMemcpyDeviceToHost, s));
  }
  if (logits) VSIM_HIP(hipMemcpyAsync(logits, m->score_x, sizeof(float) * B * V, hipMemcpyDeviceToHost, s));
  RC(finish_call(m, nk));
  if (next) memcpy(next, m->score_out_host, sizeof(int32_t) * B);
  return VSIM_OK;
}
}  // namespace

int vsim_model_decode_batch(vsim_model *m, int B, const int32_t *seq, const int32_t *n_past, const int32_t *tokens,
                            float *logits, int32_t *next) {
  return decode_batch_impl(m, VSIM_MODE_EXACT, B, seq, n_past, tokens, logits, next);
}

int vsim_model_decode_batch_fast(vsim_model *m, int B, const int32_t *seq, const int32_t *n_past,
                                 const int32_t *tokens, float *logits, int32_t *next) {
  return decode_batch_impl(m, VSIM_MODE_FAST, B, seq, n_past, tokens, logits, next);
}

int vsim_model_decode_batch_w4a16(vsim_model *m, int B, const int32_t *seq, const int32_t *n_past,
                                  const int32_t *tokens, float *logits, int32_t *next) {
  return decode_batch_impl(m, VSIM_MODE_W4A16, B, seq, n_past, tokens, logits, next);
}

int vsim_model_decode_batch_sample(vsim_model *m, int mode, int B, const int32_t *seq, const int32_t *n_past,
                                   const int32_t *tokens, vsim_sampler *const *samplers, int32_t *next) {
  if (mode != VSIM_MODE_EXACT && mode != VSIM_MODE_FAST) {
    set_error("decode_batch_sample: mode must be VSIM_MODE_EXACT or VSIM_MODE_FAST");
    return VSIM_EINVAL;
  }
  if (!samplers || !next) { set_error("decode_batch_sample: null argument"); return VSIM_EINVAL; }
  return decode_batch_impl(m, mode, B, seq, n_past, tokens, nullptr, next, samplers);
}

int vsim_model_decode_batch_sample_w4a16(vsim_model *m, int B, const int32_t *seq, const int32_t *n_past,
                                         const int32_t *tokens, vsim_sampler *const *samplers, int32_t *next) {
  if (!samplers || !next) { set_error("decode_batch_sample: null argument"); return VSIM_EINVAL; }
  return decode_batch_impl(m, VSIM_MODE_W4A16, B, seq, n_past, tokens, nullptr, next, samplers);
}

int vsim_model_decode_runs(vsim_model *m, int mode, int S, const int32_t *seq, const int32_t *n_past,
                           const int32_t *len, const int32_t *tokens, float *logits, int32_t *next) {
  if (!m || !seq || !n_past || !len || !tokens) { set_error("decode_runs: null argument"); return VSIM_EINVAL; }
  if (!m->first || !m->last) { set_error("decode_runs: needs a whole model"); return VSIM_EINVAL; }
  if (mode != VSIM_MODE_EXACT && mode != VSIM_MODE_FAST && mode != VSIM_MODE_W4A16) {
    set_error("decode_runs: mode must be VSIM_MODE_EXACT, VSIM_MODE_FAST or VSIM_MODE_W4A16");
    return VSIM_EINVAL;
  }
  if (mode == VSIM_MODE_EXACT && m->mode != VSIM_MODE_EXACT) {
    set_error("decode_runs: exact products on a model in exact mode only");
    return VSIM_EINVAL;
  }
  if (S < 1) { set_error("decode_runs: S < 1"); return VSIM_EINVAL; }
  const int V = m->hp.n_vocab, nslot = 1 + (int)m->kslot.size();
  // the rows of the batch: run s as len[s] rows of slot seq[s] at n_past[s], n_past[s] + 1, ..
  int32_t row_seq[VSIM_BATCH_MAX], row_npast[VSIM_BATCH_MAX];
  int N = 0;
  for (int s = 0; s < S; ++s) {
    if (len[s] < 1) { set_error("decode_runs: a run needs at least one token"); return VSIM_EINVAL; }
    if (len[s] > VSIM_BATCH_MAX - N) { set_error("decode_runs: more than 32 rows in all"); return VSIM_EINVAL; }
    if (seq[s] < 0 || seq[s] >= nslot) { set_error("decode_runs: slot outside the reserve (seq_reserve)"); return VSIM_EINVAL; }
    for (int a = 0; a < s; ++a)
      if (seq[a] == seq[s]) { set_error("decode_runs: a slot is named twice (one run per slot)"); return VSIM_EINVAL; }
    if (n_past[s] < 0 || n_past[s] > m->n_ctx - len[s]) {
      set_error("decode_runs: a run outside [0, n_ctx)");
      return VSIM_EINVAL;
    }
    for (int j = 0; j < len[s]; ++j, ++N) {
      if (tokens[N] < 0 || tokens[N] >= V) { set_error("decode_runs: token id out of range"); return VSIM_EINVAL; }
      row_seq[N] = seq[s];
      row_npast[N] = n_past[s] + j;
    }
  }
  return decode_rows_impl(m, mode, N, row_seq, row_npast, tokens, logits, next, nullptr, true);
}

int vsim_model_seq_copy(vsim_model *m, int dst, int src, int n_tokens) {
  if (!m) { set_error("seq_copy: null model"); return VSIM_EINVAL; }
  if (m->borrowed || !m->first || !m->last) {
    set_error("seq_copy: needs a whole model that owns its KV cache");
    return VSIM_EINVAL;
  }
  const int nslot = 1 + (int)m->kslot.size();
  if (dst < 0 || dst >= nslot || src < 0 || src >= nslot) { set_error("seq_copy: slot outside the reserve (seq_reserve)"); return VSIM_EINVAL; }
  if (dst == src) { set_error("seq_copy: dst == src"); return VSIM_EINVAL; }
  if (n_tokens < 1 || n_tokens > m->n_ctx) { set_error("seq_copy: n_tokens must be in 1..n_ctx"); return VSIM_EINVAL; }
  VSIM_HIP(hipSetDevice(m->device));
  // a slot is [layers][n_ctx][E]: the first n_tokens rows of every layer, one strided copy per cache
  const size_t pitch = (size_t)m->n_ctx * E_(m) * sizeof(float), width = (size_t)n_tokens * E_(m) * sizeof(float);
  const size_t layers = (size_t)(m->l1 - m->l0);
  VSIM_HIP(hipMemcpy2DAsync(slot_k(m, dst), pitch, slot_k(m, src), pitch, width, layers, hipMemcpyDeviceToDevice, m->stream));
  VSIM_HIP(hipMemcpy2DAsync(slot_v(m, dst), pitch, slot_v(m, src), pitch, width, layers, hipMemcpyDeviceToDevice, m->stream));
  return VSIM_OK;
}

int vsim_score_set_chunk_rows(int rows) { return g_score_chunk_rows.exchange(rows > 0 ? rows : 0); }

int vsim_model_eval_score(vsim_model *m, int n_past, const int32_t *tokens, int N, const float *resid_in,
                          const int32_t *targets, double *logprob, int32_t *argmax, float *logits_all) {
  if (!m) { set_error("eval_score: null model"); return VSIM_EINVAL; }
  if (!m->last) { set_error("eval_score: needs the stage that owns the head (layer_end == n_layer)"); return VSIM_EINVAL; }
  if (N <= 0 || n_past < 0 || n_past + N > m->n_ctx) { set_error("eval_score: n_past + N exceeds n_ctx"); return VSIM_EINVAL; }
  const int E = m->hp.n_embd, V = m->hp.n_vocab;
  for (int i = 0; targets && i < N; ++i)
    if (targets[i] < -1 || targets[i] >= V) { set_error("eval_score: target id outside [-1, n_vocab)"); return VSIM_EINVAL; }
  m->st_npast = -1;  // as an eval: a stage step needs a new stage_begin
  VSIM_HIP(hipSetDevice(m->device));
  const ErrScope es(m);
  RC(ensure_scratch(m, N));
  const int C = score_chunk_rows(m);
  RC(ensure_score_scratch(m, C));
  hipStream_t s = m->stream;
  int nk = 0;
  const BatchDesc D{.kind = BatchKind::PROMPT, .N = N, .n_past = n_past, .kcache = m->kcache, .vcache = m->vcache,
                    .mode = m->mode, .who = "eval_score"};
  RC(enqueue_prompt(m, D, tokens, resid_in, nk));
  for (int i = 0; i < N; ++i) m->score_tgt_host[i] = targets ? targets[i] : -1;
  VSIM_HIP(hipMemcpyAsync(m->score_tgt, m->score_tgt_host, N * sizeof(int32_t), hipMemcpyHostToDevice, s));
  // the results of all rows: N doubles, then N ints (one copy out at the end)
  double *lp_dev = (double *)m->score_out;
  int32_t *am_dev = (int32_t *)(lp_dev + N);
  // The head, C rows at a time: final LayerNorm, lm_head, k_score_rows.  The chunk's row count
  // picks the product (run_head), so fast-mode bits may depend on C; exact mode's do not.
  for (int r0 = 0; r0 < N; r0 += C) {
    const int c = std::min(C, N - r0);
    const BatchDesc chunk{.kind = BatchKind::PROMPT, .N = c, .mode = m->mode, .who = "eval_score"};
    RC(run_head(m, chunk, m->inpL + (size_t)r0 * E, m->score_x, "lm_head (score)", nk));
    LAUNCH(m, nk, launch_score_rows(m->score_x, V, c, m->score_tgt + r0, lp_dev + r0, am_dev + r0, s), "k_score_rows",
           (double)c * V * sizeof(float));
    if (logits_all)
      VSIM_HIP(hipMemcpyAsync(logits_all + (size_t)r0 * V, m->score_x, sizeof(float) * c * V, hipMemcpyDeviceToHost, s));
  }
  VSIM_HIP(hipMemcpyAsync(m->score_out_host, m->score_out, (size_t)N * (sizeof(double) + sizeof(int32_t)),
                          hipMemcpyDeviceToHost, s));
  RC(finish_call(m, nk));
  if (logprob) memcpy(logprob, m->score_out_host, sizeof(double) * N);
  if (argmax) memcpy(argmax, (const double *)m->score_out_host + N, sizeof(int32_t) * N);
  return VSIM_OK;
}

int vsim_model_stage_bind(vsim_model *m, const int32_t *tok_in, const float *resid_in, float *resid_out,
                          int32_t *tok_out) {
  if (!m) { set_error("stage_bind: null model"); return VSIM_EINVAL; }
  if (m->mode == VSIM_MODE_W4A16) { set_error("stage_bind: no pipeline stages in VSIM_MODE_W4A16"); return VSIM_EINVAL; }
  if ((m->first && !tok_in) || (!m->first && !resid_in) || (m->last && !tok_out) || (!m->last && !resid_out)) {
    set_error("stage_bind: first stage needs tok_in, later stages resid_in, the last tok_out, the others resid_out");
    return VSIM_EINVAL;
  }
  VSIM_HIP(hipSetDevice(m->device));
  RC(ensure_scratch(m, 1));
  // the captured step reads the bound addresses: recapture on the next step
  if (m->st_tok_in != tok_in || m->st_resid_in != resid_in || m->st_resid_out != resid_out || m->st_tok_out != tok_out)
    drop(m->step[STEP_STAGE]);
  m->st_tok_in = tok_in;
  m->st_resid_in = resid_in;
  m->st_resid_out = resid_out;
  m->st_tok_out = tok_out;
  return VSIM_OK;
}

int vsim_model_stage_begin(vsim_model *m, int n_past) {
  if (!m || n_past < 0 || n_past >= m->n_ctx) { set_error("stage_begin: n_past outside the context"); return VSIM_EINVAL; }
  if (m->mode == VSIM_MODE_W4A16) { set_error("stage_begin: no pipeline stages in VSIM_MODE_W4A16"); return VSIM_EINVAL; }
  if (!m->st_tok_in && !m->st_resid_in) { set_error("stage_begin: stage_bind first"); return VSIM_EINVAL; }
  VSIM_HIP(hipSetDevice(m->device));
  RC(ensure_scratch(m, 1));
  m->npast_host[0] = n_past;
  VSIM_HIP(hipMemcpyAsync(m->npast_dev, m->npast_host, sizeof(int), hipMemcpyHostToDevice, m->stream));
  VSIM_HIP(hipStreamSynchronize(m->stream));
  m->st_npast = n_past;
  return VSIM_OK;
}

int vsim_model_stage_step(vsim_model *m) {
  if (m && m->mode == VSIM_MODE_W4A16) { set_error("stage_step: no pipeline stages in VSIM_MODE_W4A16"); return VSIM_EINVAL; }
  if (!m || m->st_npast < 0) { set_error("stage_step: stage_begin first"); return VSIM_EINVAL; }
  if (m->st_npast + 1 > m->n_ctx) { set_error("stage_step: context full"); return VSIM_EINVAL; }
  VSIM_HIP(hipSetDevice(m->device));
  const ErrScope es(m);
  m->prof_npast = m->st_npast;
  int nk = 0;
  RC(run_step(m, STEP_STAGE, m->graph_enabled, nk));
  m->st_npast++;
  if (m->profile) return finish_call(m, nk);  // (the event pairs need the stream drained)
  m->kernels_last = nk;
  return VSIM_OK;  // (steps run asynchronously: vsim_model_sync checks them)
}

int vsim_model_debug_poison(vsim_model *m, int n_tokens) {
  if (!m || n_tokens <= 0) { set_error("debug_poison: bad argument"); return VSIM_EINVAL; }
  VSIM_HIP(hipSetDevice(m->device));
  RC(ensure_scratch(m, n_tokens));
  RC(ensure_pf_scratch(m));
  auto nan_fill = [&](void *p, size_t bytes) -> int {
    if (p && bytes) VSIM_HIP(hipMemsetD32Async((hipDeviceptr_t)p, 0x7FC00000u, bytes / 4, m->stream));
    return VSIM_OK;
  };
  for (const ScratchBuf &b : scratch_table(m, m->n_max))
    if (b.flags & S_POISON) RC(nan_fill(*b.p, b.bytes));
  // ... and what the scratch table does not own
  const size_t kv = (size_t)std::max(1, m->l1 - m->l0) * m->n_ctx * E_(m) * sizeof(float);
  RC(nan_fill(m->pf_scratch, m->pf_bytes & ~(size_t)3));
  for (int sl = 0; sl <= (int)m->kslot.size(); ++sl) {
    RC(nan_fill(slot_k(m, sl), kv));
    RC(nan_fill(slot_v(m, sl), kv));
  }
  VSIM_HIP(hipStreamSynchronize(m->stream));
  return VSIM_OK;
}

int vsim_model_sync(vsim_model *m) {
  if (!m) { set_error("sync: null model"); return VSIM_EINVAL; }
  VSIM_HIP(hipSetDevice(m->device));
  RC(spin_read(m));
  VSIM_HIP(hipStreamSynchronize(m->stream));
  return spin_check(m);
}

int vsim_model_set_profile(vsim_model *m, int enable) {
  m->profile = enable != 0;
  m->prof_kinds.clear();
  m->prof_pending.clear();
  m->prof_used = 0;
  return VSIM_OK;
}

int vsim_model_profile_stats(vsim_model *m, double *gemv_ms, long *gemv_launches, double *gemv_bytes) {
  double ms = 0.0, by = 0.0;
  long n = 0;
  for (const auto &k : m->prof_kinds) {
    ms += k.ms;
    by += k.bytes;
    n += k.n;
  }
  if (gemv_ms) *gemv_ms = ms;
  if (gemv_launches) *gemv_launches = n;
  if (gemv_bytes) *gemv_bytes = by;
  return VSIM_OK;
}

int vsim_model_profile_kernel(vsim_model *m, int i, char *name, int name_cap, double *ms, long *launches,
                              double *bytes) {
  if (!m || i < 0 || i >= (int)m->prof_kinds.size()) return VSIM_EINVAL;
  const auto &k = m->prof_kinds[i];
  if (name && name_cap > 0) {
    std::strncpy(name, k.name.c_str(), (size_t)name_cap - 1);
    name[name_cap - 1] = 0;
  }
  if (ms) *ms = k.ms;
  if (launches) *launches = k.n;
  if (bytes) *bytes = k.bytes;
  return VSIM_OK;
}

}  // extern "C"
