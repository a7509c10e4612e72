// vsim_amd/csrc/capi.cpp — the C-ABI entry points of libvsim_hip.so:
//   * drop-in replacements for the reference offload layer (imax.c:52-142, 1133-2292),
//   * vsim_ggml_* hooks for the ops the reference computes in static ggml.c kernels,
//   * op-level device API (vsim_op_*).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <unordered_map>
#include <map>
#include <vector>

#include "common.hpp"
#include "decode_jobs.hpp"
#include "fast.hpp"
#include "graph.hpp"
#include "../../include/vsim_hip.h"

namespace vsim {
int tables_host(uint16_t *exp_f16, uint16_t *gelu_f16);
}  // namespace vsim

using namespace vsim;

#define RC(x)                \
  do {                       \
    int rc_ = (x);           \
    if (rc_) return rc_;     \
  } while (0)

namespace {

// ---- the exact decode step's kernels on caller buffers, their jobs built by decode_jobs.hpp as
// model.cpp's enqueue_decode builds them.
//
// What a call allocates for itself, in one block: `head` bytes for the entry, then the RoPE table
// built here on the host when the caller brought none (such a call waits for the stream before it
// returns: the block is freed with this object).
struct CallBuf {
  uint8_t *buf = nullptr;
  size_t head = 0;
  std::vector<double2> cs;
  ~CallBuf() {
    if (buf) (void)hipFree(buf);
  }
  int alloc(size_t head_bytes, bool want_table, int n_pos, int n_rot) {
    head = head_bytes;
    if (want_table) {
      cs.resize((size_t)n_pos * (n_rot / 2));
      rope_table_host(cs.data(), n_pos, n_rot);
    }
    if (head + cs.size()) VSIM_HIP(hipMalloc(&buf, head + cs.size() * sizeof(double2)));
    return VSIM_OK;
  }
  const double2 *table() const { return (const double2 *)(buf + head); }
  bool upload_table(hipStream_t s) const {
    return cs.empty() ||
           hipMemcpyAsync(buf + head, cs.data(), cs.size() * sizeof(double2), hipMemcpyHostToDevice, s) == hipSuccess;
  }
};
// launch(table) behind the upload of a table built here; waits for the stream
template <class Launch>
int with_rope_table(int n_pos, int n_rot, hipStream_t s, Launch launch) {
  CallBuf own;
  RC(own.alloc(0, true, n_pos, n_rot));
  int rc = own.upload_table(s) ? launch(own.table()) : VSIM_EHIP;
  if (hipStreamSynchronize(s) != hipSuccess && rc == 0) rc = VSIM_EHIP;
  return rc;
}

// The attention of a vsim_attn_batch_args (its RoPE and exp tables apart, which a call may have to
// make first); false when an argument fails the checks that every attention entry makes.
bool attn_desc(const vsim_attn_batch_args *a, int nsplit, AttnDesc *D) {
  if (!a || !a->q || !a->k || !a->v || !a->kc || !a->vc || !a->n_past || !a->oq || !a->oxd || a->d <= 0 ||
      a->H <= 0 || a->n_ctx <= 0 || a->n_rot < 0 || a->n_rot > a->d || a->n_rot % 2)
    return false;
  *D = AttnDesc{.d = a->d, .H = a->H, .n_rot = a->n_rot, .style = a->style, .n_ctx = a->n_ctx, .nsplit = nsplit,
                .kqv_nth = a->kqv_nth, .scale = a->scale, .alibi = a->alibi, .q = a->q, .k = a->k, .v = a->v,
                .cs = (const double2 *)a->cs, .o = {q4_rows(a->oq, a->d * a->H, a->B > 0 ? a->B : 0), a->oxd},
                .out = a->out};
  return true;
}

// One k_layer_tail launch on the call's operands, for vsim_op_tail_attn and vsim_op_tail_ln: the
// call's own block (the tail workspace for width ws_E unless the caller brought one, zeroed; the RoPE
// table unless the caller brought one), the epoch word, the cache pointers read back, launch(A, W)
// under the tag of (epoch, il), then every head part's flag checked against that tag and, with
// check_spin, the bounded waits' counter against its value before the launch.  A caller's
// workspace is written at its epoch word only (stale granules stay where they are).
template <class Launch>
int tail_call(const char *who, const vsim_attn_batch_args *a, AttnDesc D, void *caller_ws, int ws_E, unsigned epoch,
              int il, bool check_spin, hipStream_t s, Launch launch) {
  DevTables tab;
  RC(tables_get(&tab));
  const int na = a->H * D.nsplit;
  CallBuf own;
  RC(own.alloc(caller_ws ? 0 : tail_ws_bytes(ws_E), !a->cs && a->n_rot > 0, a->n_ctx, a->n_rot));
  const TailWs W = tail_ws_carve(caller_ws ? caller_ws : own.buf, ws_E);
  const unsigned tag = (epoch << 8) | (unsigned)(il + 1);
  unsigned *spin = check_spin ? spin_error_counter() : nullptr;
  unsigned spin0 = 0, spin1 = 0;
  float *kc = nullptr, *vc = nullptr;
  std::vector<unsigned long long> flags(na);
  if ((own.head && hipMemsetAsync(own.buf, 0, own.head, s) != hipSuccess) ||
      hipMemcpyAsync(W.ep, &epoch, sizeof(epoch), hipMemcpyHostToDevice, s) != hipSuccess || !own.upload_table(s) ||
      hipMemcpyAsync(&kc, a->kc, sizeof(kc), hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipMemcpyAsync(&vc, a->vc, sizeof(vc), hipMemcpyDeviceToHost, s) != hipSuccess ||
      (spin && hipMemcpyAsync(&spin0, spin, sizeof(spin0), hipMemcpyDeviceToHost, s) != hipSuccess) ||
      hipStreamSynchronize(s) != hipSuccess)
    return VSIM_EHIP;
  if (!kc || !vc) return VSIM_EINVAL;
  if (!a->cs) D.cs = own.table();
  D.etab = tab.exp_f16;
  RC(launch(attn_job(D, kc, vc, a->n_past), W));
  if (hipMemcpyAsync(flags.data(), W.hflag, na * sizeof(unsigned long long), hipMemcpyDeviceToHost, s) != hipSuccess ||
      (spin && hipMemcpyAsync(&spin1, spin, sizeof(spin1), hipMemcpyDeviceToHost, s) != hipSuccess) ||
      hipStreamSynchronize(s) != hipSuccess)
    return VSIM_EHIP;
  int rc = VSIM_OK;
  for (int i = 0; i < na; ++i)
    if ((unsigned)(flags[i] >> 32) != tag) {
      set_error(std::string(who) + ": a head part did not raise its flag");
      rc = VSIM_EHIP;
    }
  if (spin1 != spin0) {
    set_error(std::string(who) + ": a bounded wait inside the layer tail gave up");
    rc = VSIM_ESPIN;
  }
  return rc;
}

}  // namespace

extern "C" {

// ---------------------------------------------------------------- op-level API
int vsim_op_q4_repack(const void *aos, void *soa, int rows, int k, void *stream) {
  return launch_q4_repack(aos, soa, rows, k, (hipStream_t)stream);
}
int vsim_op_q4_unpack(const void *soa, void *aos, int rows, int k, void *stream) {
  return launch_q4_unpack(soa, aos, rows, k, (hipStream_t)stream);
}
int vsim_op_act_repack(const void *aos, void *xq, int n, int k, void *stream) {
  return launch_act_repack(aos, xq, n, k, (hipStream_t)stream);
}
int vsim_op_act_unpack(const void *xq, void *aos, int n, int k, void *stream) {
  return launch_act_unpack(xq, aos, n, k, (hipStream_t)stream);
}
int vsim_op_q4_quantize(const float *x, int k, int n, void *xq, float *xd, void *stream) {
  return launch_q4_quantize(x, k, n, xq, xd, (hipStream_t)stream);
}
int vsim_op_q4_quantize_w(const void *x, int src_type, int rows, int k, void *w, int w_rows, int row0, void *aos,
                          uint64_t *hist, void *stream) {
  return launch_quantize_w(x, src_type, rows, k, w, w_rows, row0, aos, hist, (hipStream_t)stream);
}
int vsim_op_q4_gemv(const void *w, int M, int K, const void *xq, const float *xd, int n, const float *bias, float *y,
                    int mode, void *stream) {
  return launch_q4_gemv(w, M, K, xq, xd, n, bias, y, mode, (hipStream_t)stream);
}
int vsim_op_q4_gemm_rows(const void *w, int M, int K, const float *xd, int n, const float *bias, float *y,
                         void *stream) {
  if (!w || !y || M <= 0 || K <= 0 || K % QK) { set_error("q4_gemm_rows: bad argument"); return VSIM_EINVAL; }
  return launch_gemm_exact_rows(w4_view(w, M, K), xd, n, bias, y, (hipStream_t)stream);
}
int vsim_op_q4_gemm_fast_rows(const void *w, int M, int K, const void *xq, int n, const float *bias, float *y,
                              void *stream) {
  if (!w || !xq || !y || M <= 0 || K <= 0 || K % QK || n < 1 || n > VSIM_BATCH_MAX) {
    set_error("q4_gemm_fast_rows: 1..32 activation rows, K a multiple of 32, w, xq and y required");
    return VSIM_EINVAL;
  }
  return launch_gemm_fast_rows(w4_view(w, M, K), xq, n, bias, y, (hipStream_t)stream);
}
int vsim_op_w4a16_rows(const float *x, int K, int n, void *x16, int32_t *e, void *stream) {
  if (!x || !x16 || !e || K <= 0 || K % QK || n < 1 || n > VSIM_BATCH_MAX) {
    set_error("w4a16_rows: 1..32 rows, K a multiple of 32, x, x16 and e required");
    return VSIM_EINVAL;
  }
  return launch_w4a16_rows(x, K, n, x16, e, (hipStream_t)stream);
}
int vsim_op_q4_gemm_w4a16_rows(const void *w, int M, int K, const void *x16, const int32_t *e, int n, const float *bias,
                               float *y, void *stream) {
  if (!w || !x16 || !e || !y || M <= 0 || K <= 0 || K % QK || n < 1 || n > VSIM_BATCH_MAX) {
    set_error("q4_gemm_w4a16_rows: 1..32 activation rows, K a multiple of 32, M > 0, w, x16, e and y required");
    return VSIM_EINVAL;
  }
  return launch_gemm_w4a16_rows(w4_view(w, M, K), x16, e, n, bias, y, (hipStream_t)stream);
}
int vsim_op_q4_gemm_w4a16_tile(const void *w, int M, int K, const void *x16, const int32_t *e, int n, const float *bias,
                               float *y, void *stream) {
  if (!w || !x16 || !e || !y || M <= 0 || K <= 0 || K % QK || n < 1) {
    set_error("q4_gemm_w4a16_tile: at least one activation row, K a multiple of 32, M > 0, w, x16, e and y required");
    return VSIM_EINVAL;
  }
  return launch_gemm_w4a16_tile(w4_view(w, M, K), x16, e, n, bias, y, (hipStream_t)stream);
}
int vsim_w4a16_set_tile_gemm(int v) { return w4a16_set_tile_gemm(v); }
int vsim_op_w4a16_ln(const vsim_w4a16_ln_args *a, void *stream) {
  if (!a) { set_error("w4a16_ln: null argument"); return VSIM_EINVAL; }
  DevTables tab;  // (the device's LayerNorm counters come with its tables)
  RC(tables_get(&tab));
  // a second norm given in part goes through as it is, for the launcher to refuse
  const NormRow n2{a->w2, a->b2};
  const bool two = a->w2 || a->b2 || a->x16_2 || a->e2;
  const W4a16Operand o1{(_Float16 *)a->x16_1, a->e1}, o2{(_Float16 *)a->x16_2, a->e2};
  return launch_w4a16_ln(w4a16_ln_job(a->x, a->n, NormRow{a->w1, a->b1}, o1, two ? &n2 : nullptr, o2),
                         (hipStream_t)stream);
}
int vsim_op_w4a16_gelu(const float *x, const float *bias, int K, void *x16, int32_t *e, float *g_or_null,
                       void *stream) {
  return launch_w4a16_gelu(x, bias, K, x16, e, g_or_null, (hipStream_t)stream);
}
int vsim_op_w4a16_gemv(const vsim_w4a16_gemv_args *a, void *stream) {
  if (!a || a->nj < 1 || a->nj > 4) { set_error("w4a16_gemv: 1..4 jobs"); return VSIM_EINVAL; }
  W4a16Gemv B{};
  for (int i = 0; i < a->nj; ++i) {
    const vsim_w4a16_gemv_job &j = a->j[i];
    if (!j.w || j.M <= 0 || j.K <= 0 || j.K % QK) {
      set_error("w4a16_gemv: every job needs K a positive multiple of 32, M > 0, w, x16, e and y");
      return VSIM_EINVAL;
    }
    B.j[B.nj++] = w4a16_gemv_job(j.w, j.M, j.K, {(_Float16 *)j.x16, (int32_t *)j.e}, j.bias, j.y, j.res, j.res_a);
  }
  return launch_w4a16_gemv(B, (hipStream_t)stream);
}
int vsim_batch_set_gemm(int enable) { return batch_set_gemm(enable); }
int vsim_batch_set_fast_gemm(int enable) { return batch_set_fast_gemm(enable); }
namespace {
// vsim_op_attn_decode_batch, and with runs vsim_op_attn_decode_runs: the same arguments and checks,
// k_kv_rows + k_attn_decode_runs in place of the one launch
int attn_rows_op(const vsim_attn_batch_args *a, void *stream, bool runs) {
  AttnDesc D;
  if (!attn_desc(a, 1, &D)) {
    set_error(runs ? "attn_decode_runs: bad argument" : "attn_decode_batch: bad argument");
    return VSIM_EINVAL;
  }
  DevTables tab;
  RC(tables_get(&tab));
  D.etab = tab.exp_f16;
  hipStream_t s = (hipStream_t)stream;
  const AttnRows R{a->kc, a->vc, 0, a->n_past};
  auto launch = [&](const double2 *cs) {
    D.cs = cs;
    return launch_attn_decode_batch(attn_job(D, nullptr, nullptr, nullptr), R, a->B, a->n_ctx, s, runs);
  };
  return a->n_rot > 0 && !a->cs ? with_rope_table(a->n_ctx, a->n_rot, s, launch) : launch(D.cs);
}
}  // namespace
int vsim_op_attn_decode_batch(const vsim_attn_batch_args *a, void *stream) { return attn_rows_op(a, stream, false); }
int vsim_op_attn_decode_runs(const vsim_attn_batch_args *a, void *stream) { return attn_rows_op(a, stream, true); }

// Weight-only mode's fp16 attention: the single-query form on a vsim_attn_batch_args (out required;
// no Q4 row, no ALiBi) and the prompt form on the caller's scratch.
namespace {
int attn_w4a16_rows_op(const vsim_attn_batch_args *a, void *stream, bool runs) {
  if (!a || !a->q || !a->k || !a->v || !a->kc || !a->vc || !a->n_past || !a->out || a->oq || a->oxd || a->alibi ||
      a->d <= 0 || a->H <= 0 || a->n_ctx <= 0 || a->n_rot < 0 || a->n_rot > a->d || a->n_rot % 2 || a->B < 1 ||
      a->B > VSIM_BATCH_MAX || !attn_w4a16_supported(a->d, a->d * a->H)) {
    set_error(runs ? "attn_w4a16_runs: bad argument (head dim 64, 96, 128 or 256, n_embd a multiple of 64, 1..32 "
                     "rows, out given, oq / oxd / alibi NULL)"
                   : "attn_w4a16_rows: bad argument (head dim 64, 96, 128 or 256, n_embd a multiple of 64, 1..32 rows, out "
                     "given, oq / oxd / alibi NULL)");
    return VSIM_EINVAL;
  }
  AttnJob A{};
  A.q = a->q;
  A.k = a->k;
  A.v = a->v;
  A.d = a->d;
  A.H = a->H;
  A.n_rot = a->n_rot;
  A.style = a->style;
  A.n_ctx = a->n_ctx;
  A.scale = a->scale;
  A.out = a->out;
  hipStream_t s = (hipStream_t)stream;
  const AttnRows R{a->kc, a->vc, 0, a->n_past};
  auto launch = [&](const double2 *cs) {
    A.cs = cs;
    return launch_attn_w4a16_rows(A, R, a->B, s, runs);
  };
  return a->n_rot > 0 && !a->cs ? with_rope_table(a->n_ctx, a->n_rot, s, launch) : launch((const double2 *)a->cs);
}
}  // namespace
int vsim_op_attn_w4a16_rows(const vsim_attn_batch_args *a, void *stream) { return attn_w4a16_rows_op(a, stream, false); }
int vsim_op_attn_w4a16_runs(const vsim_attn_batch_args *a, void *stream) { return attn_w4a16_rows_op(a, stream, true); }
int vsim_op_attn_w4a16_prompt(const float *Q, const float *kc, const float *vc, int d, int H, int N, int n_past,
                              float scale, float *out, void *scratch, size_t scratch_bytes, void *stream) {
  return launch_attn_w4a16_tile(Q, kc, vc, d, H, N, n_past, scale, out, (hipStream_t)stream, scratch, scratch_bytes);
}

// The heads of k_layer_tail alone (attn_body<704, true>: 11 waves, write-through stores, nsplit
// workgroups per head): launch_layer_tail with neither an fc_out nor an out-projection job, so
// every workgroup takes the head role, on flags and an epoch word of the call's own (epoch 1, layer 0).
int vsim_op_tail_attn(const vsim_attn_batch_args *a, int nsplit, void *stream) {
  AttnDesc D;
  if (!attn_desc(a, nsplit, &D) || a->B != 1 || nsplit < 1 || nsplit > 2 ||
      (long long)a->H * nsplit > TAIL_MAX_HEADS) {
    set_error("tail_attn: bad argument (one row, nsplit 1 or 2, at most 128 head parts)");
    return VSIM_EINVAL;
  }
  hipStream_t s = (hipStream_t)stream;
  return tail_call("tail_attn", a, D, nullptr, 0, 1, 0, false, s, [&](const AttnJob &A, const TailWs &W) {
    const GemvBatch none{};
    return launch_layer_tail(none, none, A, TailSync{W.hflag, W.ep, 0}, a->n_ctx, s);
  });
}
// The whole k_layer_tail with its LayerNorm (TailJob::ln): launch_layer_tail(Bf, Bo, A, sy, n_ctx, s, &N)
// on the call's operands, over the caller's workspace or one of the call's own (decode_jobs.hpp's
// TailWs, the block the executor allocates).
size_t vsim_op_tail_ln_ws_bytes(int E) { return E > 0 && E % QK == 0 ? tail_ws_bytes((size_t)E) : 0; }
int vsim_op_tail_ln(const vsim_tail_ln_args *t, void *stream) {
  const vsim_attn_batch_args *a = t ? &t->attn : nullptr;
  AttnDesc D;
  if (!attn_desc(a, t ? t->nsplit : 0, &D) || a->B != 1 || t->nsplit < 1 || t->nsplit > 2 ||
      (long long)a->H * t->nsplit > TAIL_MAX_HEADS || (long long)a->d * a->H > LNT_MAX_TILES * T32 || a->d % QK ||
      a->d > 256 || a->d % t->nsplit || (a->d / t->nsplit) % QK) {
    set_error("tail_ln: bad attention row (one row, d % 32 == 0, d <= 256, nsplit 1 or 2 with whole 32-blocks per "
              "part, at most 128 head parts, E <= 8192)");
    return VSIM_EINVAL;
  }
  const int E = a->d * a->H;
  if (E % QK || !t->wo || !t->wf || !t->xd || t->K <= 0 || t->K % QK || !t->x || !t->fb || !t->w1 || !t->b1 ||
      !t->jout || !t->q1 || !t->xd1) {
    set_error("tail_ln: wo, wf, xd (K a multiple of 32), x, fb, w1, b1, jout, q1 and xd1 are required");
    return VSIM_EINVAL;
  }
  const bool two = t->w2 || t->b2 || t->q2 || t->xd2;
  if (two && (!t->w2 || !t->b2 || !t->q2 || !t->xd2)) {
    set_error("tail_ln: the second norm needs w2, b2, q2 and xd2");
    return VSIM_EINVAL;
  }
  if (t->il < 0 || t->il > 254) {
    set_error("tail_ln: the layer index of the tag is 0..254");
    return VSIM_EINVAL;
  }
  if (t->ws && (t->ws_bytes < tail_ws_bytes(E) || ((uintptr_t)t->ws & 255))) {
    set_error("tail_ln: the workspace is vsim_op_tail_ln_ws_bytes(E) bytes, 256-byte aligned");
    return VSIM_EINVAL;
  }
  if (!tail_ln_ok(E)) {
    set_error("tail_ln: E/32 must stay below the CU count (every out-projection tile resident at once)");
    return VSIM_EINVAL;
  }
  hipStream_t s = (hipStream_t)stream;
  return tail_call("tail_ln", a, D, t->ws, E, t->epoch, t->il, true, s, [&](const AttnJob &A, const TailWs &W) {
    // fc_out on the caller's factors, the out-projection on the heads' output
    const GemvBatch Bf = gemv_batch({gemv_job(t->wf, E, t->K, t->xd, Q4Rows{}, nullptr, nullptr)});
    const GemvBatch Bo = gemv_batch({gemv_job(t->wo, E, E, D.o, nullptr, nullptr)});
    const NormRow n1{t->w1, t->b1, {q4_rows(t->q1, E), t->xd1}}, n2{t->w2, t->b2, {q4_rows(t->q2, E), t->xd2}};
    const TailLn N = tail_ln_job(t->x, t->jout, t->ab, t->fb, n1, two ? &n2 : nullptr, W, dev_stats(), t->il);
    return launch_layer_tail(Bf, Bo, A, TailSync{W.hflag, W.ep, t->il}, a->n_ctx, s, &N);
  });
}
// k_ln_quant on the call's operands: launch_ln_quant on decode_jobs.hpp's ln_quant_jobs, the second
// job joining the same operands without storing them.
int vsim_op_ln_quant(const vsim_ln_quant_args *a, void *stream) {
  // the row in dynamic LDS beside ln_exact_lds_t's static words, within the 64 KB a launch gets unasked
  constexpr int LNQ_MAX_N = (65536 - 256) / 4 / QK * QK;
  if (!a || a->n <= 0 || a->n % QK || a->n > LNQ_MAX_N) {
    set_error("ln_quant: n must be a positive multiple of 32, at most 16320 (the row lives in 64 KB of LDS)");
    return VSIM_EINVAL;
  }
  if (!a->x || !a->w1 || !a->b1 || !a->q1 || !a->xd1) {
    set_error("ln_quant: x, w1, b1, q1 and xd1 are required");
    return VSIM_EINVAL;
  }
  const bool two = a->w2 || a->b2 || a->q2 || a->xd2;
  if (two && (!a->w2 || !a->b2 || !a->q2 || !a->xd2)) {
    set_error("ln_quant: the second norm needs w2, b2, q2 and xd2");
    return VSIM_EINVAL;
  }
  if ((a->jab && !a->ja) || (a->jfb && !a->jf)) {
    set_error("ln_quant: a join bias without its operand (jab needs ja, jfb needs jf)");
    return VSIM_EINVAL;
  }
  if (a->jout && !a->ja && !a->jf) {
    set_error("ln_quant: jout without a join operand is never written");
    return VSIM_EINVAL;
  }
  const size_t nbytes = (size_t)a->n * sizeof(float);
  const void *ins[] = {a->x, a->w1, a->b1, a->w2, a->b2, a->ja, a->jab, a->jf, a->jfb};
  for (const void *p : ins) {
    if ((uintptr_t)p & 15) {
      set_error("ln_quant: x, the affines and the join operands must be 16-byte aligned");
      return VSIM_EINVAL;
    }
    if (p && a->jout && (uintptr_t)p < (uintptr_t)a->jout + nbytes && (uintptr_t)a->jout < (uintptr_t)p + nbytes) {
      set_error("ln_quant: jout overlaps an input (every slice workgroup reads the whole row)");
      return VSIM_EINVAL;
    }
  }
  if (((uintptr_t)a->jout & 15) || (((uintptr_t)a->q1 | (uintptr_t)a->xd1 | (uintptr_t)a->q2 | (uintptr_t)a->xd2 |
                                      (uintptr_t)a->epoch) & 3)) {
    set_error("ln_quant: jout must be 16-byte aligned, q1, xd1, q2, xd2 and epoch 4-byte aligned");
    return VSIM_EINVAL;
  }
  DevTables tab;
  RC(tables_get(&tab));  // (the device's fallback counters come with its tables)
  const NormRow n1{a->w1, a->b1, {q4_rows(a->q1, a->n), a->xd1}}, n2{a->w2, a->b2, {q4_rows(a->q2, a->n), a->xd2}};
  const LnJoin join{a->ja, a->jab, a->jf, a->jfb, a->jout};
  const LnQuantPair P = ln_quant_jobs(a->x, n1, two ? &n2 : nullptr, &join, a->epoch);
  return launch_ln_quant(P.j1, P.second(), a->n, (hipStream_t)stream);
}
// launch_gemv_chain_batch (k_gemv_solo or k_gemv_chain32, as gemv_chain_solo decides) on the call's jobs.
int vsim_op_gemv_batch(const vsim_gemv_batch_args *a, int32_t *kernel, void *stream) {
  if (!a || a->nj < 1 || a->nj > 4) { set_error("gemv_batch: 1 to 4 jobs"); return VSIM_EINVAL; }
  bool gelu = false;
  for (int i = 0; i < a->nj; ++i) {
    const vsim_gemv_batch_job &j = a->j[i];
    if (!j.w || !j.xd || j.M <= 0 || j.K <= 0 || j.K % QK || (!j.gelu_q && !j.y) ||
        (j.gelu_q && (!j.bias || !j.oq || !j.oxd || j.M % T32))) {
      set_error("gemv_batch: bad job (w, xd, M > 0, K a positive multiple of 32; y unless gelu_q; gelu_q needs "
                "bias, oq, oxd and whole 32-row tiles)");
      return VSIM_EINVAL;
    }
    if ((((uintptr_t)j.w | (uintptr_t)j.xd) & 15) ||
        (((uintptr_t)j.bias | (uintptr_t)j.y | (uintptr_t)j.oq | (uintptr_t)j.oxd) & 3)) {
      set_error("gemv_batch: w and xd must be 16-byte aligned, bias, y, oq and oxd 4-byte aligned");
      return VSIM_EINVAL;
    }
    gelu |= j.gelu_q != 0;
  }
  DevTables tab{};
  if (gelu) RC(tables_get(&tab));
  GemvBatch B{};
  B.nj = a->nj;
  for (int i = 0; i < a->nj; ++i) {
    const vsim_gemv_batch_job &j = a->j[i];
    B.j[i] = gemv_job(j.w, j.M, j.K, j.xd, Q4Rows{}, j.bias, j.y);
    if (j.gelu_q) gelu_quant_into(B.j[i], tab.gelu_f16, ActRow{q4_rows(j.oq, j.M), j.oxd});
  }
  if (kernel) *kernel = gemv_chain_solo(B) ? 1 : 0;
  return launch_gemv_chain_batch(B, (hipStream_t)stream);
}
int vsim_op_q4_expand_f16(const void *w, int M, int K, void *w16, void *stream) {
  if (!w || !w16 || M <= 0 || K <= 0 || K % QK) { set_error("q4_expand_f16: bad argument"); return VSIM_EINVAL; }
  return launch_w4_expand_f16(w4_view(w, M, K), w16, (hipStream_t)stream);
}
int vsim_op_gemm_f16(const void *w16, int M, int K, const void *x16, int n, const float *bias, float *y,
                     void *stream) {
  if (!w16 || !x16 || !y) { set_error("gemm_f16: null argument"); return VSIM_EINVAL; }
  return launch_gemm_f16_256(w16, M, K, x16, n, bias, y, (hipStream_t)stream);
}
int vsim_op_act_quant_f16(const float *x, int K, int n, const float *bias, int gelu, void *x16, void *stream) {
  if (!x || !x16) { set_error("act_quant_f16: null argument"); return VSIM_EINVAL; }
  return launch_act_quant_f16(x, K, n, bias, gelu != 0, x16, (hipStream_t)stream);
}
int vsim_op_gemm_f16_gelu_q(const void *w16, int M, int K, const void *x16, int n, const float *bias, void *q16,
                            void *stream) {
  if (!w16 || !x16 || !q16) { set_error("gemm_f16_gelu_q: null argument"); return VSIM_EINVAL; }
  return launch_gemm_f16_256(w16, M, K, x16, n, bias, nullptr, (hipStream_t)stream, q16);
}
int vsim_op_gemm_f16_rope(const void *w16, int M, int K, const void *x16, int n, const float *bias, float *y,
                          const double *cs, int d, int n_rot, int p0, void *stream) {
  if (!w16 || !x16 || !y || !cs || p0 < 0) { set_error("gemm_f16_rope: bad argument"); return VSIM_EINVAL; }
  G2Epi e;
  e.cs = (const double2 *)cs;
  e.d = d;
  e.n_rot = n_rot;
  e.p0 = p0;
  return launch_gemm_f16_256(w16, M, K, x16, n, bias, y, (hipStream_t)stream, nullptr, &e);
}
int vsim_op_gemm_f16_join(const void *w16, int M, int K, const void *x16, int n, const float *bias, float *res,
                          const float *res_a, void *stream) {
  if (!w16 || !x16 || !res) { set_error("gemm_f16_join: null argument"); return VSIM_EINVAL; }
  G2Epi e;
  e.res = res;
  e.res_a = res_a;
  return launch_gemm_f16_256(w16, M, K, x16, n, bias, res, (hipStream_t)stream, nullptr, &e);
}
int vsim_op_gemm_q4_256(const void *w, int M, int K, const void *x16, int n, const float *bias, float *y, void *q16,
                        const double *cs, int d, int n_rot, int p0, int join, const float *res_a, void *stream) {
  if (!w || !x16 || (!q16 && !y) || M <= 0 || K <= 0 || K % QK || p0 < 0) {
    set_error("gemm_q4_256: bad argument");
    return VSIM_EINVAL;
  }
  if ((q16 != nullptr) + (cs != nullptr) + (join != 0) > 1) {
    set_error("gemm_q4_256: one epilogue at a time (q16, cs or join)");
    return VSIM_EINVAL;
  }
  G2Epi e;
  if (cs) {
    e.cs = (const double2 *)cs;
    e.d = d;
    e.n_rot = n_rot;
    e.p0 = p0;
  } else if (join) {
    e.res = y;
    e.res_a = res_a;
  }
  return launch_gemm_q4_256(w4_view(w, M, K), x16, n, bias, q16 ? nullptr : y, (hipStream_t)stream, q16,
                            cs || join ? &e : nullptr);
}
int vsim_op_get_rows(const void *w, int K, int V, const int32_t *rows, int n, float *y, void *stream) {
  return launch_get_rows(w, K, V, rows, n, y, (hipStream_t)stream);
}
int vsim_norm_fallbacks(unsigned out[2]) { return vsim::norm_stats(out); }
int vsim_spin_timeouts(unsigned *out) { return vsim::spin_timeouts(out); }

int vsim_op_norm(const float *x, float *y, int k, int rows, const float *w, const float *b, void *stream) {
  return launch_norm(x, y, k, rows, w, b, (hipStream_t)stream);
}
int vsim_op_gelu(const float *x, float *y, int n, void *stream) {
  return launch_gelu(x, y, n, nullptr, 1, (hipStream_t)stream);
}
int vsim_op_argmax(const float *x, int n, int32_t *out, void *stream) {
  // one zeroed 16-byte workspace per (device, stream), kept: the kernel leaves it zeroed, so the
  // call is a single launch (no allocation, no synchronization, capturable) like the model's
  static std::mutex mu;
  static std::map<std::pair<int, void *>, unsigned long long *> wss;
  int dev = 0;
  VSIM_HIP(hipGetDevice(&dev));
  unsigned long long *ws = nullptr;
  {
    std::lock_guard<std::mutex> lk(mu);
    unsigned long long *&w = wss[{dev, stream}];
    if (!w) {
      VSIM_HIP(hipMalloc((void **)&w, 2 * sizeof(unsigned long long)));
      VSIM_HIP(hipMemset(w, 0, 2 * sizeof(unsigned long long)));
    }
    ws = w;
  }
  return launch_argmax(x, n, (int *)out, ws, (hipStream_t)stream);
}
int vsim_op_topk(const float *x, int n, const int32_t *win, int nw, double scale, double repeat_penalty, int k,
                 double *val, int32_t *id, void *stream) {
  // one workspace per (device, stream), kept, as vsim_op_argmax's: the kernel leaves its counter zero
  static std::mutex mu;
  static std::map<std::pair<int, void *>, void *> wss;
  int dev = 0;
  VSIM_HIP(hipGetDevice(&dev));
  void *ws = nullptr;
  {
    std::lock_guard<std::mutex> lk(mu);
    void *&w = wss[{dev, stream}];
    if (!w) {
      VSIM_HIP(hipMalloc(&w, TOPK_WS_BYTES));
      VSIM_HIP(hipMemset(w, 0, TOPK_WS_BYTES));
    }
    ws = w;
  }
  return launch_topk(x, n, nullptr, win, nw, scale, repeat_penalty, k, val, id, ws, (hipStream_t)stream);
}
static_assert(sizeof(vsim_topk_params) == sizeof(TopkParams) && offsetof(vsim_topk_params, scale) == offsetof(TopkParams, scale) &&
                  offsetof(vsim_topk_params, penalty) == offsetof(TopkParams, penalty) &&
                  offsetof(vsim_topk_params, k) == offsetof(TopkParams, k) &&
                  offsetof(vsim_topk_params, nw) == offsetof(TopkParams, nw) &&
                  offsetof(vsim_topk_params, win) == offsetof(TopkParams, win),
              "vsim_topk_params is TopkParams");
static_assert(sizeof(vsim_topk_out) == sizeof(TopkOut) && offsetof(vsim_topk_out, val) == offsetof(TopkOut, val) &&
                  offsetof(vsim_topk_out, id) == offsetof(TopkOut, id),
              "vsim_topk_out is TopkOut");
int vsim_op_topk_rows(const float *x, int ldx, int n, int B, const vsim_topk_params *pb, vsim_topk_out *out,
                      void *stream) {
  // VSIM_BATCH_MAX row blocks per (device, stream), kept, as vsim_op_topk's: every row's counter is left zero
  static std::mutex mu;
  static std::map<std::pair<int, void *>, void *> wss;
  int dev = 0;
  VSIM_HIP(hipGetDevice(&dev));
  void *ws = nullptr;
  {
    std::lock_guard<std::mutex> lk(mu);
    void *&w = wss[{dev, stream}];
    if (!w) {
      VSIM_HIP(hipMalloc(&w, VSIM_BATCH_MAX * TOPK_WS_BYTES));
      VSIM_HIP(hipMemset(w, 0, VSIM_BATCH_MAX * TOPK_WS_BYTES));
    }
    ws = w;
  }
  return launch_topk_rows(x, ldx, n, B, (const TopkParams *)pb, (TopkOut *)out, ws, (hipStream_t)stream);
}
int vsim_topk_rows_set_wg(int per_row) { return topk_rows_set_wg(per_row); }
int vsim_op_logprob(const float *x, int V, int R, const int32_t *target, double *logprob, int32_t *argmax, void *stream) {
  return launch_score_rows(x, V, R, target, logprob, argmax, (hipStream_t)stream);
}
int vsim_op_attn_softmax(float *p, int nc, int nr, int nz, int n_past, float scale, void *stream) {
  return launch_attn_softmax(p, nc, nr, nz, n_past, scale, (hipStream_t)stream);
}
int vsim_op_rope(int style, float *x, int d, int H, int T, int n_past, int n_dims, int mode, void *stream) {
  if (n_dims <= 0 || n_dims % 2 || n_dims > d) { set_error("rope: bad n_dims"); return VSIM_EINVAL; }
  const int n_pos = (mode == 0 ? n_past + T : T);
  hipStream_t s = (hipStream_t)stream;
  return with_rope_table(n_pos, n_dims, s, [&](const double2 *cs) {
    return launch_rope(style, x, d, H, T, n_past, n_dims, mode, cs, s);
  });
}
int vsim_op_kq(const float *K, int ldk, const float *Q, int ldq, int d, int H, int nk, int n, float *kq, void *stream) {
  return launch_kq(K, ldk, Q, ldq, d, H, nk, n, kq, (hipStream_t)stream);
}
int vsim_op_kqv(const float *V, int ldv, const float *S, int d, int H, int nk, int n, float *out, void *stream) {
  return launch_kqv(V, ldv, S, d, H, nk, n, out, 0, (hipStream_t)stream);
}
int vsim_op_kq_causal(const float *K, int ldk, const float *Q, int ldq, int d, int H, int nk, int n, int n_past,
                      float *kq, void *stream) {
  if (n_past < 0) { set_error("kq_causal: n_past must be >= 0"); return VSIM_EINVAL; }
  return launch_kq(K, ldk, Q, ldq, d, H, nk, n, kq, (hipStream_t)stream, n_past);
}
int vsim_op_kqv_causal(const float *V, int ldv, const float *S, int d, int H, int nk, int n, int n_past, float *out,
                       void *stream) {
  if (n_past < 0) { set_error("kqv_causal: n_past must be >= 0"); return VSIM_EINVAL; }
  return launch_kqv(V, ldv, S, d, H, nk, n, out, 0, (hipStream_t)stream, n_past);
}
int vsim_op_attn_prefill(const float *Q, const float *kc, const float *vc, int d, int H, int N, int n_past,
                         float scale, float *out, void *stream) {
  return launch_attn_prefill_f16(Q, kc, vc, d, H, N, n_past, scale, out, (hipStream_t)stream);
}
int vsim_op_attn_prefill_q16(const float *Q, const float *kc, const float *vc, int d, int H, int N, int n_past,
                             float scale, void *out16, void *stream) {
  return launch_attn_prefill_f16(Q, kc, vc, d, H, N, n_past, scale, nullptr, (hipStream_t)stream, nullptr, 0, false,
                                 out16);
}
int vsim_op_attn_prefill_layout(int E, int nk, size_t *bytes, size_t *vt_off, int *ldt) {
  if (E <= 0 || nk <= 0) { set_error("attn_prefill_layout: bad argument"); return VSIM_EINVAL; }
  if (bytes) *bytes = attn_prefill_scratch(E, nk);
  if (vt_off) *vt_off = (size_t)(attn_prefill_vt16(nullptr, E, nk) - attn_prefill_k16(nullptr, E, nk));
  if (ldt) *ldt = attn_prefill_ldt(nk);
  return VSIM_OK;
}
int vsim_op_attn_prefill_scratch(const float *Q, const float *kc, const float *vc, int d, int H, int N, int n_past,
                                 float scale, float *out, void *out16, void *scratch, size_t scratch_bytes, int fresh,
                                 void *stream) {
  // (the launcher allocates its own when the caller's is too small: here that is an error)
  if (!Q || !kc || !vc || (!out && !out16) || d <= 0 || H <= 0 || N <= 0 || n_past < 0 || !scratch ||
      scratch_bytes < attn_prefill_scratch(d * H, n_past + N)) {
    set_error("attn_prefill_scratch: bad argument (scratch smaller than vsim_op_attn_prefill_layout's bytes?)");
    return VSIM_EINVAL;
  }
  return launch_attn_prefill_f16(Q, kc, vc, d, H, N, n_past, scale, out16 ? nullptr : out, (hipStream_t)stream, scratch,
                                 scratch_bytes, fresh != 0, out16);
}
int vsim_op_gemm_q4_256_h16(const void *w, int M, int K, const void *x16, int n, const float *bias, float *y,
                            const double *cs, int d, int n_rot, int p0, void *h16, int h16_ld, int h16_t,
                            void *stream) {
  if (!w || !x16 || !y || !h16 || M <= 0 || K <= 0 || K % QK || p0 < 0) {
    set_error("gemm_q4_256_h16: bad argument");
    return VSIM_EINVAL;
  }
  G2Epi e;
  if (cs) {
    e.cs = (const double2 *)cs;
    e.d = d;
    e.n_rot = n_rot;
  }
  e.p0 = p0;
  e.h16 = (_Float16 *)h16;
  e.h16_ld = h16_ld;
  e.h16_t = h16_t;
  return launch_gemm_q4_256(w4_view(w, M, K), x16, n, bias, y, (hipStream_t)stream, nullptr, &e);
}
// ---- the fast decode step's launches (fast_decode.hip) on caller buffers.  The launchers
// check the shapes the kernels stage in LDS; the checks here are the ones the model's own
// shapes make unnecessary (null operands, whole tiles where a kernel writes all 32 rows).
static_assert(FD_PAD == VSIM_FAST_PAD, "include/vsim_hip.h states the weight slack");

int vsim_op_fast_gemv(const vsim_fast_gemv_args *a, void *stream) {
  if (!a || a->nj < 1 || a->nj > 4) { set_error("fast_gemv: 1 to 4 jobs"); return VSIM_EINVAL; }
  const int K = a->j[0].k;
  if (K <= 0 || K % QK) { set_error("fast_gemv: k must be a positive multiple of 32"); return VSIM_EINVAL; }
  FastJob jobs[4];
  Q4Rows gelu_out;  // the GELU job's output row has `rows` values
  bool rope = false, pos = false;
  for (int i = 0; i < a->nj; ++i) {
    const vsim_fast_job &j = a->j[i];
    const bool whole = j.rows % T32 == 0;
    if (!j.w || j.rows <= 0 || j.k != K || j.epi < FE_STORE || j.epi > FE_V || (j.act != 0 && j.act != 1) ||
        (j.epi != FE_GELU_Q && !j.y) || (j.epi != FE_STORE && !whole) || (j.epi == FE_GELU_Q && (!j.bias || !a->oq)) ||
        (a->lnx ? !a->lnw[j.act] || !a->lnb[j.act] : !a->xq[j.act])) {
      set_error("fast_gemv: bad job (operand missing, k differs, or a partial tile under a non-store epilogue)");
      return VSIM_EINVAL;
    }
    rope |= j.epi == FE_ROPE_Q || j.epi == FE_ROPE_K;
    pos |= j.epi >= FE_ROPE_Q;
    if (j.epi == FE_GELU_Q) gelu_out = q4_rows(a->oq, j.rows);
    jobs[i] = fast_job(j.w, j.rows, j.k, j.bias, j.y, j.epi, j.act);
  }
  if (pos && !a->n_past) { set_error("fast_gemv: n_past missing"); return VSIM_EINVAL; }
  if (rope && (!a->cs || a->d <= 0 || a->n_rot <= 0 || a->n_rot % 2 || a->n_rot > a->d || (a->style != 0 && a->style != 1) ||
               (a->style == 0 ? a->d % T32 != 0 || a->n_rot > T32 : a->d % 2 != 0))) {
    set_error("fast_gemv: RoPE needs cs, an even n_rot <= d, and its pairs inside one 32-row tile");
    return VSIM_EINVAL;
  }
  if (a->clear && a->nclear < 0) { set_error("fast_gemv: nclear < 0"); return VSIM_EINVAL; }
  DevTables tab;
  RC(tables_get(&tab));
  auto row = [&](const void *xq) { return xq ? q4_rows(xq, K) : Q4Rows{}; };
  const FastAct act{.lnx = a->lnx,
                    .n = {NormRow{a->lnw[0], a->lnb[0]}, NormRow{a->lnw[1], a->lnb[1]}},
                    .x = {row(a->xq[0]), row(a->xq[1])}};
  const FastPos at{a->n_past, (const double2 *)a->cs, a->d, a->n_rot, a->style};
  return launch_fast_gemv(fast_gemv(act, jobs, a->nj, tab.gelu_f16, gelu_out, at, a->clear, a->nclear), K,
                          (hipStream_t)stream);
}

int vsim_op_fast_tail(const vsim_fast_tail_args *a, void *stream) {
  if (!a || !a->wf || !a->xf || !a->ffp || !a->q || !a->kc || !a->vc || !a->n_past || !a->part || !a->hcnt || !a->oq) {
    set_error("fast_tail: null argument");
    return VSIM_EINVAL;
  }
  if (a->rows <= 0 || a->rows % T32 || a->k <= 0 || a->k % QK || a->sf < 1 || a->sf > 8 || a->d <= 0 || a->H < 1 ||
      a->nchunk < 1) {
    set_error("fast_tail: bad shape (whole 32-row tiles, k a multiple of 32, 1 <= sf <= 8)");
    return VSIM_EINVAL;
  }
  const FastTail T = fast_tail_job(
      w4_view(a->wf, a->rows, a->k), q4_rows(a->xf, a->k), a->ffp, a->sf,
      FastAttn{.q = a->q, .kc = a->kc, .vc = a->vc, .npast = a->n_past, .d = a->d, .H = a->H, .nchunk = a->nchunk,
               .scale = a->scale, .part = a->part, .hcnt = a->hcnt, .o = q4_rows(a->oq, a->d * a->H)});
  // the per-head counters are this call's (the model zeroes them from the layer's GEMV launch)
  VSIM_HIP(hipMemsetAsync(a->hcnt, 0, (size_t)4 * a->H * sizeof(unsigned), (hipStream_t)stream));
  return launch_fast_tail(T, (hipStream_t)stream);
}

int vsim_op_fast_oproj_join(const void *w, int E, const void *xq, const float *bo, const float *ffp, int sf,
                            const float *bproj, const float *x, float *out, void *stream) {
  if (!w || !xq || !ffp || !bproj || !x || !out || E <= 0 || E % QK || sf < 1 || sf > 8) {
    set_error("fast_oproj_join: bad argument");
    return VSIM_EINVAL;
  }
  return launch_fast_oproj_join(fast_oproj_job(w4_view(w, E, E), q4_rows(xq, E), bo, ffp, sf, bproj, x, out),
                                (hipStream_t)stream);
}
int vsim_op_tables(uint16_t *exp_f16_host, uint16_t *gelu_f16_host) { return tables_host(exp_f16_host, gelu_f16_host); }
int vsim_gemm_set_streamk(int enable) { return gemm_set_streamk(enable); }
int vsim_gemm_set_qk_pair(int mode) { return gemm_set_qk_pair(mode); }
int vsim_gemm_set_tile_order(int cols) { return gemm_set_tile_order(cols); }
int vsim_op_gemm_q4_256_pair(const void *w0, const void *w1, int M, int K, const void *x16, int n, float *y0, float *y1,
                             const double *cs, int d, int n_rot, int p0, void *stream) {
  if (!w0 || !w1 || !x16 || !y0 || !y1 || !cs || M <= 0 || K <= 0 || K % QK || p0 < 0 || n <= 0) {
    set_error("gemm_q4_256_pair: bad argument");
    return VSIM_EINVAL;
  }
  G2Epi e;
  e.cs = (const double2 *)cs;
  e.d = d;
  e.n_rot = n_rot;
  e.p0 = p0;
  return launch_gemm_q4_256_pair(w4_view(w0, M, K), w4_view(w1, M, K), x16, n, y0, y1, e, e, (hipStream_t)stream);
}
int vsim_op_gemm_q4_256_pair_h16(const void *w0, const void *w1, int M, int K, const void *x16, int n, float *y0,
                                 float *y1, const double *cs, int d, int n_rot, int p0, void *h16_1, void *stream) {
  if (!w0 || !w1 || !x16 || !y0 || !y1 || !cs || !h16_1 || M <= 0 || K <= 0 || K % QK || p0 < 0 || n <= 0) {
    set_error("gemm_q4_256_pair_h16: bad argument");
    return VSIM_EINVAL;
  }
  G2Epi e0;
  e0.cs = (const double2 *)cs;
  e0.d = d;
  e0.n_rot = n_rot;
  e0.p0 = p0;
  G2Epi e1 = e0;  // (as run_layer's er / ek)
  e1.h16 = (_Float16 *)h16_1;
  return launch_gemm_q4_256_pair(w4_view(w0, M, K), w4_view(w1, M, K), x16, n, y0, y1, e0, e1, (hipStream_t)stream);
}
int vsim_op_norm_f16q(const float *x, int k, int rows, const float *w, const float *b, void *x16, void *stream) {
  return launch_norm_f16q(x, x16, k, rows, w, b, (hipStream_t)stream);
}
// ---- the launches of the fast-mode prompt layer (run_layer) that had no entry of their own
int vsim_op_gemm_q4_f16x(const void *w, int M, int K, const void *x16, int n, const float *bias, float *y,
                         void *stream) {
  if (!w || !x16 || !y || M <= 0 || K <= 0 || K % QK || n <= 0) { set_error("gemm_q4_f16x: bad argument"); return VSIM_EINVAL; }
  return launch_gemm_f16x(w4_view(w, M, K), x16, n, bias, y, (hipStream_t)stream);
}
int vsim_op_rope_kv_write(int style, float *Q, const float *K, const float *V, float *kcache, float *vcache, int d,
                          int H, int N, int n_past, int n_rot, void *stream) {
  if (!Q || !K || !V || !kcache || !vcache || d <= 0 || H <= 0 || N <= 0 || n_past < 0 || (style != 0 && style != 1) ||
      n_rot < 0 || n_rot % 2 || n_rot > d) {
    set_error("rope_kv_write: bad argument");
    return VSIM_EINVAL;
  }
  hipStream_t s = (hipStream_t)stream;
  if (n_rot == 0) return launch_rope_kv_write(style, Q, K, V, kcache, vcache, d, H, N, n_past, 0, nullptr, s);
  return with_rope_table(n_past + N, n_rot, s, [&](const double2 *cs) {
    return launch_rope_kv_write(style, Q, K, V, kcache, vcache, d, H, N, n_past, n_rot, cs, s);
  });
}
int vsim_op_add_residual(float *inpL, const float *attn, const float *ff, int n, int order_ff_first, void *stream) {
  if (!inpL || !ff || (!order_ff_first && !attn) || n <= 0) { set_error("add_residual: bad argument"); return VSIM_EINVAL; }
  return launch_add_residual(inpL, attn, ff, n, order_ff_first ? 1 : 0, (hipStream_t)stream);
}
int vsim_op_add_rows(float *x, const float *b, int n, void *stream) {
  if (!x || !b || n <= 0) { set_error("add_rows: bad argument"); return VSIM_EINVAL; }
  return launch_add_bias(x, b, n, 1, (hipStream_t)stream);
}
int vsim_op_gelu_bias(const float *x, float *y, int n, const float *bias, int bias_len, void *stream) {
  if (!x || !y || !bias || n <= 0 || bias_len <= 0) { set_error("gelu_bias: bad argument"); return VSIM_EINVAL; }
  return launch_gelu(x, y, n, bias, bias_len, (hipStream_t)stream);
}
int vsim_op_attn_softmax_alibi(float *p, int nc, int nr, int nz, int n_past, float scale, const float *alibi,
                               void *stream) {
  if (!p || !alibi || nc <= 0 || nr <= 0 || nz <= 0 || n_past < 0) { set_error("attn_softmax_alibi: bad argument"); return VSIM_EINVAL; }
  return launch_attn_softmax(p, nc, nr, nz, n_past, scale, (hipStream_t)stream, alibi, false);
}
int vsim_op_alibi_slopes(float *slopes_host, int n_head) {
  if (!slopes_host || n_head <= 0) { set_error("alibi_slopes: bad argument"); return VSIM_EINVAL; }
  alibi_slopes_host(slopes_host, n_head);
  return VSIM_OK;
}
int vsim_op_kqv_causal_merged(const float *V, int ldv, const float *S, int d, int H, int nk, int n, int n_past,
                              float *out, void *stream) {
  if (n_past < 0) { set_error("kqv_causal_merged: n_past must be >= 0"); return VSIM_EINVAL; }
  return launch_kqv(V, ldv, S, d, H, nk, n, out, 1, (hipStream_t)stream, n_past);
}

}  // extern "C"

// ---------------------------------------------------------------- drop-in state
namespace {

struct WEntry {
  void *dev;
  int rows, k;
};

struct DropIn {
  std::mutex mu;
  bool ready = false;
  int device = 0;
  int mode = VSIM_MODE_EXACT;
  hipStream_t stream = nullptr;
  std::unordered_map<const void *, WEntry> wcache;
  uint8_t *act_aos = nullptr, *act_soa = nullptr;
  float *xd = nullptr, *y = nullptr, *tmp = nullptr;
  size_t act_cap = 0, xd_cap = 0, y_cap = 0, tmp_cap = 0;
  uint64_t calls = 0, h2d = 0, d2h = 0, cached = 0;
} g;

int grow(void **p, size_t *cap, size_t want) {
  if (want <= *cap) return VSIM_OK;
  if (*p) (void)hipFree(*p);
  *p = nullptr;
  const size_t n = want + want / 2;
  VSIM_HIP(hipMalloc(p, n));
  *cap = n;
  return VSIM_OK;
}

int ensure_init() {
  if (g.ready) return VSIM_OK;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    set_error("init_xmax: no HIP device");
    return VSIM_ENODEV;
  }
  const char *e = getenv("VSIM_DEVICE");
  g.device = e ? atoi(e) : 0;
  if (g.device < 0 || g.device >= ndev) g.device = 0;
  const char *md = getenv("VSIM_MODE");
  g.mode = (md && !strcmp(md, "fast")) ? VSIM_MODE_FAST : VSIM_MODE_EXACT;
  VSIM_HIP(hipSetDevice(g.device));
  VSIM_HIP(hipStreamCreateWithFlags(&g.stream, hipStreamNonBlocking));
  DevTables t;
  RC(tables_get(&t));
  g.ready = true;
  return VSIM_OK;
}

[[noreturn]] void die(const char *where) {
  // the reference exits on offload errors (imax.c:64-69, 2042-2049)
  printf("%s: %s\n", where, vsim_last_error());
  fflush(stdout);
  exit(1);
}

int upload_tensor(const ggml_tensor *t, void **dev, size_t *cap) {
  size_t nb = (size_t)t->ne[0] * t->ne[1] * t->ne[2] * t->ne[3] * sizeof(float);
  RC(grow(dev, cap, nb));
  VSIM_HIP(hipMemcpyAsync(*dev, t->data, nb, hipMemcpyHostToDevice, g.stream));
  g.h2d += nb;
  return VSIM_OK;
}

bool contiguous_f32(const ggml_tensor *t) {
  return t->type == GGML_TYPE_F32 && t->nb[0] == 4 && t->nb[1] == t->nb[0] * t->ne[0] &&
         t->nb[2] == t->nb[1] * t->ne[1] && t->nb[3] == t->nb[2] * t->ne[2];
}

}  // namespace

extern "C" {

// imax.c:52-142: device init.  Same symbol, called once by vsim.cpp:788 after the model
// load; selects the GPU (VSIM_DEVICE), builds the fp16 tables, creates the stream.
void init_xmax(void) {
  std::lock_guard<std::mutex> lk(g.mu);
  if (ensure_init()) die("init_xmax");
  hipDeviceProp_t p;
  if (hipGetDeviceProperties(&p, g.device) == hipSuccess)
    printf("vsim-hip: device %d %s (%s), %d CUs, mode=%s\n", g.device, p.name, p.gcnArchName, p.multiProcessorCount,
           g.mode == VSIM_MODE_EXACT ? "exact" : "fast");
}

// imax.c:1133-1139 signature, called from ggml.c:5115 in the COMPUTE phase of every
// Q4_0 x F32 mul_mat with params->wdata = the Q4_0-quantized src1 rows (INIT phase,
// ggml.c:5024-5041).  Thread 0 runs the whole product on the GPU; other threads of the
// reference's pool return at once and meet thread 0 at ggml's barrier.
void imax_ggml_compute_forward_mul_mat_q4_0_f32(int THREAD, int LANE, const struct ggml_compute_params *params,
                                                const struct ggml_tensor *src0, const struct ggml_tensor *src1,
                                                struct ggml_tensor *dst) {
  (void)THREAD;
  (void)LANE;
  if (params->type != GGML_TASK_COMPUTE || params->ith != 0) return;
  std::lock_guard<std::mutex> lk(g.mu);
  if (ensure_init()) die("imax_ggml_compute_forward_mul_mat_q4_0_f32");
  const int K = src0->ne[0], M = src0->ne[1], N = src1->ne[1];
  if (src0->type != GGML_TYPE_Q4_0 || src0->ne[2] != 1 || src0->ne[3] != 1 || src1->ne[2] != 1 ||
      src1->ne[3] != 1 || K % QK || src0->nb[1] != (size_t)K / QK * QBYTES || dst->nb[0] != 4 ||
      dst->nb[1] != (size_t)M * 4) {
    printf("imax_ggml_compute_forward_mul_mat_q4_0_f32: unsupported shape ne00=%d ne01=%d ne02=%d ne11=%d\n", K, M,
           src0->ne[2], N);
    exit(1);
  }
  hipStream_t s = g.stream;
  if (hipSetDevice(g.device) != hipSuccess) die("hipSetDevice");
  // device weight cache, keyed by the host tensor (model weights live for the run)
  auto it = g.wcache.find(src0->data);
  if (it == g.wcache.end() || it->second.rows != M || it->second.k != K) {
    const size_t wb = (size_t)M * K / QK * QBYTES;
    void *dev = nullptr, *stage = nullptr;
    if (hipMalloc(&dev, w4_bytes(M, K)) != hipSuccess || hipMalloc(&stage, wb) != hipSuccess) die("weight cache alloc");
    if (hipMemcpyAsync(stage, src0->data, wb, hipMemcpyHostToDevice, s) != hipSuccess) die("weight upload");
    if (launch_q4_repack(stage, dev, M, K, s)) die("weight repack");
    if (hipStreamSynchronize(s) != hipSuccess) die("weight upload sync");
    (void)hipFree(stage);
    if (it != g.wcache.end()) (void)hipFree(it->second.dev);
    g.wcache[src0->data] = WEntry{dev, M, K};
    g.h2d += wb;
    g.cached += wb;
    it = g.wcache.find(src0->data);
  }
  const size_t ab = (size_t)N * K / QK * QBYTES;
  if (grow((void **)&g.act_aos, &g.act_cap, ab) || grow((void **)&g.act_soa, &g.tmp_cap, ab) ||
      grow((void **)&g.xd, &g.xd_cap, (size_t)N * K * 4) || grow((void **)&g.y, &g.y_cap, (size_t)N * M * 4))
    die("activation alloc");
  if (hipMemcpyAsync(g.act_aos, params->wdata, ab, hipMemcpyHostToDevice, s) != hipSuccess) die("activation upload");
  if (launch_act_repack(g.act_aos, g.act_soa, N, K, s)) die("activation repack");
  if (launch_q4_dequant(g.act_soa, N, K, g.xd, s)) die("activation dequant");
  if (launch_q4_gemv(it->second.dev, M, K, g.act_soa, g.xd, N, nullptr, g.y, g.mode, s)) die("gemv");
  if (hipMemcpyAsync(dst->data, g.y, (size_t)N * M * 4, hipMemcpyDeviceToHost, s) != hipSuccess) die("result copy");
  if (hipStreamSynchronize(s) != hipSuccess) die("gemv sync");
  g.calls++;
  g.h2d += ab;
  g.d2h += (size_t)N * M * 4;
}

void vsim_dropin_stats(uint64_t *calls, uint64_t *h2d, uint64_t *d2h, uint64_t *cached) {
  std::lock_guard<std::mutex> lk(g.mu);
  if (calls) *calls = g.calls;
  if (h2d) *h2d = g.h2d;
  if (d2h) *d2h = g.d2h;
  if (cached) *cached = g.cached;
}

void vsim_dropin_reset(void) {
  std::lock_guard<std::mutex> lk(g.mu);
  for (auto &kv : g.wcache) (void)hipFree(kv.second.dev);
  g.wcache.clear();
  g.calls = g.h2d = g.d2h = g.cached = 0;
}

// ---- hooks for the reference's static ggml.c kernels (host tensors in/out, exact) ----
// Contract (include/vsim_hip.h): a hook is called by every thread of the reference's pool in
// every phase of the node.  Its checks read tensor metadata only, so all threads reach the
// same verdict: either every thread gets VSIM_EINVAL and runs its own CPU slice, or thread 0
// runs the whole op in its COMPUTE phase and every other call returns 0 ("handled": the INIT
// and FINALIZE phases then have nothing left to do).  A device failure after the checks exits,
// as the reference's offload layer does (imax.c:2042-2049).
namespace {

size_t f32_span(const ggml_tensor *t) {
  size_t s = 4;
  for (int i = 0; i < 4; ++i)
    if (t->ne[i] > 1) s += (size_t)(t->ne[i] - 1) * t->nb[i];
  return s;
}

GT gt_dev(const ggml_tensor *t, const void *dev) {
  GT g;
  g.p = (const char *)dev;
  for (int i = 0; i < 4; ++i) {
    g.ne[i] = t->ne[i];
    g.nb[i] = (long long)t->nb[i];
  }
  return g;
}

// cached device buffers of the hooks (grown, never freed per call)
void *hb[4] = {nullptr, nullptr, nullptr, nullptr};
size_t hcap[4] = {0, 0, 0, 0};
double2 *hcs = nullptr;
size_t hcs_cap = 0;

void *hbuf(int i, size_t bytes, const char *what) {
  if (grow(&hb[i], &hcap[i], bytes)) die(what);
  return hb[i];
}

void to_dev(void *dev, const void *host, size_t bytes) {
  if (hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, g.stream) != hipSuccess) die("hook upload");
  g.h2d += bytes;
}

void to_host(void *host, const void *dev, size_t bytes) {
  if (hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, g.stream) != hipSuccess ||
      hipStreamSynchronize(g.stream) != hipSuccess)
    die("hook download");
  g.d2h += bytes;
}

bool handled_elsewhere(const ggml_compute_params *params) {
  return params->type != GGML_TASK_COMPUTE || params->ith != 0;
}

void lock_and_init(const char *who) {
  if (ensure_init()) die(who);
  if (hipSetDevice(g.device) != hipSuccess) die(who);
}

}  // namespace

// ggml_compute_forward_gptneox_rope_f32 (ggml.c:6086) / ggml_compute_forward_rope_f32
// (ggml.c:5919): src0 [d, H, T] contiguous F32, src1 I32 {n_past, n_dims, mode}, in place.
static int rope_hook(int style, const struct ggml_compute_params *params, const struct ggml_tensor *src0,
                     const struct ggml_tensor *src1, struct ggml_tensor *dst) {
  const int32_t *pr = src1 && src1->type == GGML_TYPE_I32 ? (const int32_t *)src1->data : nullptr;
  if (!contiguous_f32(src0) || src0->ne[3] != 1 || dst->data != src0->data || !pr || pr[1] <= 0 || pr[1] % 2 ||
      pr[1] > src0->ne[0] || (pr[2] != 0 && pr[2] != 1)) {
    set_error("rope hook: needs a contiguous in-place F32 [d,H,T] tensor and {n_past, n_dims, mode}");
    return VSIM_EINVAL;
  }
  if (handled_elsewhere(params)) return 0;
  std::lock_guard<std::mutex> lk(g.mu);
  lock_and_init("rope hook");
  const int d = src0->ne[0], H = src0->ne[1], T = src0->ne[2], n_past = pr[0], n_dims = pr[1], mode = pr[2];
  const size_t nb = (size_t)d * H * T * 4;
  const int n_pos = mode == 0 ? n_past + T : T;
  std::vector<double2> cs((size_t)n_pos * (n_dims / 2));
  rope_table_host(cs.data(), n_pos, n_dims);
  float *x = (float *)hbuf(0, nb, "rope hook alloc");
  if (grow((void **)&hcs, &hcs_cap, cs.size() * sizeof(double2))) die("rope hook alloc");
  to_dev(x, src0->data, nb);
  to_dev(hcs, cs.data(), cs.size() * sizeof(double2));
  if (launch_rope(style, x, d, H, T, n_past, n_dims, mode, hcs, g.stream)) die("rope hook");
  to_host(dst->data, x, nb);
  return 0;
}

int vsim_ggml_gptneox_rope_f32(const struct ggml_compute_params *params, const struct ggml_tensor *src0,
                               const struct ggml_tensor *src1, struct ggml_tensor *dst) {
  return rope_hook(0, params, src0, src1, dst);
}

int vsim_ggml_rope_f32(const struct ggml_compute_params *params, const struct ggml_tensor *src0,
                       const struct ggml_tensor *src1, struct ggml_tensor *dst) {
  return rope_hook(1, params, src0, src1, dst);
}

// ggml_compute_forward_soft_max_f32 (ggml.c:5825): rows of ne0, in place (scale = 1,
// no mask: the reference applies scale and diag_mask_inf as separate nodes before).
int vsim_ggml_soft_max_f32(const struct ggml_compute_params *params, const struct ggml_tensor *src0,
                           struct ggml_tensor *dst) {
  if (!contiguous_f32(src0) || dst->data != src0->data) {
    set_error("soft_max hook: needs a contiguous in-place F32 tensor");
    return VSIM_EINVAL;
  }
  if (handled_elsewhere(params)) return 0;
  std::lock_guard<std::mutex> lk(g.mu);
  lock_and_init("soft_max hook");
  const int nc = src0->ne[0], nr = src0->ne[1] * src0->ne[2] * src0->ne[3];
  const size_t nb = (size_t)nc * nr * 4;
  float *x = (float *)hbuf(0, nb, "soft_max hook alloc");
  to_dev(x, src0->data, nb);
  if (launch_attn_softmax(x, nc, nr, 1, nc, 1.0f, g.stream)) die("soft_max hook");
  to_host(dst->data, x, nb);
  return 0;
}

// ggml_compute_forward_mul_mat_f32 (ggml.c:4355-4595) for any strided F32 views: src0 rows
// contiguous -> double-accumulated dots (the KQ product, vsim.cpp:583); src0 transposed ->
// sequential mads in params->nth column partials, summed in thread order (the KQV product,
// vsim.cpp:607), the grouping the reference's pool uses at that thread count.
int vsim_ggml_mul_mat_f32(const struct ggml_compute_params *params, const struct ggml_tensor *src0,
                          const struct ggml_tensor *src1, struct ggml_tensor *dst) {
  const bool types = src0->type == GGML_TYPE_F32 && src1->type == GGML_TYPE_F32 && dst->type == GGML_TYPE_F32;
  const bool shapes = src0->ne[0] == src1->ne[0] && src0->ne[2] == src1->ne[2] && src0->ne[3] == src1->ne[3] &&
                      dst->ne[0] == src0->ne[1] && dst->ne[1] == src1->ne[1] && dst->ne[2] == src0->ne[2] &&
                      dst->ne[3] == src1->ne[3];
  const bool dot = src0->nb[1] >= src0->nb[0];
  const bool layout = dot ? (src0->nb[0] == 4 && src1->nb[0] == 4 && dst->nb[0] == 4)
                          : (src0->nb[1] == 4 && contiguous_f32(dst));
  if (!types || !shapes || !layout || params->nth <= 0) {
    set_error("mul_mat_f32 hook: unsupported F32 operands");
    return VSIM_EINVAL;
  }
  if (handled_elsewhere(params)) return 0;
  std::lock_guard<std::mutex> lk(g.mu);
  lock_and_init("mul_mat_f32 hook");
  const size_t sa = f32_span(src0), sb = f32_span(src1), sd = f32_span(dst);
  char *da = (char *)hbuf(1, sa, "mul_mat_f32 hook alloc");
  char *db = (char *)hbuf(2, sb, "mul_mat_f32 hook alloc");
  char *dd = (char *)hbuf(3, sd, "mul_mat_f32 hook alloc");
  to_dev(da, src0->data, sa);
  to_dev(db, src1->data, sb);
  int rc;
  if (dot) {
    to_dev(dd, dst->data, sd);  // strided dst: the bytes between its elements stay as they were
    rc = launch_g_mm_dot(gt_dev(dst, dd), gt_dev(src0, da), gt_dev(src1, db), src0->ne[0], g.stream);
  } else {
    rc = launch_g_mm_mad((float *)dd, gt_dev(src0, da), gt_dev(src1, db), src1->ne[0], params->nth, dst->ne[0],
                         dst->ne[1], dst->ne[2], dst->ne[3], g.stream);
  }
  if (rc) die("mul_mat_f32 hook");
  to_host(dst->data, dd, sd);
  return 0;
}

}  // extern "C"
