// vsim_amd/csrc/decode_jobs.hpp — the kernel arguments of the three single-token decode steps (exact,
// fast, weight-only), built in one place.
//
// Host code only.  model.cpp's executor (enqueue_decode, the rows batch, enqueue_decode_fast,
// enqueue_decode_w4a16) and capi.cpp's op entries (vsim_op_attn_decode_batch, _tail_attn, _tail_ln,
// _ln_quant, _gemv_batch; _fast_gemv, _fast_tail, _fast_oproj_join; _w4a16_ln, _w4a16_gemv) fill
// GemvJob, LnQuantJob, TailLn and AttnJob, FastGemv, FastTail and FastOproj, W4a16Ln and W4a16Gemv
// through these builders, so a field or a layout rule is stated once and the op entries' tests pin
// the code the executor runs.  The kernel-argument structs themselves (common.hpp, fast.hpp) keep
// their flat fields: the views below never travel to the device.
#pragma once

#include <cmath>
#include <initializer_list>

#include "common.hpp"
#include "fast.hpp"

namespace vsim {

// ---------------------------------------------------------------- Q4 activation rows
// `rows` Q4 SoA activation rows of k values (launch_q4_quantize's layout): the 16-byte nibble
// groups of every row's k/32 blocks first, then the scales of the same blocks.
struct Q4Rows {
  uint8_t *qs = nullptr;
  float *d = nullptr;
};
inline Q4Rows q4_rows(const void *base, int k, int rows = 1) {
  uint8_t *p = (uint8_t *)base;
  return {p, (float *)(p + (size_t)rows * (k / QK) * 16)};
}
// an activation row as the exact kernels read and write it: quantized, and its dequantized factors
struct ActRow {
  Q4Rows q;
  float *xd = nullptr;
};

// ---------------------------------------------------------------- tail workspace
// The layer tail's hand-off block (TailSync, TailLn), one allocation: the step epoch on a 256-byte
// line of its own, og [E], jg [E], rec [2 E/32], the heads' flags [TAIL_MAX_HEADS].  Zeroed at
// allocation (tag 0 never matches).  E = 0: the epoch and the flags alone (a tail without TailLn).
struct TailWs {
  unsigned *ep = nullptr;
  unsigned long long *og = nullptr, *jg = nullptr;
  uint4 *rec = nullptr;
  unsigned long long *hflag = nullptr;
};
inline size_t tail_ws_bytes(size_t E) {
  return 256 + 2 * E * sizeof(unsigned long long) + 2 * (E / QK) * sizeof(uint4) +
         (size_t)TAIL_MAX_HEADS * sizeof(unsigned long long);
}
inline TailWs tail_ws_carve(void *base, size_t E) {
  TailWs w;
  if (!base) return w;
  w.ep = (unsigned *)base;
  w.og = (unsigned long long *)((uint8_t *)base + 256);
  w.jg = w.og + E;
  w.rec = (uint4 *)(w.jg + E);
  w.hflag = (unsigned long long *)(w.rec + 2 * (E / QK));
  return w;
}

// ---------------------------------------------------------------- attention
// The reference's KQ scale 1/sqrt(n_embd/n_head) with its float and double roundings (vsim.cpp:588)
inline float default_attn_scale(int E, int H) { return (float)(1.0f / std::sqrt((double)(float(E) / H))); }

// One decode attention over the new q / k / v rows [E]: what AttnJob says apart from the cache and
// the position, which a single-token step gives per layer and a rows batch per row (AttnRows).
struct AttnDesc {
  int d = 0, H = 0, n_rot = 0, style = 0, n_ctx = 0, nsplit = 1, kqv_nth = 0;
  float scale = 0.0f;
  const float *alibi = nullptr;
  const float *q = nullptr, *k = nullptr, *v = nullptr;
  const double2 *cs = nullptr;     // RoPE table (n_rot > 0)
  const uint16_t *etab = nullptr;  // DevTables::exp_f16
  ActRow o;                        // the out-projection's activation row(s)
  float *out = nullptr;            // optional float copy
};
inline AttnJob attn_job(const AttnDesc &D, float *kc, float *vc, const int *npast) {
  return AttnJob{.q = D.q, .k = D.k, .v = D.v, .kc = kc, .vc = vc, .npast = npast, .cs = D.cs, .etab = D.etab, .d = D.d,
                 .H = D.H, .n_rot = D.n_rot, .style = D.style, .n_ctx = D.n_ctx, .nsplit = D.nsplit,
                 .kqv_nth = D.kqv_nth, .scale = D.scale, .alibi = D.alibi, .oq_qs = D.o.q.qs, .oq_d = D.o.q.d,
                 .oxd = D.o.xd, .out = D.out};
}

// ---------------------------------------------------------------- LayerNorm + quantize
// one norm's affine and the row it leaves
struct NormRow {
  const float *w = nullptr, *b = nullptr;
  ActRow o;
};
// the residual join ahead of a norm (LnQuantJob): row = x + ((ja + jab) + (jf + jfb)), to jout if non-null
struct LnJoin {
  const float *ja = nullptr, *jab = nullptr, *jf = nullptr, *jfb = nullptr;
  float *jout = nullptr;
};
// One or two norms of one row for launch_ln_quant(j1, second(), n, s).  Both jobs join the same
// operands; the first alone stores the joined row and advances the epoch.
struct LnQuantPair {
  LnQuantJob j1, j2;
  bool two;
  const LnQuantJob *second() const { return two ? &j2 : nullptr; }
};
inline LnQuantPair ln_quant_jobs(const float *x, const NormRow &n1, const NormRow *n2, const LnJoin *join,
                                 unsigned *ep) {
  const LnJoin none, &j = join ? *join : none;
  const NormRow &m2 = n2 ? *n2 : n1;
  return LnQuantPair{
      LnQuantJob{.x = x, .w = n1.w, .b = n1.b, .qs = n1.o.q.qs, .d = n1.o.q.d, .xd = n1.o.xd, .ja = j.ja, .jab = j.jab,
                 .jf = j.jf, .jfb = j.jfb, .jout = j.jout, .ep = ep},
      LnQuantJob{.x = x, .w = m2.w, .b = m2.b, .qs = m2.o.q.qs, .d = m2.o.q.d, .xd = m2.o.xd, .ja = j.ja, .jab = j.jab,
                 .jf = j.jf, .jfb = j.jfb, .jout = nullptr, .ep = nullptr},
      n2 != nullptr};
}

// The next LayerNorm(s) inside the layer tail: x + ((attention + ab) + (fc_out + fb)) to jout, norm 1
// and optionally norm 2 of it, over the workspace's granules under the tag of layer il.
inline TailLn tail_ln_job(const float *x, float *jout, const float *ab, const float *fb, const NormRow &n1,
                          const NormRow *n2, const TailWs &ws, unsigned *stats, int il) {
  const NormRow none, &m2 = n2 ? *n2 : none;
  return TailLn{.x = x, .ab = ab, .fb = fb, .jout = jout, .w1 = n1.w, .b1 = n1.b, .q1 = n1.o.q.qs, .d1 = n1.o.q.d,
                .xd1 = n1.o.xd, .w2 = m2.w, .b2 = m2.b, .q2 = m2.o.q.qs, .d2 = m2.o.q.d, .xd2 = m2.o.xd, .og = ws.og,
                .jg = ws.jg, .rec = ws.rec, .ep = ws.ep, .stats = stats, .il = il};
}

// ---------------------------------------------------------------- GEMV jobs
// y = W x (+ bias), W a Q4_0 [M][K] weight, x one activation row: its factors xd (exact mode) and
// its quants xq (fast mode; none where only the exact kernels run)
inline GemvJob gemv_job(const void *W, int M, int K, const float *xd, const Q4Rows &xq, const float *bias, float *y) {
  return GemvJob{.w = w4_view(W, M, K), .xd = xd, .xqs = xq.qs, .xdd = xq.d, .bias = bias, .y = y, .epi = EPI_STORE};
}
inline GemvJob gemv_job(const void *W, int M, int K, const ActRow &x, const float *bias, float *y) {
  return gemv_job(W, M, K, x.xd, x.q, bias, y);
}
// the GELU + quantize epilogue (EPI_GELU_Q): the job's result leaves as the next product's row o
inline void gelu_quant_into(GemvJob &J, const uint16_t *gelu_tab, const ActRow &o) {
  J.epi = EPI_GELU_Q;
  J.gelu_tab = gelu_tab;
  J.oq_qs = o.q.qs;
  J.oq_d = o.q.d;
  J.oxd = o.xd;
}
inline GemvBatch gemv_batch(std::initializer_list<GemvJob> jobs) {
  GemvBatch B{};
  for (const GemvJob &J : jobs) B.j[B.nj++] = J;
  return B;
}

// ---------------------------------------------------------------- fast step (fast.hpp)
// fc_out's K splits: FD_SF, doubled until one split's activation slice fits the LDS staging (at most
// FD_MAXE values), at most 8 (launch_fast_tail refuses a slice that is still too long)
inline int fast_sf(int E) {
  int sf = FD_SF;
  while (sf < 8 && 4 * E / sf > FD_MAXE) sf *= 2;
  return sf;
}
// the attention's chunk workgroups per head over a context of n_ctx positions
inline int fast_nchunk(int n_ctx) { return (n_ctx + FD_CHUNK - 1) / FD_CHUNK; }

inline FastJob fast_job(const void *W, int M, int K, const float *bias, float *y, int epi, int act) {
  return FastJob{.w = w4_view(W, M, K), .bias = bias, .y = y, .epi = epi, .act = act};
}
// A GEMV batch's two activations (chosen per job by `act`): the LayerNorm of the residual row lnx with
// the affine n[act] in every workgroup's prologue (the rows stay in LDS: n[].o unused), or, lnx
// null, the Q4 rows x[act]
struct FastAct {
  const float *lnx = nullptr;
  NormRow n[2];
  Q4Rows x[2];
};
// the position and the rotation of the FE_ROPE_Q / FE_ROPE_K / FE_V epilogues
struct FastPos {
  const int *npast = nullptr;
  const double2 *cs = nullptr;
  int d = 0, n_rot = 0, style = 0;
};
// k_fast_gemv's batch.  gelu_tab and the row o (of that job's M values) go with an FE_GELU_Q job;
// the head dim only with a RoPE job (1 otherwise: the kernel takes row % d); under a prologue no
// global activation rows; clear[0 .. nclear) are the counters workgroup 0 zeroes.
inline FastGemv fast_gemv(const FastAct &A, const FastJob *jobs, int nj, const uint16_t *gelu_tab, const Q4Rows &o,
                          const FastPos &pos, unsigned *clear, int nclear) {
  bool gelu = false, rope = false;
  for (int i = 0; i < nj; ++i) {
    gelu |= jobs[i].epi == FE_GELU_Q;
    rope |= jobs[i].epi == FE_ROPE_Q || jobs[i].epi == FE_ROPE_K;
  }
  const Q4Rows none, &x0 = A.lnx ? none : A.x[0], &x1 = A.lnx ? none : A.x[1];
  FastGemv P{.xq = {x0.qs, x1.qs}, .xd = {x0.d, x1.d}, .nj = nj, .gelu_tab = gelu ? gelu_tab : nullptr,
             .oq_qs = gelu ? o.qs : nullptr, .oq_d = gelu ? o.d : nullptr, .npast = pos.npast, .cs = pos.cs,
             .d = rope ? pos.d : 1, .n_rot = pos.n_rot, .style = pos.style, .lnx = A.lnx,
             .lnw = {A.n[0].w, A.n[1].w}, .lnb = {A.n[0].b, A.n[1].b}, .clear = clear, .nclear = clear ? nclear : 0};
  for (int i = 0; i < nj; ++i) P.j[i] = jobs[i];
  return P;
}

// k_fast_tail's attention half: the rotated q [H d] against the layer's cache (the new row in place)
// in nchunk chunks per head; part [H][nchunk][d + 2], hcnt [4 H] counters, o the merged output row
struct FastAttn {
  const float *q = nullptr, *kc = nullptr, *vc = nullptr;
  const int *npast = nullptr;
  int d = 0, H = 0, nchunk = 0;
  float scale = 0.0f;
  float *part = nullptr;
  unsigned *hcnt = nullptr;
  Q4Rows o;
};
// fc_out (weight wf, its activation xf: the batch's GELU row) in sf K splits to ffp [sf][rows], beside A
inline FastTail fast_tail_job(const W4 &wf, const Q4Rows &xf, float *ffp, int sf, const FastAttn &A) {
  return FastTail{.wf = wf, .xf_qs = xf.qs, .xf_d = xf.d, .ffp = ffp, .sf = sf, .q = A.q, .kc = A.kc, .vc = A.vc,
                  .npast = A.npast, .d = A.d, .H = A.H, .nchunk = A.nchunk, .scale = A.scale, .part = A.part,
                  .hcnt = A.hcnt, .oq_qs = A.o.qs, .oq_d = A.o.d};
}
// out = res + ((w x + bo) + (sum of ffp's sf rows + bproj)), x the tail's merged attention row
inline FastOproj fast_oproj_job(const W4 &w, const Q4Rows &x, const float *bo, const float *ffp, int sf,
                                const float *bproj, const float *res, float *out) {
  return FastOproj{.w = w, .xq = x.qs, .xd = x.d, .bo = bo, .ffp = ffp, .sf = sf, .bproj = bproj, .x = res, .out = out};
}

// ---------------------------------------------------------------- weight-only step (common.hpp)
// A row operand of weight-only mode in the exact step's buffers: the halves live where the row's
// factors are ([K] halves in room for [K] floats), the exponent where its nibbles are
struct W4a16Operand {
  _Float16 *h = nullptr;
  int32_t *e = nullptr;
};
inline W4a16Operand w4a16_operand(const ActRow &r) { return {(_Float16 *)r.xd, (int32_t *)r.q.qs}; }

// y = W x (+ bias), or that + res, or res + (res_a + that)
inline W4a16GemvJob w4a16_gemv_job(const void *W, int M, int K, const W4a16Operand &x, const float *bias, float *y,
                                   const float *res = nullptr, const float *res_a = nullptr) {
  return W4a16GemvJob{.w = w4_view(W, M, K), .x16 = x.h, .e = x.e, .bias = bias, .res = res, .res_a = res_a, .y = y};
}
inline W4a16Gemv w4a16_gemv(std::initializer_list<W4a16GemvJob> jobs) {
  W4a16Gemv B{};
  for (const W4a16GemvJob &J : jobs) B.j[B.nj++] = J;
  return B;
}
// the norm n1 of x[n] to the operand o1 and, n2 given, the norm n2 to o2 (n[].o unused); without n2
// nothing of a second norm is passed on, with it all four fields as they are
inline W4a16Ln w4a16_ln_job(const float *x, int n, const NormRow &n1, const W4a16Operand &o1, const NormRow *n2 = nullptr,
                            const W4a16Operand &o2 = {}) {
  const NormRow none, &m2 = n2 ? *n2 : none;
  const W4a16Operand p2 = n2 ? o2 : W4a16Operand{};
  return W4a16Ln{.x = x, .n = n, .w1 = n1.w, .b1 = n1.b, .h1 = o1.h, .e1 = o1.e, .w2 = m2.w, .b2 = m2.b, .h2 = p2.h,
                 .e2 = p2.e};
}

}  // namespace vsim
