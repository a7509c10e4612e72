// vsim_amd/csrc/attn_w4a16.hip — weight-only mode's fp16 MFMA attention (opt-in: vsim_w4a16_set_attn).
//
// The contract is a formula per row, not a kernel.  For one head of D dims and a query at absolute
// position p, over keys 0..p of that sequence's fp32 cache (tests/attn_ref.py's arithmetic):
//   q16 = fp16(float32(q) * qs),  qs = float32(scale) * float32(log2 e);  k16 = fp16(k), v16 = fp16(v)
//   key blocks of 64, aligned to key 0 (not to n_past, not to the batch), visited 0, 1, .., p / 64;
//   per block  S = K16 · q16 on v_mfma_f32_32x32x16_f16, D / 16 steps in order from C = 0, keys the
//              A rows, queries the B columns;
//              keys > p are left out of the maximum and get p_k = 0 exactly;
//              m' = max(m, block max), alpha = exp2f(m - m'), p_k = exp2f(s_k - m');
//              l = l alpha + sum p_k: the lane's 32 keys in register order (tile 0 then tile 1, the
//              accumulator's registers 0..15 each), then + the other half's sum (lane ^ 32);
//              O = O alpha, then O += V16^T · fp16(P)^T on the same MFMA, steps (tile t, half s2) in
//              the order (0,0) (0,1) (1,0) (1,1), 32 dims per accumulator tile;
//   y = O / l + 0.0f  (a float division per element).
// Nothing a row's result depends on comes from another row: not its wave's other queries, not N,
// n_past, B, the slot, or cache rows past p.  Both forms below instantiate the same two __device__
// phases (aw_scores, aw_softmax_pv) of one 32-query group x 64-key block, with the same MFMA shape,
// operand roles and k-step order; the single-query form fills all 32 query columns with its one
// query and keeps column 0.
//
// Two hazards and their rules.
//  * Stale cache rows.  A slot's rows past p hold what an earlier sequence left, NaN and Inf
//    included, and 0 x NaN inside the P·V MFMA is NaN.  Rule: the V operand of a key past the
//    sequence's last key is zero and its K operand is the last key's row (clamped); its score is
//    masked whatever it is.  The prompt form gets this from k_kv_f16's zero padding of V^T and from
//    clamping the K row index to the query block's last key; the single-query form zeroes V and
//    clamps K as it converts each block.  (A key between a row's p and its wave's last key is a
//    real key of the prompt: its V is finite in fp16 unless |v| >= 65520, which no model row is.)
//  * Sign of zero.  The prompt form runs a key block for every query of a wave when any of them
//    sees it; a row that sees none of its keys gets alpha = 1, p = 0 and `+ 0` on every O element,
//    which turns a -0 (alpha underflowed to 0 on a negative O) into +0.  The same holds for masked
//    keys inside a row's last block, whose V the single-query form zeroes (+0) and the prompt form
//    does not (p x v may be -0).  A zero's sign in O never changes a non-zero sum, so the two forms
//    differ at most in the sign of an O that is zero at the end.  Rule: canonical zero -- both forms
//    add + 0.0f after the division, so y is never -0.
//
// RoPE of q and the new k, the fp32 cache write and the out-projection's operand stay the exact
// path's, bits included (attn.hpp / k_rope_kv_write; k_w4a16_rows over the whole attention row).
#include <mutex>

#include "kern.hpp"
#include "../../include/vsim_hip.h"

namespace vsim {

namespace {

typedef _Float16 whalf8 __attribute__((ext_vector_type(8)));
typedef _Float16 whalf4 __attribute__((ext_vector_type(4)));
typedef float wf32x16 __attribute__((ext_vector_type(16)));

constexpr int AW_BQ = 128, AW_BK = 64, AW_THREADS = 256;
constexpr int AW_VLD = AW_BK + 8;                        // V^T tile [dim][key], halves
__host__ __device__ constexpr int aw_kld(int D) { return D + 8; }  // K tile [key][dim], halves

// S^T of one 64-key block for a wave's 32 query columns: tiles t = 0, 1 hold keys 32 t + row.
// Lane (r, hl): K row r of the tile as the A operand, query column r's fragment as B.
template <int D>
__device__ __forceinline__ void aw_scores(const whalf8 (&qf)[D / 16], const _Float16 *Ks, int r, int hl,
                                          wf32x16 (&st)[2]) {
  constexpr int KLD = aw_kld(D);
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    st[t] = (wf32x16){};
#pragma unroll
    for (int s = 0; s < D / 16; ++s) {
      const whalf8 kf = *(const whalf8 *)&Ks[(32 * t + r) * KLD + 16 * s + 8 * hl];
      st[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qf[s], st[t], 0, 0, 0);
    }
  }
}

// The block's mask, running maximum, probabilities, sum and O^T += V^T · P^T for the lane's query
// at absolute position qpos; k0 the block's first key.  Vt in vt_pos order.
template <int D>
__device__ __forceinline__ void aw_softmax_pv(wf32x16 (&st)[2], const _Float16 *Vt, int k0, int qpos, int r, int hl,
                                              wf32x16 (&o)[D / 32], float &mrow, float &lrow) {
  constexpr int NT = D / 32;
  float bm = -INFINITY;
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      const int key = k0 + 32 * t + (g & 3) + 8 * (g >> 2) + 4 * hl;
      if (key > qpos) st[t][g] = -INFINITY;
      bm = fmaxf(bm, st[t][g]);
    }
  bm = fmaxf(bm, __shfl_xor(bm, 32, 64));
  const float mnew = fmaxf(mrow, bm);  // (finite: key 0 is visible to every query)
  const float alpha = exp2f(mrow - mnew);
  float ls = 0.0f;
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      const float p = st[t][g] == -INFINITY ? 0.0f : exp2f(st[t][g] - mnew);
      st[t][g] = p;
      ls += p;
    }
  ls += __shfl_xor(ls, 32, 64);
  lrow = lrow * alpha + ls;
  mrow = mnew;
#pragma unroll
  for (int i = 0; i < NT; ++i) o[i] = o[i] * alpha;
  // k-step s2 of tile t covers keys 32 t + 16 s2 + 8 (j >> 2) + 4 hl + (j & 3): chunk 4 t + 2 s2 + hl
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      whalf8 pf;
#pragma unroll
      for (int j = 0; j < 8; ++j) pf[j] = (_Float16)st[t][8 * s2 + j];
#pragma unroll
      for (int i = 0; i < NT; ++i) {
        const whalf8 vf = *(const whalf8 *)&Vt[(32 * i + r) * AW_VLD + 8 * (4 * t + 2 * s2 + hl)];
        o[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pf, o[i], 0, 0, 0);
      }
    }
}

// y = O / l + 0.0f of the lane's query: rows = dims (reg & 3) + 8 (reg >> 2) + 4 hl of tile i
template <int D>
__device__ __forceinline__ void aw_store(const wf32x16 (&o)[D / 32], float lrow, int hl, float *orow) {
#pragma unroll
  for (int i = 0; i < D / 32; ++i)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int dd = 32 * i + 8 * g + 4 * hl;
      *(float4 *)(orow + dd) = make_float4(o[i][4 * g] / lrow + 0.0f, o[i][4 * g + 1] / lrow + 0.0f,
                                           o[i][4 * g + 2] / lrow + 0.0f, o[i][4 * g + 3] / lrow + 0.0f);
    }
}

template <int D>
__device__ __forceinline__ void aw_qfrag(const float *qr, float qscale, int hl, whalf8 (&qf)[D / 16]) {
#pragma unroll
  for (int s = 0; s < D / 16; ++s) {
    const float4 a = *(const float4 *)(qr + 16 * s + 8 * hl), b = *(const float4 *)(qr + 16 * s + 8 * hl + 4);
    whalf8 f;
    f[0] = (_Float16)(a.x * qscale);
    f[1] = (_Float16)(a.y * qscale);
    f[2] = (_Float16)(a.z * qscale);
    f[3] = (_Float16)(a.w * qscale);
    f[4] = (_Float16)(b.x * qscale);
    f[5] = (_Float16)(b.y * qscale);
    f[6] = (_Float16)(b.z * qscale);
    f[7] = (_Float16)(b.w * qscale);
    qf[s] = f;
  }
}

}  // namespace

// The prompt form.  One workgroup = one head x 128 queries (4 waves of 32), keys from the fp16
// K16 / V^T scratch (k_kv_f16) in tiles of 64 through two LDS buffers, as k_attn_prefill_f16 stages
// them; any N >= 1 and any n_past.  Workgroups longest causal range first.
template <int D>
__global__ void __launch_bounds__(AW_THREADS) k_attn_w4a16_tile(const float *__restrict__ Q,
                                                                 const _Float16 *__restrict__ k16,
                                                                 const _Float16 *__restrict__ vt16, int E, int H,
                                                                 int N, int n_past, int ldt, float qscale,
                                                                 float *__restrict__ out) {
  constexpr int KLD = aw_kld(D), VLD = AW_VLD, NT = D / 32;
  constexpr int KCH = AW_BK * D / 8 / AW_THREADS;  // 16-byte chunks per thread per operand tile
  extern __shared__ __attribute__((aligned(16))) _Float16 lds[];
  // buffer b: K tile at lds + b * AW_BK * KLD, V^T tile at lds + 2 * AW_BK * KLD + b * D * VLD
  const int nqb = (N + AW_BQ - 1) / AW_BQ;
  const int h = blockIdx.x % H, q0 = (nqb - 1 - (int)blockIdx.x / H) * AW_BQ;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, hl = lane >> 5;
  const int qw = q0 + wave * 32;           // this wave's first query
  const int myq = min(qw + r, N - 1);      // this lane's query (a column past N repeats the last)
  const int qpos = n_past + myq;
  const _Float16 *kbase = k16 + (size_t)h * D, *vbase = vt16 + (size_t)h * D * ldt;
  whalf8 qf[D / 16];
  aw_qfrag<D>(Q + (size_t)myq * E + h * D, qscale, hl, qf);
  wf32x16 o[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) o[i] = (wf32x16){};
  float mrow = -INFINITY, lrow = 0.0f;

  const int klast = n_past + min(q0 + AW_BQ, N) - 1;  // last key any query of the block sees
  const int nkb = klast / AW_BK + 1;                  // (klast < ldt: the V^T columns exist)
  u32x4 rk[KCH], rv[KCH];
  auto kload = [&](int kb) __attribute__((always_inline)) {
    const int k0 = kb * AW_BK;
#pragma unroll
    for (int c = 0; c < KCH; ++c) {
      const int c8 = tid + AW_THREADS * c;
      const int key = k0 + c8 / (D / 8), col = 8 * (c8 % (D / 8));
      rk[c] = *(const u32x4 *)(kbase + (size_t)min(key, klast) * E + col);
    }
  };
  auto vload = [&](int kb) __attribute__((always_inline)) {
    const int k0 = kb * AW_BK;
#pragma unroll
    for (int c = 0; c < KCH; ++c) {
      const int c8 = tid + AW_THREADS * c;
      rv[c] = *(const u32x4 *)(vbase + (size_t)(c8 / 8) * ldt + k0 + 8 * (c8 % 8));
    }
  };
  auto kstore = [&](int buf) __attribute__((always_inline)) {
    _Float16 *Ks = lds + buf * AW_BK * KLD;
#pragma unroll
    for (int c = 0; c < KCH; ++c) {
      const int c8 = tid + AW_THREADS * c;
      *(u32x4 *)&Ks[(c8 / (D / 8)) * KLD + 8 * (c8 % (D / 8))] = rk[c];
    }
  };
  auto vstore = [&](int buf) __attribute__((always_inline)) {
    _Float16 *Vt = lds + 2 * AW_BK * KLD + buf * D * VLD;
#pragma unroll
    for (int c = 0; c < KCH; ++c) {
      const int c8 = tid + AW_THREADS * c;
      *(u32x4 *)&Vt[(c8 / 8) * VLD + 8 * (c8 % 8)] = rv[c];
    }
  };
  kload(0);
  vload(0);
  kstore(0);
  vstore(0);
  __syncthreads();
  for (int kb = 0; kb < nkb; ++kb) {
    const int k0 = kb * AW_BK, buf = kb & 1;
    const bool next = kb + 1 < nkb;
    // next tile: K rows load during this tile's S^T, V^T rows during its P·V.  (D = 256: loaded and
    // stored between the phases instead -- 64 staging registers beside 64 of Q, 128 of O^T and 32
    // of S^T do not fit one wave's 512.)
    constexpr bool PIPE = D < 256;
    if (PIPE && next) kload(kb + 1);
    const _Float16 *Ks = lds + buf * AW_BK * KLD;
    const _Float16 *Vt = lds + 2 * AW_BK * KLD + buf * D * VLD;
    // wave-uniform: some query of the wave sees a key of the block.  A query that sees none goes
    // through the block with alpha = 1 and p = 0 (the header's zero-sign rule).
    const bool vis = k0 <= n_past + min(qw + 31, N - 1);
    wf32x16 st[2];
    if (vis) aw_scores<D>(qf, Ks, r, hl, st);
    if (next) {
      if (!PIPE) kload(kb + 1);
      kstore(buf ^ 1);
      if (PIPE) vload(kb + 1);
    }
    if (vis) aw_softmax_pv<D>(st, Vt, k0, qpos, r, hl, o, mrow, lrow);
    if (next) {
      if (!PIPE) vload(kb + 1);
      vstore(buf ^ 1);
    }
    __syncthreads();
  }
  if (qw + r < N) aw_store<D>(o, lrow, hl, out + (size_t)myq * E + h * D);
}

// The single-query form.  One workgroup = one (row, head): RoPE of q and the new k and the K / V
// cache row with attn.hpp's arithmetic; then, per 64-key block of the row's fp32 cache, all
// threads convert the block to the fp16 K tile and the V^T tile (rounded as k_kv_f16 rounds, V^T in
// vt_pos order, V zero and K clamped past p) and wave 0 runs the shared phases with its one query
// in all 32 columns.  No LDS score row: n_ctx does not bound it.  (One wave computes: the key
// blocks of a row are a chain, and 31 of the MFMA's 32 query columns are idle as it is.)
// KW = false (k_attn_w4a16_runs, rows that may share a cache): RoPE of q only and no cache store --
// k_kv_rows wrote every row's K / V rows in the launch before; a run's later rows lie past p, where
// K is clamped and V zeroed as for any stale row.
template <int D, bool KW>
__device__ __forceinline__ void aw_rows_body(AttnJob A, AttnRows R, float qscale) {
  constexpr int KLD = aw_kld(D), VLD = AW_VLD, NT = D / 32;
  extern __shared__ __attribute__((aligned(16))) _Float16 lds[];
  _Float16 *Ks = lds, *Vt = lds + AW_BK * KLD;
  float *qh = (float *)(Vt + D * VLD), *kh = qh + D;
  const int h = blockIdx.x, b = blockIdx.y, E = D * A.H;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, hl = lane >> 5;
  const float *q = A.q + (size_t)b * E;
  [[maybe_unused]] const float *k = A.k + (size_t)b * E, *v = A.v + (size_t)b * E;
  float *kc = R.kc[b] + R.loff, *vc = R.vc[b] + R.loff;
  const int p = R.npast[b];
  for (int i = tid; i < D; i += AW_THREADS) {
    qh[i] = q[h * D + i];
    if constexpr (KW) {
      kh[i] = k[h * D + i];
      vc[(size_t)p * E + h * D + i] = v[h * D + i];
    }
  }
  __syncthreads();
  // RoPE (kern.hpp rope_head, the exact heads' lines), position p for both q and k
  rope_head<true, KW>(qh, kh, A.cs, A.n_rot, A.style, p, tid, AW_THREADS);
  __syncthreads();
  if constexpr (KW)
    for (int i = tid; i < D; i += AW_THREADS) kc[(size_t)p * E + h * D + i] = kh[i];
  whalf8 qf[D / 16];
  aw_qfrag<D>(qh, qscale, hl, qf);
  wf32x16 o[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) o[i] = (wf32x16){};
  float mrow = -INFINITY, lrow = 0.0f;
  const float *kb0 = kc + h * D, *vb0 = vc + h * D;
  const int nkb = p / AW_BK + 1;
  // A block's fp32 rows go through registers: every thread's loads of a tile are issued together
  // (K: 64 keys x D / 4 float4, chunk e = key e / (D / 4); V: D dims x 16 quads of keys, chunk e =
  // dim e % D of quad e / D), and -- but for D = 256, whose wave 0 has no registers to spare -- the
  // next block's are in flight while wave 0 computes.
  constexpr int CH = 16 * D / AW_THREADS;
  constexpr bool PIPE = D < 256;
  f32x4 rk[CH], rv[CH];  // (D = 256: never live together)
  auto kload = [&](int kb) __attribute__((always_inline)) {
    const int k0 = kb * AW_BK;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int e = tid + AW_THREADS * c;
      const int kk = e / (D / 4), c4 = (e % (D / 4)) * 4;
      rk[c] = *(const f32x4 *)(kb0 + (size_t)min(k0 + kk, p) * E + c4);  // (K clamped past p)
    }
  };
  auto vload = [&](int kb) __attribute__((always_inline)) {
    const int k0 = kb * AW_BK;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int e = tid + AW_THREADS * c;
      const int dim = e % D, key = k0 + (e / D) * 4;
#pragma unroll
      for (int j = 0; j < 4; ++j) rv[c][j] = key + j <= p ? vb0[(size_t)(key + j) * E + dim] : 0.0f;  // (V zero past p)
    }
  };
  auto kstore = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int e = tid + AW_THREADS * c;
      const int kk = e / (D / 4), c4 = (e % (D / 4)) * 4;
      const whalf4 hk = {(_Float16)rk[c][0], (_Float16)rk[c][1], (_Float16)rk[c][2], (_Float16)rk[c][3]};
      *(whalf4 *)&Ks[kk * KLD + c4] = hk;
    }
  };
  auto vstore = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int e = tid + AW_THREADS * c;
      const int dim = e % D, k4 = (e / D) * 4;
      const whalf4 hv = {(_Float16)rv[c][0], (_Float16)rv[c][1], (_Float16)rv[c][2], (_Float16)rv[c][3]};
      *(whalf4 *)&Vt[dim * VLD + vt_pos(k4)] = hv;  // (a quad stays whole)
    }
  };
  __syncthreads();  // the new row's stores before the loads that read it back
  if (PIPE) {
    kload(0);
    vload(0);
  }
  for (int kb = 0; kb < nkb; ++kb) {
    __syncthreads();  // wave 0 is done with the previous tiles
    if (PIPE) {
      kstore();
      vstore();
    } else {  // (one operand at a time through the same registers)
      kload(kb);
      kstore();
      vload(kb);
      vstore();
    }
    __syncthreads();
    if (PIPE && kb + 1 < nkb) {
      kload(kb + 1);
      vload(kb + 1);
    }
    if (wave == 0) {
      wf32x16 st[2];
      aw_scores<D>(qf, Ks, r, hl, st);
      aw_softmax_pv<D>(st, Vt, kb * AW_BK, p, r, hl, o, mrow, lrow);
    }
  }
  if (wave == 0 && r == 0) aw_store<D>(o, lrow, hl, A.out + (size_t)b * E + h * D);
}

template <int D>
__global__ void __launch_bounds__(AW_THREADS) k_attn_w4a16_rows(AttnJob A, AttnRows R, float qscale) {
  aw_rows_body<D, true>(A, R, qscale);
}

template <int D>
__global__ void __launch_bounds__(AW_THREADS) k_attn_w4a16_runs(AttnJob A, AttnRows R, float qscale) {
  aw_rows_body<D, false>(A, R, qscale);
}

namespace {

template <int D>
constexpr size_t aw_tile_lds() {
  return (size_t)(2 * AW_BK * aw_kld(D) + 2 * D * AW_VLD) * sizeof(_Float16);
}
template <int D>
constexpr size_t aw_rows_lds() {
  return (size_t)(AW_BK * aw_kld(D) + D * AW_VLD) * sizeof(_Float16) + 2 * D * sizeof(float);
}

template <int D>
bool aw_prepare_d() {
  hipFuncAttributes fa;
  return hipFuncSetAttribute((const void *)k_attn_w4a16_tile<D>, hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)aw_tile_lds<D>()) == hipSuccess &&
         hipFuncSetAttribute((const void *)k_attn_w4a16_rows<D>, hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)aw_rows_lds<D>()) == hipSuccess &&
         hipFuncSetAttribute((const void *)k_attn_w4a16_runs<D>, hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)aw_rows_lds<D>()) == hipSuccess &&
         hipFuncGetAttributes(&fa, (const void *)k_attn_w4a16_runs<D>) == hipSuccess &&
         hipFuncGetAttributes(&fa, (const void *)k_attn_w4a16_tile<D>) == hipSuccess &&
         hipFuncGetAttributes(&fa, (const void *)k_attn_w4a16_rows<D>) == hipSuccess;
}

}  // namespace

bool attn_w4a16_supported(int d, int E) { return (d == 64 || d == 96 || d == 128 || d == 256) && E % 64 == 0; }

// the kernels' LDS attributes, once per process (and their code objects loaded before a timed call)
int attn_w4a16_prepare() {
  static std::once_flag once;
  static int rc = VSIM_OK;
  std::call_once(once, [] {
    if (!(aw_prepare_d<64>() && aw_prepare_d<96>() && aw_prepare_d<128>() && aw_prepare_d<256>())) {
      set_error("w4a16 attention: kernel attributes refused");
      rc = VSIM_EHIP;
    }
  });
  return rc;
}

int launch_attn_w4a16_tile(const float *Q, const float *kc, const float *vc, int d, int H, int N, int n_past,
                           float scale, float *out, hipStream_t s, void *scratch, size_t scratch_bytes) {
  if (!Q || !kc || !vc || !out || H <= 0 || N < 1 || n_past < 0 || !attn_w4a16_supported(d, d * H)) {
    set_error("attn_w4a16_prompt: head dim 64, 96, 128 or 256, n_embd a multiple of 64, N >= 1, n_past >= 0");
    return VSIM_EINVAL;
  }
  const int E = d * H, nk = n_past + N;
  const int ldt = attn_prefill_ldt(nk);
  if (!scratch || scratch_bytes < attn_prefill_scratch(E, nk)) {
    set_error("attn_w4a16_prompt: scratch smaller than vsim_op_attn_prefill_layout's bytes");
    return VSIM_EINVAL;
  }
  if (int rc = attn_w4a16_prepare()) return rc;
  _Float16 *k16 = attn_prefill_k16(scratch, E, nk), *vt16 = attn_prefill_vt16(scratch, E, nk);
  if (int rc = launch_kv_f16(kc, vc, E, d, nk, ldt, k16, vt16, s)) return rc;
  const float qscale = scale * 1.4426950408889634f;  // exp(x) = exp2(x * log2 e)
  const dim3 grid(((N + AW_BQ - 1) / AW_BQ) * H);
#define AWT(DD)                                                                                                   \
  hipLaunchKernelGGL(k_attn_w4a16_tile<DD>, grid, dim3(AW_THREADS), aw_tile_lds<DD>(), s, Q, k16, vt16, E, H, N, \
                     n_past, ldt, qscale, out)
  switch (d) {
    case 64: AWT(64); break;
    case 96: AWT(96); break;
    case 128: AWT(128); break;
    default: AWT(256); break;
  }
#undef AWT
  VSIM_HIP(hipGetLastError());
  return VSIM_OK;
}

int launch_attn_w4a16_rows(const AttnJob &A, const AttnRows &R, int B, hipStream_t s, bool runs) {
  if (!attn_w4a16_supported(A.d, A.d * A.H) || A.H <= 0) {
    set_error("attn_w4a16_rows: head dim 64, 96, 128 or 256 and n_embd a multiple of 64");
    return VSIM_EINVAL;
  }
  if (B < 1 || B > VSIM_BATCH_MAX || !R.kc || !R.vc || !R.npast || !A.q || !A.k || !A.v || !A.out || A.alibi ||
      A.n_rot < 0 || A.n_rot > A.d || A.n_rot % 2 || (A.n_rot > 0 && !A.cs)) {
    set_error("attn_w4a16_rows: 1..32 rows with their caches and positions, q, k, v and out; no ALiBi");
    return VSIM_EINVAL;
  }
  if (int rc = attn_w4a16_prepare()) return rc;
  const float qscale = A.scale * 1.4426950408889634f;
  const dim3 grid(A.H, B);
  if (runs)
    if (int rc = launch_kv_rows(A, R, B, s)) return rc;
#define AWR(DD)                                                                                                \
  if (runs)                                                                                                    \
    hipLaunchKernelGGL(k_attn_w4a16_runs<DD>, grid, dim3(AW_THREADS), aw_rows_lds<DD>(), s, A, R, qscale);     \
  else                                                                                                         \
    hipLaunchKernelGGL(k_attn_w4a16_rows<DD>, grid, dim3(AW_THREADS), aw_rows_lds<DD>(), s, A, R, qscale)
  switch (A.d) {
    case 64: AWR(64); break;
    case 96: AWR(96); break;
    case 128: AWR(128); break;
    default: AWR(256); break;
  }
#undef AWR
  VSIM_HIP(hipGetLastError());
  return VSIM_OK;
}

int launch_attn_w4a16_runs(const AttnJob &A, const AttnRows &R, int B, hipStream_t s) {
  return launch_attn_w4a16_rows(A, R, B, s, true);
}

}  // namespace vsim
