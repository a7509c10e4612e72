// vsim_amd/csrc/layer.hip — fused kernels of the single-token decode step.
//
// One decoder layer (vsim.cpp:521-696 for GPT-NeoX with parallel residual, the same ops for
// GPT-J) = 2 launches in exact mode since r06 (3 for layer 0 and the serial fallback):
//   1. k_ln_quant      (the previous layer's residual join +) LayerNorm(s) + affine +
//                      activation quantization (ggml.c:4246, 5024-5041): inpL -> Q4_0
//                      activation row(s) and their xd factors; layer 0 only when the tail
//                      runs the next LayerNorm itself (gemv_chain.hip, TailLn)
//   2. GEMV batch      {fc_in, Q, K, V} in one launch; fc_in's epilogue adds the bias, looks
//                      up GELU and quantizes each 32-row tile into the fc_out activation
//   3. k_layer_tail    (gemv_chain.hip) fc_out beside the attention heads (attn.hpp: RoPE,
//                      KV-cache write, KQ with a double accumulator, scale/softmax with the
//                      fp16 exp table, KQV as a sequential float chain, quantization) and the
//                      out-projection; k_attn_decode below is the same head as its own launch
//                      for contexts whose scores do not fit the tail's LDS
// Every value is computed with the reference's operation order and rounding (exact mode);
// the fast mode swaps in the integer-dot GEMV bodies.  n_past is read from device memory so
// the whole step can be captured once in a hipGraph and replayed per token.
#include <cstdlib>

#include "attn.hpp"
#include "kern.hpp"
#include "../../include/vsim_hip.h"

namespace vsim {

// ------------------------------------------------------------------ 1. LN + quantize
// One 1024-thread workgroup per LayerNorm (two for GPT-NeoX's parallel-residual pair); the
// normalized row is quantized by whole waves, two 32-blocks per wave step.
constexpr int LNQ_THREADS = 512;

// LNQ_SPLIT workgroups per LayerNorm: each computes the whole row's statistics (the row is
// 16 KB, read from L2) and normalizes, writes and quantizes one slice of LNQ_SPLIT, so the
// latency-bound per-element phases run on LNQ_SPLIT CUs.
constexpr int LNQ_SPLIT = 8;
__global__ void __launch_bounds__(LNQ_THREADS) k_ln_quant(LnQuantJob j0, LnQuantJob j1, int n, unsigned *stats) {
  extern __shared__ __attribute__((aligned(16))) float row[];
  const int part = blockIdx.x % LNQ_SPLIT;
  const LnQuantJob &J = blockIdx.x < LNQ_SPLIT ? j0 : j1;
  if (blockIdx.x == 0 && threadIdx.x == 0 && J.ep) *J.ep += 1u;
  const int nb = n / QK;
  const int b0 = part * nb / LNQ_SPLIT, b1 = (part + 1) * nb / LNQ_SPLIT;  // this slice's blocks
  ln_quant_job<LNQ_THREADS>(J, row, n, part == 0 ? stats : nullptr, b0, b1);
}

int launch_ln_quant(const LnQuantJob &j0, const LnQuantJob *j1, int n, hipStream_t s) {
  const dim3 grid((j1 ? 2 : 1) * LNQ_SPLIT);
  hipLaunchKernelGGL(k_ln_quant, grid, dim3(LNQ_THREADS), (size_t)n * 4, s, j0, j1 ? *j1 : j0, n, dev_stats());
  VSIM_HIP(hipGetLastError());
  return VSIM_OK;
}

__global__ void k_residual_join(const float *x, const float *a, const float *ab, const float *f, const float *fb,
                                float *out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float ff = f[i] + fb[i];
  if (!a) {  // serial residual: x + (ff + b)
    out[i] = x[i] + ff;
    return;
  }
  const float attn = ab ? a[i] + ab[i] : a[i];
  out[i] = x[i] + (attn + ff);
}

int launch_residual_join(const float *x, const float *a, const float *ab, const float *f, const float *fb, float *out,
                         int n, hipStream_t s) {
  hipLaunchKernelGGL(k_residual_join, dim3((n + 255) / 256), dim3(256), 0, s, x, a, ab, f, fb, out, n);
  VSIM_HIP(hipGetLastError());
  return VSIM_OK;
}

// ------------------------------------------------------------------ GEMV epilogues
// Called by all 64 lanes of wave 0 with the row sums in lanes 0..31.
__device__ __forceinline__ void gemv_epilogue(const GemvJob &J, int t, float s, int lane) {
  const int row = t * T32 + lane;
  if (J.epi == EPI_GELU_Q) {
    float g = 0.0f;
    if (lane < T32) {
      const float v = s + J.bias[row];
      g = h2f(J.gelu_tab[f2h(v)]);
      if (J.y) J.y[row] = g;
    }
    quantize_block_lanes(g, lane, J.oq_qs + (size_t)t * 16, J.oq_d + t, J.oxd + (size_t)t * QK);
  } else if (lane < T32 && row < J.w.rows) {
    J.y[row] = J.bias ? s + J.bias[row] : s;
  }
}

// ------------------------------------------------------------------ fast GEMV + epilogues
constexpr int FW = 8;  // waves per workgroup of the fast kernels
__global__ void __launch_bounds__(64 * FW) k_gemv_fast_epi(GemvBatch B) {
  __shared__ float part[FW * 2][T32];
  int t = blockIdx.x, ji = 0;
  while (ji + 1 < B.nj && t >= B.j[ji].w.tiles) { t -= B.j[ji].w.tiles; ++ji; }
  const GemvJob &J = B.j[ji];
  const int nb = J.w.nb();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r = lane & (T32 - 1), h = lane >> 5;
  const uint8_t *qs = J.w.qs + (size_t)t * nb * T32 * 16;
  const float *dd = J.w.d + (size_t)t * nb * T32;
  float acc = 0.0f;
  for (int b = 2 * wave + h; b < nb; b += 2 * FW) {
    const size_t o = (size_t)b * T32 + r;
    const uint4 q = *(const uint4 *)(qs + o * 16);
    const float d0 = dd[o];
    const uint4 xv = *(const uint4 *)(J.xqs + (size_t)b * 16);
    int sd = __builtin_amdgcn_sdot8((int)(q.x ^ 0x88888888u), (int)(xv.x ^ 0x88888888u), 0, false);
    sd = __builtin_amdgcn_sdot8((int)(q.y ^ 0x88888888u), (int)(xv.y ^ 0x88888888u), sd, false);
    sd = __builtin_amdgcn_sdot8((int)(q.z ^ 0x88888888u), (int)(xv.z ^ 0x88888888u), sd, false);
    sd = __builtin_amdgcn_sdot8((int)(q.w ^ 0x88888888u), (int)(xv.w ^ 0x88888888u), sd, false);
    acc = __builtin_fmaf(d0 * J.xdd[b], (float)sd, acc);
  }
  part[2 * wave + h][r] = acc;
  __syncthreads();
  if (wave == 0) {
    float sum = 0.0f;
    if (lane < T32) {
#pragma unroll
      for (int i = 0; i < 2 * FW; ++i) sum += part[i][lane];
    }
    gemv_epilogue(J, t, sum, lane);
  }
}

int launch_gemv_epi(const GemvBatch &B, int mode, hipStream_t s) {
  int tiles = 0;
  for (int i = 0; i < B.nj; ++i) tiles += B.j[i].w.tiles;
  if (mode == VSIM_MODE_EXACT) return launch_gemv_chain_batch(B, s);  // gemv_chain.hip
  hipLaunchKernelGGL(k_gemv_fast_epi, dim3(tiles), dim3(64 * FW), 0, s, B);
  VSIM_HIP(hipGetLastError());
  return VSIM_OK;
}

// ------------------------------------------------------------------ 3. attention (N = 1)
// attn.hpp; one 1024-thread workgroup per head
constexpr int ATT_THREADS = 1024;
__global__ void __launch_bounds__(ATT_THREADS) k_attn_decode(AttnJob A) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  attn_body<ATT_THREADS>(A, blockIdx.x, sm);
}

int launch_attn_decode(const AttnJob &A, int n_ctx, hipStream_t s) {
  const int S = A.nsplit > 1 ? A.nsplit : 1;
  if (A.d % 32 != 0 || A.d > 256 || A.n_ctx != n_ctx || A.d % S != 0 || (A.d / S) % QK != 0) {
    set_error("attention: head dim must be a multiple of 32, at most 256");
    return VSIM_EINVAL;
  }
  const size_t smem = (size_t)attn_lds_floats(A.d, n_ctx) * sizeof(float);
  hipLaunchKernelGGL(k_attn_decode, dim3(A.H * S), dim3(ATT_THREADS), smem, s, A);
  VSIM_HIP(hipGetLastError());
  return VSIM_OK;
}

// ------------------------------------------------------------------ 3b. attention, B rows
// The batched decode step: workgroup (hs, b) is the same head of row b -- its own cache, its own
// position, its own slices of Q / K / V and of the Q4 output rows -- so a row's bits are those of
// k_attn_decode on that row alone, whatever shares the launch.
template <bool KW>
__device__ __forceinline__ void attn_batch_row(AttnJob &A, const AttnRows &R, float *sm) {
  const int b = blockIdx.y, E = A.d * A.H;
  const size_t ro = (size_t)b * E, bo = (size_t)b * (E / QK);
  A.q += ro;
  A.k += ro;
  A.v += ro;
  A.kc = R.kc[b] + R.loff;
  A.vc = R.vc[b] + R.loff;
  A.npast = R.npast + b;
  A.oq_qs += bo * 16;
  A.oq_d += bo;
  A.oxd += ro;
  if (A.out) A.out += ro;
  attn_body<ATT_THREADS, false, KW>(A, blockIdx.x, sm);
}

__global__ void __launch_bounds__(ATT_THREADS) k_attn_decode_batch(AttnJob A, AttnRows R) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  attn_batch_row<true>(A, R, sm);
}

// ------------------------------------------------------------------ 3c. attention, runs of rows
// A run: consecutive tokens of one sequence as consecutive rows of the batch, row j at position
// p + j of the same cache.  One launch cannot take them -- a head writes its row's K / V rows and
// reads the cache in one workgroup, and nothing orders the workgroups of two rows -- so two do:
// k_kv_rows writes every row's new K (after RoPE) and V rows, the kernel boundary orders them, and
// k_attn_decode_runs (attn_body with KW = false) reads keys 0..p + j per row and writes nothing to the
// caches.  Row j never sees the rows after it (they lie past its position), so its bits are those of
// k_attn_decode_batch on that row alone after the j rows before it.
//
// k_kv_rows: workgroup (h, b) rotates head h of row b's key at the row's position (rope_head, the
// heads' own lines) and stores the K and V rows; d <= 256.
constexpr int KVR_THREADS = 128;
__global__ void __launch_bounds__(KVR_THREADS) k_kv_rows(AttnJob A, AttnRows R) {
  __shared__ float kh[256];
  const int h = blockIdx.x, b = blockIdx.y, d = A.d, E = A.d * A.H, tid = threadIdx.x;
  const float *k = A.k + (size_t)b * E + h * d, *v = A.v + (size_t)b * E + h * d;
  const int p = R.npast[b];
  float *kc = R.kc[b] + R.loff + (size_t)p * E + h * d, *vc = R.vc[b] + R.loff + (size_t)p * E + h * d;
  for (int i = tid; i < d; i += KVR_THREADS) {
    kh[i] = k[i];
    vc[i] = v[i];
  }
  __syncthreads();
  rope_head<false, true>(nullptr, kh, A.cs, A.n_rot, A.style, p, tid, KVR_THREADS);
  __syncthreads();
  for (int i = tid; i < d; i += KVR_THREADS) kc[i] = kh[i];
}

__global__ void __launch_bounds__(ATT_THREADS) k_attn_decode_runs(AttnJob A, AttnRows R) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  attn_batch_row<false>(A, R, sm);
}

int launch_kv_rows(const AttnJob &A, const AttnRows &R, int B, hipStream_t s) {
  if (A.d < 1 || A.d > 256 || A.H < 1 || B < 1 || B > VSIM_BATCH_MAX || !R.kc || !R.vc || !R.npast || !A.k || !A.v ||
      A.n_rot < 0 || A.n_rot > A.d || A.n_rot % 2 || (A.n_rot > 0 && !A.cs)) {
    set_error("kv_rows: 1..32 rows with their caches and positions, k and v, head dim at most 256, n_rot even");
    return VSIM_EINVAL;
  }
  hipLaunchKernelGGL(k_kv_rows, dim3(A.H, B), dim3(KVR_THREADS), 0, s, A, R);
  VSIM_HIP(hipGetLastError());
  return VSIM_OK;
}

int launch_attn_decode_batch(const AttnJob &A, const AttnRows &R, int B, int n_ctx, hipStream_t s, bool runs) {
  const int S = A.nsplit > 1 ? A.nsplit : 1;
  if (A.d % 32 != 0 || A.d > 256 || A.n_ctx != n_ctx || A.d % S != 0 || (A.d / S) % QK != 0) {
    set_error("attention: head dim must be a multiple of 32, at most 256");
    return VSIM_EINVAL;
  }
  if (B < 1 || B > VSIM_BATCH_MAX || !R.kc || !R.vc || !R.npast) {
    set_error("attn_decode_batch: 1..32 rows with their caches and positions");
    return VSIM_EINVAL;
  }
  const size_t smem = (size_t)attn_lds_floats(A.d, n_ctx) * sizeof(float);
  if (runs) {
    if (int rc = launch_kv_rows(A, R, B, s)) return rc;
    hipLaunchKernelGGL(k_attn_decode_runs, dim3(A.H * S, B), dim3(ATT_THREADS), smem, s, A, R);
  } else {
    hipLaunchKernelGGL(k_attn_decode_batch, dim3(A.H * S, B), dim3(ATT_THREADS), smem, s, A, R);
  }
  VSIM_HIP(hipGetLastError());
  return VSIM_OK;
}

int launch_attn_decode_runs(const AttnJob &A, const AttnRows &R, int B, int n_ctx, hipStream_t s) {
  return launch_attn_decode_batch(A, R, B, n_ctx, s, true);
}

}  // namespace vsim
