// vsim_amd/csrc/gemm_fast_rows.hip — fast-mode Q4_0 product for a handful of activation rows
// (1..32: the fast batched decode step, one row per sequence).
//
// Contract.  Every (weight row, activation row) pair is k_gemv_fast's value (ops_q4.hip), bit for
// bit, whatever n is and whatever rows stand beside it:
//   isum_b  = the exact integer dot of block b's 32 (nibble - 8) pairs;
//   part[p] = 0.0f; for b = p, p + 16, ... < nb: part[p] = fmaf(d_w[b] * d_x[b], (float)isum_b, part[p])
//             (the scale product rounded to fp32 on its own), p = 0 .. 15; no block: +0;
//   sum     = 0.0f; for p = 0 .. 15: sum += part[p];
//   y       = bias ? sum + bias[row] : sum.
// isum is an integer (|isum| <= 2048), so the machinery that forms it is free: here the i8 matrix
// core on nibbles unpacked to signed bytes, where the GEMV has v_dot8_i32_i4.  The fp32 steps are
// the GEMV's, in its order.
//
// Work split.  One 1024-thread workgroup takes GF_RT = 16 weight rows (half a W4T32 tile: a block's
// 16 rows are 256 contiguous bytes of nibbles and 64 of scales) and all n activation rows, so
// M = 4096 is 256 workgroups.  Wave p of the sixteen owns partial p: it walks the blocks b = p,
// p + 16, ... and keeps part[p] of its 16 x n outputs in the MFMA's accumulator layout.  The
// sixteen partials meet in LDS (16 x 32 x 16 floats, 32 KB) and threads 0..511 add them in order.
//
// One block, one wave: v_mfma_i32_16x16x32_i8 with A = the 16 weight rows, B = 16 activation rows
// (a second MFMA for rows 16..31 when n > 16).  Lane l = (c, g) = (l & 15, l >> 4) holds 8 of the
// block's 32 k of weight row c (A) and of activation row c (B).  Which k a fragment element is does
// not matter to an integer dot as long as A and B agree, and both are unpacked by the same function
// from the same bytes of their 16-byte nibble runs: bytes 8 (g >> 1) .. + 7, low nibbles for even g,
// high nibbles for odd g.  The result D[row 4 g + i][col c] (register i of lane l) is the pair
// (weight row 4 g + i, activation row c): its weight scales are one float4 per lane, its activation
// scale one float.
//
// Loads.  Every load is in bounds without slack behind the weight: a half tile's rows exist up to
// the tile's padding (d = 0, nibbles 8), blocks stop at nb (the loop runs two blocks per trip with
// the second clamped to the last block: loaded, never used), and activation rows >= n are clamped
// to row n - 1: computed, never stored.
#include "kern.hpp"
#include "../../include/vsim_hip.h"

namespace vsim {

constexpr int GF_RT = 16;      // weight rows per workgroup
constexpr int GF_WAVES = 16;   // one per partial
constexpr int GF_THREADS = 64 * GF_WAVES;

typedef int i32x4 __attribute__((ext_vector_type(4)));

// 8 nibbles (one per byte of the two words, the low ones or the high ones) as 8 signed bytes q - 8
__device__ __forceinline__ long gf_unpack(uint2 w, int hi) {
  const uint32_t a = (hi ? w.x >> 4 : w.x) & 0x0F0F0F0Fu, b = (hi ? w.y >> 4 : w.y) & 0x0F0F0F0Fu;
  // per byte q + 0x78 (<= 0x87: no carry), then the top bit flipped: q - 8 in two's complement
  const uint32_t lo = (a + 0x78787878u) ^ 0x80808080u, hh = (b + 0x78787878u) ^ 0x80808080u;
  return (long)(((unsigned long)hh << 32) | lo);
}

template <int NJ>
struct GfBlock {
  uint2 wq;       // the lane's 8 bytes of its weight row's nibble run
  f32x4 wd;       // scales of weight rows 4 g .. 4 g + 3
  uint2 xq[NJ];   // the lane's 8 bytes of its activation rows' nibble runs
  float xd[NJ];   // and those rows' scales
};

template <int NJ>
__global__ void __launch_bounds__(GF_THREADS)
    k_gemm_fast_rows(W4 W, const uint8_t *__restrict__ xqs, const float *__restrict__ xdd, int n,
                     const float *__restrict__ bias, float *__restrict__ y) {
  __shared__ float part[GF_WAVES][VSIM_BATCH_MAX][GF_RT];  // 32 KB
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane & 15, g = lane >> 4, hi = g & 1, half = g >> 1;
  const int m0 = blockIdx.x * GF_RT, M = W.rows, nb = W.nb();
  // block b of weight row m0 + r: nibbles at wq + b * 512 bytes, scale at wd + b * 32
  // (m0 + 15 < W.tiles * T32: the padding rows of the last tile exist)
  const size_t wo = W.off(m0, 0);
  const uint8_t *wq = W.qs + (wo + c) * 16 + 8 * half;
  const float *wd = W.d + wo + 4 * g;
  const uint8_t *xq[NJ];
  const float *xd[NJ];
#pragma unroll
  for (int u = 0; u < NJ; ++u) {
    const int j = min(c + 16 * u, n - 1);
    xq[u] = xqs + (size_t)j * nb * 16 + 8 * half;
    xd[u] = xdd + (size_t)j * nb;
  }
  f32x4 acc[NJ];
#pragma unroll
  for (int u = 0; u < NJ; ++u) acc[u] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

  auto fetch = [&](int b) {
    GfBlock<NJ> r;
    r.wq = *(const uint2 *)(wq + (size_t)b * (T32 * 16));
    r.wd = *(const f32x4 *)(wd + (size_t)b * T32);
#pragma unroll
    for (int u = 0; u < NJ; ++u) {
      r.xq[u] = *(const uint2 *)(xq[u] + (size_t)b * 16);
      r.xd[u] = xd[u][b];
    }
    return r;
  };
  auto step = [&](const GfBlock<NJ> &r) {
    const long a = gf_unpack(r.wq, hi);
#pragma unroll
    for (int u = 0; u < NJ; ++u) {
      const i32x4 is =
          __builtin_amdgcn_mfma_i32_16x16x32_i8(a, gf_unpack(r.xq[u], hi), i32x4{0, 0, 0, 0}, 0, 0, 0);
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[u][i] = __builtin_fmaf(r.wd[i] * r.xd[u], (float)is[i], acc[u][i]);
    }
  };
  // two blocks of the wave's strand per trip, both fetched before either is used; the second is
  // clamped to the last block when the strand has ended (wave-uniform).  Four per trip was measured:
  // faster below B = 16 (B = 8: +5 %), slower from there on (B = 32: -3.5 %), where the activation
  // rows' scattered 16-byte reads, not the weight stream's latency, set the pace
  for (int b = wave; b < nb; b += 2 * GF_WAVES) {
    const bool two = b + GF_WAVES < nb;
    const GfBlock<NJ> r0 = fetch(b), r1 = fetch(two ? b + GF_WAVES : nb - 1);
    step(r0);
    if (two) step(r1);
  }
#pragma unroll
  for (int u = 0; u < NJ; ++u) *(f32x4 *)&part[wave][c + 16 * u][4 * g] = acc[u];
  __syncthreads();
  const int r = tid & (GF_RT - 1), j = tid >> 4;
  if (j < n && m0 + r < M) {
    float sum = 0.0f;
#pragma unroll
    for (int p = 0; p < GF_WAVES; ++p) sum += part[p][j][r];
    y[(size_t)j * M + m0 + r] = bias ? sum + bias[m0 + r] : sum;
  }
}

// y[j][m] = k_gemv_fast's value of weight row m and activation row j (+ bias[m]) for j < n <= 32,
// on k_gemm_fast_rows or as one k_gemv_fast launch per row (vsim_batch_set_fast_gemm): the same bits
int launch_gemm_fast_rows(const W4 &W, const void *xq, int n, const float *bias, float *y, hipStream_t s) {
  if (W.k % QK || W.k <= 0 || W.rows <= 0 || n < 1 || n > VSIM_BATCH_MAX || !W.qs || !xq || !y) {
    set_error("q4_gemm_fast_rows: 1..32 activation rows, K a multiple of 32, w, xq and y required");
    return VSIM_EINVAL;
  }
  const ProductPlan pl = product_plan({.kind = BatchKind::ROWS_FAST, .mode = VSIM_MODE_FAST, .N = n, .M = W.rows,
                                       .K = W.k, .fast_gemm = batch_fast_gemm()});
  if (pl.kernel == ProductKernel::GEMV_FAST) return launch_gemv_rows(W, xq, nullptr, n, 1, bias, y, VSIM_MODE_FAST, s);
  const uint8_t *xqs = (const uint8_t *)xq;
  const float *xdd = (const float *)(xqs + (size_t)n * W.nb() * 16);
  const dim3 grid((W.rows + GF_RT - 1) / GF_RT);
  if (n <= 16)
    hipLaunchKernelGGL((k_gemm_fast_rows<1>), grid, dim3(GF_THREADS), 0, s, W, xqs, xdd, n, bias, y);
  else
    hipLaunchKernelGGL((k_gemm_fast_rows<2>), grid, dim3(GF_THREADS), 0, s, W, xqs, xdd, n, bias, y);
  VSIM_HIP(hipGetLastError());
  return VSIM_OK;
}

}  // namespace vsim
