// vsim_amd/csrc/gemm_w4a16_tile.hip — weight-only mode (VSIM_MODE_W4A16): a Q4_0 weight times any number
// of activation rows of k_w4a16_rows' operand, tiled over both, with the bits of k_gemm_w4a16_rows.
//
// The arithmetic per output is gemm_w4a16_rows.hip's, restated.  Every (weight row, activation row)
// pair, whatever n is, whatever tile it falls in and whatever rows stand beside it:
//   dot_b   = v_mfma_f32_16x16x32_f16's sum, from C = 0, of block b's 32 products (q - 8) * h;
//   part[p] = 0.0f; for b = p, p + 16, ... < nb: part[p] = fmaf(d_w[b], dot_b, part[p]), p = 0 .. 15;
//   sum     = 0.0f; for p = 0 .. 15: sum += part[p];
//   s       = ldexpf(sum, -e);
//   y       = bias ? s + bias[row] : s;     e == VSIM_W4A16_NONFINITE: y = NaN (0x7FC00000).
// The MFMA is the same instruction with the same operand roles and the same K placement: A = 16
// weight rows, B = 16 activation rows, lane l = (c, g) = (l & 15, l >> 4) holds elements
// 8 g .. 8 g + 7 of the block, the weight's by wa_unpack.  Nothing chains through the accumulator.
//
// Work split.  A 1024-thread workgroup takes TM = 16 NT weight rows (NT = 4, or 2 for a small
// grid) and WT_TN = 64 activation rows.  The K split is the rows kernel's: wave p owns partial p of
// the whole tile and walks the blocks b = p, p + 16, ...  Per block a wave loads NT weight
// fragments and their scales and four activation fragments, straight from global memory to
// registers (no two waves need the same bytes), and runs 4 NT MFMAs on them: every unpacked weight
// fragment meets four activation tiles, every activation fragment NT weight tiles.  The sixteen
// partials of the tile do not fit LDS at once; they meet there in four ordered rounds, one per
// 16 activation rows, and in each round one thread per output adds its sixteen in order.
//
// Loads: in bounds without slack.  The last W4T32 tile's padding rows exist (d = 0); a 16-row
// group past the last tile is clamped to the last tile's; activation rows >= n are clamped to row
// n - 1; neither is stored.
#include "w4a16.hpp"

namespace vsim {

constexpr int WT_TN = 64;          // activation rows per workgroup (product_plan's W4A16_TILE_ROWS)
constexpr int WT_NU = WT_TN / 16;  // ... as MFMA tiles
constexpr int WT_CUS = 256;        // NT = 4 from one workgroup per CU on

template <int NT>
struct WtBlock {
  uint32_t wq[NT];      // the lane's 4 bytes of its weight rows' nibble runs
  f32x4 wd[NT];         // scales of weight rows 4 g .. 4 g + 3 of each group
  wa_half8 xh[WT_NU];   // the lane's 8 halves of its activation rows
};

template <int NT>
__global__ void __launch_bounds__(WA_THREADS)
    k_gemm_w4a16_tile(W4 W, const _Float16 *__restrict__ x16, const int32_t *__restrict__ ex, int n,
                      const float *__restrict__ bias, float *__restrict__ y) {
  constexpr int TM = 16 * NT;
  // one round's partials: [wave][activation row][weight row], the weight rows' groups of four
  // XOR-swizzled by the activation row so that a wave's 16-byte stores spread over the banks
  __shared__ float part[WA_WAVES][16][TM];  // NT = 4: 64 KB
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // (a scalar: the block addresses below are)
  const int c = lane & 15, g = lane >> 4;
  const int m0 = blockIdx.x * TM, n0 = blockIdx.y * WT_TN;
  const int M = W.rows, nb = W.nb(), K = W.k;
  const int nu = min(WT_NU, (n - n0 + 15) >> 4);  // activation tiles that hold a row (workgroup-uniform)
  // Addresses are a scalar base per group and block plus one 32-bit lane offset, to spare registers.
  // Block b of group t: nibbles at wq[t] + b * 512 bytes, scales at wd[t] + b * 32 floats
  const uint8_t *wq[NT];
  const float *wd[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const size_t wo = W.off(min(m0 + 16 * t, W.tiles * T32 - 16), 0);
    wq[t] = W.qs + wo * 16;
    wd[t] = W.d + wo;
  }
  const uint32_t lq = 16 * c + 4 * g, ld = 16 * g;  // the lane's bytes into a group's nibbles and scales
  // block b of activation row n0 + j: xb + j * K + b * 32 halves (j * K < 64 K fits 32 bits: K < 2^24)
  const _Float16 *xb = x16 + (size_t)n0 * K;
  uint32_t lx[WT_NU];
#pragma unroll
  for (int u = 0; u < WT_NU; ++u) lx[u] = 2u * ((uint32_t)min(16 * u + c, n - 1 - n0) * (uint32_t)K + 8u * g);
  f32x4 acc[NT][WT_NU];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int u = 0; u < WT_NU; ++u) acc[t][u] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

  auto fetch = [&](int b) {
    WtBlock<NT> r;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      r.wq[t] = *(const uint32_t *)(wq[t] + (size_t)b * (T32 * 16) + lq);
      r.wd[t] = *(const f32x4 *)((const uint8_t *)(wd[t] + (size_t)b * T32) + ld);
    }
#pragma unroll
    for (int u = 0; u < WT_NU; ++u) r.xh[u] = *(const wa_half8 *)((const uint8_t *)(xb + (size_t)b * QK) + lx[u]);
    return r;
  };
  for (int b = wave; b < nb; b += WA_WAVES) {
    const WtBlock<NT> r = fetch(b);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const wa_half8 a = wa_unpack(r.wq[t]);
#pragma unroll
      for (int u = 0; u < WT_NU; ++u) {
        if (u < nu) {
          const f32x4 dot =
              __builtin_amdgcn_mfma_f32_16x16x32_f16(a, r.xh[u], f32x4{0.0f, 0.0f, 0.0f, 0.0f}, 0, 0, 0);
#pragma unroll
          for (int i = 0; i < 4; ++i) acc[t][u][i] = __builtin_fmaf(r.wd[t][i], dot[i], acc[t][u][i]);
        }
      }
    }
  }

  // D[4 g + i][c] (register i) of (t, u) is the pair (weight row m0 + 16 t + 4 g + i, activation
  // row n0 + 16 u + c)
  const int r = tid & (TM - 1), j = tid / TM;  // the thread's output of a round (j < 16)
  const int m = m0 + r;
  const float bv = bias && m < M ? bias[m] : 0.0f;
#pragma unroll
  for (int u = 0; u < WT_NU; ++u) {
    if (u < nu) {
      if (u) __syncthreads();
#pragma unroll
      for (int t = 0; t < NT; ++t) *(f32x4 *)&part[wave][c][(16 * t + 4 * g) ^ ((c & (4 * NT - 1)) << 2)] = acc[t][u];
      __syncthreads();
      const int row = n0 + 16 * u + j;
      if (j < 16 && row < n && m < M) {
        float sum = 0.0f;
#pragma unroll
        for (int p = 0; p < WA_WAVES; ++p) sum += part[p][j][r ^ ((j & (4 * NT - 1)) << 2)];
        const int e = ex[row];
        const float s = ldexpf(sum, e == VSIM_W4A16_NONFINITE ? 0 : -e);
        const float v = bias ? s + bv : s;
        y[(size_t)row * M + m] = e == VSIM_W4A16_NONFINITE ? __uint_as_float(0x7FC00000u) : v;
      }
    }
  }
}

// y[j][m] for j < n rows, n of any size, in one launch
int launch_gemm_w4a16_tile(const W4 &W, const void *x16, const int32_t *e, int n, const float *bias, float *y,
                           hipStream_t s) {
  if (W.k % QK || W.k <= 0 || W.rows <= 0 || n < 1 || !W.qs || !x16 || !e || !y) {
    set_error("q4_gemm_w4a16_tile: K a multiple of 32, w, x16, e and y required");
    return VSIM_EINVAL;
  }
  const unsigned gy = (n + WT_TN - 1) / WT_TN;
  if (gy > 65535u) {
    set_error("q4_gemm_w4a16_tile: more than 65535 * 64 activation rows");
    return VSIM_EINVAL;
  }
  const _Float16 *xh = (const _Float16 *)x16;
  // 64 weight rows per workgroup once that fills the CUs; 32 below, for twice the workgroups
  if ((size_t)((W.rows + 63) / 64) * gy >= WT_CUS)
    hipLaunchKernelGGL((k_gemm_w4a16_tile<4>), dim3((W.rows + 63) / 64, gy), dim3(WA_THREADS), 0, s, W, xh, e, n, bias, y);
  else
    hipLaunchKernelGGL((k_gemm_w4a16_tile<2>), dim3((W.rows + 31) / 32, gy), dim3(WA_THREADS), 0, s, W, xh, e, n, bias, y);
  VSIM_HIP(hipGetLastError());
  return VSIM_OK;
}

}  // namespace vsim
