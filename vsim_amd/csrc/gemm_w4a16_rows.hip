// vsim_amd/csrc/gemm_w4a16_rows.hip — weight-only mode (VSIM_MODE_W4A16): a Q4_0 weight times 1..32
// activation rows that are rounded to fp16, not quantized, with fp32 accumulation.
//
// Row operand (k_w4a16_rows and its float4 form k_w4a16_rows_v4, one workgroup per row).  For a row x[K]:
//   amax = the largest |x[i]| among the row's finite elements;
//   e    = 14 - floor(log2(amax)), so amax * 2^e lies in [2^14, 2^15); 0 for amax == 0;
//   h[i] = fp16_rn(x[i] * 2^e)   (the scaling exact, one rounding; small elements become fp16
//          subnormals or signed zeros).
// A row that holds a NaN or an Inf gets e = VSIM_W4A16_NONFINITE and h = +0 throughout.
// The row's h and e depend on that row alone.
//
// Product (k_gemm_w4a16_rows).  Every (weight row, activation row) pair, whatever n is and whatever
// rows stand beside it:
//   dot_b   = v_mfma_f32_16x16x32_f16's sum, from C = 0, of block b's 32 products (q - 8) * h (each
//             exact in fp32: 4 bits by 11 bits);
//   part[p] = 0.0f; for b = p, p + 16, ... < nb: part[p] = fmaf(d_w[b], dot_b, part[p]), p = 0 .. 15;
//   sum     = 0.0f; for p = 0 .. 15: sum += part[p];
//   s       = sum * 2^-e (exact unless the result is an f32 subnormal);
//   y       = bias ? s + bias[row] : s;     e == VSIM_W4A16_NONFINITE: y = NaN (0x7FC00000).
//
// Work split: gemm_fast_rows.hip's.  A 1024-thread workgroup takes 16 weight rows (half a W4T32
// tile) and all n activation rows; wave p owns partial p and walks the blocks b = p, p + 16, ...;
// one MFMA per block (a second one for rows 16..31), nothing chained through the accumulator; the
// sixteen partials meet in LDS and threads 0..511 add them in order.  A = the 16 weight rows, B = 16
// activation rows: lane l = (c, g) = (l & 15, l >> 4) holds elements 8 g .. 8 g + 7 of the block,
// of weight row c (4 bytes of its nibble run, low nibble first) and of activation row c (16
// contiguous bytes of h).  D[4 g + i][c] (register i) is the pair (weight row 4 g + i, activation
// row c); its weight scales are one float4 per lane.
//
// Loads: in bounds without slack, as there: the last tile's padding rows exist (d = 0), the second
// block of a trip is clamped to the last block, activation rows >= n are clamped to row n - 1.
#include "w4a16.hpp"

namespace vsim {

constexpr int WA_OP_NT = 256;  // the operand kernel's threads

// ------------------------------------------------------------------ the row operand
__global__ void __launch_bounds__(WA_OP_NT)
    k_w4a16_rows(const float *__restrict__ x, int K, _Float16 *__restrict__ x16, int32_t *__restrict__ e_out) {
  __shared__ uint32_t red[WA_OP_NT / 64];
  const int tid = threadIdx.x;
  const float *xr = x + (size_t)blockIdx.x * K;
  _Float16 *hr = x16 + (size_t)blockIdx.x * K;
  // |x| as bits: ordered like the values for everything finite, subnormals included; a non-finite
  // element raises the maximum to 0x7F800000 or above
  uint32_t am = 0u;
  for (int i = tid; i < K; i += WA_OP_NT) am = max(am, __float_as_uint(xr[i]) & 0x7FFFFFFFu);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) am = max(am, (uint32_t)__shfl_xor((int)am, o, 64));
  if ((tid & 63) == 0) red[tid >> 6] = am;
  __syncthreads();
  am = red[0];
#pragma unroll
  for (int w = 1; w < WA_OP_NT / 64; ++w) am = max(am, red[w]);
  const bool bad = am >= 0x7F800000u;
  int e = 0;
  if (am != 0u && !bad) {
    // floor(log2(amax)): the exponent field, or the top bit's place for a subnormal
    const int lg = (am >> 23) ? (int)(am >> 23) - 127 : (31 - __clz((int)am)) - 149;
    e = 14 - lg;
  }
  if (tid == 0) e_out[blockIdx.x] = bad ? VSIM_W4A16_NONFINITE : e;
  for (int i = tid; i < K; i += WA_OP_NT) hr[i] = bad ? (_Float16)0.0f : (_Float16)ldexpf(xr[i], e);
}

// The same operand for rows of up to WA_OPV_MAXK elements at 16-byte aligned addresses: 1,024 threads,
// the row read once as float4 (up to WA_OPV_PER per thread, kept in registers between the maximum
// and the conversion), four halves stored at a time.  The maximum does not depend on the order it is
// taken in and the conversion is per element: the bits are k_w4a16_rows'.
constexpr int WA_OPV_NT = 1024, WA_OPV_PER = 4, WA_OPV_MAXK = 4 * WA_OPV_NT * WA_OPV_PER;

__global__ void __launch_bounds__(WA_OPV_NT)
    k_w4a16_rows_v4(const float *__restrict__ x, int K, _Float16 *__restrict__ x16, int32_t *__restrict__ e_out) {
  __shared__ uint32_t red[WA_OPV_NT / 64];
  const int tid = threadIdx.x, nv = K / 4;
  const f32x4 *xr = (const f32x4 *)(x + (size_t)blockIdx.x * K);
  wa_half4 *hr = (wa_half4 *)(x16 + (size_t)blockIdx.x * K);
  f32x4 v[WA_OPV_PER];
  uint32_t am = 0u;
#pragma unroll
  for (int k = 0; k < WA_OPV_PER; ++k) {
    const int f = tid + WA_OPV_NT * k;
    v[k] = f < nv ? xr[f] : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int i = 0; i < 4; ++i) am = max(am, __float_as_uint(v[k][i]) & 0x7FFFFFFFu);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) am = max(am, (uint32_t)__shfl_xor((int)am, o, 64));
  if ((tid & 63) == 0) red[tid >> 6] = am;
  __syncthreads();
  am = red[0];
#pragma unroll
  for (int w = 1; w < WA_OPV_NT / 64; ++w) am = max(am, red[w]);
  const bool bad = am >= 0x7F800000u;
  int e = 0;
  if (am != 0u && !bad) {
    const int lg = (am >> 23) ? (int)(am >> 23) - 127 : (31 - __clz((int)am)) - 149;
    e = 14 - lg;
  }
  if (tid == 0) e_out[blockIdx.x] = bad ? VSIM_W4A16_NONFINITE : e;
#pragma unroll
  for (int k = 0; k < WA_OPV_PER; ++k) {
    const int f = tid + WA_OPV_NT * k;
    if (f >= nv) break;
    wa_half4 h;
#pragma unroll
    for (int i = 0; i < 4; ++i) h[i] = bad ? (_Float16)0.0f : (_Float16)ldexpf(v[k][i], e);
    hr[f] = h;
  }
}

// ------------------------------------------------------------------ the product
template <int NJ>
struct WaBlock {
  uint32_t wq;      // the lane's 4 bytes of its weight row's nibble run
  f32x4 wd;         // scales of weight rows 4 g .. 4 g + 3
  wa_half8 xh[NJ];  // the lane's 8 halves of its activation rows
};

template <int NJ>
__global__ void __launch_bounds__(WA_THREADS)
    k_gemm_w4a16_rows(W4 W, const _Float16 *__restrict__ x16, const int32_t *__restrict__ ex, int n,
                      const float *__restrict__ bias, float *__restrict__ y) {
  __shared__ float part[WA_WAVES][VSIM_BATCH_MAX][WA_RT];  // 32 KB
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane & 15, g = lane >> 4;
  const int m0 = blockIdx.x * WA_RT, M = W.rows, nb = W.nb(), K = W.k;
  // block b of weight row m0 + r: nibbles at wq + b * 512 bytes, scale at wd + b * 32
  // (m0 + 15 < W.tiles * T32: the padding rows of the last tile exist)
  const size_t wo = W.off(m0, 0);
  const uint8_t *wq = W.qs + (wo + c) * 16 + 4 * g;
  const float *wd = W.d + wo + 4 * g;
  const _Float16 *xp[NJ];
#pragma unroll
  for (int u = 0; u < NJ; ++u) xp[u] = x16 + (size_t)min(c + 16 * u, n - 1) * K + 8 * g;
  f32x4 acc[NJ];
#pragma unroll
  for (int u = 0; u < NJ; ++u) acc[u] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

  auto fetch = [&](int b) {
    WaBlock<NJ> r;
    r.wq = *(const uint32_t *)(wq + (size_t)b * (T32 * 16));
    r.wd = *(const f32x4 *)(wd + (size_t)b * T32);
#pragma unroll
    for (int u = 0; u < NJ; ++u) r.xh[u] = *(const wa_half8 *)(xp[u] + (size_t)b * QK);
    return r;
  };
  auto step = [&](const WaBlock<NJ> &r) {
    const wa_half8 a = wa_unpack(r.wq);
#pragma unroll
    for (int u = 0; u < NJ; ++u) {
      const f32x4 dot = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, r.xh[u], f32x4{0.0f, 0.0f, 0.0f, 0.0f}, 0, 0, 0);
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[u][i] = __builtin_fmaf(r.wd[i], dot[i], acc[u][i]);
    }
  };
  // two blocks of the wave's strand per trip, both fetched before either is used; the second is
  // clamped to the last block when the strand has ended (wave-uniform)
  for (int b = wave; b < nb; b += 2 * WA_WAVES) {
    const bool two = b + WA_WAVES < nb;
    const WaBlock<NJ> r0 = fetch(b), r1 = fetch(two ? b + WA_WAVES : nb - 1);
    step(r0);
    if (two) step(r1);
  }
#pragma unroll
  for (int u = 0; u < NJ; ++u) *(f32x4 *)&part[wave][c + 16 * u][4 * g] = acc[u];
  __syncthreads();
  const int r = tid & (WA_RT - 1), j = tid >> 4;
  if (j < n && m0 + r < M) {
    float sum = 0.0f;
#pragma unroll
    for (int p = 0; p < WA_WAVES; ++p) sum += part[p][j][r];
    const int e = ex[j];
    const float s = ldexpf(sum, e == VSIM_W4A16_NONFINITE ? 0 : -e);
    const float v = bias ? s + bias[m0 + r] : s;
    y[(size_t)j * M + m0 + r] = e == VSIM_W4A16_NONFINITE ? __uint_as_float(0x7FC00000u) : v;
  }
}

// ------------------------------------------------------------------ launchers
int launch_w4a16_rows(const float *x, int K, int n, void *x16, int32_t *e, hipStream_t s) {
  if (!x || !x16 || !e || K <= 0 || K % QK || n < 1) {
    set_error("w4a16_rows: at least one row, K a multiple of 32, x, x16 and e required");
    return VSIM_EINVAL;
  }
  if (K <= WA_OPV_MAXK && (((uintptr_t)x | (uintptr_t)x16) & 15) == 0)
    hipLaunchKernelGGL(k_w4a16_rows_v4, dim3(n), dim3(WA_OPV_NT), 0, s, x, K, (_Float16 *)x16, e);
  else
    hipLaunchKernelGGL(k_w4a16_rows, dim3(n), dim3(WA_OP_NT), 0, s, x, K, (_Float16 *)x16, e);
  VSIM_HIP(hipGetLastError());
  return VSIM_OK;
}

// y[j][m] for j < n rows, n of any size: consecutive chunks of up to VSIM_BATCH_MAX rows, one launch
// each (a row's value does not depend on its chunk)
int launch_gemm_w4a16_rows(const W4 &W, const void *x16, const int32_t *e, int n, const float *bias, float *y,
                           hipStream_t s) {
  if (W.k % QK || W.k <= 0 || W.rows <= 0 || n < 1 || !W.qs || !x16 || !e || !y) {
    set_error("q4_gemm_w4a16_rows: K a multiple of 32, w, x16, e and y required");
    return VSIM_EINVAL;
  }
  const dim3 grid((W.rows + WA_RT - 1) / WA_RT);
  for (int r0 = 0; r0 < n; r0 += VSIM_BATCH_MAX) {
    const int c = min(VSIM_BATCH_MAX, n - r0);
    const _Float16 *xc = (const _Float16 *)x16 + (size_t)r0 * W.k;
    float *yc = y + (size_t)r0 * W.rows;
    if (c <= 16)
      hipLaunchKernelGGL((k_gemm_w4a16_rows<1>), grid, dim3(WA_THREADS), 0, s, W, xc, e + r0, c, bias, yc);
    else
      hipLaunchKernelGGL((k_gemm_w4a16_rows<2>), grid, dim3(WA_THREADS), 0, s, W, xc, e + r0, c, bias, yc);
    VSIM_HIP(hipGetLastError());
  }
  return VSIM_OK;
}

}  // namespace vsim
