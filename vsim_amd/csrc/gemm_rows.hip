// vsim_amd/csrc/gemm_rows.hip — exact-mode Q4_0 product for a handful of activation rows
// (1..32: the batched decode step, one row per sequence).
//
// Every (weight row, activation row) pair is the reference's chain as gemm_exact.hip:1-12 spells
// it out -- sumf = sumf + (f0*f2 + f1*f3) per byte pair in block order, each product and sum
// rounded on its own, the bias added after -- so a row's result does not depend on n or on the
// rows beside it.  What the batch buys is chains: n of them per weight row over one pass of the
// weight stream, where the single-token GEMV has one.
//
// Work split.  One 256-thread workgroup takes GR_RT = 16 weight rows (half a W4T32 tile: each
// block's 16 rows are 256 contiguous bytes of nibbles and 64 of scales) and all n activation rows,
// so M = 4096 is 256 workgroups.  A weight block is fetched and dequantized once per workgroup,
// d*(float)(q-8) with one rounding, into LDS for every chain of the tile.
//
// Lane layout.  Lane l of wave w: weight row l & 15, activation slot s = 4 w + (l >> 4), chains
// for the activation rows s and s + 16 (NJ = 2 only when n > 16).  The 16 lanes of a DPP row thus
// share an activation row and differ in the weight row:
//   * weights: one ds_read_b128 gives a lane (f0, f1) of two byte pairs of its row; LDS is laid
//     out [block][pair group][row] in 16-byte units, so the 16 rows of a read are consecutive
//     (conflict-free) and the four DPP rows of a wave read the same addresses (broadcast);
//   * activation factors: a DPP row keeps the 32 factors of its activation row's block in two
//     VGPRs (memory slots l16 and 16 + l16 of the pair-interleaved xd, kern.hpp) and hands them
//     round with row_newbcast folded into the multiply (xbcast, kern.hpp): no LDS, no registers
//     per factor.
// Per byte pair and chain that is two multiplies, their sum and the chain add: the 2 lane-ops per
// weight-row of gemm_exact.hip's accounting, plus one 16-byte LDS read per two pairs shared by the
// lane's NJ chains.  Waves whose slots are all >= n only help staging.
//
// Pipeline.  Chunks of GR_KB = 4 blocks; thread t stages one 4-byte word (4 byte pairs) of block
// t >> 6 of the chunk.  Raw words, scales and activation factors of GR_D = 4 chunks are in flight
// in a register ring (macros, not lambdas, so the ring stays in registers): M = 4096 gives one wave
// per SIMD, so nothing but the wave's own loads in flight hides a trip to memory.  Chunk c + 1 is
// staged into the other LDS buffer after chunk c's arithmetic: one barrier per chunk, no
// cross-workgroup communication.
//
// Measured (batched decode; profiles/batch_decode_bench.txt): a block of 16 pairs costs
// one wave ~620 cycles whatever n is, about 2.4 times the issue time of its 64 VALU ops, so the
// kernel wins over the GEMV jobs only once most lanes carry a chain (n >= 12).  Forming a block's
// terms one block ahead of the chain adds (so that no op waits for the one before it) was built and
// measured slower (B = 16: 1231 against 1493 tok/s): the dependent order is not what costs.
#include "kern.hpp"
#include "../../include/vsim_hip.h"

namespace vsim {

constexpr int GR_RT = 16;       // weight rows per workgroup
constexpr int GR_KB = 4;        // blocks per staged chunk
constexpr int GR_D = 4;         // chunks in flight from memory (register ring; even)
constexpr int GR_THREADS = 256;

// pairs 2G and 2G+1 of a block: natural elements 4G .. 4G+3 at memory slots xd_slot()
template <int G>
__device__ __forceinline__ float gr_group(float acc, f32x4 w, float F0, float F1) {
  acc = acc + (w.x * xbcast<xd_slot(4 * G + 0)>(F0, F1) + w.y * xbcast<xd_slot(4 * G + 1)>(F0, F1));
  acc = acc + (w.z * xbcast<xd_slot(4 * G + 2)>(F0, F1) + w.w * xbcast<xd_slot(4 * G + 3)>(F0, F1));
  return acc;
}

template <int NJ>
__global__ void __launch_bounds__(GR_THREADS)
    k_gemm_exact_rows(W4 W, const float *__restrict__ xd, int n, const float *__restrict__ bias, float *__restrict__ y) {
  __shared__ f32x4 Lw[2][GR_KB][8][GR_RT];  // 16 KB
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l16 = lane & 15, slot = 4 * wave + (lane >> 4);
  const int m0 = blockIdx.x * GR_RT, M = W.rows, K = W.k, nb = W.nb();
  const int nchunk = (nb + GR_KB - 1) / GR_KB;

  // ---- loader: block lb of the chunk, row lr of the tile, word lw of the block (pairs 4 lw .. + 3)
  // (m0 + lr < W.tiles * T32: the padding rows of the last tile exist, d = 0)
  const int lb = tid >> 6, lr = tid & 15, lw = (tid >> 4) & 3;
  const size_t wo = W.off(m0 + lr, 0);  // block b of the row: wo + b * T32
  const uint32_t *wq = (const uint32_t *)(W.qs + wo * 16) + lw;
  const float *wd = W.d + wo;
  // ring slot c % GR_D holds chunk c: the raw word and scale until the chunk is staged, the
  // activation factors until it is computed
  uint32_t rq[GR_D];
  float rd[GR_D];
  float x0[GR_D][NJ][GR_KB], x1[GR_D][NJ][GR_KB];
  const bool active = 4 * wave < n;  // wave-uniform
  const float *xr[NJ];
#pragma unroll
  for (int u = 0; u < NJ; ++u) xr[u] = xd + (size_t)min(slot + 16 * u, n - 1) * K + l16;
// Every load and LDS store of the loop is unconditional (blocks past the end are clamped to the
// last one: loaded and staged, never used), and so is every barrier: with no branch round a memory
// operation the compiler counts the loads in flight and waits for the oldest only (vmcnt(n));
// with the loads under `if (block < nb)` it waited for all of them before each barrier, and the
// ring bought nothing.
#define GR_FETCH_W(S, C)                                   \
  {                                                        \
    const int b_ = min((C) * GR_KB + lb, nb - 1);          \
    rq[S] = wq[(size_t)b_ * (T32 * 4)];                    \
    rd[S] = wd[(size_t)b_ * T32];                          \
  }
#define GR_FETCH_X(S, C)                                                     \
  {                                                                          \
    _Pragma("unroll") for (int i_ = 0; i_ < GR_KB; ++i_) {                   \
      const int b_ = min((C) * GR_KB + i_, nb - 1);                          \
      _Pragma("unroll") for (int u_ = 0; u_ < NJ; ++u_) {                    \
        x0[S][u_][i_] = xr[u_][(size_t)b_ * QK];                             \
        x1[S][u_][i_] = xr[u_][(size_t)b_ * QK + 16];                        \
      }                                                                      \
    }                                                                        \
  }
#define GR_STAGE_W(S, BUF)                                                                   \
  {                                                                                          \
    float f_[8];                                                                             \
    _Pragma("unroll") for (int j_ = 0; j_ < 4; ++j_) {                                       \
      const uint32_t byte_ = (rq[S] >> (8 * j_)) & 0xFFu;                                    \
      f_[2 * j_] = rd[S] * (float)((int)(byte_ & 0xF) - 8); /* d0*(float)(n-8): one rounding */ \
      f_[2 * j_ + 1] = rd[S] * (float)((int)(byte_ >> 4) - 8);                               \
    }                                                                                        \
    Lw[BUF][lb][2 * lw][lr] = f32x4{f_[0], f_[1], f_[2], f_[3]};                             \
    Lw[BUF][lb][2 * lw + 1][lr] = f32x4{f_[4], f_[5], f_[6], f_[7]};                         \
  }

  float acc[NJ];
#pragma unroll
  for (int u = 0; u < NJ; ++u) acc[u] = 0.0f;
#pragma unroll
  for (int s = 0; s < GR_D; ++s) {
    GR_FETCH_W(s, s)
    GR_FETCH_X(s, s)
  }
  GR_STAGE_W(0, 0)
  // whole rounds of GR_D chunks: the chunks past the last one have no blocks (kb <= 0)
  for (int c0 = 0; c0 < nchunk; c0 += GR_D) {
#pragma unroll
    for (int s = 0; s < GR_D; ++s) {  // (GR_D even: chunk c's LDS buffer is s & 1)
      const int c = c0 + s;
      __syncthreads();  // chunk c is staged; every read of the other buffer (chunk c - 1) is done
      GR_FETCH_W(s, c + GR_D)  // (chunk c's word and scale were staged before the barrier)
      if (active) {
        const int kb = nb - c * GR_KB;
#pragma unroll
        for (int i = 0; i < GR_KB; ++i) {
          if (i < kb) {
            f32x4 w[8];
#pragma unroll
            for (int g = 0; g < 8; ++g) w[g] = Lw[s & 1][i][g][l16];
#pragma unroll
            for (int u = 0; u < NJ; ++u) {
              float a = acc[u];
              a = gr_group<0>(a, w[0], x0[s][u][i], x1[s][u][i]);
              a = gr_group<1>(a, w[1], x0[s][u][i], x1[s][u][i]);
              a = gr_group<2>(a, w[2], x0[s][u][i], x1[s][u][i]);
              a = gr_group<3>(a, w[3], x0[s][u][i], x1[s][u][i]);
              a = gr_group<4>(a, w[4], x0[s][u][i], x1[s][u][i]);
              a = gr_group<5>(a, w[5], x0[s][u][i], x1[s][u][i]);
              a = gr_group<6>(a, w[6], x0[s][u][i], x1[s][u][i]);
              a = gr_group<7>(a, w[7], x0[s][u][i], x1[s][u][i]);
              acc[u] = a;
            }
          }
        }
      }
      GR_FETCH_X(s, c + GR_D)
      GR_STAGE_W((s + 1) % GR_D, (s + 1) & 1)
    }
  }
#undef GR_FETCH_W
#undef GR_FETCH_X
#undef GR_STAGE_W

  const int m = m0 + l16;
  if (active && m < M) {
    const float bv = bias ? bias[m] : 0.0f;
#pragma unroll
    for (int u = 0; u < NJ; ++u) {
      const int j = slot + 16 * u;
      if (j < n) y[(size_t)j * M + m] = bias ? acc[u] + bv : acc[u];
    }
  }
}

// y[j][m] = exact Q4_0 dot of weight row m and activation row j (+ bias[m]) for j < n <= 32; xd:
// [n][K] activation factors (pair-interleaved, kern.hpp)
int launch_gemm_exact_rows(const W4 &W, const float *xd, int n, const float *bias, float *y, hipStream_t s) {
  if (W.k % QK || W.k <= 0 || W.rows <= 0 || n < 1 || n > VSIM_BATCH_MAX || !xd || !y) {
    set_error("q4_gemm_rows: 1..32 activation rows, K a multiple of 32, xd required");
    return VSIM_EINVAL;
  }
  const dim3 grid((W.rows + GR_RT - 1) / GR_RT);
  if (n <= 16)
    hipLaunchKernelGGL((k_gemm_exact_rows<1>), grid, dim3(GR_THREADS), 0, s, W, xd, n, bias, y);
  else
    hipLaunchKernelGGL((k_gemm_exact_rows<2>), grid, dim3(GR_THREADS), 0, s, W, xd, n, bias, y);
  VSIM_HIP(hipGetLastError());
  return VSIM_OK;
}

}  // namespace vsim
