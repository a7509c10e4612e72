// vsim_amd/csrc/w4a16_decode.hip — weight-only mode (VSIM_MODE_W4A16): the kernels of the single-token
// decode step.  Each gives, bit for bit, what the general path's kernels give on the same row
// (gemm_w4a16_rows.hip, ops_elt.hip); what changes is how many launches a layer takes and how much
// of a weight a workgroup has in flight.
//
// k_w4a16_ln    ln_exact_lds (k_norm_exact's arithmetic, certificates and fallbacks) of one row, then
//               k_w4a16_rows' operand of the normalized row taken from LDS: the maximum of |w y + b|
//               over the affine's outputs, e, h = fp16_rn(. * 2^e).  A second workgroup runs a second
//               norm of the same row (GPT-NeoX's two-norm layer).  The f32 row never leaves LDS.
// k_w4a16_gelu  g = table[f2h(x + bias)] (k_gelu: the f32 add first), then the operand of g: the
//               maximum over the outputs g, not the inputs.  One workgroup; rows of up to
//               WD_G_MAXK elements (24,576: fc_in of n_embd = 6144) keep g in registers between
//               the maximum and the conversion, longer ones make g a second time.
// k_gemv_w4a16  k_gemm_w4a16_rows at one activation row, for up to four jobs.  The MFMA, the
//               placement of weights and of the activation row in its fragments (the row is column 0 of
//               B, where the rows kernel has it at n = 1; the other columns are zero), wave p's walk b = p,
//               p + 16, ... through fmaf(d_w[b], dot_b, part[p]), the in-order sum of the sixteen
//               partials, the 2^-e scaling, the bias and the NaN rule are that kernel's.  New: the
//               partials take 1 KB of LDS instead of 32 KB, a wave fetches WD_UN blocks per trip
//               before it uses any (the rows kernel: 2), and the epilogue can join:
//               y = res + (res_a + v), or v + res, reading only the elements it writes.
//
// Loads: in bounds without slack.  The last tile's padding rows exist (d = 0), blocks past a
// wave's strand are clamped to the last block and not used, and only elements < M of bias, res,
// res_a and y are touched.
#include "w4a16.hpp"

namespace vsim {

// ------------------------------------------------------------------ LayerNorm -> operand
__global__ void __launch_bounds__(NORM_THREADS) k_w4a16_ln(W4a16Ln A, unsigned *stats) {
  extern __shared__ __attribute__((aligned(16))) float xrow[];
  __shared__ uint32_t red[NORM_THREADS / 64];
  const bool second = blockIdx.x == 1;
  ln_exact_lds(A.x, xrow, A.n, second ? A.w2 : A.w1, second ? A.b2 : A.b1, stats);  // (ends on a barrier)
  const int tid = threadIdx.x, nv = A.n / 4;
  uint32_t am = 0u;
  for (int f = tid; f < nv; f += NORM_THREADS) {
    const f32x4 v = ((const f32x4 *)xrow)[f];
#pragma unroll
    for (int i = 0; i < 4; ++i) am = max(am, wa_abs_bits(v[i]));
  }
  const int e = wa_exponent(wa_block_max<NORM_THREADS>(am, red));
  if (tid == 0) (second ? A.e2 : A.e1)[0] = e;
  wa_half4 *hr = (wa_half4 *)(second ? A.h2 : A.h1);
  for (int f = tid; f < nv; f += NORM_THREADS) {
    const f32x4 v = ((const f32x4 *)xrow)[f];
    wa_half4 h;
#pragma unroll
    for (int i = 0; i < 4; ++i) h[i] = wa_half(v[i], e);
    hr[f] = h;
  }
}

int launch_w4a16_ln(const W4a16Ln &A, hipStream_t s) {
  if (!A.x || !A.w1 || !A.b1 || !A.h1 || !A.e1 || A.n <= 0 || A.n % QK) {
    set_error("w4a16_ln: n a positive multiple of 32, x, w1, b1, x16_1 and e1 required");
    return VSIM_EINVAL;
  }
  const bool two = A.w2 || A.b2 || A.h2 || A.e2;
  if (two && (!A.w2 || !A.b2 || !A.h2 || !A.e2)) {
    set_error("w4a16_ln: the second norm needs w2, b2, x16_2 and e2");
    return VSIM_EINVAL;
  }
  if ((size_t)A.n * 4 > 64 * 1024) {
    set_error("w4a16_ln: row longer than 16384");
    return VSIM_EINVAL;
  }
  if ((((uintptr_t)A.x | (uintptr_t)A.w1 | (uintptr_t)A.b1 | (uintptr_t)A.h1 | (uintptr_t)A.w2 | (uintptr_t)A.b2 |
        (uintptr_t)A.h2) & 15) != 0) {
    set_error("w4a16_ln: x, the affines and the operands must be 16-byte aligned");
    return VSIM_EINVAL;
  }
  hipLaunchKernelGGL(k_w4a16_ln, dim3(two ? 2 : 1), dim3(NORM_THREADS), (size_t)A.n * 4, s, A, dev_stats());
  VSIM_HIP(hipGetLastError());
  return VSIM_OK;
}

// ------------------------------------------------------------------ bias + GELU -> operand
constexpr int WD_G_NT = 1024, WD_G_PER = 6, WD_G_MAXK = 4 * WD_G_NT * WD_G_PER;

__device__ __forceinline__ f32x4 wd_gelu4(const f32x4 *x, const f32x4 *bias, int f, const uint16_t *tab) {
  f32x4 v = x[f];
  if (bias) v = v + bias[f];
  f32x4 g;
#pragma unroll
  for (int i = 0; i < 4; ++i) g[i] = h2f(tab[f2h(v[i])]);
  return g;
}

__global__ void __launch_bounds__(WD_G_NT)
    k_w4a16_gelu(const float *__restrict__ x, const float *__restrict__ bias, int K, _Float16 *__restrict__ x16,
                 int32_t *__restrict__ e_out, float *__restrict__ g_out, const uint16_t *__restrict__ tab) {
  __shared__ uint32_t red[WD_G_NT / 64];
  const int tid = threadIdx.x, nv = K / 4;
  const f32x4 *xr = (const f32x4 *)x, *br = (const f32x4 *)bias;
  wa_half4 *hr = (wa_half4 *)x16;
  const bool keep = K <= WD_G_MAXK;  // (uniform)
  f32x4 g[WD_G_PER];
  uint32_t am = 0u;
  if (keep) {
#pragma unroll
    for (int k = 0; k < WD_G_PER; ++k) {
      const int f = tid + WD_G_NT * k;
      g[k] = f < nv ? wd_gelu4(xr, br, f, tab) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int i = 0; i < 4; ++i) am = max(am, wa_abs_bits(g[k][i]));
    }
  } else {
    for (int f = tid; f < nv; f += WD_G_NT) {
      const f32x4 v = wd_gelu4(xr, br, f, tab);
#pragma unroll
      for (int i = 0; i < 4; ++i) am = max(am, wa_abs_bits(v[i]));
    }
  }
  const int e = wa_exponent(wa_block_max<WD_G_NT>(am, red));
  if (tid == 0) e_out[0] = e;
  auto put = [&](int f, const f32x4 &v) {
    wa_half4 h;
#pragma unroll
    for (int i = 0; i < 4; ++i) h[i] = wa_half(v[i], e);
    hr[f] = h;
    if (g_out) ((f32x4 *)g_out)[f] = v;
  };
  if (keep) {
#pragma unroll
    for (int k = 0; k < WD_G_PER; ++k) {
      const int f = tid + WD_G_NT * k;
      if (f < nv) put(f, g[k]);
    }
  } else {
    for (int f = tid; f < nv; f += WD_G_NT) put(f, wd_gelu4(xr, br, f, tab));
  }
}

int launch_w4a16_gelu(const float *x, const float *bias, int K, void *x16, int32_t *e, float *g_out, hipStream_t s) {
  if (!x || !x16 || !e || K <= 0 || K % QK) {
    set_error("w4a16_gelu: K a positive multiple of 32, x, x16 and e required");
    return VSIM_EINVAL;
  }
  if ((((uintptr_t)x | (uintptr_t)bias | (uintptr_t)x16 | (uintptr_t)g_out) & 15) != 0) {
    set_error("w4a16_gelu: x, bias, x16 and g must be 16-byte aligned");
    return VSIM_EINVAL;
  }
  DevTables t;
  if (int rc = tables_get(&t)) return rc;
  hipLaunchKernelGGL(k_w4a16_gelu, dim3(1), dim3(WD_G_NT), 0, s, x, bias, K, (_Float16 *)x16, e, g_out, t.gelu_f16);
  VSIM_HIP(hipGetLastError());
  return VSIM_OK;
}

// ------------------------------------------------------------------ the single-row products
constexpr int WD_UN = 4;  // blocks of a wave's strand in flight per trip

struct WdBlock {
  uint32_t wq;  // the lane's 4 bytes of its weight row's nibble run
  f32x4 wd;     // scales of weight rows 4 g .. 4 g + 3
  wa_half8 xh;  // the lane's 8 halves of the activation row
};

// the launch's jobs and where each one's workgroups begin (g0[nj] = the grid)
struct WdLaunch {
  W4a16Gemv B;
  int g0[5];
};

__global__ void __launch_bounds__(WA_THREADS) k_gemv_w4a16(WdLaunch L) {
  __shared__ float part[WA_WAVES][WA_RT];  // 1 KB
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane & 15, g = lane >> 4;
  // the workgroup's job (uniform; selected, not indexed, so the jobs stay in scalar registers)
  int ji = 0;
#pragma unroll
  for (int i = 1; i < 4; ++i)
    if (i < L.B.nj && (int)blockIdx.x >= L.g0[i]) ji = i;
  W4a16GemvJob J = L.B.j[0];
  int first = L.g0[0];
#pragma unroll
  for (int i = 1; i < 4; ++i)
    if (ji == i) {
      J = L.B.j[i];
      first = L.g0[i];
    }
  const W4 &W = J.w;
  const int m0 = ((int)blockIdx.x - first) * WA_RT, M = W.rows, nb = W.nb();
  // block b of weight row m0 + r: nibbles at wq + b * 512 bytes, scale at wd + b * 32
  // (m0 + 15 < W.tiles * T32: the padding rows of the last tile exist)
  const size_t wo = W.off(m0, 0);
  const uint8_t *wq = W.qs + (wo + c) * 16 + 4 * g;
  const float *wd = W.d + wo + 4 * g;
  const _Float16 *xp = J.x16 + 8 * g;
  f32x4 acc = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

  // The one activation row is column 0 of B, and only column 0 of D leaves the kernel: the lanes
  // c == 0 alone fetch the row's halves and the scales of their four weight rows (4 lanes of a
  // wave instead of 64 asking for the same 64 bytes); the other columns multiply zeros.  A column
  // of D depends on its own column of B only.
  auto fetch = [&](int b) {
    WdBlock r;
    r.wq = *(const uint32_t *)(wq + (size_t)b * (T32 * 16));
    r.wd = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    r.xh = wa_half8{0, 0, 0, 0, 0, 0, 0, 0};
    if (c == 0) {
      r.wd = *(const f32x4 *)(wd + (size_t)b * T32);
      r.xh = *(const wa_half8 *)(xp + (size_t)b * QK);
    }
    return r;
  };
  // WD_UN blocks of the wave's strand per trip, all fetched before any is used; those past the
  // strand's end are clamped to the last block and skipped (wave-uniform).  The empty asm counts
  // the fetched values as used where it stands, so that no load sinks into the branches below it
  // (the compiler otherwise loads each block where it is consumed: one block in flight).
  // Measured on GPT-J-6B's step (profiles/w4a16_step_bench.txt has the final form): 8 blocks per
  // trip (about 100 VGPRs, one workgroup per CU) 332 tok/s; 4 per trip (two per CU) 365; the next
  // trip prefetched into a second register set, 4 + 4 blocks 291 and 2 + 2 blocks 345.
  for (int b = wave; b < nb; b += WD_UN * WA_WAVES) {
    WdBlock r[WD_UN];
#pragma unroll
    for (int u = 0; u < WD_UN; ++u) r[u] = fetch(min(b + u * WA_WAVES, nb - 1));
#pragma unroll
    for (int u = 0; u < WD_UN; ++u) asm volatile("" : "+v"(r[u].wq), "+v"(r[u].wd), "+v"(r[u].xh));
#pragma unroll
    for (int u = 0; u < WD_UN; ++u) {
      if (b + u * WA_WAVES >= nb) break;
      const f32x4 dot =
          __builtin_amdgcn_mfma_f32_16x16x32_f16(wa_unpack(r[u].wq), r[u].xh, f32x4{0.0f, 0.0f, 0.0f, 0.0f}, 0, 0, 0);
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i] = __builtin_fmaf(r[u].wd[i], dot[i], acc[i]);
    }
  }
  // D[4 g + i][0]: column 0's lanes hold the row's sixteen values
  if (c == 0) *(f32x4 *)&part[wave][4 * g] = acc;
  __syncthreads();
  const int r = tid;
  if (r < WA_RT && m0 + r < M) {
    float sum = 0.0f;
#pragma unroll
    for (int p = 0; p < WA_WAVES; ++p) sum += part[p][r];
    const int e = J.e[0];
    const float s = ldexpf(sum, e == VSIM_W4A16_NONFINITE ? 0 : -e);
    const float sb = J.bias ? s + J.bias[m0 + r] : s;
    const float v = e == VSIM_W4A16_NONFINITE ? __uint_as_float(0x7FC00000u) : sb;
    float y = v;
    if (J.res) y = J.res_a ? J.res[m0 + r] + (J.res_a[m0 + r] + v) : v + J.res[m0 + r];
    J.y[m0 + r] = y;
  }
}

int launch_w4a16_gemv(const W4a16Gemv &B, hipStream_t s) {
  if (B.nj < 1 || B.nj > 4) {
    set_error("w4a16_gemv: 1..4 jobs");
    return VSIM_EINVAL;
  }
  WdLaunch L{};
  L.B = B;
  int grid = 0;
  for (int i = 0; i < B.nj; ++i) {
    const W4a16GemvJob &j = B.j[i];
    if (j.w.k <= 0 || j.w.k % QK || j.w.rows <= 0 || !j.w.qs || !j.x16 || !j.e || !j.y) {
      set_error("w4a16_gemv: every job needs K a positive multiple of 32, M > 0, w, x16, e and y");
      return VSIM_EINVAL;
    }
    if (j.res_a && !j.res) {
      set_error("w4a16_gemv: res_a without res");
      return VSIM_EINVAL;
    }
    if ((((uintptr_t)j.w.qs | (uintptr_t)j.x16) & 15) != 0) {
      set_error("w4a16_gemv: w and x16 must be 16-byte aligned");
      return VSIM_EINVAL;
    }
    L.g0[i] = grid;
    grid += (j.w.rows + WA_RT - 1) / WA_RT;
  }
  for (int i = B.nj; i < 5; ++i) L.g0[i] = grid;
  hipLaunchKernelGGL(k_gemv_w4a16, dim3(grid), dim3(WA_THREADS), 0, s, L);
  VSIM_HIP(hipGetLastError());
  return VSIM_OK;
}

}  // namespace vsim
