// vsim_amd/csrc/quantize_w.hip — the model quantizer's kernel for gfx950: F32 / F16 weight rows
// to Q4_0, written as W4T32 (the device layout), as AoS blocks (the file format), or both, with
// the reference tools' 16-bin histogram of the codes.
//
// Reference behaviour restated (not translated): ggml_quantize_q4_0, utils.cpp:425-482, as the
// quantize_* tools drive it (quantize_gptneox.cpp:143-311).  Per 32-block:
//   amax = std::max(amax, fabsf(v))      a NaN weight is ignored (std::max keeps its first
//                                        argument when the comparison is false), unlike the
//                                        activation quantizer's MAX macro (q4_block, kern.hpp)
//   d = amax / 7, id = d ? 1 / d : 0     both correctly rounded (no fast-math, -ffp-contract=off)
//   code = (int8_t)round(v * id) + 8     the x86 cast (x86_round_i8): inf and NaN give code 8
//                                        (computed by qw_code below, per block class)
//   element 2l in the low nibble of byte l; hist[code]++
//
// Shape: the kernel is a stream, 4 B (F32) or 2 B (F16) in and 0.625 B out per weight.  A
// workgroup stages a tile of 32 rows x 256 columns in LDS, every row one contiguous run of 1 KB
// (512 B for F16), then thread (r = tid % 32, b = tid / 32) quantizes block b of row r from LDS.
// In that order a wave's W4T32 stores are two whole block columns: 1 KB of nibbles and 256 B of
// scales, contiguous.  The AoS blocks go back through LDS and leave as runs of 160 B per row.
// The LDS row pitch is an odd multiple of 16 B, so the 16-lane groups of a ds_read_b128 fall on
// distinct banks (MI355X_MICROARCH.md, LDS).  Workgroups walk the tiles with a grid stride and
// keep their histogram in LDS, so that a launch ends with 16 global atomics per workgroup.
#include <hip/hip_fp16.h>

#include "kern.hpp"

namespace vsim {

namespace {

constexpr int QW_ROWS = T32;            // tile rows: one W4T32 tile
constexpr int QW_COLS = 256;            // tile columns: 8 blocks
constexpr int QW_BLK = QW_COLS / QK;    // blocks per tile row
constexpr int QW_THREADS = QW_ROWS * QW_BLK;
constexpr int QW_OPITCH = QW_BLK * 5 + 1;  // AoS staging: 5 dwords per block, one of padding per row
constexpr unsigned QW_MAX_GRID = 2048;     // 8 workgroups for each of 256 CUs

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

struct QwArgs {
  const void *x;             // [rows][k] of T
  int rows, k;
  uint8_t *w_qs;             // W4T32 planes of the whole weight (null: no W4T32 output)
  float *w_d;
  int row0;                  // first row of this chunk inside the weight (a multiple of 32)
  int pad;                   // the chunk ends the weight: write the last tile's padding rows
  uint32_t *aos;             // [rows][k/32] blocks of 5 dwords (null: none)
  unsigned long long *hist;  // 16 counters (null: none)
  int ctiles;
  unsigned tiles;
};

// (int8_t)round(v) + 8 for |v| < 8 or NaN, which is every product of a block whose id is finite
// (|x| <= amax, or x is a NaN that amax ignored): what x86_round_i8(v) + 8 gives there, in a
// third of the instructions -- the kernel's time is VALU time as much as memory time.
// v * 2^21 is exact and the conversion truncates it to a fixed-point number with 21 fraction bits,
// which keeps every comparison with n + 0.5; adding one half (less one unit for negatives, so that
// the floor of the arithmetic shift rounds their ties away from zero) and 8 and shifting is then
// round-half-away-from-zero plus 8.  v_cvt_i32_f32 turns NaN into 0, the low byte of the INT_MIN
// that the x86 conversion returns, so NaN gets code 8; written as the instruction because the C
// cast of a NaN is undefined.
__device__ __forceinline__ int qw_code(float v) {
  int fx;
  asm("v_cvt_i32_f32 %0, %1" : "=v"(fx) : "v"(v * 2097152.0f));
  return (fx + ((1 << 20) + (8 << 21)) + (fx >> 31)) >> 21;
}

// the 32 values of block bl of tile row r, widened exactly (v_cvt_f32_f16 keeps subnormal halves)
template <typename T>
__device__ __forceinline__ void qw_block_from_lds(const uint4 *s_in, int r, int bl, float *v);

template <>
__device__ __forceinline__ void qw_block_from_lds<float>(const uint4 *s_in, int r, int bl, float *v) {
  const f32x4 *p = (const f32x4 *)s_in + r * ((QW_COLS + 4) / 4) + bl * (QK / 4);
#pragma unroll
  for (int i = 0; i < QK / 4; ++i) {
    const f32x4 t = p[i];
    v[4 * i] = t.x; v[4 * i + 1] = t.y; v[4 * i + 2] = t.z; v[4 * i + 3] = t.w;
  }
}

template <>
__device__ __forceinline__ void qw_block_from_lds<__half>(const uint4 *s_in, int r, int bl, float *v) {
  const f16x8 *p = (const f16x8 *)s_in + r * ((QW_COLS + 8) / 8) + bl * (QK / 8);
#pragma unroll
  for (int i = 0; i < QK / 8; ++i) {
    const f16x8 t = p[i];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[8 * i + e] = (float)t[e];
  }
}

template <typename T>
__global__ __launch_bounds__(QW_THREADS) void k_quantize_w(QwArgs a) {
  constexpr int EPV = 16 / (int)sizeof(T);  // elements per 16-byte vector
  constexpr int VPR = QW_COLS / EPV;        // vectors per tile row
  constexpr int VPITCH = VPR + 1;           // LDS row pitch in vectors (odd: see the file comment)
  __shared__ uint4 s_in[QW_ROWS * VPITCH];
  __shared__ uint32_t s_out[QW_ROWS * QW_OPITCH];
  __shared__ unsigned long long s_hist[16];
  const int t = threadIdx.x;
  const int r = t & (QW_ROWS - 1), bl = t >> 5;
  const int nb = a.k / QK;
  if (t < 16) s_hist[t] = 0;
  __syncthreads();
  for (unsigned tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
    const int ct = (int)(tile % (unsigned)a.ctiles), rt = (int)(tile / (unsigned)a.ctiles);
    const int col0 = ct * QW_COLS, rowb = rt * QW_ROWS;
    const int ncol = min(QW_COLS, a.k - col0);  // a multiple of 32
    const int nrow = min(QW_ROWS, a.rows - rowb);
    for (int i = t; i < QW_ROWS * VPR; i += QW_THREADS) {
      const int rr = i / VPR, cv = i % VPR;
      if (rr < nrow && cv * EPV < ncol)
        s_in[rr * VPITCH + cv] = *(const uint4 *)((const T *)a.x + ((size_t)(rowb + rr) * a.k + col0 + cv * EPV));
    }
    __syncthreads();
    const bool have = bl * QK < ncol;
    const bool live = have && r < nrow;
    uint32_t w[4] = {0x88888888u, 0x88888888u, 0x88888888u, 0x88888888u};
    float d = 0.0f;
    unsigned long long c0 = 0, c1 = 0;  // this block's counts of codes 0..7 and 8..15, one byte each
    if (live) {
      float v[QK];
      qw_block_from_lds<T>(s_in, r, bl, v);
      float amax = 0.0f;
#pragma unroll
      // std::max(amax, f) = amax < f ? f : amax ignores a NaN f, and amax itself is never NaN: that
      // is fmaxf, one v_max_f32
      for (int l = 0; l < QK; ++l) amax = fmaxf(amax, fabsf(v[l]));
      d = amax / 7.0f;
      float id = d != 0.0f ? 1.0f / d : 0.0f;
      // An id that overflowed makes every product inf or NaN, which the x86 cast turns into code 8:
      // a NaN id does the same through qw_code.  Every other block has |v * id| < 8 or NaN.
      id = id == INFINITY ? NAN : id;
#pragma unroll
      for (int i = 0; i < 4; ++i) w[i] = 0;
#pragma unroll
      for (int l = 0; l < QK; l += 2) {
        const int q0 = qw_code(v[l] * id), q1 = qw_code(v[l + 1] * id);
        w[l / 8] |= (uint32_t)(q0 | (q1 << 4)) << (8 * ((l / 2) & 3));
        if (a.hist) {
          const unsigned long long i0 = 1ull << (8 * (q0 & 7)), i1 = 1ull << (8 * (q1 & 7));
          c0 += q0 & 8 ? 0 : i0;
          c1 += q0 & 8 ? i0 : 0;
          c0 += q1 & 8 ? 0 : i1;
          c1 += q1 & 8 ? i1 : 0;
        }
      }
    }
    if (a.w_qs && (live || (have && a.pad))) {  // padding rows as k_w4_pack writes them: d = 0, q = 8
      const int R = a.row0 + rowb + r;
      const size_t o = ((size_t)(R / T32) * nb + (ct * QW_BLK + bl)) * T32 + r;
      *(uint4 *)(a.w_qs + o * 16) = make_uint4(w[0], w[1], w[2], w[3]);
      a.w_d[o] = d;
    }
    if (a.aos && live) {
      uint32_t *o = s_out + r * QW_OPITCH + bl * 5;
      o[0] = __float_as_uint(d);
      o[1] = w[0]; o[2] = w[1]; o[3] = w[2]; o[4] = w[3];
    }
    if (a.hist) {  // wave sums of the byte counters, widened to 16 bits (at most 64 * 32 per code)
      const unsigned long long c[2] = {c0, c1};
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const unsigned lo = (unsigned)(c[j / 4] >> (16 * (j & 3))) & 0xFFu;
        const unsigned hi = (unsigned)(c[j / 4] >> (16 * (j & 3) + 8)) & 0xFFu;
        const int s = dpp::lane63(dpp::reduce((int)(lo | (hi << 16)), 0, [](int x, int y) { return x + y; }));
        if ((t & 63) == 0) {
          if (s & 0xFFFF) atomicAdd(&s_hist[2 * j], (unsigned long long)(s & 0xFFFF));
          if ((unsigned)s >> 16) atomicAdd(&s_hist[2 * j + 1], (unsigned long long)((unsigned)s >> 16));
        }
      }
    }
    __syncthreads();  // every read of s_in is done; s_out is complete
    if (a.aos) {
      const int nw = ncol / QK * 5;
      for (int i = t; i < QW_ROWS * QW_BLK * 5; i += QW_THREADS) {
        const int rr = i / (QW_BLK * 5), wd = i % (QW_BLK * 5);
        if (rr < nrow && wd < nw)
          a.aos[((size_t)(rowb + rr) * nb + (size_t)ct * QW_BLK) * 5 + wd] = s_out[rr * QW_OPITCH + wd];
      }
    }
  }
  if (a.hist) {
    __syncthreads();
    if (t < 16 && s_hist[t]) atomicAdd(a.hist + t, s_hist[t]);
  }
}

}  // namespace

int launch_quantize_w(const void *x, int src_type, int rows, int k, void *w, int w_rows, int row0, void *aos,
                      uint64_t *hist, hipStream_t s) {
  if (!x || (src_type != VSIM_SRC_F32 && src_type != VSIM_SRC_F16)) {
    set_error("q4_quantize_w: src_type must be VSIM_SRC_F32 or VSIM_SRC_F16");
    return VSIM_EINVAL;
  }
  if (rows <= 0 || k <= 0 || k % QK) { set_error("q4_quantize_w: k must be a multiple of 32"); return VSIM_EINVAL; }
  if (!w && !aos) { set_error("q4_quantize_w: no output (w and aos both NULL)"); return VSIM_EINVAL; }
  if (w && (row0 < 0 || row0 % T32 || (long long)row0 + rows > w_rows)) {
    set_error("q4_quantize_w: row0 must be a multiple of 32 and row0 + rows <= w_rows");
    return VSIM_EINVAL;
  }
  if (((uintptr_t)x & 15) || ((uintptr_t)w & 15) || ((uintptr_t)aos & 3) || ((uintptr_t)hist & 7)) {
    set_error("q4_quantize_w: misaligned pointer (x, w: 16 bytes; aos: 4; hist: 8)");
    return VSIM_EINVAL;
  }
  QwArgs a{};
  a.x = x;
  a.rows = rows;
  a.k = k;
  if (w) {
    const W4 W = w4_view(w, w_rows, k);
    a.w_qs = (uint8_t *)W.qs;
    a.w_d = (float *)W.d;
    a.row0 = row0;
    a.pad = row0 + rows == w_rows;
  }
  a.aos = (uint32_t *)aos;
  a.hist = (unsigned long long *)hist;
  a.ctiles = (k + QW_COLS - 1) / QW_COLS;
  const unsigned long long tiles = (unsigned long long)a.ctiles * ((rows + QW_ROWS - 1) / QW_ROWS);
  if (tiles > 0x7FFFFFFFull) { set_error("q4_quantize_w: chunk too large"); return VSIM_EINVAL; }
  a.tiles = (unsigned)tiles;
  const dim3 grid(a.tiles < QW_MAX_GRID ? a.tiles : QW_MAX_GRID);
  if (src_type == VSIM_SRC_F16)
    hipLaunchKernelGGL(k_quantize_w<__half>, grid, dim3(QW_THREADS), 0, s, a);
  else
    hipLaunchKernelGGL(k_quantize_w<float>, grid, dim3(QW_THREADS), 0, s, a);
  VSIM_HIP(hipGetLastError());
  return VSIM_OK;
}

}  // namespace vsim
