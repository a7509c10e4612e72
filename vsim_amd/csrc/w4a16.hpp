// vsim_amd/csrc/w4a16.hpp — what the weight-only mode's kernels share (gemm_w4a16_rows.hip,
// w4a16_decode.hip): the fragment types, the nibble unpack and the row operand's exponent and
// conversion, so that every kernel that makes or consumes an operand spells them the same way.
#pragma once

#include "kern.hpp"
#include "../../include/vsim_hip.h"

namespace vsim {

constexpr int WA_RT = 16;     // weight rows per workgroup
constexpr int WA_WAVES = 16;  // one per partial
constexpr int WA_THREADS = 64 * WA_WAVES;

typedef _Float16 wa_half8 __attribute__((ext_vector_type(8)));
typedef _Float16 wa_half4 __attribute__((ext_vector_type(4)));
typedef _Float16 wa_half2 __attribute__((ext_vector_type(2)));

// 8 nibbles of one word (element t at bits 4 t) as 8 halves q - 8: 0x6400 | q is the half 1024 + q
__device__ __forceinline__ wa_half8 wa_unpack(uint32_t w) {
  wa_half8 r;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t by = (w >> (8 * j)) & 0xFFu;
    const uint32_t bits = 0x64006400u | (by & 0xFu) | ((by & 0xF0u) << 12);
    const wa_half2 v = __builtin_bit_cast(wa_half2, bits) - wa_half2{(_Float16)1032.0f, (_Float16)1032.0f};
    r[2 * j] = v[0];
    r[2 * j + 1] = v[1];
  }
  return r;
}

// |x| as bits: ordered like the values for everything finite, subnormals included; a non-finite
// element raises a maximum of these to 0x7F800000 or above
__device__ __forceinline__ uint32_t wa_abs_bits(float x) { return __float_as_uint(x) & 0x7FFFFFFFu; }

// The maximum of `am` over the NT threads of the workgroup, in every thread (red: NT / 64 words)
template <int NT>
__device__ __forceinline__ uint32_t wa_block_max(uint32_t am, uint32_t *red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) am = max(am, (uint32_t)__shfl_xor((int)am, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = am;
  __syncthreads();
  am = red[0];
#pragma unroll
  for (int w = 1; w < NT / 64; ++w) am = max(am, red[w]);
  return am;
}

// The row's exponent from the maximum of its |x| bits: 14 - floor(log2(amax)), 0 for an all-zero
// row, VSIM_W4A16_NONFINITE for a row that holds a NaN or an Inf
__device__ __forceinline__ int wa_exponent(uint32_t am) {
  if (am >= 0x7F800000u) return VSIM_W4A16_NONFINITE;
  if (am == 0u) return 0;
  // floor(log2(amax)): the exponent field, or the top bit's place for a subnormal
  const int lg = (am >> 23) ? (int)(am >> 23) - 127 : (31 - __clz((int)am)) - 149;
  return 14 - lg;
}

// h = fp16_rn(x * 2^e), +0 in a non-finite row
__device__ __forceinline__ _Float16 wa_half(float x, int e) {
  return e == VSIM_W4A16_NONFINITE ? (_Float16)0.0f : (_Float16)ldexpf(x, e);
}

}  // namespace vsim
