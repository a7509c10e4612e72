// vsim_amd/csrc/score.hip — per-row log-probability and greedy id of a block of logit rows.
//
// Scoring a text asks, for every position, how likely the model found the token that came
// next: logprob = x[t] - log(sum_j exp(x[j])) of that position's logits row x.  k_score_rows does
// that for R rows x[R][V] that stay on the device (the model's lm_head product over a chunk of
// prompt rows, vsim_model_eval_score), so only 12 bytes per position leave it instead of a row.
//
// Definition (vsim_op_logprob).  Per row, with m the row's maximum (a float, exact):
//   s   = sum_j exp((double)x[j] - (double)m)        in double
//   lse = (double)m + log(s)
//   logprob = (double)x[t] - lse                     t = the row's target id
// and argmax = k_argmax's greedy id (first maximum, -0.0 == +0.0, the first NaN if any: the same
// 64-bit keys, am_key in kern.hpp).  A target of -1 (or, at this level, any id outside [0, V))
// means "no target": logprob = 0 and the sum is skipped.  A row with a NaN, or whose maximum is
// +inf or -inf, has no log-sum-exp: logprob = NaN, decided from the maximum alone, so the kernel
// always terminates.  -inf entries beside a finite maximum contribute exp(-inf) = 0.
//
// Order.  One workgroup of 1024 threads per row.  Thread t adds the terms j = t, t + 1024,
// t + 2048, .. in that order into its own double; the 64 partials of a wave are added by the DPP
// tree of wave_sum_d, and thread 0 adds the 16 waves' sums in wave order.  Nothing of that
// depends on R, on the row's place in the launch or on timing (no atomics): a row's two outputs
// are a function of the row's contents alone, bit for bit.  Two passes over the row (keys, then
// terms); the second finds the row's 4 V bytes in L2.  16 waves per row because the passes wait
// on loads and on the double exp's latency, not on bandwidth: at n_vocab = 50400 a 256-row chunk
// took 97 us with 4 waves per row and takes 38 us with 16 (profiles/score_bench.txt).
//
// Alignment.  Rows start at x + i V: any 4-byte boundary when V is odd.  Every load is a 4-byte
// load; consecutive lanes read consecutive floats, so the loads coalesce without wide accesses.
#include <hip/hip_runtime.h>

#include "kern.hpp"

namespace vsim {

constexpr int SC_T = 1024;

__global__ void __launch_bounds__(SC_T)
    k_score_rows(const float *__restrict__ x, int V, const int32_t *__restrict__ target, double *__restrict__ logprob,
                 int32_t *__restrict__ argmax) {
  __shared__ unsigned long long sk[SC_T / 64];
  __shared__ double ss[SC_T / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t row = blockIdx.x;
  const float *xr = x + row * (size_t)V;

  // pass 1: the greedy id and, from it, the maximum
  unsigned long long best = 0;
  for (int j = tid; j < V; j += SC_T) best = max(best, am_key(xr[j], j));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) best = max(best, (unsigned long long)__shfl_xor(best, o, 64));
  if (lane == 0) sk[wave] = best;
  __syncthreads();
  best = sk[0];
#pragma unroll
  for (int w = 1; w < SC_T / 64; ++w) best = max(best, sk[w]);
  const int bi = (int)(0xFFFFFFFFu - (uint32_t)best);  // in [0, V): V >= 1, every key carries its index
  if (argmax && tid == 0) argmax[row] = bi;
  if (!logprob) return;

  const int t = target ? target[row] : -1;
  if (t < 0 || t >= V) {  // no target
    if (tid == 0) logprob[row] = 0.0;
    return;
  }
  const float m = xr[bi];
  if (m != m || m == INFINITY || m == -INFINITY) {  // (uniform: every thread read the same word)
    if (tid == 0) logprob[row] = __longlong_as_double(0x7FF8000000000000ll);
    return;
  }

  // pass 2: the terms, in the fixed order above
  const double md = (double)m;
  double s = 0.0;
#pragma unroll 4
  for (int j = tid; j < V; j += SC_T) s += exp((double)xr[j] - md);
  s = wave_sum_d(s);
  if (lane == 0) ss[wave] = s;
  __syncthreads();
  if (tid != 0) return;
  s = ss[0];
#pragma unroll
  for (int w = 1; w < SC_T / 64; ++w) s += ss[w];
  const double lse = md + log(s);
  logprob[row] = (double)xr[t] - lse;
}

int launch_score_rows(const float *x, int V, int R, const int32_t *target, double *logprob, int32_t *argmax,
                      hipStream_t s) {
  if (!x || V < 1 || R < 0 || (!logprob && !argmax)) {
    set_error("logprob: needs x, V >= 1, R >= 0 and at least one of logprob, argmax");
    return VSIM_EINVAL;
  }
  if (R == 0) return VSIM_OK;
  hipLaunchKernelGGL(k_score_rows, dim3((unsigned)R), dim3(SC_T), 0, s, x, V, target, logprob, argmax);
  VSIM_HIP(hipGetLastError());
  return VSIM_OK;
}

}  // namespace vsim
