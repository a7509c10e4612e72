// vsim_amd/csrc/sample.hip — the O(n_vocab) stage of the reference's sampler on the device.
//
// sample_top_p_top_k_repeat_penalty (utils.cpp:339-371) turns every logit into a double
// candidate (temperature scale, repetition penalty for the ids of the last-n window) and
// partial_sorts the k largest to the front.  k_sample_topk does that part: one launch, up to
// 64 workgroups, the k candidates out in order.  The k-element rest (exp, top-p, the draw)
// stays on the host (sampler.cpp): its exp is glibc's double exp.
//
// Order.  Every candidate becomes (key, id): key = the double's bits mapped to an unsigned
// order (-0.0 -> +0.0), and a candidate is ahead of another when its key is larger or, keys
// equal, its id is lower.  That is a strict total order of distinct ids for every input, NaN
// included (a NaN's key is whatever its bits map to), so every step below terminates and the
// result does not depend on how the row is split.  Bit 31 of the stored id carries "id is in
// the window", so the value is recomputed from x[id] at the end (the key lost -0.0's sign).
//
// A wave keeps its best 64 in order, one per lane.  A batch of 64 new candidates (one per
// lane) is filtered against the k-th entry by a ballot.  A few survivors are broadcast one by
// one and inserted by a one-lane shift of the entries behind them (tk_merge's loop); more are sorted
// across the lanes (bitonic, 21 compare-exchange steps) and merged into the list as a whole
// (tk_merge_sorted: the lane-wise better of the list and the reversed other list is a bitonic
// sequence holding the best 64 of both; 6 more steps order it).  Every step is one round of
// cross-lane reads, and those rounds, not the row's 200 KB, are the kernel's time: hence
// 16 waves per workgroup, one batch each at GPT-J's n_vocab.  The waves of a workgroup merge
// their lists pairwise through LDS (4 rounds); the last workgroup's waves merge the
// workgroups' lists from ws, 4 each at 64 workgroups, then pairwise again.
//
// Window.  A workgroup walks one span of at most 8192 consecutive ids (further spans only when
// n > 64 * 8192) and keeps the span's window membership as a bitmap in LDS, built from the
// window once per span: one bit test per logit instead of nw compares.
#include <hip/hip_runtime.h>

#include <atomic>
#include <string>

#include "common.hpp"

namespace vsim {

constexpr int TK_T = 1024, TK_WAVES = TK_T / 64, TK_SPAN = 8192;
constexpr int TOPK_ROWS_WG = 256;  // workgroups of all rows together (one per CU) before a row gets fewer
constexpr uint32_t TK_ID = 0x7FFFFFFFu, TK_INWIN = 0x80000000u;  // id bits; "penalised" flag

__device__ __forceinline__ unsigned long long tk_key(double c) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(c);
  if (c == 0.0) return 0x8000000000000000ull;
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ bool tk_ahead(unsigned long long ka, uint32_t ia, unsigned long long kb, uint32_t ib) {
  return ka > kb || (ka == kb && (ia & TK_ID) < (ib & TK_ID));
}
// the reference's candidate, in its order of operations (utils.cpp:352-362)
__device__ __forceinline__ double tk_cand(float x, bool inwin, double scale, double penalty) {
  const double c = (double)x * scale;
  if (!inwin) return c;
  return x < 0.0f ? c * penalty : c / penalty;
}
__device__ __forceinline__ uint32_t tk_rl(uint32_t v, int l) {
  return (uint32_t)__builtin_amdgcn_readlane((int)v, l);
}
__device__ __forceinline__ unsigned long long tk_rl64(unsigned long long v, int l) {
  return ((unsigned long long)tk_rl((uint32_t)(v >> 32), l) << 32) | tk_rl((uint32_t)v, l);
}

// One compare-exchange with lane ^ d: this lane keeps the better of the two entries
// (take_better) or the worse.  Distinct entries are strictly ordered, so the two lanes agree;
// equal ones are both "none".
__device__ __forceinline__ void tk_cx(unsigned long long &K, uint32_t &I, int d, bool take_better) {
  const unsigned long long ok = __shfl_xor(K, d, 64);
  const uint32_t oi = __shfl_xor(I, d, 64);
  if (tk_ahead(ok, oi, K, I) == take_better) {
    K = ok;
    I = oi;
  }
}
// Bitonic sort of one entry per lane, worst first (lane 63 ends with the best).
__device__ __forceinline__ void tk_sort_asc(unsigned long long &K, uint32_t &I) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int size = 2; size <= 64; size <<= 1) {
    const bool desc = (lane & size) != 0;  // size 64: no lane, the whole wave ascending
#pragma unroll
    for (int d = size >> 1; d > 0; d >>= 1) tk_cx(K, I, d, ((lane & d) == 0) == desc);
  }
}
// (LK, LI), best first, becomes the best 64 of itself and another list given worst first.
__device__ __forceinline__ void tk_merge_sorted(unsigned long long &LK, uint32_t &LI, unsigned long long rk,
                                                uint32_t ri) {
  const int lane = threadIdx.x & 63;
  if (tk_ahead(rk, ri, LK, LI)) {
    LK = rk;
    LI = ri;
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) tk_cx(LK, LI, d, (lane & d) == 0);
}

// Merge one candidate per lane (ck, ci; "none" = (0, TK_ID), behind every real one) into the
// wave's ordered list (LK, LI: lane j holds the j-th best).  Only the first kk entries matter.
// Called by all 64 lanes together.
constexpr int TK_INSERT_MAX = 8;  // survivors inserted one by one; more: sort and merge
__device__ __forceinline__ void tk_merge(unsigned long long &LK, uint32_t &LI, unsigned long long ck, uint32_t ci,
                                         int kk) {
  const int lane = threadIdx.x & 63;
  unsigned long long tK = tk_rl64(LK, kk - 1);
  uint32_t tI = tk_rl(LI, kk - 1);
  const bool live = tk_ahead(ck, ci, tK, tI);
  unsigned long long mask = __ballot(live);
  if (__popcll(mask) > TK_INSERT_MAX) {
    if (!live) {
      ck = 0;
      ci = TK_ID;
    }
    tk_sort_asc(ck, ci);
    if (tk_rl(LI, 0) == TK_ID && tk_rl64(LK, 0) == 0) {  // the list is empty: the batch reversed is the list
      LK = __shfl(ck, 63 - lane, 64);
      LI = __shfl(ci, 63 - lane, 64);
    } else {
      tk_merge_sorted(LK, LI, ck, ci);
    }
    return;
  }
  while (mask) {
    const int b = __ffsll((long long)mask) - 1;
    const unsigned long long nk = tk_rl64(ck, b);
    const uint32_t ni = tk_rl(ci, b);
    // the lanes the new entry is ahead of are a suffix: the first of them takes it, the
    // others take their left neighbour's
    const unsigned long long uk = __shfl_up(LK, 1, 64);
    const uint32_t ui = __shfl_up(LI, 1, 64);
    if (tk_ahead(nk, ni, LK, LI)) {
      const bool first = lane == 0 || !tk_ahead(nk, ni, uk, ui);
      LK = first ? nk : uk;
      LI = first ? ni : ui;
    }
    tK = tk_rl64(LK, kk - 1);
    tI = tk_rl(LI, kk - 1);
    mask = __ballot(tk_ahead(ck, ci, tK, tI)) & ~((2ull << b) - 1ull);
  }
}

// The workgroup's waves merge their lists pairwise through LDS; wave 0 ends with the best 64.
// Called by the whole workgroup.
__device__ __forceinline__ void tk_merge_waves(unsigned long long &LK, uint32_t &LI, unsigned long long *sK,
                                               uint32_t *sI) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int step = 1; step < TK_WAVES; step <<= 1) {
    __syncthreads();  // the previous round's (or an earlier use's) reads are done
    sK[tid] = LK;
    sI[tid] = LI;
    __syncthreads();
    if ((wave & (2 * step - 1)) == 0) {
      const int r = (wave + step) * 64 + 63 - lane;  // the other wave's list worst first
      tk_merge_sorted(LK, LI, sK[r], sI[r]);
    }
  }
}

// One row's candidates, by the G workgroups the row is split over (this one is the g-th): the
// body of k_sample_topk (one row, G = the grid) and of k_sample_topk_rows (G workgroups per row,
// one ws block per row).  The result is the best kk of the row under the total order above, so it
// depends neither on G nor on which workgroup walks which span.  ws: the row's TOPK_WS_BYTES, its
// first word zero (left zero).  Called by the whole workgroup.
__device__ __forceinline__ void tk_row(const float *__restrict__ x, int n, const int32_t *win, int nw, double scale,
                                       double penalty, int k, double *__restrict__ val, int32_t *__restrict__ id,
                                       unsigned char *ws, int g, int G) {
  __shared__ uint32_t bm[TK_SPAN / 32];
  __shared__ unsigned long long sK[TK_T];
  __shared__ uint32_t sI[TK_T];
  __shared__ int s_last;
  // (the callers checked the limits; a block holding anything else must still stay in bounds)
  const int kk = k < 1 ? 1 : k > VSIM_TOPK_MAX ? VSIM_TOPK_MAX : k;
  nw = nw < 0 ? 0 : nw > VSIM_WINDOW_MAX ? VSIM_WINDOW_MAX : nw;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned *cnt = (unsigned *)ws;
  unsigned long long *wK = (unsigned long long *)(ws + 256);
  uint32_t *wI = (uint32_t *)(ws + 256 + (size_t)TOPK_MAX_WG * 64 * sizeof(unsigned long long));

  // spans of S <= 8192 consecutive ids, dealt round-robin: one per workgroup while the
  // workgroup's share fits a span, else the share in equal spans
  const long long per = (((long long)n + G - 1) / G + 255) & ~255ll;
  const long long nsp = (per + TK_SPAN - 1) / TK_SPAN;
  const int S = (int)(((per + nsp - 1) / nsp + 255) & ~255ll);
  const long long nspan = ((long long)n + S - 1) / S;
  unsigned long long LK = 0;
  uint32_t LI = TK_ID;
  for (long long c = g; c < nspan; c += G) {
    const long long base = c * S;
    const int len = n - base < S ? (int)(n - base) : S;
    if (tid < S / 32) bm[tid] = 0;
    __syncthreads();
    for (int j = tid; j < nw; j += TK_T) {
      const long long t = (long long)win[j] - base;
      if (t >= 0 && t < len) atomicOr(&bm[t >> 5], 1u << (t & 31));
    }
    __syncthreads();
    for (int o = wave * 64; o < len; o += TK_T) {
      const int i = o + lane;
      unsigned long long ck = 0;
      uint32_t ci = TK_ID;
      if (i < len) {
        const bool in = (bm[i >> 5] >> (i & 31)) & 1u;
        ck = tk_key(tk_cand(x[base + i], in, scale, penalty));
        ci = (uint32_t)(base + i) | (in ? TK_INWIN : 0u);
      }
      tk_merge(LK, LI, ck, ci, kk);
    }
    __syncthreads();  // the bitmap is rebuilt for the next span
  }

  // the workgroup's list
  tk_merge_waves(LK, LI, sK, sI);
  if (wave == 0) {
    // The hand-off is the first row of MI355X_MICROARCH.md's sc1 hand-off table, as k_argmax's: the
    // one storing wave writes its list with device-coherent (sc1) stores and drains them
    // (vmcnt(0)); then one lane adds to the row's unsharded counter.  The workgroup whose add
    // returns G - 1 reads the row's lists with sc1 loads, the adding wave after its add returned,
    // the other waves behind the workgroup barrier below.  Nobody waits for anybody.
    __hip_atomic_store(&wK[g * 64 + lane], LK, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&wI[g * 64 + lane], LI, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (lane == 0)
      s_last = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)G - 1;
  }
  __syncthreads();
  if (!s_last) return;

  // the row's last workgroup: wave w merges lists w, w + 16, ..; then the waves as above
  LK = 0;
  LI = TK_ID;
  for (int q = wave; q < G; q += TK_WAVES) {
    const int r = q * 64 + 63 - lane;  // the list worst first
    const unsigned long long ck = __hip_atomic_load(&wK[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t ci = __hip_atomic_load(&wI[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    tk_merge_sorted(LK, LI, ck, ci);
  }
  tk_merge_waves(LK, LI, sK, sI);
  if (wave != 0) return;
  if (lane < kk) {
    int i = (int)(LI & TK_ID);
    if (i >= n) i = n - 1;  // (k <= n: never a "none" entry; stays in bounds whatever the block held)
    val[lane] = tk_cand(x[i], (LI & TK_INWIN) != 0, scale, penalty);
    id[lane] = i;
  }
  if (lane == 0) __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(TK_T)
    k_sample_topk(const float *__restrict__ x, int n, const TopkParams *__restrict__ pb, const int32_t *win, int nw,
                  double scale, double penalty, int k, double *__restrict__ val, int32_t *__restrict__ id,
                  unsigned char *ws) {
  if (pb) {
    win = pb->win;
    nw = pb->nw;
    scale = pb->scale;
    penalty = pb->penalty;
    k = pb->k;
  }
  tk_row(x, n, win, nw, scale, penalty, k, val, id, ws, blockIdx.x, gridDim.x);
}

// B rows in one launch: grid (G, B), workgroup (g, b) is the g-th of row b's G.  Row b reads
// x + b * ldx and pb[b], writes out[b] and hands off through its own block of ws; the rows share
// nothing, so a row's result is k_sample_topk's of that row alone.
__global__ void __launch_bounds__(TK_T)
    k_sample_topk_rows(const float *__restrict__ x, long long ldx, int n, const TopkParams *__restrict__ pb,
                       TopkOut *__restrict__ out, unsigned char *ws) {
  const int b = blockIdx.y;
  const TopkParams *p = pb + b;
  tk_row(x + (size_t)b * ldx, n, p->win, p->nw, p->scale, p->penalty, p->k, out[b].val, out[b].id,
         ws + (size_t)b * TOPK_WS_BYTES, blockIdx.x, gridDim.x);
}

int launch_topk(const float *x, int n, const TopkParams *pb, const int32_t *win, int nw, double scale, double penalty,
                int k, double *val, int32_t *id, void *ws, hipStream_t s) {
  if (!x || !val || !id || !ws || n < 1) { set_error("topk: bad argument"); return VSIM_EINVAL; }
  if (!pb) {
    const int kmax = n < VSIM_TOPK_MAX ? n : VSIM_TOPK_MAX;
    if (k < 1 || k > kmax) {
      set_error("topk: k must be in 1..min(n, " + std::to_string(VSIM_TOPK_MAX) + ")");
      return VSIM_EINVAL;
    }
    if (nw < 0 || nw > VSIM_WINDOW_MAX || (nw > 0 && !win)) {
      set_error("topk: window must hold 0.." + std::to_string(VSIM_WINDOW_MAX) + " ids");
      return VSIM_EINVAL;
    }
  }
  int g = (n + 1023) / 1024;
  g = g < 1 ? 1 : g > TOPK_MAX_WG ? TOPK_MAX_WG : g;
  hipLaunchKernelGGL(k_sample_topk, dim3(g), dim3(TK_T), 0, s, x, n, pb, win, nw, scale, penalty, k, val, id,
                     (unsigned char *)ws);
  VSIM_HIP(hipGetLastError());
  return VSIM_OK;
}

static std::atomic<int> g_rows_wg{0};
int topk_rows_set_wg(int per_row) {
  return g_rows_wg.exchange(per_row < 0 ? 0 : per_row > TOPK_MAX_WG ? TOPK_MAX_WG : per_row);
}

int launch_topk_rows(const float *x, int ldx, int n, int B, const TopkParams *pb, TopkOut *out, void *ws, hipStream_t s) {
  if (!x || !pb || !out || !ws || n < 1 || ldx < n || B < 1 || B > VSIM_BATCH_MAX) {
    set_error("topk_rows: bad argument (1 <= B <= " + std::to_string(VSIM_BATCH_MAX) + ", 1 <= n <= ldx)");
    return VSIM_EINVAL;
  }
  // Workgroups per row: k_sample_topk's (1024 ids each, at most 64) while all rows' together are
  // at most one per CU; beyond that the rows supply the parallelism and a workgroup walks a longer
  // share, which costs it little (after its first batches few candidates pass the k-th entry)
  // while every workgroup less is a list less to hand off and merge.  Measured at 32 rows
  // (profiles/batch_sample_bench.txt): 8 per row beat 16, 32 and 64 at n = 50,400 and 250,880.
  // topk_rows_set_wg overrides (same results: tk_row).
  int g = (n + 1023) / 1024;
  g = g < 1 ? 1 : g > TOPK_MAX_WG ? TOPK_MAX_WG : g;
  const int fixed = g_rows_wg.load();
  if (fixed > 0)
    g = g < fixed ? g : fixed;
  else if (B * g > TOPK_ROWS_WG)
    g = TOPK_ROWS_WG / B;  // >= 8
  hipLaunchKernelGGL(k_sample_topk_rows, dim3(g, B), dim3(TK_T), 0, s, x, (long long)ldx, n, pb, out,
                     (unsigned char *)ws);
  VSIM_HIP(hipGetLastError());
  return VSIM_OK;
}

}  // namespace vsim
