/* include/vsim_hip.h — C-ABI of libvsim_hip.so, the MI355X (gfx950) replacement for the
 * reference's imax.c / emax7lib.c offload layer.
 *
 * Three layers, all plain C types (no torch / HIP types in any signature):
 *
 *  1. Drop-in entry points with the reference's own symbol names and signatures, so a
 *     reference build links libvsim_hip.so where it linked imax.o:
 *       init_xmax()                                   replaces imax.c:52-142
 *       imax_ggml_compute_forward_mul_mat_q4_0_f32()  replaces imax.c:1133-2292
 *                                                     (called from ggml.c:5115)
 *     plus vsim_ggml_* hooks for the ops that have no offload boundary in the reference
 *     (RoPE ggml.c:6086/5919, soft_max ggml.c:5825, KQ/KQV mul_mat ggml.c:4355).
 *  2. Op-level device API (vsim_op_*): every hot op on device pointers, in the exact
 *     (reference-bit-identical) or fast numeric mode.  Used by the parity tests.
 *  3. Model-level executor (vsim_model_*): device-resident GPT-NeoX (vsim.cpp:470-747)
 *     and GPT-J graphs, whole decode step captured in a hipGraph; host<->device traffic
 *     per token is the token ids in and one logits row out (vsim.cpp:736-737), or, for the
 *     greedy and the sampled step, a token id or at most 64 (value, id) candidates out.
 *  plus the sampler object (vsim_sampler_*): the reference's sampler with its O(n_vocab)
 *     stage on the device,
 *  and the model quantizer (vsim_op_q4_quantize_w, vsim_model_load_file_ex,
 *     vsim_model_set_tensor_src, vsim_quantize_file): the converters' F32 / F16 files to Q4_0
 *     with the semantics of the reference's quantize_* tools, while loading or file to file.
 *
 * Device weight layout ("W4T32"): a Q4_0 matrix of M rows x K weights keeps the
 * reference's 0.625 B/weight but splits the 20-byte blocks (ggml.c:204-251) into a
 * 16-byte nibble plane followed by an fp32 scale plane, with rows grouped in tiles of 32
 * and, inside a tile, block b of all 32 rows stored contiguously (512 B of nibbles,
 * 128 B of scales) so row-per-lane waves read whole cache lines.  M is padded to a
 * multiple of 32: vsim_q4_bytes(M, K) = ceil(M/32)*32 * K/32 * 20 bytes.
 * Activation rows (vsim_op_q4_quantize output, "Q4 SoA"): nibble plane [n][K/32][16] then
 * scale plane [n][K/32], n*K/32*20 bytes.
 *
 * Every function returns 0 on success or a negative VSIM_E* code; vsim_last_error()
 * describes the last failure of the calling thread.
 */
#ifndef VSIM_HIP_H
#define VSIM_HIP_H

#include <stddef.h>
#include <stdint.h>

#include "ggml_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VSIM_OK 0
#define VSIM_EINVAL (-1)
#define VSIM_EHIP (-2)
#define VSIM_ENOMEM (-3)
#define VSIM_EFILE (-4)
#define VSIM_ENODEV (-5)
#define VSIM_ESPIN (-6) /* a bounded cross-workgroup wait inside a fused kernel gave up: the
                           call's results are not valid (vsim_spin_timeouts counts them)  */

/* numeric modes */
#define VSIM_MODE_EXACT 0 /* bit-identical to the reference at --threads 1            */
#define VSIM_MODE_FAST 1  /* split-K integer-dot GEMV: same math, different rounding  */
#define VSIM_MODE_W4A16 2 /* weight-only: Q4_0 weights, activation rows rounded to fp16 (not
                             quantized), fp32 accumulation -- not the reference's arithmetic;
                             see vsim_op_q4_gemm_w4a16_rows and vsim_model_set_mode          */

/* architectures */
#define VSIM_ARCH_GPTNEOX 0 /* vsim.cpp:470-747                                      */
#define VSIM_ARCH_GPTJ 1    /* ggml GPT-J graph composed from the same ops           */
#define VSIM_ARCH_BLOOM 2   /* BLOOM graph (ALiBi, fused QKV) composed from the same ops
                               + ggml_alibi (ggml.c:6184-6244); convert_bloom_to_ggml.py */

const char *vsim_last_error(void);
int vsim_device_count(void);
size_t vsim_q4_bytes(int rows, int k);

/* ---------------------------------------------------------------- 1. drop-in ----- */
void init_xmax(void);
void imax_ggml_compute_forward_mul_mat_q4_0_f32(int THREAD, int LANE, const struct ggml_compute_params *params,
                                                const struct ggml_tensor *src0, const struct ggml_tensor *src1,
                                                struct ggml_tensor *dst);
/* New hooks (same (params, src0, src1, dst) shape as the static ggml.c kernels they
 * replace; host tensors in, host tensors out, exact mode).  Called by every thread of the
 * reference's pool in every phase: the checks read metadata only, so all threads agree -
 * either every call returns VSIM_EINVAL (each thread runs its own CPU slice) or thread 0's
 * COMPUTE call runs the whole op and every call returns 0 (handled; INIT / FINALIZE have
 * nothing left to do).  mul_mat_f32 takes any strided F32 views; its transposed-src0 branch
 * (KQV) groups the partial sums by params->nth as ggml.c:4535-4581 + 4469-4493 does.  A
 * device failure after the checks exits, as the offload layer does (imax.c:2042-2049). */
int vsim_ggml_gptneox_rope_f32(const struct ggml_compute_params *params, const struct ggml_tensor *src0,
                               const struct ggml_tensor *src1, struct ggml_tensor *dst);
int vsim_ggml_rope_f32(const struct ggml_compute_params *params, const struct ggml_tensor *src0,
                       const struct ggml_tensor *src1, struct ggml_tensor *dst);
int vsim_ggml_soft_max_f32(const struct ggml_compute_params *params, const struct ggml_tensor *src0,
                           struct ggml_tensor *dst);
int vsim_ggml_mul_mat_f32(const struct ggml_compute_params *params, const struct ggml_tensor *src0,
                          const struct ggml_tensor *src1, struct ggml_tensor *dst);
/* Device executor for the reference's graph: the drop-in for ggml_graph_compute
 * (ggml.c:8245-8700, called at vsim.cpp:725 as ggml_graph_compute(ctx0, &gf)).  Walks
 * cgraph->nodes[] in order on the GPU with the exact-mode kernels; the eval context's arena
 * (ctx's mem_buffer) and every leaf outside it (model weights, KV cache: mirrored once, then
 * device-resident) are mirrored at the same offsets, and the last node's bytes are copied
 * back to its host address.  The KQV product's thread-partial grouping follows
 * cgraph->n_threads, so the logits equal the reference's at any --threads.
 * vsim_graph_compute prints the error and exits (as the reference's offload layer does,
 * imax.c:2042-2049); vsim_graph_compute_rc returns VSIM_E* instead and leaves host memory
 * untouched when a node is not supported (all nodes are checked before any runs).
 * The parameter tensors of scale (the factor), diag_mask_inf (n_past), rope and gptneox_rope
 * ({n_past, n_dims, mode}) are read from host memory when the node is enqueued, so they must be
 * leafs (op NONE): one that is itself a node of the graph is refused with VSIM_EINVAL
 * ("parameter must be a leaf"), where the reference would read it at compute time. */
void vsim_graph_compute(struct ggml_context *ctx, struct ggml_cgraph *cgraph);
int vsim_graph_compute_rc(struct ggml_context *ctx, struct ggml_cgraph *cgraph);
/* copy one tensor of the last computed graph back to its host address */
int vsim_graph_sync_tensor(const struct ggml_tensor *t);
/* forget every mirror (weights, KV cache, arena) */
void vsim_graph_reset(void);
void vsim_graph_stats(uint64_t *computes, uint64_t *nodes, uint64_t *h2d_bytes, uint64_t *d2h_bytes);
/* per-op device time (event pair per node; also VSIM_GRAPH_PROFILE=1): enable resets the
 * totals; the report is a text table with the reference's monitor.c row names
 * (monitor.c:182-262, show_time_sep).  Returns the report's full length. */
int vsim_graph_set_profile(int enable);
int vsim_graph_profile_report(char *buf, size_t cap);
/* Decode fast path of vsim_graph_compute.  A single-token eval of gptneox_eval
 * (vsim.cpp:470-747, use_parallel_residual = 1) is recognised node by node (42 nodes per
 * layer in ggml_build_forward_expand order, plus get_rows and the final norm + lm_head) and
 * runs as the model executor's fused decode step -- 2 launches per layer (since r06), replayed as one
 * hipGraph -- on the weights and KV cache the per-node path mirrored, with the KQV grouping of
 * cgraph->n_threads.  Every other graph (prompt batches, the serial residual) runs per node.
 * VSIM_GRAPH_FAST=0 turns the fast path off.
 * vsim_graph_match checks a graph on the host only (no device needed): 0 and the recognised
 * shape in `info`, or VSIM_EINVAL with the first mismatch in vsim_last_error(). */
typedef struct {
  int32_t n_layer, n_embd, n_head, n_rot, n_vocab, n_ctx, n_past, token;
} vsim_graph_match_info;
int vsim_graph_match(const struct ggml_cgraph *cgraph, vsim_graph_match_info *info);
/* evals that took the fast path, and fast-path plans built (one per set of weight tensors) */
void vsim_graph_fast_stats(uint64_t *fast_evals, uint64_t *plans);
/* drop-in statistics: calls, bytes moved host<->device, device weight-cache size */
void vsim_dropin_stats(uint64_t *calls, uint64_t *h2d_bytes, uint64_t *d2h_bytes, uint64_t *cached_bytes);
void vsim_dropin_reset(void);

/* ------------------------------------------------------- 2. op-level (device ptrs) -- */
/* `stream` is a hipStream_t passed as void* (NULL = default stream). */
/* weights: ggml AoS blocks <-> W4T32 */
int vsim_op_q4_repack(const void *aos, void *w, int rows, int k, void *stream);
int vsim_op_q4_unpack(const void *w, void *aos, int rows, int k, void *stream);
/* activation rows: ggml AoS blocks <-> Q4 SoA */
int vsim_op_act_repack(const void *aos, void *xq, int n, int k, void *stream);
int vsim_op_act_unpack(const void *xq, void *aos, int n, int k, void *stream);
/* quantize_row_q4_0 (ggml.c:209-251) of n rows of k floats: xq in Q4 SoA, xd = the
 * dequantized values d*(q-8) the exact GEMV multiplies with (ggml.c:497-498). */
int vsim_op_q4_quantize(const float *x, int k, int n, void *xq, float *xd, void *stream);
/* The model quantizer's kernel (k_quantize_w): ggml_quantize_q4_0 (utils.cpp:425-482, as
 * quantize_gptneox.cpp:143-311 drives it) of `rows` rows of k F32 or F16 weights, x a row-major
 * device buffer (16-byte aligned, k % 32 == 0; F16 is widened exactly, subnormals kept).
 *   w     W4T32 target: an existing weight of w_rows rows x k, of which rows [row0, row0 + rows)
 *         are written (row0 % 32 == 0), so a tensor can be quantized in row chunks.  The chunk
 *         that ends the tensor (row0 + rows == w_rows) also writes the last tile's padding rows
 *         as vsim_op_q4_repack does (d = 0, nibbles 0x88).  May be NULL.
 *   aos   the file format: rows * k/32 row-major 20-byte blocks of this chunk.  May be NULL.
 *   hist  16 device words the caller zeroes: hist[code] += 1 for every weight of the chunk
 *         (padding rows are never counted; integer adds, so the order does not matter).  May be NULL.
 * w and aos may both be given; one of them must be.  VSIM_EINVAL for k % 32 != 0, row0 % 32 != 0,
 * row0 + rows > w_rows, both targets NULL, a bad src_type or a misaligned pointer.  Enqueued on
 * stream, not synchronized.
 * The one difference from vsim_op_q4_quantize (quantize_row_q4_0): the weight quantizer takes
 * amax with std::max(amax, fabsf(v)), under which a NaN weight is IGNORED -- the block keeps the
 * d of its other values and the NaN element gets code 8 -- where the activation quantizer's MAX
 * macro lets a NaN replace the running maximum.  A +-Inf weight gives d = inf and every code 8; a
 * block whose d is so small that 1/d overflows gives every code 8 (the x86 cast of inf and NaN). */
#define VSIM_SRC_F32 0
#define VSIM_SRC_F16 1
int vsim_op_q4_quantize_w(const void *x, int src_type, int rows, int k, void *w, int w_rows, int row0, void *aos,
                          uint64_t *hist, void *stream);
/* y[n][M] = W[M][K] . q4_0(x)[n][K] (+ bias[M] if bias != NULL, added after the dot
 * as ggml_add does, vsim.cpp:545-547) */
int vsim_op_q4_gemv(const void *w, int M, int K, const void *xq, const float *xd, int n, const float *bias,
                    float *y, int mode, void *stream);
/* The batched decode step's product (k_gemm_exact_rows, exact mode only): y[n][M] for n = 1 ..
 * VSIM_BATCH_MAX activation rows, every (weight row, activation row) the reference's chain --
 * sumf = sumf + (f0*f2 + f1*f3) per byte pair in block order, each product and sum rounded on its
 * own, the bias added after -- hence bit for bit vsim_op_q4_gemv(..., VSIM_MODE_EXACT) on the same
 * operands, row by row, whatever n is.  Each weight block is fetched and dequantized once per
 * workgroup (16 weight rows) for all n rows, where the GEMV streams the weight once per four rows.
 * xd: vsim_op_q4_quantize's factors [n][K].  VSIM_EINVAL for n outside 1..VSIM_BATCH_MAX,
 * K % 32 != 0 or a NULL xd.  Enqueued on stream, not synchronized. */
#define VSIM_BATCH_MAX 32
int vsim_op_q4_gemm_rows(const void *w, int M, int K, const float *xd, int n, const float *bias, float *y,
                         void *stream);
/* Process-wide choice of the product kernel of vsim_model_decode_batch: 0: vsim_op_q4_gemv's
 * dispatch, as a short prompt's products take it (chain-GEMV jobs, four rows per launch); 1
 * (default): k_gemm_exact_rows from B = 12 rows on, the GEMV jobs below, which is where each was
 * measured faster (profiles/batch_decode_bench.txt); 2: k_gemm_exact_rows at every B.  All three
 * give the same bits.  Other values select 1.  Returns the previous value. */
int vsim_batch_set_gemm(int enable);
/* The fast batched decode step's product (k_gemm_fast_rows): y[n][M] = W[M][K] . q4_0(x)[n][K]
 * (+ bias) for n = 1 .. VSIM_BATCH_MAX activation rows, every weight block fetched and unpacked once
 * per workgroup (16 weight rows) for all n rows.  Contract: each output is bit for bit what
 * vsim_op_q4_gemv(..., n = 1, VSIM_MODE_FAST) gives for that (weight row, activation row) alone,
 * whatever n is and whatever rows stand beside it:
 *   isum_b  = the exact integer dot of block b's 32 (nibble - 8) pairs (formed on the i8 matrix
 *             core here, with v_dot8_i32_i4 there: an integer either way);
 *   part[p] = 0.0f; for b = p, p + 16, p + 32, ... < K/32:
 *               part[p] = fmaf(d_w[b] * d_x[b], (float)isum_b, part[p])     (p = 0 .. 15; the scale
 *             product rounded to fp32 first; a partial with no block stays +0);
 *   sum     = 0.0f; for p = 0 .. 15: sum += part[p];
 *   y       = bias ? sum + bias[row] : sum.
 * xq: vsim_op_q4_quantize's Q4 SoA rows (nibbles [n][K/32][16], then scales [n][K/32]).  The weight
 * is W4T32 and needs no VSIM_FAST_PAD behind it; activation rows >= n are not read and y rows >= n
 * not written.  VSIM_EINVAL for n outside 1..VSIM_BATCH_MAX, K % 32 != 0, M <= 0 or a NULL w, xq
 * or y.  Enqueued on stream, not synchronized. */
int vsim_op_q4_gemm_fast_rows(const void *w, int M, int K, const void *xq, int n, const float *bias, float *y,
                              void *stream);
/* ---- weight-only mode (VSIM_MODE_W4A16): the row operand and the product (gemm_w4a16_rows.hip).
 * Every product of the mode is these two kernels; everything that is not a product stays the exact
 * path's kernel.
 *
 * Row operand (k_w4a16_rows).  For each of n rows x[K] (f32), on its own:
 *   amax = the largest |x[i]| among the row's finite elements (f32 subnormals count as they are);
 *   e    = 14 - floor(log2(amax)): the integer that puts amax * 2^e into [2^14, 2^15); e = 0 for
 *          an all-zero row (-0.0 is zero);
 *   h[i] = fp16_rn(x[i] * 2^e): the scaling is exact, the conversion rounds to nearest even; no
 *          finite row overflows fp16.  Elements more than 2^28 or so below amax become fp16
 *          subnormals (kept as such in x16, multiples of 2^-24) or signed zeros.
 * Subnormal rule: gfx950's v_mfma_f32_16x16x32_f16 takes fp16 subnormal A / B inputs at their value
 * (it does not flush them; measured, tests/test_gpu_w4a16_ops.py), so the product below uses every h
 * as stored.
 * Non-finite rule: a row that holds a NaN or an Inf gets e = VSIM_W4A16_NONFINITE and h = +0
 * throughout, and every output of that row is the quiet NaN 0x7FC00000.  No other row is touched.
 * x16 [n][K] halves (16-byte aligned), e [n]; x at any 4-byte alignment (16-byte aligned rows of up
 * to 16,384 elements take a faster form of the kernel, same bits).  One launch per distinct operand: Q, K and V share
 * theirs.
 *
 * Product (k_gemm_w4a16_rows): y[n][M] for n = 1 .. VSIM_BATCH_MAX rows against a W4T32 weight, every
 * weight block fetched and unpacked once per workgroup (16 weight rows) for all n rows.  Per
 * (weight row, activation row), with nb = K / 32:
 *   dot_b   = the matrix core's sum, from C = 0, of block b's 32 products (q - 8) * h (each exact
 *             in fp32; the order of the 32 adds is the instruction's, fixed);
 *   part[p] = 0.0f; for b = p, p + 16, p + 32, ... < nb:
 *               part[p] = fmaf(d_w[b], dot_b, part[p])          (p = 0 .. 15; no block: stays +0);
 *   sum     = 0.0f; for p = 0 .. 15: sum += part[p];
 *   s       = sum * 2^-e                (exact, unless s is an f32 subnormal: then rounded once);
 *   y       = bias ? s + bias[row] : s.
 * Contract (a), row independence, bit for bit: output (j, m) depends on activation row j and weight
 * row m only -- not on n, on j's index in the launch or on the other rows.
 * Contract (b): against the same formula evaluated in double on the same h,
 *   |y - y64| <= c(K) 2^-24 sum_b |d_w[b]| sum_i |q_i - 8| |h_i| 2^-e  (+ the bias add's rounding,
 *   + 2^-149 where s is subnormal),  c(K) = 32 + ceil(nb / 16) + 16 + 1
 * (32 adds inside the MFMA, the partial's fmas, the partial adds, one unit for the second-order
 * terms: tests/w4a16_ref.py derives it).
 * Activation rows >= n are not read, y rows >= n not written, nothing behind the weight is read.
 * VSIM_EINVAL for n outside 1..VSIM_BATCH_MAX, K % 32 != 0, M <= 0 or a NULL w, x, x16, e or y (bias
 * may be NULL).  Both are enqueued on stream and not synchronized. */
#define VSIM_W4A16_NONFINITE (-2147483647 - 1)
int vsim_op_w4a16_rows(const float *x, int K, int n, void *x16, int32_t *e, void *stream);
int vsim_op_q4_gemm_w4a16_rows(const void *w, int M, int K, const void *x16, const int32_t *e, int n,
                               const float *bias, float *y, void *stream);
/* vsim_op_q4_gemm_w4a16_tile (k_gemm_w4a16_tile): the same product for any n >= 1 in one launch, tiled
 * over 64 (or 32) weight rows x 64 activation rows per workgroup, so that the weight streams once
 * per 64 activation rows.  y [n][M] is bit for bit vsim_op_q4_gemm_w4a16_rows on consecutive chunks
 * of 32 rows: the formula above per (weight row, activation row) pair -- the same MFMA from C = 0
 * per block, the same sixteen fma strands, the same ordered sum -- with contracts (a) and (b), the
 * NaN rule and the read and write limits unchanged.  It always runs the tile kernel
 * (vsim_w4a16_set_tile_gemm does not apply to it).  VSIM_EINVAL as vsim_op_q4_gemm_w4a16_rows, without
 * the upper limit on n. */
int vsim_op_q4_gemm_w4a16_tile(const void *w, int M, int K, const void *x16, const int32_t *e, int n,
                               const float *bias, float *y, void *stream);
/* Process-wide choice of how the products of a weight-only prompt batch (vsim_model_eval at N > 1,
 * _eval_seq, _eval_score) run: 0: k_gemm_w4a16_rows on chunks of 32 rows at every N (the weight
 * streams once per chunk); 1 (default): k_gemm_w4a16_tile from the smallest N where it was measured
 * faster by more than 5 % (profiles/w4a16_prompt_bench.txt), the chunks below; 2: k_gemm_w4a16_tile
 * at every N.  All three give the same bits.  The batched step (vsim_model_decode_batch_w4a16) and
 * the single-token step are not affected.  Other values select 1.  Returns the previous value. */
int vsim_w4a16_set_tile_gemm(int v);
/* ---- weight-only mode: the fp16 MFMA attention (attn_w4a16.hip), opt-in.
 *
 * vsim_w4a16_set_attn: process-wide switch.  0 (default): the mode's attention is the exact path's
 * (KQ with double sums, the fp16-table softmax, the KQV float chains).  1: on a graph without ALiBi
 * with head dim 64, 96, 128 or 256 and n_embd a multiple of 64, every path of a weight-only model
 * -- prompt, slot, vsim_model_eval_score, the batched step, the single-token step -- at every N runs
 * the attention below; any other model, and exact and fast mode, are not affected.  The setting
 * changes the mode's bits, not its promise (vsim_model_set_mode): a row's logits are the same bits
 * on every path.  Other values select 0.  Models drop their captured step graphs when they next
 * run after a change.  Returns the previous value.
 *
 * The contract, per row (a formula, not a kernel).  One head of D dims, a query at absolute
 * position p, keys 0..p of that sequence's fp32 cache:
 *   q16 = fp16(float32(q) * qs), qs = float32(scale) * float32(log2 e); k16 = fp16(k), v16 = fp16(v);
 *   key blocks of 64 aligned to key 0 (not to n_past, not to the batch), visited 0, 1, ..., p / 64
 *   and no others; per block S = K16 . q16 on v_mfma_f32_32x32x16_f16, chained over D / 16 steps
 *   from C = 0, keys the A rows, queries the B columns; keys past p are left out of the maximum and
 *   get p_k = 0 exactly; m' = max(m, block max), alpha = exp2f(m - m'), p_k = exp2f(s_k - m');
 *   l = l alpha + sum p_k (the lane's keys in register order, then the other half-wave's sum);
 *   O = O alpha, then O += V16^T . fp16(P)^T on the same MFMA, k-steps in key order;
 *   y = O / l + 0.0f.
 * Nothing a row's result depends on comes from another row: not its wave's other queries, not N,
 * n_past, B, the slot, or cache rows past p.  Both entries run the same device code per 32-query
 * group x 64-key block.  RoPE of q and of the new k, the fp32 cache write and the out-projection's
 * operand (vsim_op_w4a16_rows over the whole attention row) stay the exact path's, bits included.
 *   Stale cache rows: a slot's rows past p may hold NaN or Inf, and 0 x NaN inside the P.V MFMA is
 *   NaN.  Rule: the V operand of a key past the sequence's last key is zero and its K operand is the
 *   last key's row; its score is masked whatever it is.
 *   Sign of zero: the prompt form runs a key block for every query of a wave when one of them sees
 *   it, which adds +0 to O of a row that sees none of it and turns a -0 into +0; masked keys inside
 *   a row's last block do the same through p x v.  Only the sign of an O that ends as zero can differ.
 *   Rule: canonical zero -- both forms add + 0.0f after the division; y is never -0.
 * Accuracy: tests/attn_ref.py's bound (c 2^-11 A + T, and 2e-2 max|V| against fp64).
 *
 * vsim_op_attn_w4a16_prompt (k_kv_f16 + k_attn_w4a16_tile): N >= 1 queries Q [N][H d] (after RoPE) at
 * positions n_past .. n_past + N - 1 over the cache rows kc, vc [n_past + N][H d]; out [N][H d].
 * scratch: vsim_op_attn_prefill_layout(H d, n_past + N)'s bytes, in its layout (required).
 * VSIM_EINVAL for another head dim, H d % 64, N < 1, n_past < 0, a NULL or a short scratch.
 *
 * vsim_op_attn_w4a16_rows (k_attn_w4a16_rows): B rows, one new token each, every row on a cache and
 * at a position of its own, arguments as vsim_op_attn_decode_batch's.  Per row and head: RoPE and the
 * K / V cache row exactly as that entry writes them (no row past p is written), then the attention
 * above over the row's fp32 cache, each 64-key block converted to fp16 on the fly; no LDS score row,
 * so n_ctx does not bound it.  a->out is required; a->oq, a->oxd and a->alibi must be NULL;
 * a->kqv_nth is ignored.  VSIM_EINVAL for another head dim, H d % 64, B outside 1..VSIM_BATCH_MAX or a
 * missing pointer.  Both are enqueued on stream, not synchronized (the rows entry waits when it has
 * to build the RoPE table itself, as vsim_op_attn_decode_batch does). */
int vsim_w4a16_set_attn(int v);
int vsim_op_attn_w4a16_prompt(const float *Q, const float *kc, const float *vc, int d, int H, int N, int n_past,
                              float scale, float *out, void *scratch, size_t scratch_bytes, void *stream);
/* ---- weight-only mode: the kernels of the single-token step (w4a16_decode.hip).  Each is, bit for
 * bit, a composition of entries above on the same row; none has a tolerance of its own.
 *
 * vsim_op_w4a16_ln (k_w4a16_ln): for one row x[n],
 *   (x16_1, e1) = vsim_op_w4a16_rows(vsim_op_norm(x, w1, b1)), and, when the second norm is given,
 *   (x16_2, e2) = vsim_op_w4a16_rows(vsim_op_norm(x, w2, b2)) as a second workgroup of the launch.
 * The f32 norm row is not written anywhere.  The maximum behind e is taken over the affine's outputs
 * w y + b.  vsim_norm_fallbacks counts what vsim_op_norm would count for the same rows (each norm
 * counts on its own).  VSIM_EINVAL: n not a positive multiple of 32 or beyond 16,384 (the LDS row,
 * vsim_op_norm's limit); a NULL x, w1, b1, x16_1 or e1; a second norm with some but not all of w2, b2,
 * x16_2, e2; x, an affine vector or an operand not 16-byte aligned. */
typedef struct {
  const float *x; /* [n] */
  int32_t n;
  const float *w1, *b1;
  void *x16_1; /* [n] halves */
  int32_t *e1;
  const float *w2, *b2; /* all four NULL: one norm */
  void *x16_2;
  int32_t *e2;
} vsim_w4a16_ln_args;
int vsim_op_w4a16_ln(const vsim_w4a16_ln_args *a, void *stream);
/* vsim_op_w4a16_gelu (k_w4a16_gelu): for one row x[K],
 *   g[i] = fp16->fp32(table_gelu_f16[fp32->fp16(x[i] + bias[i])])   (vsim_op_gelu; bias NULL: no add),
 *   (x16, e) = vsim_op_w4a16_rows(g), and g itself to g_or_null when given.
 * The maximum behind e is taken over g, not over x + bias; a row whose g is all zero gets e = 0; an
 * x + bias beyond fp16 range reads the table's entry for +-inf, which is not finite, so such a row
 * is VSIM_W4A16_NONFINITE although its input is finite.  K of any size (rows up to 24,576 keep g in registers, longer rows make it
 * twice; same bits).  VSIM_EINVAL: K not a positive multiple of 32; a NULL x, x16 or e; x, bias, x16
 * or g not 16-byte aligned. */
int vsim_op_w4a16_gelu(const float *x, const float *bias, int K, void *x16, int32_t *e, float *g_or_null,
                       void *stream);
/* vsim_op_w4a16_gemv (k_gemv_w4a16): nj = 1..4 products in one launch, each of a W4T32 weight
 * w [M][K] with a single-row operand (x16, e) of its own.  Per job, with
 *   v = vsim_op_q4_gemm_w4a16_rows(w, M, K, x16, e, n = 1, bias)      (bit for bit, NaN rule included),
 *   y = v                      (res NULL),
 *   y = v + res                (res alone),
 *   y = res + (res_a + v)      (res and res_a; both orders are the residual joins' of the model).
 * A thread reads only the res / res_a elements it writes, so y may be res.  A job's outputs do not
 * depend on the jobs beside it.  Nothing past M is written or read of bias, res, res_a and y, nothing
 * past K of x16, nothing behind the weight.  VSIM_EINVAL: nj outside 1..4; a job with K not a positive
 * multiple of 32, M <= 0, or a NULL w, x16, e or y; res_a without res; w or x16 not 16-byte aligned.
 * All three are enqueued on stream and not synchronized. */
typedef struct {
  const void *w; /* W4T32 [M][K] */
  int32_t M, K;
  const void *x16; /* [K] halves */
  const int32_t *e;
  const float *bias, *res, *res_a; /* [M] each, or NULL */
  float *y;                        /* [M] */
} vsim_w4a16_gemv_job;
typedef struct {
  vsim_w4a16_gemv_job j[4];
  int32_t nj;
} vsim_w4a16_gemv_args;
int vsim_op_w4a16_gemv(const vsim_w4a16_gemv_args *a, void *stream);
/* Process-wide switch of weight-only mode's single-token step (vsim_model_set_mode): 1 (default) the
 * fused step, 0 the general path for every single-token call, as before the step existed.  Same bits
 * either way.  Models drop their captured step graphs when they next run after a change.  Returns
 * the previous value. */
int vsim_w4a16_set_step(int enable);
/* Process-wide choice of how vsim_op_q4_gemm_fast_rows and the products of
 * vsim_model_decode_batch_fast run: 0: one k_gemv_fast launch per row (the weight streams once per
 * row); 1 (default): k_gemm_fast_rows from the smallest row count where it was measured faster by
 * more than 5 % (profiles/batch_fast_bench.txt), the per-row launches below; 2: k_gemm_fast_rows at
 * every n.  All three give the same bits.  Other values select 1.  Returns the previous value. */
int vsim_batch_set_fast_gemm(int enable);
/* The batched decode step's attention (k_attn_decode_batch): B rows, one new token each, every row
 * against a KV cache and at a position of its own.  Per row and head it is the exact single-query
 * attention of the single-token step: RoPE of q and the new k at the row's position (style 0
 * rotate-half, 1 GPT-J pairs, n_rot = 0 none), the new K / V row written into the row's cache at
 * that position, KQ with a double accumulator in the reference's order (ggml.c:4760-4800), scale
 * (+ the head's ALiBi slope), soft_max with the fp16 exp table (ggml.c:5825), KQV as the
 * sequential float chain over the keys (kqv_nth > 1: the reference pool's key runs at --threads
 * kqv_nth), and quantize_row_q4_0 of the output row for the out-projection.  A row's results
 * depend on that row's operands only -- not on B or on the rows beside it.  All pointers are
 * device pointers.  Two rows must not share a cache.  d % 32 == 0, d <= 256, 1 <= B <=
 * VSIM_BATCH_MAX, n_past[b] < n_ctx, else VSIM_EINVAL (positions are read on the device and are
 * the caller's to keep in range).  Enqueued on stream, not synchronized. */
typedef struct {
  const float *q, *k, *v;   /* [B][H d]: the rows after bias, before RoPE */
  float *const *kc;         /* [B] device array: row b's key cache [n_ctx][H d] */
  float *const *vc;         /* [B] device array: row b's value cache */
  const int32_t *n_past;    /* [B] device array: row b's position */
  const double *cs;         /* RoPE table [n_ctx][n_rot/2] {cos, sin} of the angles p * 10000^(-2j/n_rot);
                               NULL with n_rot > 0: built and uploaded by the call, which then also
                               waits for the stream, as vsim_op_rope does */
  const float *alibi;       /* [H] head slopes, or NULL */
  int32_t B, d, H, n_rot, style, n_ctx, kqv_nth;
  float scale;
  float *out;               /* [B][H d] f32 output, or NULL */
  void *oq;                 /* the output as Q4 SoA rows: nibbles [B][H d/32][16], then scales [B][H d/32] */
  float *oxd;               /* [B][H d] its factors d*(q-8), pair-interleaved as vsim_op_q4_quantize's */
} vsim_attn_batch_args;
int vsim_op_attn_decode_batch(const vsim_attn_batch_args *a, void *stream);
/* weight-only mode's single-query fp16 attention on the same arguments (vsim_w4a16_set_attn above) */
int vsim_op_attn_w4a16_rows(const vsim_attn_batch_args *a, void *stream);
/* Runs of rows: the two entries above for batches whose rows may share a cache, provided the rows
 * that share one sit at distinct positions -- a run is len >= 1 consecutive tokens of one sequence as
 * len consecutive rows at positions p, p + 1, .., p + len - 1 of its cache.  Two launches on the
 * stream, no waits between workgroups: k_kv_rows does RoPE of every row's new key at the row's
 * position and writes every row's K and V cache rows (the heads' own arithmetic and bits, from one
 * shared device function), then k_attn_decode_runs / k_attn_w4a16_runs, the same heads without their
 * cache writes, RoPE q and read keys and values 0..n_past[b] of the row's cache, its own included.
 * A row never reads a cache row past its own position (the fp16 form clamps K and zeroes V there),
 * so row j of a run has bit for bit the out / oq / oxd that vsim_op_attn_decode_batch /
 * vsim_op_attn_w4a16_rows give it as the only row of a call made after rows 0..j-1 were stepped one
 * call at a time, and the cache rows written are the same.  Arguments and errors as the entry's
 * above. */
int vsim_op_attn_decode_runs(const vsim_attn_batch_args *a, void *stream);
int vsim_op_attn_w4a16_runs(const vsim_attn_batch_args *a, void *stream);
/* The same single-query attention for one row (a->B == 1) as the fused layer tail runs it: the
 * head role of k_layer_tail alone (704 threads per workgroup, write-through output stores, each
 * head over nsplit = 1 or 2 workgroups that halve its KQV columns), with neither an fc_out nor an
 * out-projection job in the launch.  The call brings its own head-flag buffer and epoch word and
 * fails with VSIM_EHIP if a head part did not raise its flag.  Arguments, outputs and bits are
 * those of vsim_op_attn_decode_batch with B = 1.  The shape must fit the fused kernel: d % 32 == 0,
 * d <= 256, (d / nsplit) % 32 == 0, H * nsplit <= 128, and q, k, the n_ctx scores and two V tiles
 * within the kernel's LDS (the model's executor fuses only up to 75264 bytes of them, n_ctx + 2 d
 * <= 2432; the kernel itself takes more, so this entry also reaches n_ctx = 2048 at d = 256);
 * else VSIM_EINVAL.
 * Unlike the batch entry this one waits for the stream before it returns. */
int vsim_op_tail_attn(const vsim_attn_batch_args *a, int nsplit, void *stream);
/* The whole fused layer tail with the next LayerNorm in it (k_layer_tail with its TailLn, what every
 * exact decode step of the parallel-residual graphs runs once per layer), on the call's operands:
 *   heads   the single-query attention of `attn` (B == 1), each head over nsplit workgroups; its Q4
 *           row attn.oq / attn.oxd (and attn.out) are outputs of this call as well;
 *   a       = wo . that row            (W4T32 [E][E], E = d H; the exact chain of vsim_op_q4_gemv)
 *   f       = wf . xd                  (W4T32 [E][K]; xd [K] the factors of vsim_op_q4_quantize)
 *   v[i]    = x[i] + ((a[i] + ab[i]) + (f[i] + fb[i]))   in float32 (ab NULL: a[i] alone) -> jout
 *   y       = ggml_compute_forward_norm_f32 of v (mean and sum of squares summed in order in double,
 *             scale (float)(1/sqrt(s2/E + 1e-5f)), y = (float)(v - mean) * scale)
 *   z1      = w1 * y + b1  (two float roundings), quantize_row_q4_0 -> q1 (Q4 SoA: nibbles [E/32][16],
 *             then scales [E/32]) and its factors xd1 [E], as vsim_op_q4_quantize's of z1;
 *   z2      likewise from the same y with w2, b2 into q2, xd2 when all four are given (none: one norm).
 * Bit for bit the reference's values; how the kernel gets there (per-tile partial sums, the mean and
 * moments certificates, the sequential fallbacks) shows only in vsim_norm_fallbacks: a launch adds at
 * most one to each counter ([0] the mean was not certified, [1] the fallback's scale interval was
 * ambiguous and the sum of squares was redone in order).
 * Hand-offs inside the launch are tagged epoch << 8 | il + 1 (il = 0..254).  ws NULL: the call brings
 * a zeroed workspace of its own.  ws given (vsim_op_tail_ln_ws_bytes(E) bytes, 256-byte aligned,
 * zeroed by the caller before its first use): the call writes the epoch word and reuses whatever
 * granules earlier calls left, which never match as long as the tag differs from the previous
 * call's on that workspace -- the executor's situation from layer to layer and step to step.
 * VSIM_EINVAL for what the fused kernel refuses: B != 1, nsplit outside 1..2, d % 32, d > 256,
 * (d / nsplit) % 32, H nsplit > 128, the LDS bound of vsim_op_tail_attn, K % 32, E/32 not below the
 * device's CU count (every out-projection tile must be resident at once), il outside 0..254, a
 * missing operand, an incomplete second norm, a short or misaligned ws.  VSIM_EHIP if a head part
 * did not raise its flag, VSIM_ESPIN if a bounded wait inside the kernel gave up during the call
 * (vsim_spin_timeouts grew).  Stream-ordered; waits for the stream before it returns. */
typedef struct {
  vsim_attn_batch_args attn; /* the attention row, B == 1 */
  int32_t nsplit;            /* workgroups per head, 1 or 2 */
  int32_t K;                 /* fc_out's inner size */
  const void *wo;            /* out-projection weight, W4T32 [E][E] */
  const void *wf;            /* fc_out weight, W4T32 [E][K] */
  const float *xd;           /* [K] fc_out's activation factors */
  const float *x;            /* [E] residual in */
  const float *ab, *fb;      /* [E] biases of the two branches (ab may be NULL) */
  const float *w1, *b1;      /* [E] norm 1 affine */
  const float *w2, *b2;      /* [E] norm 2 affine, or both NULL */
  float *jout;               /* [E] the joined row v */
  void *q1;                  /* norm 1 as Q4 SoA */
  float *xd1;                /* [E] its factors */
  void *q2;                  /* norm 2 outputs, or both NULL */
  float *xd2;
  uint32_t epoch;            /* the tag: epoch << 8 | il + 1 */
  int32_t il;
  void *ws;                  /* optional caller-owned workspace */
  size_t ws_bytes;
} vsim_tail_ln_args;
size_t vsim_op_tail_ln_ws_bytes(int E); /* 0 for an E that is no positive multiple of 32 */
int vsim_op_tail_ln(const vsim_tail_ln_args *a, void *stream);
/* The exact decode step's LayerNorm launch (k_ln_quant: 8 slice workgroups of 512 threads per norm)
 * on the call's operands, one launch_ln_quant:
 *   v[i]   = x[i]                                     no join operand
 *          = x[i] + ((ja[i] + jab[i]) + (jf[i] + jfb[i]))   in float32; jab NULL: ja[i] alone, jfb NULL:
 *            jf[i] alone; ja NULL: x[i] + (jf[i] + jfb[i]); jf NULL: x[i] + (ja[i] + jab[i])
 *            (the four forms the model's graphs use) -> jout when given
 *   y      = ggml_compute_forward_norm_f32 of v, as vsim_op_tail_ln's
 *   z1     = w1 * y + b1 (two float roundings), quantize_row_q4_0 -> q1 (Q4 SoA: nibbles [n/32][16], then
 *            scales [n/32]) and its factors xd1 [n], as vsim_op_q4_quantize's of z1
 *   z2     likewise with w2, b2 into q2, xd2 when all four are given (none: one norm).  The second
 *            norm is a job of its own in the launch: it joins the same operands and stores no jout.
 *   *epoch += 1 when epoch is given (a device word: the decode step's tag counter).
 * Bit for bit the reference's values.  How the kernel gets there shows only in vsim_norm_fallbacks:
 * every slice workgroup computes the whole row's statistics, slice 0 of each norm counts, so a call
 * adds at most one per norm to each counter ([0] the mean certificate failed and the sum was redone
 * in order, [1] the scale interval was ambiguous and the sum of squares was redone in order).
 * VSIM_EINVAL for what the launch cannot take: n no positive multiple of 32 or beyond the 64 KB of
 * dynamic LDS the row needs (n <= 16320), x, w1, b1, q1 or xd1 missing, an incomplete second norm,
 * jab without ja, jfb without jf, jout without a join operand, jout overlapping an input (the
 * slices read the whole of every input while others store), or x, w*, b*, j* not 16-byte aligned
 * (float4 accesses), q*, xd*, epoch not 4-byte aligned.  Enqueued on stream, not synchronized. */
typedef struct {
  const float *x;              /* [n] the row (the residual in) */
  int32_t n;
  const float *w1, *b1;        /* [n] norm 1 affine */
  void *q1;                    /* norm 1 as Q4 SoA */
  float *xd1;                  /* [n] its factors */
  const float *w2, *b2;        /* norm 2: all four or none */
  void *q2;
  float *xd2;
  const float *ja, *jab;       /* [n] optional join operands, see above */
  const float *jf, *jfb;
  float *jout;                 /* [n] the joined row, or NULL */
  uint32_t *epoch;             /* device word advanced by one, or NULL */
} vsim_ln_quant_args;
int vsim_op_ln_quant(const vsim_ln_quant_args *a, void *stream);
/* The exact decode step's GEMV batch ({fc_in + bias + GELU + requantize, Q, K, V} in the model): one
 * launch_gemv_chain_batch in exact mode on nj = 1..4 jobs, workgroups taking job 0's rows, then job
 * 1's, ...  Per job y = W . xd in the reference's chain (vsim_op_q4_gemv's, on the factors xd of
 * vsim_op_q4_quantize), then
 *   gelu_q == 0:  y[row] = dot (+ bias[row])
 *   gelu_q != 0:  g = gelu table[fp16(dot + bias[row])] (the library's table, vsim_op_tables), y[row] =
 *                 g when y is given, and each 32 rows quantize_row_q4_0 into block row/32 of oq (Q4 SoA,
 *                 M/32 blocks) and oxd [M], as vsim_op_q4_quantize's of g -- also where a block mixes
 *                 the table's NaN (for -inf) or inf with finite values: quantize_row_q4_0's amax =
 *                 MAX(amax, fabsf(v)) in element order (a NaN replaces the maximum, the next element
 *                 the NaN) and its unmasked vi0 | vi1 << 4 for codes outside 0..15.
 * A job's outputs do not depend on the jobs beside it.  *kernel (host, may be NULL) reports what
 * the launch chose for the batch: 1 k_gemv_solo (the jobs have at least 192 groups of 64 rows), 0
 * k_gemv_chain32.
 * VSIM_EINVAL for nj outside 1..4, M <= 0, K no positive multiple of 32, a NULL w or xd, a NULL y
 * without gelu_q, gelu_q with a NULL bias, oq or oxd or with M % 32 != 0, w or xd not 16-byte aligned
 * (16-byte weight loads and LDS-DMA of the factors), bias, y, oq or oxd not 4-byte aligned.  w holds
 * vsim_q4_bytes(M, K) bytes (whole 32-row tiles).  Enqueued on stream, not synchronized. */
typedef struct {
  const void *w;               /* W4T32 [M][K] */
  int32_t M, K;
  const float *xd;             /* [K] activation factors */
  const float *bias;           /* [M] or NULL (required with gelu_q) */
  float *y;                    /* [M], or NULL with gelu_q */
  int32_t gelu_q;
  void *oq;                    /* gelu_q: the output row as Q4 SoA (nibbles [M/32][16], then scales [M/32]) */
  float *oxd;                  /* gelu_q: [M] its factors */
} vsim_gemv_batch_job;
typedef struct {
  vsim_gemv_batch_job j[4];
  int32_t nj;
} vsim_gemv_batch_args;
int vsim_op_gemv_batch(const vsim_gemv_batch_args *a, int32_t *kernel, void *stream);
/* Long-prompt GEMM pieces (fast mode, N >= 256 inside the model): the fp16 image [M][K] of a
 * W4T32 weight (values d*(q-8) rounded to fp16), and Y[n][m] (+bias[m]) = sum_k W16[m][k] *
 * X16[n][k] on the 256 x 256-tile fp16 MFMA GEMM (K % 64 == 0; X16 [n][K] fp16). */
int vsim_op_q4_expand_f16(const void *w, int M, int K, void *w16, void *stream);
int vsim_op_gemm_f16(const void *w16, int M, int K, const void *x16, int n, const float *bias, float *y,
                     void *stream);
/* The activation step between two prompt GEMMs: x [n][K] f32 -> (x + bias, GELU table: when
 * gelu != 0) -> quantize_row_q4_0 per 32-block -> the values d*(q-8) as fp16 [n][K].  And the
 * fc_in GEMM with that step in its epilogue (q16 [n][M] instead of y; M % 32 == 0). */
int vsim_op_act_quant_f16(const float *x, int K, int n, const float *bias, int gelu, void *x16, void *stream);
int vsim_op_gemm_f16_gelu_q(const void *w16, int M, int K, const void *x16, int n, const float *bias, void *q16,
                            void *stream);
/* The same GEMM with the prompt layer's next step in its f32 epilogue:
 *  _rope: GPT-J rotary pairs (rows m, m+1 with m % d < n_rot, even m) at position p0 + n, as
 *    the rope + KV-write step of vsim.cpp:553-580 computes them (double cos/sin table cs
 *    [pos][n_rot/2][2], the products and differences in double, rounded to float);
 *  _join: the residual, res = res + (res_a + y) (vsim.cpp:694-695), or y + res when res_a is
 *    NULL (vsim.cpp:657), in place.  M % 4 == 0. */
int vsim_op_gemm_f16_rope(const void *w16, int M, int K, const void *x16, int n, const float *bias, float *y,
                          const double *cs, int d, int n_rot, int p0, void *stream);
int vsim_op_gemm_f16_join(const void *w16, int M, int K, const void *x16, int n, const float *bias, float *res,
                          const float *res_a, void *stream);
/* The model's long-prompt GEMM: the products of vsim_op_gemm_f16* straight from the W4T32
 * weight w, dequantized in LDS to the same fp16 halves (no image).  Epilogue, one at a time:
 * q16 != NULL the GELU-quantize one (y unused, bias required), cs != NULL the RoPE one into y,
 * join != 0 the residual join in place (y = res, res_a as in vsim_op_gemm_f16_join); else the
 * plain store (+ bias). */
int vsim_op_gemm_q4_256(const void *w, int M, int K, const void *x16, int n, const float *bias, float *y, void *q16,
                        const double *cs, int d, int n_rot, int p0, int join, const float *res_a, void *stream);
int vsim_op_get_rows(const void *w, int K, int V, const int32_t *rows, int n, float *y, void *stream);
/* ggml_norm (ggml.c:4246-4304); optional affine y = w*y + b (w, b may be NULL) */
int vsim_op_norm(const float *x, float *y, int k, int rows, const float *w, const float *b, void *stream);
/* cumulative counts of exact-LayerNorm rows that needed the sequential fallback:
 * out[0] = mean not certified, out[1] = variance scale not certified (summed over devices) */
int vsim_norm_fallbacks(unsigned out[2]);
/* cumulative count of bounded cross-workgroup waits that gave up, summed over devices and models:
 * the fused layer tail's waits (its attention heads, the in-tail LayerNorm's granules), the
 * barrier-free chain GEMV's ring hand-off, the prompt GEMM's stream-K finisher.  0 in every healthy
 * run; the model calls (eval, eval_argmax, generate, sync) count their own launches' timeouts and
 * return VSIM_ESPIN when that model's count grew. */
int vsim_spin_timeouts(unsigned *out);
int vsim_op_gelu(const float *x, float *y, int n, void *stream);
/* Greedy token of a logit row: *out = numpy.argmax(x[0:n]) (first index among equal maxima, -0.0 ==
 * +0.0, the first NaN if any); x and out device pointers; enqueued on stream, not synchronized.
 * The model's greedy step (vsim_model_eval_argmax / vsim_model_generate) runs the same kernel in
 * place of the reference's host-side greedy pick (sample_top_k with top_k = 1, utils.cpp:339-371,
 * called from vsim.cpp's main loop).  Ties differ: the reference orders equal logits by
 * std::partial_sort over (logit, id) pairs, whose order among equal keys the standard leaves
 * unspecified; this kernel returns the first index, as numpy does.  Distinct maxima agree. */
int vsim_op_argmax(const float *x, int n, int32_t *out, void *stream);
/* The O(n) stage of the reference's sampler (sample_top_p_top_k_repeat_penalty, utils.cpp:339-371:
 * repetition penalty, temperature scale, top-k) on the device, one launch (k_sample_topk):
 *   candidate c[i] = (double)x[i] * scale                          id i not in win[0:nw]
 *                    x[i] < 0 ? c[i] * repeat_penalty : c[i] / repeat_penalty   id i in win
 * in double and in that order (scale = 1.0 / temp); val[0:k], id[0:k] = the k largest candidates
 * in descending order.  x, win, val, id are device pointers (x any 4-byte alignment; win may hold
 * duplicates and ids outside [0, n), which match nothing); enqueued on stream, not synchronized.
 * Limits: 1 <= k <= min(n, VSIM_TOPK_MAX), 0 <= nw <= VSIM_WINDOW_MAX, else VSIM_EINVAL.
 * Ties: equal candidates (-0.0 == +0.0) are ordered by the lower id first, inside the list and at
 * the k-th boundary.  The reference's std::partial_sort over (value, id) pairs leaves the order
 * of equal values unspecified; distinct values agree with it exactly.  With a NaN logit the
 * reference's order is undefined and so is this one (the kernel still terminates and writes k
 * distinct ids of [0, n)).  val holds the candidates' own bits (a -0.0 stays -0.0).
 * The workspace is the library's, one per (device, stream), zero between launches: calls on one
 * stream may follow each other without a synchronize. */
#define VSIM_TOPK_MAX 64
#define VSIM_WINDOW_MAX 1024
int vsim_op_topk(const float *x, int n, const int32_t *win, int nw, double scale, double repeat_penalty, int k,
                 double *val, int32_t *id, void *stream);
/* vsim_op_topk for B logits rows in one launch (k_sample_topk_rows), every row with parameters of
 * its own: row b reads x + b * ldx (f32, ldx >= n, so rows need 4-byte alignment only) and the
 * device block pb[b], and writes out[b].val[0:k_b], out[b].id[0:k_b].
 * Contract: row b's k_b (value, id) pairs are bit for bit what vsim_op_topk gives for that row
 * alone with pb[b]'s win[0:nw], scale, penalty and k -- the same candidate formula, the same
 * (value, lower id first) total order, so the same tie rule.  A row's result does not depend on
 * B, on its index in the batch or on the other rows: the rows share no state (each hands off
 * through its own block of the workspace), and within a row the total order makes the result
 * independent of how the row is split over waves and workgroups.  Entries of out[b] past k_b are
 * not written.
 * The parameter blocks live on the device and are read when the kernel runs; it clamps k to
 * 1..VSIM_TOPK_MAX and nw to 0..VSIM_WINDOW_MAX and stays in bounds and terminates for any block
 * contents (k > n: the entries past n repeat id n - 1).  Callers that want errors check on the
 * host, as vsim_model_decode_batch_sample does.  NaN logits: as vsim_op_topk, per row.
 * VSIM_EINVAL for B outside 1..VSIM_BATCH_MAX, n < 1, ldx < n or a NULL pointer.
 * The workspace (B blocks) is the library's, one per (device, stream), every block's counter zero
 * between launches: calls on one stream may follow each other, and vsim_op_topk, without a
 * synchronize. */
typedef struct vsim_topk_params {
  double scale, penalty; /* 1 / temp; the repetition penalty */
  int32_t k, nw;         /* candidates wanted; ids in win */
  int32_t win[VSIM_WINDOW_MAX];
} vsim_topk_params;
typedef struct vsim_topk_out {
  double val[VSIM_TOPK_MAX];
  int32_t id[VSIM_TOPK_MAX];
} vsim_topk_out;
int vsim_op_topk_rows(const float *x, int ldx, int n, int B, const vsim_topk_params *pb /* device [B] */,
                      vsim_topk_out *out /* device [B] */, void *stream);
/* Workgroups per row of k_sample_topk_rows, process-wide: 0 (default) = as many as
 * k_sample_topk's (one per 1024 ids, at most 64) while all rows' together stay within 256, else
 * 256 / B; 1..64 = at most that many.  Same results either way (the contract above); for tests
 * and measurements.  Returns the previous setting. */
int vsim_topk_rows_set_wg(int per_row);
/* Scoring: the log-probability a logits row gives one token, and the row's greedy id, for R rows
 * x[R][V] (f32, row stride V, so any 4-byte alignment) in one launch (k_score_rows, score.hip).
 * Per row i, with m the row's maximum (a float, exact) and t = target[i]:
 *   s = sum_j exp((double)x[i][j] - (double)m)   in double
 *   lse = (double)m + log(s)
 *   logprob[i] = (double)x[i][t] - lse
 *   argmax[i]  = vsim_op_argmax's id (first maximum, -0.0 == +0.0, the first NaN if any)
 * t == -1 means "no target": logprob[i] = 0.0, argmax[i] is still written.  Ids outside [-1, V) are
 * the caller's bug at this level; the kernel treats them as -1 instead of reading out of bounds.
 * Order rule: one workgroup per row; thread k of 1024 adds the terms j = k, k + 1024, .. in that
 * order, the partials are added by one fixed tree.  A row's outputs therefore depend on that
 * row's contents only -- not on R, on the rows beside it in the launch, or on the run: the same
 * row gives the same bits every time.  (Another summation order, e.g. a host reference's,
 * differs by at most (V - 1) 2^-53 relative in s.)
 * NaN / Inf rule: -inf entries contribute 0.  A row holding a NaN, or whose maximum is +inf or
 * -inf, has logprob = NaN (and argmax by the rule above); the kernel terminates on every input.
 * All pointers are device pointers; logprob or argmax may be NULL (not both), target may be NULL
 * (all -1).  Enqueued on stream, not synchronized.  VSIM_EINVAL for V < 1, R < 0 or both outputs
 * NULL; R == 0 is a no-op. */
int vsim_op_logprob(const float *x, int V, int R, const int32_t *target, double *logprob, int32_t *argmax,
                    void *stream);
/* scale -> diag_mask_inf(n_past) -> soft_max over p[nz][nr][nc], in place */
int vsim_op_attn_softmax(float *p, int nc, int nr, int nz, int n_past, float scale, void *stream);
/* style 0 = GPT-NeoX rotate-half (ggml.c:6086), 1 = GPT-J pairs (ggml.c:5919);
 * x[T][H][d] in place; mode 0: p = n_past+i2, mode 1: i2 >= n_past only, p = i2 */
int vsim_op_rope(int style, float *x, int d, int H, int T, int n_past, int n_dims, int mode, void *stream);
int vsim_op_kq(const float *K, int ldk, const float *Q, int ldq, int d, int H, int nk, int n, float *kq,
               void *stream);
int vsim_op_kqv(const float *V, int ldv, const float *S, int d, int H, int nk, int n, float *out, void *stream);
/* the same with the prompt's causal mask (query j sees keys <= n_past + j, ggml.c:5764-5798):
 * KQ leaves fully masked 64 x 64 tiles unwritten (diag_mask_inf overwrites them), KQV stops each
 * query tile's chains at its last unmasked key (every later probability is +0) - the model's
 * exact prompt path (run_layer) */
int vsim_op_kq_causal(const float *K, int ldk, const float *Q, int ldq, int d, int H, int nk, int n, int n_past,
                      float *kq, void *stream);
int vsim_op_kqv_causal(const float *V, int ldv, const float *S, int d, int H, int nk, int n, int n_past, float *out,
                       void *stream);
/* Fast-mode prompt attention (fp16 MFMA, one pass with an online softmax): for N queries
 * Q [N][d*H] at positions n_past.., keys/values kc/vc [n_past+N][d*H] (post-RoPE K),
 * out[q][h*d + dd] = softmax_k(scale * K.Q, causal) . V.  d in {64, 96, 128, 256}. */
int vsim_op_attn_prefill(const float *Q, const float *kc, const float *vc, int d, int H, int N, int n_past,
                         float scale, float *out, void *stream);
/* The same attention (d = 256 only) written as the next GEMM's fp16 operand out16 [N][d*H]:
 * quantize_row_q4_0 (ggml.c:209-251) of each 32-value block of the output row, the values
 * d*(q-8) as fp16 -- what vsim_op_act_quant_f16 makes of vsim_op_attn_prefill's out. */
int vsim_op_attn_prefill_q16(const float *Q, const float *kc, const float *vc, int d, int H, int N, int n_past,
                             float scale, void *out16, void *stream);
/* The fp16 scratch of the prompt attention for nk = n_past + N keys of width E = d*H: *bytes its
 * size, K16[key][E] (row-major, as the cache) at its start, Vt16[h][dim][*ldt] at half offset
 * *vt_off (each head's V transposed; *ldt = nk rounded up to the 64-key tile, the columns
 * [nk, *ldt) zero).  Within each group of 16 keys V^T holds them in the order 0-3, 8-11, 4-7,
 * 12-15 (the middle quads swapped).  Any of the three outputs may be NULL. */
int vsim_op_attn_prefill_layout(int E, int nk, size_t *bytes, size_t *vt_off, int *ldt);
/* vsim_op_attn_prefill / _q16 (out16 != NULL: d = 256, out unused) on the caller's scratch of at
 * least that size, as the model's prompt layer calls it: the kernel that fills the scratch from
 * kc / vc runs first and the copies stay there afterwards.  fresh != 0: the new keys
 * [n_past, n_past + N) are already in the scratch (vsim_op_gemm_q4_256_h16 put them there) and
 * only the cached keys before n_past are converted, the V^T padding zeroed. */
int vsim_op_attn_prefill_scratch(const float *Q, const float *kc, const float *vc, int d, int H, int N, int n_past,
                                 float scale, float *out, void *out16, void *scratch, size_t scratch_bytes, int fresh,
                                 void *stream);
/* vsim_op_gemm_q4_256 (plain or RoPE epilogue) that also leaves the fp16 rounding of every
 * y[n][m] in the prompt attention's scratch, as the model's K and V projections of a long GPT-J
 * prompt do: with cs (RoPE, the K projection) row-major at h16[(p0 + n) * M + m], h16_t = 0;
 * without cs (the V projection) transposed at h16[m * h16_ld + pos(p0 + n)], h16_t != 0 and
 * h16_ld >= p0 + n, pos the key order of vsim_op_attn_prefill_layout.  Nothing else of h16 is
 * written.  M % 4 == 0. */
int vsim_op_gemm_q4_256_h16(const void *w, int M, int K, const void *x16, int n, const float *bias, float *y,
                            const double *cs, int d, int n_rot, int p0, void *h16, int h16_ld, int h16_t,
                            void *stream);
/* The long-prompt GEMM (vsim_op_gemm_q4_256, the model's N >= 256 path) splits the K range of
 * grids with fewer 256 x 256 tiles than CUs between two workgroups (stream-K: every CU busy, the
 * two partial sums added once; a different summation order than one pass, same per-element
 * bound).  enable = 0 keeps one pass per tile.  Process-wide; returns the previous setting. */
int vsim_gemm_set_streamk(int enable);
/* Two long-prompt GEMMs of one shape with the RoPE epilogue (the GPT-J prompt's Q and K
 * projections, vsim.cpp:540-580: ggml_mul_mat (ggml.c:4891-5165) then ggml_rope mode 0) in one
 * launch: y0 = RoPE(w0 x), y1 = RoPE(w1 x), M % 256 == 0, K % 128 == 0, positions p0 + n.  The
 * tile grid covers both; a remainder beyond whole rounds of the CUs is split as above.  Same
 * per-element bound as vsim_op_gemm_q4_256 with cs. */
int vsim_op_gemm_q4_256_pair(const void *w0, const void *w1, int M, int K, const void *x16, int n, float *y0, float *y1,
                             const double *cs, int d, int n_rot, int p0, void *stream);
/* The same launch with the second weight's row-major fp16 copy (vsim_op_gemm_q4_256_h16 with cs),
 * as the model's paired Q / K launch passes it: h16_1[(p0 + n) * M + m] = fp16(y1[n][m]). */
int vsim_op_gemm_q4_256_pair_h16(const void *w0, const void *w1, int M, int K, const void *x16, int n, float *y0,
                                 float *y1, const double *cs, int d, int n_rot, int p0, void *h16_1, void *stream);
/* mode 0: the model runs its prompt Q and K projections as two launches; 1 (default): one
 * paired launch, its remainder past whole rounds of the CUs split as above; 2: paired, whole
 * tiles only.  Process-wide; returns the previous setting. */
int vsim_gemm_set_qk_pair(int mode);
/* Order of the long-prompt GEMM's 256 x 256 tiles over the grid: groups of `cols` tile-columns
 * (256 tokens each), each group walked row by row, so the tiles one XCD runs together share
 * fewer activation slices; 0 = one group (row-major).  Used only when it divides the tile
 * columns.  Outputs do not depend on the order, except that a stream-K split then falls at other
 * tiles (same per-element bound).  Process-wide; returns the previous setting. */
int vsim_gemm_set_tile_order(int cols);
/* Fast-mode prompt LayerNorm (ggml_norm + affine, ggml.c:4246-4304, double sums in any order)
 * straight to the next GEMM's fp16 operand: quantize_row_q4_0 per 32-value block, d*(q-8) as
 * fp16 -- what vsim_op_act_quant_f16 makes of the normalized rows. */
int vsim_op_norm_f16q(const float *x, int k, int rows, const float *w, const float *b, void *x16, void *stream);
/* ---- the fast-mode prompt layer, launch by launch (run_layer / PromptBatch::mm / run_head in
 * VSIM_MODE_FAST): with the entries above, these make every launch of a prompt eval callable on
 * caller buffers, with the model's arguments.  Which launch the model takes follows from values
 * alone (N rows at n_past, E = n_embd, H heads of d = E / H dims, F = 4 E):
 *   N < 8     the rows stay f32 / Q4: vsim_op_norm, vsim_op_q4_quantize once per distinct activation
 *             (the norm's rows serve Q, K, V -- and fc_in of a one-norm graph), vsim_op_q4_gemv in
 *             VSIM_MODE_FAST, vsim_op_gelu_bias in place, and the attention as vsim_op_kq_causal,
 *             vsim_op_attn_softmax (vsim_op_attn_softmax_alibi for BLOOM), vsim_op_kqv_causal_merged.
 *   N >= 8    every activation is the GEMMs' fp16 operand: vsim_op_norm_f16q, vsim_op_act_quant_f16
 *             (the attention's output; fc_in's with bias and GELU), and the products on
 *             vsim_op_gemm_q4_f16x -- or, from N >= 256 with E % 64 == 0, on vsim_op_gemm_q4_256,
 *             where fc_in takes the GELU-quantize epilogue (q16), fc_out the residual join (join = 1
 *             with res_a = the out-projection's rows for a parallel residual, NULL for GPT-NeoX's
 *             serial one; BLOOM's fc_out stays plain), and a GPT-J layer's Q and K the RoPE epilogue
 *             with p0 = n_past, K and V written straight to their cache rows.  Q and K of such a
 *             layer are one vsim_op_gemm_q4_256_pair* launch when E % 256 == 0 (unless
 *             vsim_gemm_set_qk_pair(0)), else two launches.
 *             The attention is vsim_op_attn_prefill_scratch on the model's own scratch when d is one
 *             of 64, 96, 128, 256 and E % 64 == 0 and the graph has no ALiBi (else the three exact
 *             kernels as for N < 8); with the RoPE epilogue the K and V launches are the _h16 forms
 *             (K16 rows at the scratch's start, V^T at vt_off with h16_ld = ldt, both of
 *             vsim_op_attn_prefill_layout(E, n_past + N)) and fresh = 1; d = 256 writes out16 = the
 *             out-projection's operand and no vsim_op_act_quant_f16 follows.
 *   Without the RoPE epilogue Q, K, V land in row buffers and vsim_op_rope_kv_write moves them.
 *   The joins outside an epilogue: vsim_op_add_residual; a two-norm serial graph first copies the
 *   out-projection's rows and adds the residual to the copy (vsim_op_add_rows: attn + inpL), which
 *   its second norm reads; BLOOM ends a layer with a copy of that joined row and vsim_op_add_rows of
 *   fc_out's rows (inpFF + ff).
 *   The last row's head of an eval is the N = 1 case: vsim_op_norm, vsim_op_q4_quantize,
 *   vsim_op_q4_gemv; vsim_model_eval_score's chunks of C rows take the N = C rule.
 *
 * vsim_op_gemm_q4_f16x: y[n][M] (+ bias[M]) = the W4T32 weight w [M][K] times the fp16 operand x16
 * [n][K] on the small-tile fp16 MFMA GEMM (k_gemm_q4_f16; K % 32 == 0): vsim_op_q4_gemv's
 * VSIM_MODE_FAST product at n >= 8 without its conversion of Q4 rows, the weight's values d*(q-8)
 * rounded once to fp16, fp32 accumulation. */
int vsim_op_gemm_q4_f16x(const void *w, int M, int K, const void *x16, int n, const float *bias, float *y,
                         void *stream);
/* The prompt's RoPE + KV-cache write (vsim.cpp:553-580) in one launch: Q [N][H d] rotated in place
 * at positions n_past + i; K rotated into kcache rows n_past + i, V copied into vcache rows n_past +
 * i (kcache, vcache: one layer's [n_ctx][H d]).  style as vsim_op_rope; only the first n_rot dims of
 * a head rotate (n_rot = 0: none, BLOOM); the double products are rounded once to float.  The
 * cos / sin table is the library's own, as the model builds it; the call waits for the stream. */
int vsim_op_rope_kv_write(int style, float *Q, const float *K, const float *V, float *kcache, float *vcache, int d,
                          int H, int N, int n_past, int n_rot, void *stream);
/* The residual join of n values: inpL = inpL + (attn + ff) (vsim.cpp:694-695), or with
 * order_ff_first != 0 inpL = ff + inpL (vsim.cpp:657; attn unused, may be NULL).  And x += b over n
 * values, the elementwise use of the bias add (vsim.cpp:629: cur + inpL). */
int vsim_op_add_residual(float *inpL, const float *attn, const float *ff, int n, int order_ff_first, void *stream);
int vsim_op_add_rows(float *x, const float *b, int n, void *stream);
/* vsim_op_gelu of x[i] + bias[i % bias_len] (ggml_add, then ggml_gelu: vsim.cpp:680-683) */
int vsim_op_gelu_bias(const float *x, float *y, int n, const float *bias, int bias_len, void *stream);
/* vsim_op_attn_softmax with ggml_alibi between the scale and the mask (BLOOM): row j of head z gets
 * (j + 1) * alibi[z] added (device slopes, [nz]).  vsim_op_alibi_slopes: the slopes as the model
 * computes them, into a host array of n_head floats. */
int vsim_op_attn_softmax_alibi(float *p, int nc, int nr, int nz, int n_past, float scale, const float *alibi,
                               void *stream);
int vsim_op_alibi_slopes(float *slopes_host, int n_head);
/* vsim_op_kqv_causal with the heads merged as the model stores them: out[q][h d + c]. */
int vsim_op_kqv_causal_merged(const float *V, int ldv, const float *S, int d, int H, int nk, int n, int n_past,
                              float *out, void *stream);
/* ---- fast-mode decode step, kernel by kernel (fast_decode.hip; the launches of the model's
 * fast step with the same parameter blocks).  Q4 SoA rows are vsim_op_q4_quantize's xq for n = 1:
 * the nibble plane [k/32][16], then the k/32 float scales.
 * Weights are W4T32 (vsim_op_q4_repack) and need VSIM_FAST_PAD readable bytes after the tensor:
 * the weight stream loads whole batches past a wave's block range (and past the tensor's end)
 * and zeroes their scales, so allocate vsim_q4_bytes(rows, k) + VSIM_FAST_PAD and repack into the
 * front.  A bias is read for every row of the last 32-row tile: rows rounded up to 32 floats.
 * All three enqueue on `stream` and do not synchronize. */
#define VSIM_FAST_PAD 65536
enum { VSIM_FE_STORE = 0, VSIM_FE_GELU_Q = 1, VSIM_FE_ROPE_Q = 2, VSIM_FE_ROPE_K = 3, VSIM_FE_V = 4 };
typedef struct {
  const void *w;     /* W4T32 rows x k (+ VSIM_FAST_PAD) */
  int32_t rows, k;   /* rows % 32 == 0 unless epi == VSIM_FE_STORE */
  const float *bias; /* may be NULL (required for VSIM_FE_GELU_Q) */
  float *y;          /* STORE, ROPE_Q: [rows]; ROPE_K, V: a cache [n_ctx][rows], row *n_past is written */
  int32_t epi;       /* VSIM_FE_* */
  int32_t act;       /* activation 0 or 1 */
} vsim_fast_job;
typedef struct {
  /* the two activations, either Q4 SoA rows of k values (lnx == NULL) ... */
  const void *xq[2];
  /* ... or the LayerNorm (ggml.c:4246-4304, both moments in one double pass) of the row lnx [k]
   * with affine act, quantized (ggml.c:209-251) in every workgroup's prologue */
  const float *lnx, *lnw[2], *lnb[2];
  vsim_fast_job j[4]; /* every k equal, a multiple of 32, at most 8192 */
  int32_t nj;
  void *oq;           /* VSIM_FE_GELU_Q: gelu table (vsim_op_tables) of fp16(dot + bias), quantized:
                         Q4 SoA row of that job's `rows` values */
  /* VSIM_FE_ROPE_Q / _K: rotation at position *n_past (device), cs [pos][n_rot/2] {cos, sin}
   * doubles; style 0 rotate-half (d % 32 == 0, n_rot <= 32), 1 GPT-J pairs; head dim d.
   * VSIM_FE_V reads *n_past too. */
  const int32_t *n_past;
  const double *cs;
  int32_t d, n_rot, style;
  uint32_t *clear;    /* may be NULL: nclear words zeroed by the launch */
  int32_t nclear;
} vsim_fast_gemv_args;
/* One k_fast_gemv batch: the 32-row tiles of up to 4 jobs, y = W . q4(x) (+ bias), the integer
 * block dots scaled by d_w d_x and summed in a fixed order. */
int vsim_op_fast_gemv(const vsim_fast_gemv_args *a, void *stream);
typedef struct {
  /* fc_out split over K: ffp[s][rows] = rows of wf over blocks [s nb/sf, (s+1) nb/sf) of xf */
  const void *wf;    /* W4T32 rows x k (+ VSIM_FAST_PAD); rows % 32 == 0, (k/32) % sf == 0, k/sf <= 8192 */
  int32_t rows, k, sf;
  const void *xf;    /* Q4 SoA row of k values */
  float *ffp;        /* [sf][rows] */
  /* single-query attention at position *n_past over 64-position chunks: q [H d] (rotated), kc, vc
   * [>= *n_past + 1][H d] with the new row in place; part [H][nchunk][d + 2] receives every
   * chunk's (max, sum, weighted V) (chunks past *n_past: -inf, 0), oq the merged output as a
   * Q4 SoA row of H d values.  d % 32 == 0, d <= 256, nchunk <= 64, *n_past < 64 nchunk. */
  const float *q, *kc, *vc;
  const int32_t *n_past;
  int32_t d, H, nchunk;
  float scale;
  float *part;
  uint32_t *hcnt;    /* 4 H words of workspace: zeroed on the stream by this call */
  void *oq;
} vsim_fast_tail_args;
int vsim_op_fast_tail(const vsim_fast_tail_args *a, void *stream);
/* k_fast_oproj_join: out = x + ((W . xq + bo) + (sum_s ffp[s] + bproj)), W E x E W4T32 (+ VSIM_FAST_PAD),
 * xq the attention's Q4 SoA row, ffp [sf][E]; bo may be NULL.  E % 32 == 0, E <= 8192. */
int vsim_op_fast_oproj_join(const void *w, int E, const void *xq, const float *bo, const float *ffp, int sf,
                            const float *bproj, const float *x, float *out, void *stream);
/* device fp16 tables (exp, gelu) as built by ggml_init (ggml.c:1240-1251) */
int vsim_op_tables(uint16_t *exp_f16_host, uint16_t *gelu_f16_host);

/* ------------------------------------------------------------- sampler (host) ------ */
/* The reference's sampler (utils.cpp:339-422) and the last-n window of its main loop
 * (vsim.cpp:875-876) as an object.  Its work is split in two stages:
 *   candidates  penalty, temperature and the ordered top-k of the n_vocab logits: on the device
 *               (vsim_op_topk; the model's sampled step below), or on the host (sample_host);
 *   finish      on at most top_k candidates, always on the host: p = exp(c - max) in double,
 *               normalise, the top-p cut and rescale, std::discrete_distribution<> over the
 *               sampler's std::mt19937.  It stays on the host because its exp is glibc's double
 *               exp, which the device's does not reproduce bit for bit, and the sampled streams
 *               are the reference's only if every probability is.
 * The float parameters widen as the reference's do (top_p, temp, repeat_penalty: float to double;
 * top_k through (int)(float); the top-p test is top_p < 1.0f).  The window starts as
 * repeat_last_n zeros, so id 0 is penalised from the first token, as in the reference;
 * repeat_last_n = 0 means no window.  No function here needs a GPU. */
typedef struct vsim_sampler vsim_sampler;
typedef struct {
  int32_t seed, top_k, repeat_last_n;
  float top_p, temp, repeat_penalty;
} vsim_sample_params;
int vsim_sampler_create(const vsim_sample_params *p, vsim_sampler **out);
/* a token enters the window without being sampled (the prompt's): drop the oldest, append */
int vsim_sampler_accept(vsim_sampler *s, int32_t token);
/* finish on an ordered candidate list (val descending, 1 <= k <= VSIM_TOPK_MAX, else
 * VSIM_EINVAL): the token drawn, which also enters the window.  One candidate, or a top-p cut
 * down to one, draws nothing from the generator (libstdc++), and later draws depend on that. */
int vsim_sampler_pick(vsim_sampler *s, const double *val, const int32_t *id, int k, int32_t *token);
/* both stages on the host from a logits row, the reference's code as it stands (any top_k in
 * 1..n; the order of equal candidates is std::partial_sort's); the token enters the window */
int vsim_sampler_sample_host(vsim_sampler *s, const float *logits, int n, int32_t *token);
/* tokens drawn by vsim_sampler_pick (the device made the candidates) and by sample_host */
int vsim_sampler_stats(const vsim_sampler *s, uint64_t *picks, uint64_t *host_picks);
void vsim_sampler_free(vsim_sampler *s);

/* ------------------------------------------------------ 3. model-level executor ---- */
typedef struct vsim_model vsim_model;

typedef struct {
  int32_t n_vocab, n_embd, n_head, n_layer, n_rot, use_parallel_residual;
} vsim_hparams;

/* Layers [layer_begin, layer_end) live on `device`; the first stage also owns the
 * embedding, the last stage ln_f + lm_head. */
int vsim_model_create(int arch, const vsim_hparams *hp, int n_ctx, int device, int layer_begin, int layer_end,
                      vsim_model **out);
/* Load a ggml model file of `arch` (vsim.cpp:108-458 / convert_gptj_to_ggml.py format);
 * creates the model, uploads every tensor this stage owns. */
int vsim_model_load_file(const char *path, int arch, int n_ctx, int device, int layer_begin, int layer_end,
                         vsim_model **out);
/* Upload one tensor by its ggml-file name (Q4_0 tensors in the on-disk AoS format). */
int vsim_model_set_tensor(vsim_model *m, const char *name, const void *host, size_t nbytes);
/* Load with options.  flags = 0 is vsim_model_load_file exactly.  VSIM_LOAD_QUANTIZE also accepts
 * the converters' F32 / F16 files (header f16 = 0 / 1): a 2-D record whose slot is a Q4_0 matrix
 * may then have ftype 0 or 1 and is quantized on the device as it streams in
 * (vsim_model_set_tensor_src's path, read straight into the staging buffers), or ftype 2 as
 * before; the same shape, name, missing-tensor and truncation checks apply. */
#define VSIM_LOAD_QUANTIZE 1
int vsim_model_load_file_ex(const char *path, int arch, int n_ctx, int device, int layer_begin, int layer_end,
                            int flags, vsim_model **out);
/* Upload one matrix as the converters write it (src_type VSIM_SRC_F32 / VSIM_SRC_F16, row-major
 * [rows][k]) and quantize it into the slot with the reference quantizer's semantics
 * (vsim_op_q4_quantize_w).  The matrix goes through two pinned staging buffers in chunks of rows
 * (multiples of 32; about 64 MiB of source by default), the copy of one chunk overlapping the
 * kernel of the one before, so staging memory is bounded whatever the tensor's size.  BLOOM's
 * fused query_key_value is spread over its three slots as vsim_model_set_tensor does.  A 1-D
 * (F32) tensor takes vsim_model_set_tensor's path (src_type must be VSIM_SRC_F32). */
int vsim_model_set_tensor_src(vsim_model *m, const char *name, const void *host, size_t nbytes, int src_type);
/* Rows per staging chunk of the two calls above, process-wide: 0 = the default, other values are
 * rounded up to a multiple of 32.  Returns the previous value.  For tests: many chunks on tiny
 * tensors. */
int vsim_quantize_set_chunk_rows(int rows);
/* Read one tensor back in the same file format (Q4_0 as AoS blocks, F32 as floats). */
int vsim_model_get_tensor(vsim_model *m, const char *name, void *host, size_t nbytes);
/* Synthetic weights drawn on the device (N(0,std), LN gains 1+N(0,std)), quantized with
 * quantize_row_q4_0 semantics; for throughput runs of full-size configs. */
int vsim_model_randomize(vsim_model *m, uint64_t seed, float std);
/* VSIM_MODE_FAST on a model whose n_ctx exceeds 4096 (more than 64 chunks of 64 positions, the
 * limit of the fast decode step's attention merge) selects VSIM_MODE_EXACT: every eval of such a
 * model is the exact one, bit for bit.
 * VSIM_MODE_W4A16 (weight-only: every product is vsim_op_w4a16_rows + vsim_op_q4_gemm_w4a16_rows on
 * the f32 activation rows; LayerNorm, RoPE, KQ with double sums, the fp16-table softmax, the KQV
 * float chain, the table GELU, the joins and the embedding rows are the exact path's kernels; the
 * fast prompt attention, the fp16 GEMMs and their epilogues are not used; one exception, BLOOM's
 * prompt softmax: the reference adds the ALiBi term (j + 1) m_h to row j of a batch, a per-row
 * constant that no softmax depends on except in its rounding, and this mode adds the single-token
 * step's 1 m_h to every row instead, so that a row does not depend on its place in a batch; and one
 * option, vsim_w4a16_set_attn(1): KQ, softmax and KQV on fp16 MFMA under a per-row contract of their
 * own, with the promises below unchanged) is
 * accepted on a whole
 * model (layers [0, n_layer)) at any n_ctx; VSIM_EINVAL on a pipeline stage.  Every kernel of the
 * mode is per row, so in this mode, bit for bit:
 *   - an eval of N tokens leaves the cache rows of N single-token evals, and its logits row is
 *     theirs (a product of N rows is one launch of vsim_op_q4_gemm_w4a16_tile's kernel from 33 rows
 *     on, and ceil(N / 32) launches of the rows kernel on consecutive 32-row chunks below or with
 *     vsim_w4a16_set_tile_gemm(0): neither tiling nor chunking changes a row's bits);
 *   - row i of vsim_model_eval_score's logits_all is the logits row of the eval ending at i,
 *     whatever the head's chunk size;
 *   - row b of vsim_model_decode_batch_w4a16 is vsim_model_eval_seq's row for that sequence alone;
 *   - switching to another mode and back changes neither mode's bits.
 * All whole-model entry points work in the mode.  vsim_model_eval_seq and _eval_score run the general
 * path at every N, and so does vsim_model_eval at N > 1.  vsim_model_eval at N = 1, _eval_argmax,
 * _generate, _eval_sample and _generate_sampled run the mode's single-token step on slot 0
 * (w4a16_decode.hip: vsim_op_w4a16_ln, _gemv and _gelu around k_attn_decode_batch at one row; at most
 * 7 launches per parallel-residual layer, 9 per serial one, 2 for the head), replayed as a hipGraph
 * under vsim_model_set_graph like the other modes' steps, _generate without a host round trip per
 * token.  The step's logits and cache rows are the general path's, bit for bit.  Shapes the step
 * does not take run the general path as before (decided once per model): a head dim that is not a
 * multiple of 32 or exceeds 256, n_embd beyond 16,384, or a context whose attention scores do not
 * fit the attention kernel's LDS (2 d + n_ctx + 16,384 floats beyond 160 KB).  vsim_w4a16_set_step(0)
 * puts every model back on the general path.  The pipeline stage calls (vsim_model_stage_bind /
 * _begin / _step) return VSIM_EINVAL while the model is in this mode. */
int vsim_model_set_mode(vsim_model *m, int mode);
/* Allocates ahead what a prompt of up to n_tokens sets up on its first eval (the N-token
 * scratch, the fp16 key copies of the prompt attention, the GEMMs' stream-K workspace) and
 * loads the prompt kernels, so that the first prompt runs at the steady-state rate.  Optional:
 * an eval allocates whatever is missing itself.  VSIM_EINVAL if n_tokens is not in 1..n_ctx. */
int vsim_model_reserve(vsim_model *m, int n_tokens);
int vsim_model_hparams(const vsim_model *m, vsim_hparams *hp, int *n_ctx, int *layer_begin, int *layer_end);
/* One eval of N tokens at n_past (vsim.cpp:470-747).  First stage reads `tokens`;
 * non-first stages read the residual from `resid_in` (device, [N][n_embd] f32);
 * non-last stages write their residual to `resid_out` (device); the last stage copies
 * the last row of logits to `logits` (host, n_vocab floats) if non-NULL. */
int vsim_model_eval(vsim_model *m, int n_past, const int32_t *tokens, int N, const float *resid_in,
                    float *resid_out, float *logits);
/* Scoring eval: vsim_model_eval's N-token prompt pass, then the head over ALL N rows instead of
 * the last one -- per position i the log-probability of targets[i] and the greedy id
 * (vsim_op_logprob's definition, order rule and NaN / Inf rule), without the logits leaving the
 * device.  This is how a numeric path's loss is measured: score one text in exact and in fast
 * mode, or from an F16-quantized and a Q4_0 file, and compare.
 *   targets, logprob, argmax   host arrays of N (targets NULL: all -1; logprob / argmax may be
 *                              NULL).  targets[i] is usually tokens[i + 1]; -1 scores nothing.
 *   logits_all                 optional host buffer [N][n_vocab] receiving every logits row (NULL
 *                              in normal use: tests, and callers who want every row).
 * Valid on the stage that owns the head: a whole model reads `tokens`, a last pipeline stage
 * `resid_in` (device, [N][n_embd]); a stage without the head returns VSIM_EINVAL (earlier stages
 * keep using vsim_model_eval with resid_out).  VSIM_EINVAL too for a target outside
 * [-1, n_vocab) and for vsim_model_eval's n_past / N range errors; VSIM_ESPIN as vsim_model_eval.
 * The embedding and the layers are vsim_model_eval's prompt path in the model's current mode for
 * every N (N == 1 included: not the captured decode step), and the KV cache ends in the state
 * vsim_model_eval(m, n_past, tokens, N, ..) leaves, so windows chain and a decode step may follow.
 * The head runs over chunks of C rows -- final LayerNorm, lm_head product, k_score_rows, the
 * optional copy-out -- through a [C][n_vocab] f32 scratch allocated on the first scoring call;
 * C = 64 MiB / (4 n_vocab) clamped to 8..256 (vsim_score_set_chunk_rows).  One copy of N doubles
 * and N ints leaves the device at the end.
 * Exact mode: every row of logits_all, hence every argmax, is bit for bit the logits row
 * vsim_model_eval gives for the prefix ending at that position (the reference's), whatever C is.
 * Fast mode: the chunk's row count picks the lm_head kernel (256 or more rows: the 256-tile fp16
 * MFMA GEMM; 8 or more: the small-tile one; fewer: quantize + GEMV), so bits may depend on C. */
int vsim_model_eval_score(vsim_model *m, int n_past, const int32_t *tokens, int N, const float *resid_in,
                          const int32_t *targets, double *logprob, int32_t *argmax, float *logits_all);
/* Rows per head chunk of vsim_model_eval_score, process-wide: 0 = the default, other values are
 * capped at 256.  Returns the previous value.  For tests: many ragged chunks on tiny models. */
int vsim_score_set_chunk_rows(int rows);
/* ---- several sequences on one model.  A model serves n_seq sequences from n_seq KV-cache slots
 * of the shape [layers][n_ctx][n_embd] (K and V each).  Slot 0 is the cache every other entry
 * point uses (eval, eval_argmax, generate, eval_sample, eval_score, the stage calls): those keep
 * working on it exactly as before, captured decode graphs included.
 * vsim_model_seq_reserve gives the model n_seq slots (a new model has one).  Growing allocates the
 * new slots (zero-filled) and keeps the contents of the existing ones; n_seq equal to the current
 * count does nothing; fewer is VSIM_EINVAL, as is n_seq < 1.  VSIM_ENOMEM when a slot cannot be
 * allocated, and then the slots are as they were.  VSIM_EINVAL for a model on borrowed caches (the
 * graph executor's) and for a pipeline stage that is not a whole model. */
int vsim_model_seq_reserve(vsim_model *m, int n_seq);
/* vsim_model_eval of a whole model on slot seq: N tokens at n_past, the last row's logits to
 * `logits` (host, may be NULL).  Always the general (prompt) path, N == 1 included, because the
 * captured single-token graphs hold slot 0's addresses; in exact mode that path gives the same
 * bits as the captured step.  Both modes.  VSIM_EINVAL for a slot outside the reserve, a stage
 * model, and vsim_model_eval's range errors; VSIM_ESPIN as vsim_model_eval. */
int vsim_model_eval_seq(vsim_model *m, int seq, int n_past, const int32_t *tokens, int N, float *logits);
/* One decode step for B sequences at once: row b embeds tokens[b], attends over slot seq[b] at
 * position n_past[b] (positions may differ from row to row) and writes that slot's cache row
 * n_past[b].  logits (host, [B][n_vocab]) and next (host, [B]: each row's greedy id, vsim_op_argmax's
 * conventions, taken on the device) may each be NULL; only what is asked for leaves the device.
 * Contract (exact mode): row b of logits is bit for bit the row vsim_model_eval gives for that
 * sequence run alone with the same history -- the reference's row -- for every B, every mix of
 * positions and whatever else shares the batch: every product row is the reference's chain
 * (vsim_op_q4_gemm_rows), every attention row the single-token attention on its own cache
 * (vsim_op_attn_decode_batch), everything else is per row already.
 * The weights stream once per step for all B rows, which is the point: B independent chains per
 * weight row where a single sequence has one.
 * VSIM_EINVAL for B outside 1..VSIM_BATCH_MAX, a slot outside the reserve or named twice,
 * n_past[b] outside [0, n_ctx), a token outside the vocabulary, a model that is not a whole model,
 * and for a model in VSIM_MODE_FAST: this call is the exact step (a fast-mode batch is
 * vsim_model_decode_batch_fast's, below).  VSIM_ESPIN as
 * vsim_model_eval.  The step is enqueued eagerly (no hipGraph) and waits once, at its end. */
int vsim_model_decode_batch(vsim_model *m, int B, const int32_t *seq, const int32_t *n_past, const int32_t *tokens,
                            float *logits /* host [B][n_vocab] or NULL */, int32_t *next /* host [B] or NULL */);
/* The same step with fast-mode products, whatever vsim_model_set_mode says: the call names its
 * numeric path.  Arguments, checks and errors are vsim_model_decode_batch's (without the mode
 * refusal).  Every product (Q, K, V, out-projection, fc_in, fc_out, lm_head) runs on the rows' Q4_0
 * quantization through vsim_op_q4_gemm_fast_rows' dispatch (vsim_batch_set_fast_gemm), so the
 * weights stream once per step for all B rows; the other kernels are the exact step's.
 * Contract: row b of logits is bit for bit the row vsim_model_eval_seq(m, seq[b], n_past[b],
 * &tokens[b], 1, logits) gives on this model in VSIM_MODE_FAST from the same cache state, and the
 * cache rows written are the same too -- for every B, every mix of positions and whatever else
 * shares the batch -- so a slot may be advanced by either call in any order.  (A product row does
 * not depend on the batch: vsim_op_q4_gemm_fast_rows' contract; neither does any other kernel's.)
 * Fast mode's distance from the reference is that of vsim_model_eval_seq in VSIM_MODE_FAST. */
int vsim_model_decode_batch_fast(vsim_model *m, int B, const int32_t *seq, const int32_t *n_past,
                                 const int32_t *tokens, float *logits /* host [B][n_vocab] or NULL */,
                                 int32_t *next /* host [B] or NULL */);
/* The same step with weight-only products (VSIM_MODE_W4A16), whatever vsim_model_set_mode says: the
 * call names its numeric path as vsim_model_decode_batch_fast does.  Arguments, checks and errors are
 * vsim_model_decode_batch's (without the mode refusal).  Every product runs on the rows' fp16
 * operand through vsim_op_q4_gemm_w4a16_rows (the attention hands its f32 output row to the
 * out-projection), the weights stream once per step for all B rows, the other kernels are the exact
 * step's.  Contract: row b of logits is bit for bit the row vsim_model_eval_seq(m, seq[b],
 * n_past[b], &tokens[b], 1, logits) gives on this model in VSIM_MODE_W4A16 from the same cache
 * state, and the cache rows written are the same -- for every B, every mix of positions and every
 * row order -- so a slot may be advanced by either call. */
int vsim_model_decode_batch_w4a16(vsim_model *m, int B, const int32_t *seq, const int32_t *n_past,
                                  const int32_t *tokens, float *logits /* host [B][n_vocab] or NULL */,
                                  int32_t *next /* host [B] or NULL */);
/* The batched step, sampled: vsim_model_decode_batch (mode = VSIM_MODE_EXACT) or
 * vsim_model_decode_batch_fast (VSIM_MODE_FAST) up to the head, then row b's candidate stage with
 * samplers[b]'s window, k, temperature and penalty -- all rows in one k_sample_topk_rows launch
 * on the device logits -- one copy of the B candidate lists (768 bytes each) to the host, and
 * after the step's single synchronize vsim_sampler_pick per row, in row order, into next[b].
 * No logits row leaves the device.
 * A sampler outside the device stage's limits (top_k > VSIM_TOPK_MAX or > n_vocab, repeat_last_n
 * > VSIM_WINDOW_MAX, temp <= 0, repeat_penalty <= 0) takes the host path for its row only: that
 * row's logits are copied out and go through vsim_sampler_sample_host; the other rows stay on the
 * device path.  vsim_sampler_stats tells which ran.
 * Contract, exact mode: next[b] and samplers[b]'s state afterwards (window, generator, counts)
 * are those of vsim_model_eval_sample(m, samplers[b], n_past[b], tokens[b]) on that sequence
 * alone with the same history -- the reference's token wherever the candidates are distinct (tie
 * rule: vsim_op_topk).  Fast mode: those of vsim_model_eval_seq on this model in VSIM_MODE_FAST,
 * vsim_op_topk on its logits row and vsim_sampler_pick, on the same cache.  Both follow from the
 * logits rows being batch-independent already (the two calls above) and vsim_op_topk_rows' rows
 * being so too.
 * Checks and errors: those of the call the mode names (the exact step refuses a model in
 * VSIM_MODE_FAST), and VSIM_EINVAL for another mode value, a NULL sampler or `next`, a sampler
 * named twice (its generator would serve two sequences) and top_k < 1.  Nothing is enqueued and
 * no sampler is touched when a check fails. */
int vsim_model_decode_batch_sample(vsim_model *m, int mode, int B, const int32_t *seq, const int32_t *n_past,
                                   const int32_t *tokens, vsim_sampler *const *samplers /* [B] */,
                                   int32_t *next /* host [B] */);
/* The sampled batched step with weight-only products: vsim_model_decode_batch_sample's arguments,
 * checks and device / host sampler paths with vsim_model_decode_batch_w4a16 up to the head, whatever
 * the model's mode.  Contract: next[b] and samplers[b]'s state afterwards are those of
 * vsim_model_eval_seq on this model in VSIM_MODE_W4A16, vsim_op_topk on its logits row and
 * vsim_sampler_pick, on the same cache.  (An entry of its own: vsim_model_decode_batch_sample's mode
 * argument stays EXACT / FAST, every other value VSIM_EINVAL, as tests/test_gpu_batch_sample_model.py
 * pins it.) */
int vsim_model_decode_batch_sample_w4a16(vsim_model *m, int B, const int32_t *seq, const int32_t *n_past,
                                         const int32_t *tokens, vsim_sampler *const *samplers /* [B] */,
                                         int32_t *next /* host [B] */);
/* The batched step with a run of tokens per slot.  S slots; slot seq[s] contributes len[s] >= 1
 * consecutive tokens at positions n_past[s], n_past[s] + 1, .., n_past[s] + len[s] - 1, the runs
 * concatenated in `tokens` in slot order, N = sum len <= VSIM_BATCH_MAX rows in all; logits and next
 * have one row per token in that order.  mode is VSIM_MODE_EXACT, VSIM_MODE_FAST or VSIM_MODE_W4A16
 * and names the products exactly as vsim_model_decode_batch, _fast and _w4a16 do (exact is refused
 * on a model that is not in exact mode).  The weights stream once for all N rows.  Every layer's
 * attention is the two launches of vsim_op_attn_decode_runs (vsim_op_attn_w4a16_runs under
 * vsim_w4a16_set_attn(1) in weight-only mode); everything else is the batched step's.
 * Contract, in every mode: row j of slot s is bit for bit row 0 of the vsim_model_decode_batch* call
 * that `mode` names with B = 1 on that slot at n_past[s] + j, after the j rows before it were stepped
 * the same way, and the cache rows written are the same -- for every S, every mix of lengths and
 * positions and whatever shares the batch.  Greedy speculative decoding follows: feed [last token] +
 * draft as one run, and next[i] is the plain loop's token after row i wherever rows 1..i were the
 * plain loop's own tokens.
 * Rollback: a step never reads a cache row at or past the position it runs at, so after a rejected
 * draft the caller just continues from a smaller n_past; the rows the rejected tokens wrote are
 * overwritten before anything reads them.
 * VSIM_EINVAL, with nothing enqueued: S < 1, len[s] < 1, N > VSIM_BATCH_MAX, a slot outside the
 * reserve or named twice (one run per slot), n_past[s] < 0 or n_past[s] + len[s] > n_ctx, a token
 * outside the vocabulary, another mode value, a model that is not a whole model.  VSIM_ESPIN as
 * vsim_model_eval.  Enqueued eagerly (no hipGraph), one wait at the end. */
int vsim_model_decode_runs(vsim_model *m, int mode, int S, const int32_t *seq, const int32_t *n_past,
                           const int32_t *len, const int32_t *tokens /* [N], N = sum len, runs concatenated */,
                           float *logits /* host [N][n_vocab] or NULL */, int32_t *next /* host [N] or NULL */);
/* Slot fork: cache rows [0, n_tokens) of K and V of every layer go from slot src to slot dst
 * (device to device on the model's stream, one strided copy each; ordered with the steps before
 * and after it, not synchronized).  A slot holds nothing but these rows, so dst then continues
 * any sequence whose first n_tokens tokens are src's: evaluate a prompt once, sample n
 * continuations.  Slot 0 may be either side.  VSIM_EINVAL for a slot outside the reserve,
 * dst == src, n_tokens outside 1..n_ctx, a model on borrowed caches or a pipeline stage. */
int vsim_model_seq_copy(vsim_model *m, int dst, int src, int n_tokens);
/* Greedy single-token decode step of a whole-model stage: eval of `token` at n_past, then
 * the argmax of the logits on the device (numpy.argmax conventions: first maximum, first
 * NaN); only the token id leaves the device.  The reference's loop samples on the host
 * from the logits (vsim.cpp:860-891); this is its greedy case without the logits copy. */
int vsim_model_eval_argmax(vsim_model *m, int n_past, int32_t token, int32_t *next_token);
/* Device-resident greedy generation: n_steps single-token steps from (n_past, token), each
 * step's argmax feeding the next on the device (no host round trip per token); the
 * n_steps generated tokens are copied to tokens_out at the end.  Same tokens as calling
 * vsim_model_eval_argmax n_steps times. */
int vsim_model_generate(vsim_model *m, int n_past, int32_t token, int n_steps, int32_t *tokens_out);
/* Sampled single-token decode step of a whole-model stage: eval of `token` at n_past, then the
 * candidate stage of sampler s on the device logits (k_sample_topk, inside the step's hipGraph;
 * the window, k, scale and penalty are uploaded per step, so samplers may alternate on one
 * model), one copy of at most VSIM_TOPK_MAX (value, id) pairs to the host, and
 * vsim_sampler_pick there.  The logits row never leaves the device.  The same tokens as
 * vsim_model_eval + vsim_sampler_sample_host wherever the candidates are distinct (ties:
 * vsim_op_topk).  A sampler outside the device stage's limits -- top_k > VSIM_TOPK_MAX or
 * > n_vocab, repeat_last_n > VSIM_WINDOW_MAX, temp <= 0 or repeat_penalty <= 0 -- takes exactly
 * that host path instead; vsim_sampler_stats tells which ran. */
int vsim_model_eval_sample(vsim_model *m, vsim_sampler *s, int n_past, int32_t token, int32_t *next_token);
/* The loop over vsim_model_eval_sample: up to n_steps tokens from (n_past, token) into
 * tokens_out, *n_out of them; stops after a step that produced `eos` (-1: none), as the
 * reference's loop does for id 2 (vsim.cpp:894).  One host round trip per token (the finish
 * stage): a sampled loop without it would need the device's exp to be glibc's. */
int vsim_model_generate_sampled(vsim_model *m, vsim_sampler *s, int n_past, int32_t token, int n_steps, int32_t eos,
                                int32_t *tokens_out, int *n_out);
/* Pipeline stage step: the single-token step of this stage's layers between
 * device buffers the caller binds once -- tok_in (first stage: the token to embed), resid_in
 * (other stages: the [n_embd] residual from the previous stage), resid_out (non-last stages:
 * this stage's residual for the next), tok_out (last stage: the greedy token, device argmax,
 * numpy.argmax conventions).  stage_begin sets n_past on the device; every stage_step
 * enqueues one step on the model's stream without waiting (captured as a hipGraph when the
 * graph is on) and advances the device n_past, so a caller can queue steps and the
 * collective sends / receives between them on that stream without a host round trip.
 * vsim_model_sync waits for the model's stream. */
int vsim_model_stage_bind(vsim_model *m, const int32_t *tok_in, const float *resid_in, float *resid_out,
                          int32_t *tok_out);
int vsim_model_stage_begin(vsim_model *m, int n_past);
int vsim_model_stage_step(vsim_model *m);
int vsim_model_sync(vsim_model *m);
/* Test support: size the scratch for n_tokens and fill every scratch buffer and the whole KV
 * cache (every reserved sequence slot) with NaN, so that a kernel reading bytes no earlier kernel wrote shows up as a
 * changed (NaN) result.  Results of later evals must not depend on it. */
int vsim_model_debug_poison(vsim_model *m, int n_tokens);
/* Decode-step timing helpers for bench.py: the stream the executor launches on, and
 * device pointers of the last logits / residual buffers. */
void *vsim_model_stream(vsim_model *m);
const float *vsim_model_logits_dev(vsim_model *m);
/* Number of kernels one eval launches; whether the decode step replays a hipGraph. */
int vsim_model_info(vsim_model *m, int *kernels_per_eval, int *graph_enabled, size_t *weight_bytes);
int vsim_model_set_graph(vsim_model *m, int enable);
/* Per-kernel profiling for the live roofline: when enabled (this resets the totals), the
 * decode step runs without its hipGraph and an event pair on the model's stream brackets
 * every launch, tagged with the kernel's name and the algorithmic bytes it moves (Q4_0
 * weights at 0.625 B/weight, KV rows read and written, LayerNorm rows).
 * profile_kernel(i): totals of the i-th kernel name seen (VSIM_EINVAL past the last);
 * profile_stats: the sums over all of them. */
int vsim_model_set_profile(vsim_model *m, int enable);
int vsim_model_profile_kernel(vsim_model *m, int i, char *name, int name_cap, double *ms, long *launches,
                              double *bytes);
int vsim_model_profile_stats(vsim_model *m, double *gemv_ms, long *gemv_launches, double *gemv_bytes);
void vsim_model_free(vsim_model *m);

/* ------------------------------------------------------------- 4. file quantizer ---- */
/* The reference's quantize_gptneox / quantize_gptj / quantize_bloom (type 2, Q4_0) as one call:
 * magic, header and vocab are copied with the header's last field (f16) set to 2; a record that is
 * 2-D and whose name ends in "weight" must have ftype 0 (F32) or 1 (F16) and is rewritten as Q4_0
 * (ftype 2, vsim_op_q4_quantize_w's semantics, NaN rule included); every other record is copied
 * byte for byte.  The file streams through in row chunks, so memory is bounded and record sizes
 * are size_t.  device >= 0: k_quantize_w's AoS output on that GPU; device == -1: a plain host
 * loop with the same semantics (no GPU needed).  Failures are VSIM_EFILE with a reason (bad magic;
 * a truncated header, vocab or record; a 2-D weight of ftype 2 or 3; ne[0] % 32 != 0; an unknown
 * ftype) and remove the partly written output file.
 * st (may be NULL): the histogram of all codes, the bytes read and written, the records
 * quantized and copied. */
typedef struct {
  uint64_t hist[16];
  uint64_t bytes_in, bytes_out;
  int32_t n_quantized, n_copied;
} vsim_quantize_stats;
int vsim_quantize_file(const char *in, const char *out, int arch, int device, vsim_quantize_stats *st);
/* 1: vsim_quantize_file prints one line per record to stdout (name, shape, source type, sizes,
 * the record's histogram as fractions) and the totals.  Process-wide; returns the previous value. */
int vsim_quantize_set_verbose(int on);

#ifdef __cplusplus
}
#endif

#endif /* VSIM_HIP_H */
