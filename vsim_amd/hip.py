"""ctypes binding of libvsim_hip.so (include/vsim_hip.h).

The HIP library is the product; this module only marshals arguments.  There is no
CPU fallback: if the library is missing or a call fails, an exception is raised.
Device buffers are torch tensors on a ROCm device (torch is plumbing here: memory and
streams), passed to the C-ABI as raw pointers.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VSIM_LIB") or os.path.join(HERE, "_build", "libvsim_hip.so")  # VSIM_LIB: A/B builds

MODE_EXACT = 0
MODE_FAST = 1
MODE_W4A16 = 2  # weight-only: Q4_0 weights x fp16 activation rows, fp32 accumulation
W4A16_NONFINITE = -2**31  # VSIM_W4A16_NONFINITE: the exponent of a row that holds a NaN or an Inf
ARCH_GPTNEOX = 0
ARCH_GPTJ = 1
ARCH_BLOOM = 2

# symbols declared in include/vsim_hip.h (checked by tests/test_capi.py)
EXPORTS = [
    "vsim_last_error", "vsim_device_count", "vsim_q4_bytes",
    "init_xmax", "imax_ggml_compute_forward_mul_mat_q4_0_f32",
    "vsim_ggml_gptneox_rope_f32", "vsim_ggml_rope_f32", "vsim_ggml_soft_max_f32", "vsim_ggml_mul_mat_f32",
    "vsim_dropin_stats", "vsim_dropin_reset", "vsim_norm_fallbacks", "vsim_spin_timeouts",
    "vsim_op_q4_repack", "vsim_op_q4_unpack", "vsim_op_act_repack", "vsim_op_act_unpack",
    "vsim_op_q4_quantize", "vsim_op_q4_gemv", "vsim_op_q4_expand_f16", "vsim_op_gemm_f16",
    "vsim_op_act_quant_f16", "vsim_op_gemm_f16_gelu_q", "vsim_op_gemm_f16_rope", "vsim_op_gemm_f16_join",
    "vsim_op_gemm_q4_256", "vsim_op_get_rows",
    "vsim_op_norm", "vsim_op_gelu", "vsim_op_argmax", "vsim_op_attn_softmax", "vsim_op_rope", "vsim_op_kq", "vsim_op_kqv", "vsim_op_kq_causal", "vsim_op_kqv_causal",
    "vsim_op_attn_prefill", "vsim_op_attn_prefill_q16", "vsim_gemm_set_streamk", "vsim_gemm_set_qk_pair", "vsim_gemm_set_tile_order", "vsim_op_gemm_q4_256_pair", "vsim_op_norm_f16q",
    "vsim_op_tables", "vsim_op_fast_gemv", "vsim_op_fast_tail", "vsim_op_fast_oproj_join",
    "vsim_model_create", "vsim_model_load_file", "vsim_model_set_tensor", "vsim_model_get_tensor",
    "vsim_model_randomize",
    "vsim_model_set_mode", "vsim_model_reserve", "vsim_model_hparams", "vsim_model_eval", "vsim_model_eval_argmax", "vsim_model_generate",
    "vsim_model_stream",
    "vsim_model_logits_dev", "vsim_model_info", "vsim_model_set_graph", "vsim_model_set_profile",
    "vsim_model_profile_kernel", "vsim_model_profile_stats", "vsim_model_free",
    "vsim_graph_compute", "vsim_graph_compute_rc", "vsim_graph_sync_tensor", "vsim_graph_reset", "vsim_graph_stats",
    "vsim_graph_set_profile", "vsim_graph_profile_report", "vsim_graph_match", "vsim_graph_fast_stats",
    "vsim_model_stage_bind", "vsim_model_stage_begin", "vsim_model_stage_step", "vsim_model_sync",
    "vsim_model_debug_poison",
    "vsim_op_topk", "vsim_sampler_create", "vsim_sampler_accept", "vsim_sampler_pick", "vsim_sampler_sample_host",
    "vsim_sampler_stats", "vsim_sampler_free", "vsim_model_eval_sample", "vsim_model_generate_sampled",
    "vsim_op_q4_quantize_w", "vsim_model_load_file_ex", "vsim_model_set_tensor_src", "vsim_quantize_set_chunk_rows",
    "vsim_quantize_file", "vsim_quantize_set_verbose",
    "vsim_op_logprob", "vsim_model_eval_score", "vsim_score_set_chunk_rows",
    "vsim_op_q4_gemm_rows", "vsim_batch_set_gemm", "vsim_op_attn_decode_batch",
    "vsim_model_seq_reserve", "vsim_model_eval_seq", "vsim_model_decode_batch",
    "vsim_op_q4_gemm_fast_rows", "vsim_batch_set_fast_gemm", "vsim_model_decode_batch_fast",
    "vsim_op_attn_prefill_layout", "vsim_op_attn_prefill_scratch", "vsim_op_gemm_q4_256_h16",
    "vsim_op_gemm_q4_256_pair_h16",
    "vsim_op_topk_rows", "vsim_topk_rows_set_wg", "vsim_model_decode_batch_sample", "vsim_model_seq_copy",
    "vsim_op_tail_attn", "vsim_op_tail_ln", "vsim_op_tail_ln_ws_bytes",
    "vsim_op_w4a16_rows", "vsim_op_q4_gemm_w4a16_rows", "vsim_model_decode_batch_w4a16",
    "vsim_model_decode_batch_sample_w4a16",
    "vsim_op_ln_quant", "vsim_op_gemv_batch",
    "vsim_op_w4a16_ln", "vsim_op_w4a16_gelu", "vsim_op_w4a16_gemv", "vsim_w4a16_set_step",
    "vsim_op_q4_gemm_w4a16_tile", "vsim_w4a16_set_tile_gemm",
    "vsim_w4a16_set_attn", "vsim_op_attn_w4a16_prompt", "vsim_op_attn_w4a16_rows",
    "vsim_op_gemm_q4_f16x", "vsim_op_rope_kv_write", "vsim_op_add_residual", "vsim_op_add_rows",
    "vsim_op_gelu_bias", "vsim_op_attn_softmax_alibi", "vsim_op_alibi_slopes", "vsim_op_kqv_causal_merged",
    "vsim_op_attn_decode_runs", "vsim_op_attn_w4a16_runs", "vsim_model_decode_runs",
]

BATCH_MAX = 32  # VSIM_BATCH_MAX
W4A16_TILE_MIN_N = 33  # product_plan.hpp: a weight-only prompt of this many rows runs k_gemm_w4a16_tile

SRC_F32, SRC_F16 = 0, 1  # VSIM_SRC_*
LOAD_QUANTIZE = 1        # VSIM_LOAD_QUANTIZE

TOPK_MAX = 64      # VSIM_TOPK_MAX
WINDOW_MAX = 1024  # VSIM_WINDOW_MAX

_lib = None


class VsimError(RuntimeError):
    pass


# ggml ABI mirrors (include/ggml_abi.h; offsets checked against the reference's ggml.h by
# tests/test_capi.py): for callers that hand host tensors to the drop-in hooks.
GGML_TYPE_Q4_0, GGML_TYPE_I32, GGML_TYPE_F32 = 0, 4, 6
GGML_TASK_INIT, GGML_TASK_COMPUTE, GGML_TASK_FINALIZE = 0, 1, 2


class GgmlTensor(ctypes.Structure):
    _fields_ = [("type", ctypes.c_int), ("n_dims", ctypes.c_int), ("ne", ctypes.c_int * 4),
                ("nb", ctypes.c_size_t * 4), ("op", ctypes.c_int), ("is_param", ctypes.c_bool),
                ("grad", ctypes.c_void_p), ("src0", ctypes.c_void_p), ("src1", ctypes.c_void_p),
                ("opt", ctypes.c_void_p * 4), ("n_tasks", ctypes.c_int), ("perf_runs", ctypes.c_int),
                ("perf_cycles", ctypes.c_int64), ("perf_time_us", ctypes.c_int64), ("data", ctypes.c_void_p),
                ("padding", ctypes.c_char * 8)]


class GgmlComputeParams(ctypes.Structure):
    _fields_ = [("type", ctypes.c_int), ("ith", ctypes.c_int), ("nth", ctypes.c_int), ("wsize", ctypes.c_size_t),
                ("wdata", ctypes.c_void_p)]


def ggml_f32(buf, ne, nb=None, typ=GGML_TYPE_F32):
    """A host ggml_tensor over numpy array `buf` (kept alive by the caller) with shape ne and
    byte strides nb (contiguous when None)."""
    ne = list(ne) + [1] * (4 - len(ne))
    nb = [4] if nb is None else list(nb)
    while len(nb) < 4:  # the missing outer strides as ggml sets them: nb[i] = nb[i-1] * ne[i-1]
        nb.append(nb[-1] * ne[len(nb) - 1])
    t = GgmlTensor()
    t.type = typ
    t.n_dims = 4
    for i in range(4):
        t.ne[i] = ne[i]
        t.nb[i] = nb[i]
    t.data = buf.ctypes.data
    return t


class SampleParams(ctypes.Structure):
    _fields_ = [("seed", ctypes.c_int32), ("top_k", ctypes.c_int32), ("repeat_last_n", ctypes.c_int32),
                ("top_p", ctypes.c_float), ("temp", ctypes.c_float), ("repeat_penalty", ctypes.c_float)]


class TopkParams(ctypes.Structure):
    """vsim_topk_params (include/vsim_hip.h): one row's block for topk_rows, 4,120 bytes."""
    _fields_ = [("scale", ctypes.c_double), ("penalty", ctypes.c_double), ("k", ctypes.c_int32),
                ("nw", ctypes.c_int32), ("win", ctypes.c_int32 * WINDOW_MAX)]


class TopkOut(ctypes.Structure):
    """vsim_topk_out: one row's candidates, 768 bytes."""
    _fields_ = [("val", ctypes.c_double * TOPK_MAX), ("id", ctypes.c_int32 * TOPK_MAX)]


TOPK_PARAMS_DTYPE = np.dtype([("scale", "<f8"), ("penalty", "<f8"), ("k", "<i4"), ("nw", "<i4"),
                              ("win", "<i4", (WINDOW_MAX,))])
TOPK_OUT_DTYPE = np.dtype([("val", "<f8", (TOPK_MAX,)), ("id", "<i4", (TOPK_MAX,))])


# the fast decode step's launches (vsim_op_fast_* in include/vsim_hip.h)
FAST_PAD = 65536  # VSIM_FAST_PAD: readable bytes a weight needs after its last block
FE_STORE, FE_GELU_Q, FE_ROPE_Q, FE_ROPE_K, FE_V = range(5)


class FastJob(ctypes.Structure):
    _fields_ = [("w", ctypes.c_void_p), ("rows", ctypes.c_int32), ("k", ctypes.c_int32), ("bias", ctypes.c_void_p),
                ("y", ctypes.c_void_p), ("epi", ctypes.c_int32), ("act", ctypes.c_int32)]


class FastGemvArgs(ctypes.Structure):
    _fields_ = [("xq", ctypes.c_void_p * 2), ("lnx", ctypes.c_void_p), ("lnw", ctypes.c_void_p * 2),
                ("lnb", ctypes.c_void_p * 2), ("j", FastJob * 4), ("nj", ctypes.c_int32), ("oq", ctypes.c_void_p),
                ("n_past", ctypes.c_void_p), ("cs", ctypes.c_void_p), ("d", ctypes.c_int32),
                ("n_rot", ctypes.c_int32), ("style", ctypes.c_int32), ("clear", ctypes.c_void_p),
                ("nclear", ctypes.c_int32)]


class FastTailArgs(ctypes.Structure):
    _fields_ = [("wf", ctypes.c_void_p), ("rows", ctypes.c_int32), ("k", ctypes.c_int32), ("sf", ctypes.c_int32),
                ("xf", ctypes.c_void_p), ("ffp", ctypes.c_void_p), ("q", ctypes.c_void_p), ("kc", ctypes.c_void_p),
                ("vc", ctypes.c_void_p), ("n_past", ctypes.c_void_p), ("d", ctypes.c_int32), ("H", ctypes.c_int32),
                ("nchunk", ctypes.c_int32), ("scale", ctypes.c_float), ("part", ctypes.c_void_p),
                ("hcnt", ctypes.c_void_p), ("oq", ctypes.c_void_p)]


class AttnBatchArgs(ctypes.Structure):
    """vsim_attn_batch_args (include/vsim_hip.h)."""
    _fields_ = [("q", ctypes.c_void_p), ("k", ctypes.c_void_p), ("v", ctypes.c_void_p), ("kc", ctypes.c_void_p),
                ("vc", ctypes.c_void_p), ("n_past", ctypes.c_void_p), ("cs", ctypes.c_void_p),
                ("alibi", ctypes.c_void_p), ("B", ctypes.c_int32), ("d", ctypes.c_int32), ("H", ctypes.c_int32),
                ("n_rot", ctypes.c_int32), ("style", ctypes.c_int32), ("n_ctx", ctypes.c_int32),
                ("kqv_nth", ctypes.c_int32), ("scale", ctypes.c_float), ("out", ctypes.c_void_p),
                ("oq", ctypes.c_void_p), ("oxd", ctypes.c_void_p)]


class TailLnArgs(ctypes.Structure):
    """vsim_tail_ln_args (include/vsim_hip.h)."""
    _fields_ = [("attn", AttnBatchArgs), ("nsplit", ctypes.c_int32), ("K", ctypes.c_int32), ("wo", ctypes.c_void_p),
                ("wf", ctypes.c_void_p), ("xd", ctypes.c_void_p), ("x", ctypes.c_void_p), ("ab", ctypes.c_void_p),
                ("fb", ctypes.c_void_p), ("w1", ctypes.c_void_p), ("b1", ctypes.c_void_p), ("w2", ctypes.c_void_p),
                ("b2", ctypes.c_void_p), ("jout", ctypes.c_void_p), ("q1", ctypes.c_void_p), ("xd1", ctypes.c_void_p),
                ("q2", ctypes.c_void_p), ("xd2", ctypes.c_void_p), ("epoch", ctypes.c_uint32), ("il", ctypes.c_int32),
                ("ws", ctypes.c_void_p), ("ws_bytes", ctypes.c_size_t)]


class LnQuantArgs(ctypes.Structure):
    """vsim_ln_quant_args (include/vsim_hip.h)."""
    _fields_ = [("x", ctypes.c_void_p), ("n", ctypes.c_int32), ("w1", ctypes.c_void_p), ("b1", ctypes.c_void_p),
                ("q1", ctypes.c_void_p), ("xd1", ctypes.c_void_p), ("w2", ctypes.c_void_p), ("b2", ctypes.c_void_p),
                ("q2", ctypes.c_void_p), ("xd2", ctypes.c_void_p), ("ja", ctypes.c_void_p), ("jab", ctypes.c_void_p),
                ("jf", ctypes.c_void_p), ("jfb", ctypes.c_void_p), ("jout", ctypes.c_void_p),
                ("epoch", ctypes.c_void_p)]


class GemvBatchJob(ctypes.Structure):
    """vsim_gemv_batch_job (include/vsim_hip.h)."""
    _fields_ = [("w", ctypes.c_void_p), ("M", ctypes.c_int32), ("K", ctypes.c_int32), ("xd", ctypes.c_void_p),
                ("bias", ctypes.c_void_p), ("y", ctypes.c_void_p), ("gelu_q", ctypes.c_int32),
                ("oq", ctypes.c_void_p), ("oxd", ctypes.c_void_p)]


class GemvBatchArgs(ctypes.Structure):
    """vsim_gemv_batch_args (include/vsim_hip.h)."""
    _fields_ = [("j", GemvBatchJob * 4), ("nj", ctypes.c_int32)]


class W4a16LnArgs(ctypes.Structure):
    """vsim_w4a16_ln_args (include/vsim_hip.h)."""
    _fields_ = [("x", ctypes.c_void_p), ("n", ctypes.c_int32), ("w1", ctypes.c_void_p), ("b1", ctypes.c_void_p),
                ("x16_1", ctypes.c_void_p), ("e1", ctypes.c_void_p), ("w2", ctypes.c_void_p), ("b2", ctypes.c_void_p),
                ("x16_2", ctypes.c_void_p), ("e2", ctypes.c_void_p)]


class W4a16GemvJob(ctypes.Structure):
    """vsim_w4a16_gemv_job (include/vsim_hip.h)."""
    _fields_ = [("w", ctypes.c_void_p), ("M", ctypes.c_int32), ("K", ctypes.c_int32), ("x16", ctypes.c_void_p),
                ("e", ctypes.c_void_p), ("bias", ctypes.c_void_p), ("res", ctypes.c_void_p),
                ("res_a", ctypes.c_void_p), ("y", ctypes.c_void_p)]


class W4a16GemvArgs(ctypes.Structure):
    """vsim_w4a16_gemv_args (include/vsim_hip.h)."""
    _fields_ = [("j", W4a16GemvJob * 4), ("nj", ctypes.c_int32)]


class QuantizeStats(ctypes.Structure):
    _fields_ = [("hist", ctypes.c_uint64 * 16), ("bytes_in", ctypes.c_uint64), ("bytes_out", ctypes.c_uint64),
                ("n_quantized", ctypes.c_int32), ("n_copied", ctypes.c_int32)]


class HParams(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in
                ("n_vocab", "n_embd", "n_head", "n_layer", "n_rot", "use_parallel_residual")]


def lib():
    """Load libvsim_hip.so (raises if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise VsimError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
    L = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    vp, ci, cf, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
    L.vsim_last_error.restype = ctypes.c_char_p
    L.vsim_q4_bytes.restype = sz
    L.vsim_q4_bytes.argtypes = [ci, ci]
    L.vsim_op_q4_repack.argtypes = [vp, vp, ci, ci, vp]
    L.vsim_op_q4_unpack.argtypes = [vp, vp, ci, ci, vp]
    L.vsim_op_act_repack.argtypes = [vp, vp, ci, ci, vp]
    L.vsim_op_act_unpack.argtypes = [vp, vp, ci, ci, vp]
    L.vsim_op_q4_quantize.argtypes = [vp, ci, ci, vp, vp, vp]
    L.vsim_op_q4_gemv.argtypes = [vp, ci, ci, vp, vp, ci, vp, vp, ci, vp]
    L.vsim_op_get_rows.argtypes = [vp, ci, ci, vp, ci, vp, vp]
    L.vsim_op_q4_expand_f16.argtypes = [vp, ci, ci, vp, vp]
    L.vsim_op_gemm_f16.argtypes = [vp, ci, ci, vp, ci, vp, vp, vp]
    L.vsim_op_act_quant_f16.argtypes = [vp, ci, ci, vp, ci, vp, vp]
    L.vsim_op_gemm_f16_gelu_q.argtypes = [vp, ci, ci, vp, ci, vp, vp, vp]
    L.vsim_op_gemm_f16_rope.argtypes = [vp, ci, ci, vp, ci, vp, vp, vp, ci, ci, ci, vp]
    L.vsim_op_gemm_f16_join.argtypes = [vp, ci, ci, vp, ci, vp, vp, vp, vp]
    L.vsim_op_gemm_q4_256.argtypes = [vp, ci, ci, vp, ci, vp, vp, vp, vp, ci, ci, ci, ci, vp, vp]
    L.vsim_op_norm.argtypes = [vp, vp, ci, ci, vp, vp, vp]
    L.vsim_op_gelu.argtypes = [vp, vp, ci, vp]
    L.vsim_op_argmax.argtypes = [vp, ci, vp, vp]
    L.vsim_op_attn_softmax.argtypes = [vp, ci, ci, ci, ci, cf, vp]
    L.vsim_op_rope.argtypes = [ci, vp, ci, ci, ci, ci, ci, ci, vp]
    L.vsim_op_kq.argtypes = [vp, ci, vp, ci, ci, ci, ci, ci, vp, vp]
    L.vsim_op_kqv.argtypes = [vp, ci, vp, ci, ci, ci, ci, vp, vp]
    L.vsim_op_kq_causal.argtypes = [vp, ci, vp, ci, ci, ci, ci, ci, ci, vp, vp]
    L.vsim_op_kqv_causal.argtypes = [vp, ci, vp, ci, ci, ci, ci, ci, vp, vp]
    L.vsim_op_attn_prefill.argtypes = [vp, vp, vp, ci, ci, ci, ci, cf, vp, vp]
    L.vsim_op_attn_prefill_q16.argtypes = [vp, vp, vp, ci, ci, ci, ci, cf, vp, vp]
    L.vsim_gemm_set_streamk.argtypes = [ci]
    L.vsim_gemm_set_qk_pair.argtypes = [ci]
    L.vsim_gemm_set_tile_order.argtypes = [ci]
    L.vsim_op_gemm_q4_256_pair.argtypes = [vp, vp, ci, ci, vp, ci, vp, vp, vp, ci, ci, ci, vp]
    L.vsim_op_norm_f16q.argtypes = [vp, ci, ci, vp, vp, vp, vp]
    L.vsim_op_attn_prefill_layout.argtypes = [ci, ci, ctypes.POINTER(sz), ctypes.POINTER(sz), ctypes.POINTER(ci)]
    L.vsim_op_attn_prefill_scratch.argtypes = [vp, vp, vp, ci, ci, ci, ci, cf, vp, vp, vp, sz, ci, vp]
    L.vsim_op_gemm_q4_256_h16.argtypes = [vp, ci, ci, vp, ci, vp, vp, vp, ci, ci, ci, vp, ci, ci, vp]
    L.vsim_op_gemm_q4_256_pair_h16.argtypes = [vp, vp, ci, ci, vp, ci, vp, vp, vp, ci, ci, ci, vp, vp]
    L.vsim_op_tables.argtypes = [vp, vp]
    L.vsim_op_fast_gemv.argtypes = [ctypes.POINTER(FastGemvArgs), vp]
    L.vsim_op_fast_tail.argtypes = [ctypes.POINTER(FastTailArgs), vp]
    L.vsim_op_fast_oproj_join.argtypes = [vp, ci, vp, vp, vp, ci, vp, vp, vp, vp]
    L.vsim_model_create.argtypes = [ci, ctypes.POINTER(HParams), ci, ci, ci, ci, ctypes.POINTER(vp)]
    L.vsim_model_load_file.argtypes = [ctypes.c_char_p, ci, ci, ci, ci, ci, ctypes.POINTER(vp)]
    L.vsim_model_set_tensor.argtypes = [vp, ctypes.c_char_p, vp, sz]
    L.vsim_model_get_tensor.argtypes = [vp, ctypes.c_char_p, vp, sz]
    L.vsim_model_randomize.argtypes = [vp, ctypes.c_uint64, cf]
    L.vsim_model_set_mode.argtypes = [vp, ci]
    L.vsim_model_reserve.argtypes = [vp, ci]
    L.vsim_model_set_graph.argtypes = [vp, ci]
    L.vsim_model_hparams.argtypes = [vp, ctypes.POINTER(HParams), ctypes.POINTER(ci), ctypes.POINTER(ci),
                                     ctypes.POINTER(ci)]
    L.vsim_model_eval.argtypes = [vp, ci, vp, ci, vp, vp, vp]
    L.vsim_model_eval_argmax.argtypes = [vp, ci, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32)]
    L.vsim_model_generate.argtypes = [vp, ci, ctypes.c_int32, ci, ctypes.POINTER(ctypes.c_int32)]
    L.vsim_model_stream.restype = vp
    L.vsim_model_stream.argtypes = [vp]
    L.vsim_model_logits_dev.restype = vp
    L.vsim_model_logits_dev.argtypes = [vp]
    L.vsim_model_info.argtypes = [vp, ctypes.POINTER(ci), ctypes.POINTER(ci), ctypes.POINTER(sz)]
    L.vsim_model_free.argtypes = [vp]
    L.vsim_model_set_profile.argtypes = [vp, ci]
    L.vsim_model_profile_stats.argtypes = [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_long),
                                           ctypes.POINTER(ctypes.c_double)]
    L.vsim_model_profile_kernel.argtypes = [vp, ci, ctypes.c_char_p, ci, ctypes.POINTER(ctypes.c_double),
                                            ctypes.POINTER(ctypes.c_long), ctypes.POINTER(ctypes.c_double)]
    L.vsim_dropin_stats.argtypes = [ctypes.POINTER(ctypes.c_uint64)] * 4
    tp, pp = ctypes.POINTER(GgmlTensor), ctypes.POINTER(GgmlComputeParams)
    L.vsim_ggml_gptneox_rope_f32.argtypes = [pp, tp, tp, tp]
    L.vsim_ggml_rope_f32.argtypes = [pp, tp, tp, tp]
    L.vsim_ggml_soft_max_f32.argtypes = [pp, tp, tp]
    L.vsim_ggml_mul_mat_f32.argtypes = [pp, tp, tp, tp]
    L.vsim_graph_compute_rc.argtypes = [vp, vp]
    L.vsim_model_stage_bind.argtypes = [vp, vp, vp, vp, vp]
    L.vsim_model_stage_begin.argtypes = [vp, ci]
    L.vsim_model_stage_step.argtypes = [vp]
    L.vsim_model_sync.argtypes = [vp]
    L.vsim_model_debug_poison.argtypes = [vp, ci]
    L.vsim_graph_stats.argtypes = [ctypes.POINTER(ctypes.c_uint64)] * 4
    L.vsim_graph_set_profile.argtypes = [ci]
    L.vsim_graph_profile_report.argtypes = [ctypes.c_char_p, sz]
    cd, i32p = ctypes.c_double, ctypes.POINTER(ctypes.c_int32)
    L.vsim_op_topk.argtypes = [vp, ci, vp, ci, cd, cd, ci, vp, vp, vp]
    L.vsim_sampler_create.argtypes = [ctypes.POINTER(SampleParams), ctypes.POINTER(vp)]
    L.vsim_sampler_accept.argtypes = [vp, ctypes.c_int32]
    L.vsim_sampler_pick.argtypes = [vp, vp, vp, ci, i32p]
    L.vsim_sampler_sample_host.argtypes = [vp, vp, ci, i32p]
    L.vsim_sampler_stats.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
    L.vsim_sampler_free.restype = None
    L.vsim_sampler_free.argtypes = [vp]
    L.vsim_model_eval_sample.argtypes = [vp, vp, ci, ctypes.c_int32, i32p]
    L.vsim_model_generate_sampled.argtypes = [vp, vp, ci, ctypes.c_int32, ci, ctypes.c_int32, i32p,
                                              ctypes.POINTER(ci)]
    L.vsim_op_q4_quantize_w.argtypes = [vp, ci, ci, ci, vp, ci, ci, vp, vp, vp]
    L.vsim_model_load_file_ex.argtypes = [ctypes.c_char_p, ci, ci, ci, ci, ci, ci, ctypes.POINTER(vp)]
    L.vsim_model_set_tensor_src.argtypes = [vp, ctypes.c_char_p, vp, sz, ci]
    L.vsim_quantize_set_chunk_rows.argtypes = [ci]
    L.vsim_quantize_file.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ci, ci, ctypes.POINTER(QuantizeStats)]
    L.vsim_quantize_set_verbose.argtypes = [ci]
    L.vsim_op_logprob.argtypes = [vp, ci, ci, vp, vp, vp, vp]
    L.vsim_model_eval_score.argtypes = [vp, ci, vp, ci, vp, vp, vp, vp, vp]
    L.vsim_score_set_chunk_rows.argtypes = [ci]
    L.vsim_op_q4_gemm_rows.argtypes = [vp, ci, ci, vp, ci, vp, vp, vp]
    L.vsim_batch_set_gemm.argtypes = [ci]
    L.vsim_op_attn_decode_batch.argtypes = [ctypes.POINTER(AttnBatchArgs), vp]
    L.vsim_op_tail_attn.argtypes = [ctypes.POINTER(AttnBatchArgs), ci, vp]
    L.vsim_op_tail_ln.argtypes = [ctypes.POINTER(TailLnArgs), vp]
    L.vsim_op_tail_ln_ws_bytes.restype = sz
    L.vsim_op_tail_ln_ws_bytes.argtypes = [ci]
    L.vsim_model_seq_reserve.argtypes = [vp, ci]
    L.vsim_model_eval_seq.argtypes = [vp, ci, ci, vp, ci, vp]
    L.vsim_model_decode_batch.argtypes = [vp, ci, vp, vp, vp, vp, vp]
    L.vsim_op_q4_gemm_fast_rows.argtypes = [vp, ci, ci, vp, ci, vp, vp, vp]
    L.vsim_batch_set_fast_gemm.argtypes = [ci]
    L.vsim_model_decode_batch_fast.argtypes = [vp, ci, vp, vp, vp, vp, vp]
    L.vsim_op_topk_rows.argtypes = [vp, ci, ci, ci, vp, vp, vp]
    L.vsim_topk_rows_set_wg.argtypes = [ci]
    L.vsim_model_decode_batch_sample.argtypes = [vp, ci, ci, vp, vp, vp, ctypes.POINTER(vp), vp]
    L.vsim_model_seq_copy.argtypes = [vp, ci, ci, ci]
    L.vsim_op_w4a16_rows.argtypes = [vp, ci, ci, vp, vp, vp]
    L.vsim_op_q4_gemm_w4a16_rows.argtypes = [vp, ci, ci, vp, vp, ci, vp, vp, vp]
    L.vsim_model_decode_batch_w4a16.argtypes = [vp, ci, vp, vp, vp, vp, vp]
    L.vsim_model_decode_batch_sample_w4a16.argtypes = [vp, ci, vp, vp, vp, ctypes.POINTER(vp), vp]
    L.vsim_op_ln_quant.argtypes = [ctypes.POINTER(LnQuantArgs), vp]
    L.vsim_op_w4a16_ln.argtypes = [ctypes.POINTER(W4a16LnArgs), vp]
    L.vsim_op_w4a16_gelu.argtypes = [vp, vp, ci, vp, vp, vp, vp]
    L.vsim_op_w4a16_gemv.argtypes = [ctypes.POINTER(W4a16GemvArgs), vp]
    L.vsim_w4a16_set_step.argtypes = [ci]
    L.vsim_op_q4_gemm_w4a16_tile.argtypes = [vp, ci, ci, vp, vp, ci, vp, vp, vp]
    L.vsim_w4a16_set_tile_gemm.argtypes = [ci]
    L.vsim_w4a16_set_attn.argtypes = [ci]
    L.vsim_op_attn_w4a16_prompt.argtypes = [vp, vp, vp, ci, ci, ci, ci, cf, vp, vp, sz, vp]
    L.vsim_op_attn_w4a16_rows.argtypes = [ctypes.POINTER(AttnBatchArgs), vp]
    L.vsim_op_attn_decode_runs.argtypes = [ctypes.POINTER(AttnBatchArgs), vp]
    L.vsim_op_attn_w4a16_runs.argtypes = [ctypes.POINTER(AttnBatchArgs), vp]
    L.vsim_model_decode_runs.argtypes = [vp, ci, ci, vp, vp, vp, vp, vp, vp]
    L.vsim_op_gemv_batch.argtypes = [ctypes.POINTER(GemvBatchArgs), i32p, vp]
    L.vsim_op_gemm_q4_f16x.argtypes = [vp, ci, ci, vp, ci, vp, vp, vp]
    L.vsim_op_rope_kv_write.argtypes = [ci, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, vp]
    L.vsim_op_add_residual.argtypes = [vp, vp, vp, ci, ci, vp]
    L.vsim_op_add_rows.argtypes = [vp, vp, ci, vp]
    L.vsim_op_gelu_bias.argtypes = [vp, vp, ci, vp, ci, vp]
    L.vsim_op_attn_softmax_alibi.argtypes = [vp, ci, ci, ci, ci, cf, vp, vp]
    L.vsim_op_alibi_slopes.argtypes = [vp, ci]
    L.vsim_op_kqv_causal_merged.argtypes = [vp, ci, vp, ci, ci, ci, ci, ci, vp, vp]
    _lib = L
    return L


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = lib().vsim_last_error().decode(errors="replace")
        raise VsimError(f"{what} failed ({rc}): {msg}")


def ptr(t) -> int:
    """Raw pointer of a torch tensor or numpy array (None -> NULL)."""
    if t is None:
        return None
    if isinstance(t, np.ndarray):
        return t.ctypes.data
    return t.data_ptr()


def q4_bytes(rows: int, k: int) -> int:
    return int(lib().vsim_q4_bytes(rows, k))


def quantize_w(x, src_type, rows, k, w=None, w_rows=0, row0=0, aos=None, hist=None, stream=None):
    """vsim_op_q4_quantize_w on device buffers (torch tensors): x [rows][k] float32 (SRC_F32) or
    float16 (SRC_F16); w a W4T32 weight of w_rows rows of which rows [row0, row0 + rows) are written,
    aos the chunk's 20-byte blocks, hist 16 uint64 counters the caller zeroed (each may be None,
    but not both w and aos).  Enqueued on `stream`, not synchronized."""
    check(lib().vsim_op_q4_quantize_w(ptr(x), src_type, rows, k, ptr(w), w_rows, row0, ptr(aos), ptr(hist), stream),
          "q4_quantize_w")


def quantize_set_chunk_rows(rows: int) -> int:
    """Rows per staging chunk of the quantizing loader (0 = default); returns the previous value."""
    return int(lib().vsim_quantize_set_chunk_rows(int(rows)))


def quantize_file(src: str, dst: str, arch: int, device: int = 0) -> dict:
    """vsim_quantize_file: an F32 / F16 ggml file to Q4_0, on GPU `device` or (device = -1) on the
    host; returns the statistics."""
    st = QuantizeStats()
    check(lib().vsim_quantize_file(src.encode(), dst.encode(), arch, device, ctypes.byref(st)), f"quantize {src}")
    return {"hist": [int(v) for v in st.hist], "bytes_in": int(st.bytes_in), "bytes_out": int(st.bytes_out),
            "n_quantized": int(st.n_quantized), "n_copied": int(st.n_copied)}


class Sampler:
    """The reference's sampler as an object (vsim_sampler_* in include/vsim_hip.h): the last-n
    window, the generator, and the k-element finishing stage.  Host code: needs no GPU."""

    def __init__(self, seed=42, top_k=40, top_p=0.95, temp=0.8, repeat_last_n=64, repeat_penalty=1.3):
        self.h = ctypes.c_void_p()
        p = SampleParams(seed, top_k, repeat_last_n, top_p, temp, repeat_penalty)
        check(lib().vsim_sampler_create(ctypes.byref(p), ctypes.byref(self.h)), "sampler_create")

    def accept(self, token: int):
        """A token that was not sampled (the prompt's) enters the window."""
        check(lib().vsim_sampler_accept(self.h, int(token)), "sampler_accept")

    def pick(self, val, ids) -> int:
        """The finishing stage on an ordered candidate list (e.g. topk()'s); the token drawn."""
        v = np.ascontiguousarray(val, np.float64)
        i = np.ascontiguousarray(ids, np.int32)
        tok = ctypes.c_int32()
        check(lib().vsim_sampler_pick(self.h, ptr(v), ptr(i), int(v.size), ctypes.byref(tok)), "sampler_pick")
        return tok.value

    def sample_host(self, logits) -> int:
        """Both stages on the host from a logits row (the reference's code as it stands)."""
        lg = np.ascontiguousarray(logits, np.float32)
        tok = ctypes.c_int32()
        check(lib().vsim_sampler_sample_host(self.h, ptr(lg), int(lg.size), ctypes.byref(tok)), "sample_host")
        return tok.value

    def stats(self) -> dict:
        """Tokens drawn so far: by pick (device candidates) and by sample_host."""
        a, b = ctypes.c_uint64(), ctypes.c_uint64()
        check(lib().vsim_sampler_stats(self.h, ctypes.byref(a), ctypes.byref(b)), "sampler_stats")
        return {"device": a.value, "host": b.value}

    def close(self):
        if getattr(self, "h", None):
            lib().vsim_sampler_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def topk(x, n, win, scale, repeat_penalty, k, val, ids, stream=None):
    """vsim_op_topk on device buffers (torch tensors or raw addresses): x float32 [n] (an int
    address allows any 4-byte alignment), win int32 ids or None, val float64 [k], ids int32 [k].
    Enqueued on `stream` (a raw hipStream_t, None = the default stream), not synchronized."""
    def addr(t):
        return t if isinstance(t, int) or t is None else ptr(t)
    nw = 0 if win is None else int(win.numel() if hasattr(win, "numel") else win.size)
    check(lib().vsim_op_topk(addr(x), n, addr(win) if nw else None, nw, float(scale), float(repeat_penalty), k,
                             addr(val), addr(ids), stream), "topk")


def topk_rows(x, ldx, n, B, params, out, stream=None):
    """vsim_op_topk_rows on device buffers (torch tensors or raw addresses): x float32 [B][ldx] (an
    int address allows any 4-byte alignment), params B TopkParams blocks (a uint8 tensor holding
    TOPK_PARAMS_DTYPE records), out B TopkOut blocks (TOPK_OUT_DTYPE).  Row b's out.val[0:k_b],
    out.id[0:k_b] are topk()'s of that row alone.  Enqueued on `stream`, not synchronized."""
    def addr(t):
        return t if isinstance(t, int) or t is None else ptr(t)
    check(lib().vsim_op_topk_rows(addr(x), int(ldx), int(n), int(B), addr(params), addr(out), stream), "topk_rows")


def topk_rows_set_wg(per_row) -> int:
    """Workgroups per row of topk_rows (0: the default rule); same results whatever the setting.
    Returns the previous setting."""
    return int(lib().vsim_topk_rows_set_wg(int(per_row)))


def logprob(x, V, R, target, logprob, argmax, stream=None):
    """vsim_op_logprob on device buffers (torch tensors or raw addresses): x float32 [R][V] (an int
    address allows any 4-byte alignment), target int32 [R] or None (all -1), logprob float64 [R]
    and argmax int32 [R] (either may be None).  Per row: log-softmax of the target's logit with the
    sum in double and a fixed order, and the greedy id.  Enqueued on `stream`, not synchronized."""
    def addr(t):
        return t if isinstance(t, int) or t is None else ptr(t)
    check(lib().vsim_op_logprob(addr(x), V, R, addr(target), addr(logprob), addr(argmax), stream), "logprob")


def score_set_chunk_rows(rows: int) -> int:
    """Rows per head chunk of Model.score (0 = default); returns the previous value."""
    return int(lib().vsim_score_set_chunk_rows(int(rows)))


def q4_gemm_rows(w, M, K, xd, n, bias, y, stream=None):
    """vsim_op_q4_gemm_rows on device buffers (torch tensors): y [n][M] = the exact Q4_0 product
    of the W4T32 weight w [M][K] with the n (1..BATCH_MAX) activation rows whose factors are xd
    [n][K] (q4_quantize's), + bias [M] when given.  Enqueued on `stream`, not synchronized."""
    check(lib().vsim_op_q4_gemm_rows(ptr(w), M, K, ptr(xd), n, ptr(bias), ptr(y), stream), "q4_gemm_rows")


def batch_set_gemm(enable) -> int:
    """Product kernel of Model.decode_batch: 0 the GEMV-job path, 1 (default) k_gemm_exact_rows from
    the batch size on at which it was measured faster, 2 k_gemm_exact_rows always; same bits either
    way.  Returns the previous setting."""
    return int(lib().vsim_batch_set_gemm(int(enable)))


def q4_gemm_fast_rows(w, M, K, xq, n, bias, y, stream=None):
    """vsim_op_q4_gemm_fast_rows on device buffers (torch tensors): y [n][M] = the fast-mode Q4_0
    product of the W4T32 weight w [M][K] with the n (1..BATCH_MAX) activation rows xq (q4_quantize's
    Q4 SoA rows), + bias [M] when given; each value bit for bit q4_gemv's (n = 1, MODE_FAST) of
    that row alone.  Enqueued on `stream`, not synchronized."""
    check(lib().vsim_op_q4_gemm_fast_rows(ptr(w), M, K, ptr(xq), n, ptr(bias), ptr(y), stream), "q4_gemm_fast_rows")


def w4a16_rows(x, K, n, x16, e, stream=None):
    """vsim_op_w4a16_rows on device buffers (torch tensors): the weight-only mode's operand of the n
    (1..BATCH_MAX) f32 rows x [n][K]: x16 [n][K] float16 = fp16_rn(x * 2^e[row]), e int32 [n] (the
    exponent that puts the row's largest finite |x| into [2^14, 2^15); W4A16_NONFINITE and zeros for
    a row with a NaN or an Inf).  Enqueued on `stream`, not synchronized."""
    check(lib().vsim_op_w4a16_rows(ptr(x), K, n, ptr(x16), ptr(e), stream), "w4a16_rows")


def q4_gemm_w4a16_rows(w, M, K, x16, e, n, bias, y, stream=None):
    """vsim_op_q4_gemm_w4a16_rows on device buffers (torch tensors): y [n][M] = the W4T32 weight w
    [M][K] times the n (1..BATCH_MAX) rows of w4a16_rows' operand (x16, e), fp32 accumulation, + bias
    [M] when given; a row's outputs do not depend on n or on the other rows.  Enqueued on `stream`,
    not synchronized."""
    check(lib().vsim_op_q4_gemm_w4a16_rows(ptr(w), M, K, ptr(x16), ptr(e), n, ptr(bias), ptr(y), stream),
          "q4_gemm_w4a16_rows")


def q4_gemm_w4a16_tile(w, M, K, x16, e, n, bias, y, stream=None):
    """vsim_op_q4_gemm_w4a16_tile on device buffers (torch tensors): y [n][M] = the W4T32 weight w
    [M][K] times the n >= 1 rows of w4a16_rows' operand (x16, e) in one launch of the tile kernel; bit
    for bit q4_gemm_w4a16_rows on consecutive chunks of BATCH_MAX rows.  Enqueued on `stream`, not
    synchronized."""
    check(lib().vsim_op_q4_gemm_w4a16_tile(ptr(w), M, K, ptr(x16), ptr(e), n, ptr(bias), ptr(y), stream),
          "q4_gemm_w4a16_tile")


def w4a16_set_tile_gemm(v) -> int:
    """vsim_w4a16_set_tile_gemm: how a weight-only prompt batch's products run (0: the rows kernel on
    chunks of BATCH_MAX rows, 1: the tile kernel from its threshold on, 2: the tile kernel at every N;
    the same bits).  Returns the previous value."""
    return int(lib().vsim_w4a16_set_tile_gemm(int(v)))


def w4a16_ln(x, n, w1, b1, x16_1, e1, w2=None, b2=None, x16_2=None, e2=None, stream=None):
    """vsim_op_w4a16_ln on device buffers (torch tensors or None): the LayerNorm of the row x [n] with
    (w1, b1) straight to w4a16_rows' operand (x16_1, e1) of the normalized row, and with (w2, b2) to
    (x16_2, e2) when given; the bits of norm followed by w4a16_rows.  Enqueued on `stream`, not
    synchronized."""
    a = W4a16LnArgs(ptr(x), int(n), ptr(w1), ptr(b1), ptr(x16_1), ptr(e1), ptr(w2), ptr(b2), ptr(x16_2), ptr(e2))
    check(lib().vsim_op_w4a16_ln(ctypes.byref(a), stream), "w4a16_ln")


def w4a16_gelu(x, bias, K, x16, e, g=None, stream=None):
    """vsim_op_w4a16_gelu on device buffers (torch tensors or None): g = gelu(x + bias) of the row x [K]
    by the fp16 table, then w4a16_rows' operand (x16, e) of g; g [K] f32 also stored when given.
    Enqueued on `stream`, not synchronized."""
    check(lib().vsim_op_w4a16_gelu(ptr(x), ptr(bias), int(K), ptr(x16), ptr(e), ptr(g), stream), "w4a16_gelu")


def w4a16_gemv_args(jobs):
    """vsim_w4a16_gemv_args from jobs = [(w, M, K, x16, e, bias, res, res_a, y)], torch tensors or None."""
    a = W4a16GemvArgs()
    a.nj = len(jobs)
    for i, (w, M, K, x16, e, bias, res, res_a, y) in enumerate(jobs[:4]):
        a.j[i] = W4a16GemvJob(ptr(w), int(M), int(K), ptr(x16), ptr(e), ptr(bias), ptr(res), ptr(res_a), ptr(y))
    return a


def w4a16_gemv(jobs, stream=None):
    """vsim_op_w4a16_gemv on jobs (w4a16_gemv_args): up to four single-row products of W4T32 weights
    with w4a16_rows operands in one launch, each q4_gemm_w4a16_rows' bits at n = 1, then y = v,
    v + res or res + (res_a + v).  Enqueued on `stream`, not synchronized."""
    a = jobs if isinstance(jobs, W4a16GemvArgs) else w4a16_gemv_args(jobs)
    check(lib().vsim_op_w4a16_gemv(ctypes.byref(a), stream), "w4a16_gemv")


def w4a16_set_step(enable) -> int:
    """Weight-only mode's single-token step on (default) or off (every single-token call on the
    general path); same bits either way.  Process-wide; returns the previous setting."""
    return int(lib().vsim_w4a16_set_step(int(enable)))


def w4a16_set_attn(v) -> int:
    """vsim_w4a16_set_attn: weight-only mode's attention, 0 (default) the exact path's kernels, 1 the
    fp16 MFMA attention under its per-row contract on the models that take it (no ALiBi, head dim 64,
    96, 128 or 256, n_embd a multiple of 64).  Changes the mode's bits, not its promise.
    Process-wide; returns the previous setting."""
    return int(lib().vsim_w4a16_set_attn(int(v)))


def attn_prefill_layout(E, nk):
    """vsim_op_attn_prefill_layout: (bytes, V^T offset in halves, ldt) of the K16 / V^T scratch."""
    b, o, l = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_int()
    check(lib().vsim_op_attn_prefill_layout(int(E), int(nk), ctypes.byref(b), ctypes.byref(o), ctypes.byref(l)),
          "attn_prefill_layout")
    return b.value, o.value, l.value


def attn_w4a16_prompt(Q, kc, vc, d, H, N, n_past, scale, out, scratch, scratch_bytes=None, stream=None):
    """vsim_op_attn_w4a16_prompt on device buffers (torch tensors): the weight-only fp16 attention of
    N >= 1 queries Q [N][H d] (after RoPE) at positions n_past.. over the cache rows kc, vc
    [n_past + N][H d] into out [N][H d]; scratch a byte tensor of attn_prefill_layout(H d, n_past + N)'s
    size.  Enqueued on `stream`, not synchronized."""
    nb = int(scratch.numel() * scratch.element_size()) if scratch_bytes is None else int(scratch_bytes)
    check(lib().vsim_op_attn_w4a16_prompt(ptr(Q), ptr(kc), ptr(vc), d, H, N, n_past, float(scale), ptr(out),
                                          ptr(scratch), nb, stream), "attn_w4a16_prompt")


def attn_w4a16_rows(q, k, v, kc, vc, n_past, cs, B, d, H, n_rot, style, n_ctx, scale, out, stream=None):
    """vsim_op_attn_w4a16_rows on device buffers (torch tensors): attn_decode_batch's arguments without
    ALiBi and the Q4 row; out [B][H d] is required."""
    a = AttnBatchArgs(ptr(q), ptr(k), ptr(v), ptr(kc), ptr(vc), ptr(n_past), ptr(cs), None, B, d, H, n_rot,
                      style, n_ctx, 0, float(scale), ptr(out), None, None)
    check(lib().vsim_op_attn_w4a16_rows(ctypes.byref(a), stream), "attn_w4a16_rows")


def attn_w4a16_runs(q, k, v, kc, vc, n_past, cs, B, d, H, n_rot, style, n_ctx, scale, out, stream=None):
    """vsim_op_attn_w4a16_runs: attn_w4a16_rows' arguments for rows that may share a cache at distinct
    positions (runs of consecutive tokens): k_kv_rows, then the form without its cache writes."""
    a = AttnBatchArgs(ptr(q), ptr(k), ptr(v), ptr(kc), ptr(vc), ptr(n_past), ptr(cs), None, B, d, H, n_rot,
                      style, n_ctx, 0, float(scale), ptr(out), None, None)
    check(lib().vsim_op_attn_w4a16_runs(ctypes.byref(a), stream), "attn_w4a16_runs")


def batch_set_fast_gemm(enable) -> int:
    """How q4_gemm_fast_rows and Model.decode_batch_fast run their products: 0 one k_gemv_fast
    launch per row, 1 (default) k_gemm_fast_rows from the row count on at which it was measured
    faster, 2 k_gemm_fast_rows always; same bits either way.  Returns the previous setting."""
    return int(lib().vsim_batch_set_fast_gemm(int(enable)))


def attn_decode_batch(q, k, v, kc, vc, n_past, cs, alibi, B, d, H, n_rot, style, n_ctx, kqv_nth, scale, out, oq, oxd,
                      stream=None):
    """vsim_op_attn_decode_batch on device buffers (torch tensors): q, k, v [B][H d]; kc, vc int64
    tensors [B] holding each row's cache address; n_past int32 [B]; out may be None."""
    a = AttnBatchArgs(ptr(q), ptr(k), ptr(v), ptr(kc), ptr(vc), ptr(n_past), ptr(cs), ptr(alibi), B, d, H, n_rot,
                      style, n_ctx, kqv_nth, float(scale), ptr(out), ptr(oq), ptr(oxd))
    check(lib().vsim_op_attn_decode_batch(ctypes.byref(a), stream), "attn_decode_batch")


def attn_decode_runs(q, k, v, kc, vc, n_past, cs, alibi, B, d, H, n_rot, style, n_ctx, kqv_nth, scale, out, oq, oxd,
                     stream=None):
    """vsim_op_attn_decode_runs: attn_decode_batch's arguments for rows that may share a cache at
    distinct positions (runs of consecutive tokens): k_kv_rows, then the heads without their cache
    writes.  Row j of a run gets the bits of attn_decode_batch on it alone after the rows before it."""
    a = AttnBatchArgs(ptr(q), ptr(k), ptr(v), ptr(kc), ptr(vc), ptr(n_past), ptr(cs), ptr(alibi), B, d, H, n_rot,
                      style, n_ctx, kqv_nth, float(scale), ptr(out), ptr(oq), ptr(oxd))
    check(lib().vsim_op_attn_decode_runs(ctypes.byref(a), stream), "attn_decode_runs")


def tail_attn(q, k, v, kc, vc, n_past, cs, alibi, d, H, n_rot, style, n_ctx, kqv_nth, scale, out, oq, oxd, nsplit,
              stream=None):
    """vsim_op_tail_attn: one row of attn_decode_batch's operands (kc, vc int64 tensors [1]) through
    the fused layer tail's head role, each head over nsplit (1 or 2) workgroups."""
    a = AttnBatchArgs(ptr(q), ptr(k), ptr(v), ptr(kc), ptr(vc), ptr(n_past), ptr(cs), ptr(alibi), 1, d, H, n_rot,
                      style, n_ctx, kqv_nth, float(scale), ptr(out), ptr(oq), ptr(oxd))
    check(lib().vsim_op_tail_attn(ctypes.byref(a), int(nsplit), stream), "tail_attn")


def tail_ln_ws_bytes(E: int) -> int:
    """Bytes of a caller-owned tail_ln workspace for width E (zero it before its first use)."""
    return int(lib().vsim_op_tail_ln_ws_bytes(int(E)))


def tail_ln_args(attn, nsplit, wo, wf, xd, K, x, ab, fb, w1, b1, w2, b2, jout, q1, xd1, q2, xd2, epoch, il, ws=None):
    """vsim_tail_ln_args from an AttnBatchArgs (B = 1) and torch tensors (or None)."""
    nws = 0 if ws is None else int(ws.numel() * ws.element_size())
    return TailLnArgs(attn, int(nsplit), int(K), ptr(wo), ptr(wf), ptr(xd), ptr(x), ptr(ab), ptr(fb), ptr(w1), ptr(b1),
                      ptr(w2), ptr(b2), ptr(jout), ptr(q1), ptr(xd1), ptr(q2), ptr(xd2), int(epoch), int(il), ptr(ws),
                      nws)


def tail_ln(args, stream=None):
    """vsim_op_tail_ln: the fused layer tail with its LayerNorm on the operands of `args`
    (tail_ln_args); waits for the stream."""
    check(lib().vsim_op_tail_ln(ctypes.byref(args), stream), "tail_ln")


def ln_quant_args(x, n, w1, b1, q1, xd1, w2=None, b2=None, q2=None, xd2=None, ja=None, jab=None, jf=None, jfb=None,
                  jout=None, epoch=None):
    """vsim_ln_quant_args from torch tensors (or None)."""
    return LnQuantArgs(ptr(x), int(n), ptr(w1), ptr(b1), ptr(q1), ptr(xd1), ptr(w2), ptr(b2), ptr(q2), ptr(xd2),
                       ptr(ja), ptr(jab), ptr(jf), ptr(jfb), ptr(jout), ptr(epoch))


def ln_quant(args, stream=None):
    """vsim_op_ln_quant: k_ln_quant on the operands of `args` (ln_quant_args); stream-ordered."""
    check(lib().vsim_op_ln_quant(ctypes.byref(args), stream), "ln_quant")


def gemv_batch_args(jobs):
    """vsim_gemv_batch_args from jobs = [(w, M, K, xd, bias, y, gelu_q, oq, oxd)], torch tensors or None."""
    a = GemvBatchArgs()
    a.nj = len(jobs)
    for i, (w, M, K, xd, bias, y, gelu_q, oq, oxd) in enumerate(jobs[:4]):
        a.j[i] = GemvBatchJob(ptr(w), int(M), int(K), ptr(xd), ptr(bias), ptr(y), int(gelu_q), ptr(oq), ptr(oxd))
    return a


def gemv_batch(jobs, stream=None) -> int:
    """vsim_op_gemv_batch on jobs (gemv_batch_args); returns the kernel it chose: 1 k_gemv_solo, 0
    k_gemv_chain32.  Stream-ordered."""
    a = jobs if isinstance(jobs, GemvBatchArgs) else gemv_batch_args(jobs)
    kern = ctypes.c_int32(-1)
    check(lib().vsim_op_gemv_batch(ctypes.byref(a), ctypes.byref(kern), stream), "gemv_batch")
    return int(kern.value)


def fast_gemv(jobs, xq=(None, None), lnx=None, lnw=(None, None), lnb=(None, None), oq=None, n_past=None, cs=None,
              d=0, n_rot=0, style=0, clear=None, nclear=0, stream=None):
    """vsim_op_fast_gemv: jobs = [(w, rows, k, bias, y, epi, act)], operands torch tensors or None."""
    a = FastGemvArgs()
    for i in range(2):
        a.xq[i], a.lnw[i], a.lnb[i] = ptr(xq[i]), ptr(lnw[i]), ptr(lnb[i])
    a.lnx, a.oq, a.n_past, a.cs, a.clear = ptr(lnx), ptr(oq), ptr(n_past), ptr(cs), ptr(clear)
    a.d, a.n_rot, a.style, a.nclear, a.nj = d, n_rot, style, nclear, len(jobs)
    for i, (w, rows, k, bias, y, epi, act) in enumerate(jobs[:4]):
        a.j[i] = FastJob(ptr(w), rows, k, ptr(bias), ptr(y), epi, act)
    check(lib().vsim_op_fast_gemv(ctypes.byref(a), stream), "fast_gemv")


def fast_tail(wf, rows, k, sf, xf, ffp, q, kc, vc, n_past, d, H, nchunk, scale, part, hcnt, oq, stream=None):
    """vsim_op_fast_tail on torch tensors."""
    a = FastTailArgs(ptr(wf), rows, k, sf, ptr(xf), ptr(ffp), ptr(q), ptr(kc), ptr(vc), ptr(n_past), d, H, nchunk,
                     float(scale), ptr(part), ptr(hcnt), ptr(oq))
    check(lib().vsim_op_fast_tail(ctypes.byref(a), stream), "fast_tail")


def fast_oproj_join(w, E, xq, bo, ffp, sf, bproj, x, out, stream=None):
    """vsim_op_fast_oproj_join on torch tensors (bo may be None)."""
    check(lib().vsim_op_fast_oproj_join(ptr(w), E, ptr(xq), ptr(bo), ptr(ffp), sf, ptr(bproj), ptr(x), ptr(out),
                                        stream), "fast_oproj_join")


class Model:
    """Device-resident model executor (vsim_model_* in include/vsim_hip.h)."""

    def __init__(self, handle, arch):
        self.h = handle
        self.arch = arch
        hp = HParams()
        n_ctx, lb, le = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        check(lib().vsim_model_hparams(self.h, ctypes.byref(hp), ctypes.byref(n_ctx), ctypes.byref(lb),
                                       ctypes.byref(le)), "hparams")
        self.hp = hp
        self.n_ctx = n_ctx.value
        self.layer_begin, self.layer_end = lb.value, le.value
        self.n_vocab, self.n_embd = hp.n_vocab, hp.n_embd
        self.first = self.layer_begin == 0
        self.last = self.layer_end == hp.n_layer

    @classmethod
    def load(cls, path, arch, n_ctx=512, device=0, layer_begin=0, layer_end=-1, quantize=False):
        """quantize=True also takes the converters' F32 / F16 files, quantized on the device as they
        load (vsim_model_load_file_ex with VSIM_LOAD_QUANTIZE)."""
        h = ctypes.c_void_p()
        check(lib().vsim_model_load_file_ex(path.encode(), arch, n_ctx, device, layer_begin, layer_end,
                                            LOAD_QUANTIZE if quantize else 0, ctypes.byref(h)), f"load {path}")
        return cls(h, arch)

    @classmethod
    def create(cls, arch, hp: dict, n_ctx=512, device=0, layer_begin=0, layer_end=-1):
        h = ctypes.c_void_p()
        c = HParams(**hp)
        check(lib().vsim_model_create(arch, ctypes.byref(c), n_ctx, device, layer_begin, layer_end,
                                      ctypes.byref(h)), "create")
        return cls(h, arch)

    def randomize(self, seed=0, std=0.02):
        check(lib().vsim_model_randomize(self.h, seed, std), "randomize")

    def set_tensor_src(self, name: str, values: np.ndarray):
        """Upload one tensor as float32 / float16 values; a matrix is quantized into its Q4_0 slot."""
        v = np.ascontiguousarray(values)
        if v.dtype not in (np.float32, np.float16):
            raise TypeError("set_tensor_src takes float32 or float16 values")
        check(lib().vsim_model_set_tensor_src(self.h, name.encode(), ptr(v), v.nbytes,
                                              SRC_F16 if v.dtype == np.float16 else SRC_F32), f"set_tensor_src {name}")

    def get_tensor(self, name: str, nbytes: int) -> np.ndarray:
        """One tensor in the ggml file's format (Q4_0 AoS blocks / F32), as raw bytes."""
        buf = np.zeros(nbytes, np.uint8)
        check(lib().vsim_model_get_tensor(self.h, name.encode(), ptr(buf), nbytes), f"get_tensor {name}")
        return buf

    def set_mode(self, mode):
        check(lib().vsim_model_set_mode(self.h, mode), "set_mode")

    def reserve(self, n_tokens):
        """Allocates a prompt of up to n_tokens' buffers and loads its kernels ahead of the first eval."""
        check(lib().vsim_model_reserve(self.h, n_tokens), "reserve")

    def set_graph(self, enable: bool):
        check(lib().vsim_model_set_graph(self.h, 1 if enable else 0), "set_graph")

    def eval(self, n_past, tokens=None, resid_in=None, resid_out=None, want_logits=True):
        N = len(tokens) if tokens is not None else int(resid_in.shape[0])
        tok = np.ascontiguousarray(tokens, np.int32) if tokens is not None else None
        lg = np.zeros(self.n_vocab, np.float32) if (want_logits and self.last) else None
        check(lib().vsim_model_eval(self.h, n_past, ptr(tok), N, ptr(resid_in), ptr(resid_out), ptr(lg)), "eval")
        return lg

    def score(self, n_past, tokens=None, targets=None, resid_in=None, want_logits=False):
        """vsim_model_eval_score: the prompt pass over `tokens` (or a last stage's resid_in) at
        n_past, then per position the log-probability of targets[i] and the greedy id, computed on
        the device.  targets=None scores each token's successor: tokens[1:] + [-1] (-1: nothing
        to score).  Returns (logprob float64 [N], argmax int32 [N]) and, with want_logits, every
        logits row [N][n_vocab] too."""
        N = len(tokens) if tokens is not None else int(resid_in.shape[0])
        tok = np.ascontiguousarray(tokens, np.int32) if tokens is not None else None
        if targets is None:
            targets = list(tokens[1:]) + [-1] if tokens is not None else [-1] * N
        tgt = np.ascontiguousarray(targets, np.int32)
        if tgt.size != N:
            raise ValueError("score: one target per position")
        lp, am = np.zeros(N, np.float64), np.zeros(N, np.int32)
        lg = np.zeros((N, self.n_vocab), np.float32) if want_logits else None
        check(lib().vsim_model_eval_score(self.h, n_past, ptr(tok), N, ptr(resid_in), ptr(tgt), ptr(lp), ptr(am),
                                          ptr(lg)), "score")
        return (lp, am, lg) if want_logits else (lp, am)

    def seq_reserve(self, n_seq: int):
        """Give the model n_seq KV-cache slots (slot 0 is the cache every other call uses)."""
        check(lib().vsim_model_seq_reserve(self.h, int(n_seq)), "seq_reserve")

    def eval_seq(self, seq, n_past, tokens, want_logits=True):
        """Model.eval of `tokens` at n_past on sequence slot `seq`; the last row's logits."""
        tok = np.ascontiguousarray(tokens, np.int32)
        lg = np.zeros(self.n_vocab, np.float32) if want_logits else None
        check(lib().vsim_model_eval_seq(self.h, int(seq), int(n_past), ptr(tok), int(tok.size), ptr(lg)), "eval_seq")
        return lg

    def decode_batch(self, seqs, n_past, tokens, want_logits=True):
        """One decode step for len(seqs) sequences: row b feeds tokens[b] to slot seqs[b] at
        position n_past[b].  Returns (logits [B][n_vocab] or None, next int32 [B]: each row's
        greedy id, taken on the device)."""
        return self._decode_batch(lib().vsim_model_decode_batch, "decode_batch", seqs, n_past, tokens, want_logits)

    def decode_batch_fast(self, seqs, n_past, tokens, want_logits=True):
        """decode_batch with fast-mode products, whatever the model's mode: every row bit for bit
        eval_seq's row of that sequence on this model in MODE_FAST.  Same return shape."""
        return self._decode_batch(lib().vsim_model_decode_batch_fast, "decode_batch_fast", seqs, n_past, tokens,
                                  want_logits)

    def decode_batch_w4a16(self, seqs, n_past, tokens, want_logits=True):
        """decode_batch with weight-only products (MODE_W4A16), whatever the model's mode: every row
        bit for bit eval_seq's row of that sequence on this model in MODE_W4A16.  Same return shape."""
        return self._decode_batch(lib().vsim_model_decode_batch_w4a16, "decode_batch_w4a16", seqs, n_past, tokens,
                                  want_logits)

    def _decode_batch(self, fn, who, seqs, n_past, tokens, want_logits):
        sq = np.ascontiguousarray(seqs, np.int32)
        npst = np.ascontiguousarray(n_past, np.int32)
        tok = np.ascontiguousarray(tokens, np.int32)
        if not (sq.size == npst.size == tok.size):
            raise ValueError(f"{who}: one slot, position and token per row")
        B = int(sq.size)
        lg = np.zeros((B, self.n_vocab), np.float32) if want_logits else None
        nxt = np.zeros(max(B, 1), np.int32)
        check(fn(self.h, B, ptr(sq), ptr(npst), ptr(tok), ptr(lg), ptr(nxt)), who)
        return lg, nxt[:B]

    def decode_runs(self, seqs, n_past, runs, mode, want_logits=True):
        """vsim_model_decode_runs: one batched step in which slot seqs[s] takes the token list runs[s]
        at positions n_past[s], n_past[s] + 1, ..; mode (MODE_EXACT, MODE_FAST or MODE_W4A16) names the
        products.  Every row is bit for bit the one-row decode_batch* step of that mode on the slot
        after the rows before it.  Returns (logits [N][n_vocab] in run order or None, [next ids of
        each run as an int32 array])."""
        sq = np.ascontiguousarray(seqs, np.int32)
        npst = np.ascontiguousarray(n_past, np.int32)
        runs = [np.ascontiguousarray(r, np.int32).reshape(-1) for r in runs]
        if not (sq.size == npst.size == len(runs)):
            raise ValueError("decode_runs: one slot, position and run per sequence")
        ln = np.ascontiguousarray([r.size for r in runs], np.int32)
        tok = np.ascontiguousarray(np.concatenate(runs) if runs else [], np.int32)
        N = int(tok.size)
        lg = np.zeros((N, self.n_vocab), np.float32) if want_logits else None
        nxt = np.zeros(max(N, 1), np.int32)
        check(lib().vsim_model_decode_runs(self.h, int(mode), int(sq.size), ptr(sq), ptr(npst), ptr(ln), ptr(tok),
                                           ptr(lg), ptr(nxt)), "decode_runs")
        ends = np.cumsum(ln)
        return lg, [nxt[e - l:e] for e, l in zip(ends, ln)]

    def decode_batch_sample(self, seqs, n_past, tokens, samplers, fast=False, mode=None):
        """One sampled decode step for len(seqs) sequences: decode_batch (or decode_batch_fast), then
        row b's token drawn by samplers[b] -- the candidate stage of all rows in one launch on the
        device, the draw on the host.  Every row's token and sampler state are those of eval_sample
        on that sequence alone.  mode (MODE_EXACT, MODE_FAST or MODE_W4A16) names the step's numeric
        path and overrides `fast` when given.  Returns next int32 [B]."""
        if mode is None:
            mode = MODE_FAST if fast else MODE_EXACT
        sq = np.ascontiguousarray(seqs, np.int32)
        npst = np.ascontiguousarray(n_past, np.int32)
        tok = np.ascontiguousarray(tokens, np.int32)
        samplers = list(samplers)
        if not (sq.size == npst.size == tok.size == len(samplers)):
            raise ValueError("decode_batch_sample: one slot, position, token and sampler per row")
        B = int(sq.size)
        hs = (ctypes.c_void_p * max(B, 1))(*[None if sm is None else sm.h for sm in samplers])
        nxt = np.zeros(max(B, 1), np.int32)
        if int(mode) == MODE_W4A16:  # (an entry of its own: the C call's mode argument stays EXACT / FAST)
            check(lib().vsim_model_decode_batch_sample_w4a16(self.h, B, ptr(sq), ptr(npst), ptr(tok), hs, ptr(nxt)),
                  "decode_batch_sample")
        else:
            check(lib().vsim_model_decode_batch_sample(self.h, int(mode), B, ptr(sq), ptr(npst),
                                                       ptr(tok), hs, ptr(nxt)), "decode_batch_sample")
        return nxt[:B]

    def seq_copy(self, dst, src, n_tokens):
        """Slot fork: the first n_tokens cache rows of slot src go to slot dst (on the model's stream)."""
        check(lib().vsim_model_seq_copy(self.h, int(dst), int(src), int(n_tokens)), "seq_copy")

    def eval_argmax(self, n_past, token) -> int:
        """Greedy decode step: the next token (argmax of the logits, taken on the device)."""
        nxt = ctypes.c_int32()
        check(lib().vsim_model_eval_argmax(self.h, n_past, int(token), ctypes.byref(nxt)), "eval_argmax")
        return nxt.value

    def generate(self, n_past, token, n_steps) -> list:
        """n_steps greedy decode steps kept on the device; returns the generated tokens."""
        out = (ctypes.c_int32 * max(n_steps, 1))()
        check(lib().vsim_model_generate(self.h, n_past, int(token), n_steps, out), "generate")
        return list(out[:n_steps])

    def eval_sample(self, sampler: Sampler, n_past, token) -> int:
        """Sampled decode step: top-k of the penalised logits on the device, the draw on the host."""
        nxt = ctypes.c_int32()
        check(lib().vsim_model_eval_sample(self.h, sampler.h, n_past, int(token), ctypes.byref(nxt)), "eval_sample")
        return nxt.value

    def generate_sampled(self, sampler: Sampler, n_past, token, n_steps, eos=-1) -> list:
        """Up to n_steps sampled decode steps; stops after a step that produced `eos`."""
        out = (ctypes.c_int32 * max(n_steps, 1))()
        n = ctypes.c_int()
        check(lib().vsim_model_generate_sampled(self.h, sampler.h, n_past, int(token), n_steps, eos, out,
                                                ctypes.byref(n)), "generate_sampled")
        return list(out[:n.value])

    def info(self):
        k, g, w = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
        check(lib().vsim_model_info(self.h, ctypes.byref(k), ctypes.byref(g), ctypes.byref(w)), "info")
        return {"kernels_per_eval": k.value, "graph": bool(g.value), "weight_bytes": w.value}

    def set_profile(self, enable: bool):
        check(lib().vsim_model_set_profile(self.h, 1 if enable else 0), "set_profile")

    def profile_stats(self):
        ms, n, b = ctypes.c_double(), ctypes.c_long(), ctypes.c_double()
        check(lib().vsim_model_profile_stats(self.h, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(b)), "prof")
        return {"gemv_ms": ms.value, "gemv_launches": n.value, "gemv_bytes": b.value}

    def profile_kernels(self) -> list:
        """Per-kernel totals since set_profile(True): [{name, ms, launches, bytes}]."""
        out, i = [], 0
        name = ctypes.create_string_buffer(96)
        ms, n, b = ctypes.c_double(), ctypes.c_long(), ctypes.c_double()
        while lib().vsim_model_profile_kernel(self.h, i, name, 96, ctypes.byref(ms), ctypes.byref(n),
                                              ctypes.byref(b)) == 0:
            out.append({"name": name.value.decode(), "ms": ms.value, "launches": n.value, "bytes": b.value})
            i += 1
        return out

    def stream(self) -> int:
        return lib().vsim_model_stream(self.h)

    def stage_bind(self, tok_in=0, resid_in=0, resid_out=0, tok_out=0):
        """Bind the pipeline-stage buffers (device addresses, e.g. torch tensors' data_ptr())."""
        check(lib().vsim_model_stage_bind(self.h, tok_in or None, resid_in or None, resid_out or None,
                                          tok_out or None), "stage_bind")

    def stage_begin(self, n_past: int):
        check(lib().vsim_model_stage_begin(self.h, n_past), "stage_begin")

    def stage_step(self):
        """Enqueue one stage step on the model's stream (no wait)."""
        check(lib().vsim_model_stage_step(self.h), "stage_step")

    def sync(self):
        check(lib().vsim_model_sync(self.h), "sync")

    def debug_poison(self, n_tokens: int):
        """Fill the scratch and the KV cache with NaN (test support, include/vsim_hip.h)."""
        check(lib().vsim_model_debug_poison(self.h, n_tokens), "debug_poison")

    def close(self):
        if getattr(self, "h", None):
            lib().vsim_model_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def norm_fallbacks():
    """Exact-LayerNorm rows that took the sequential fallback so far: (mean, variance)."""
    out = (ctypes.c_uint * 2)()
    check(lib().vsim_norm_fallbacks(out), "norm_fallbacks")
    return int(out[0]), int(out[1])


def spin_timeouts():
    """Bounded cross-workgroup waits that gave up so far (0 in a healthy run)."""
    out = ctypes.c_uint()
    check(lib().vsim_spin_timeouts(ctypes.byref(out)), "spin_timeouts")
    return int(out.value)


def dropin_stats():
    v = [ctypes.c_uint64() for _ in range(4)]
    lib().vsim_dropin_stats(*[ctypes.byref(x) for x in v])
    return {"calls": v[0].value, "h2d": v[1].value, "d2h": v[2].value, "cached": v[3].value}
