"""fp64 restatement of one layer of a fast-mode prompt eval (run_layer in VSIM_MODE_FAST,
vsim_amd/csrc/model.cpp), stage by stage, with the bound each stage's device output has to meet.
numpy only.  Used by tests/test_gpu_fast_prompt_layer.py on the intermediates of the model's launches
made through the op entries, and shown to have teeth by tests/test_fast_prompt_ref_cpu.py.

The restatement is written from the reference's layer, not from run_layer: vsim.cpp:526-695 for
GPT-NeoX (both residual forms) and GPT-J (ggml_rope pairs, one norm, no q/k/v/out biases), and the
oracle's eval_bloom for BLOOM (fused q|k|v rows, ggml_alibi, inpFF = attn + inpL kept as the
residual).  Weights are the file's (modelgen.read_model + dequantize_q4_0); positions, the causal
mask and the ALiBi slopes come from their definitions.

Every stage is teacher-forced: its fp64 value is computed from the DEVICE's actual input to that
stage, so quantization flips never compound and each stage is held to the bound of its own
arithmetic (u = 2^-24, h = 2^-11):

LayerNorm     y = w (x - mean) s + b, s = 1 / sqrt(var + 1e-5f).  The device forms both sums in
              double (error far below u), then rounds (float)(x - mean), (float)s, their product and
              w times it: four relative roundings of |w (x - mean) s|, and the add of b rounds at
              |y|.  |y - y64| <= 4.5 u |w (x - mean) s| + u |y64| (the half covers second order and
              the double sums).
fp16 GEMM     fast_ref.gemm_f16_tol on the fp16-rounded operands (fast_ref.w16_of; the activation
              operand is the device's own fp16 rows): 4 K u sum |w16 x16| + 1e-6 |b|.
Q4 GEMV       (fewer than 8 rows) 4 K u sum |w x| on the Q4_0 values of both operands
              (tests/test_gpu_ops.py test_gemv_fast_within_bound), + u |y64| for a bias add.
Quantized operands (norm_f16q, act_quant_f16, the GELU-quantize epilogue, the d = 256 attention):
              q4_f16_check, which is fast_ref.q4_check on the fp16 values d (q - 8): codes of
              unambiguous elements exact, ambiguous ones within one step, the block scale within the
              amax tolerance; a value d q is rounded once more to fp16 (h |d q|, 2^-25 for a denormal).
              The share of ambiguous elements is returned; the tests cap it at 2 %.
Fused quantizers.  Two launches quantize a value that never reaches memory as f32: fc_in's
              GELU-quantize epilogue (N >= 256) and the d = 256 attention.  Held to the bound of the
              value they quantize (4 K u sum |w16 x16|, c 2^-11 A + T), 2.3 - 5.4 % of their elements
              would be ambiguous, past the cap, and an ambiguous element is only held to a step.  They
              are pinned harder instead: the caller also makes the two-launch form on the same
              operands (the plain GEMM, then act_quant_f16 with bias and GELU; the same attention
              kernel writing f32, then act_quant_f16), whose f32 value meets its bound, whose
              quantization is checked from that f32 value (one float add: under 1 % ambiguous), and
              whose fp16 operand the fused launch must equal bit for bit (kind `bits`: the project's
              contract for both epilogues, tests/test_gpu_ops.py).
Q4 rows       (fewer than 8 rows) quantize_row_q4_0 of the device's f32 rows, exactly.
RoPE in a GEMM epilogue: fast_ref.rope_ref's rule, c v - s v' with |c|, |s| <= 1 adds the partner's
              bound, and the double result is rounded once (u |y64|).
GELU          g(s) = 0.5 s (1 + tanh(0.79788456 s (1 + 0.044715 s^2))) through the fp16 table:
              the argument is rounded to fp16 (h |s|, 2^-25 for a denormal), g is LIP-Lipschitz
              (LIP = 1.13 >= max |g'| = 1.1290, asserted on a grid by the CPU tests), the table holds
              fp16(float(g)) (h (1 + 2^-12) |g| + 2^-25):
              |g - g64| <= LIP (tol_s + h |s| + 2^-25) + h (1 + 2^-12) |g64| + 2^-25.
Attention     the fp16 MFMA kernels: attn_ref.Ref, |y - ref16| <= c 2^-11 A + T and its 2e-2 max |V|
              tier.  The three exact kernels (BLOOM at every N, every graph below 8 rows): derived in
              attn_exact below.
Elementwise   the separate RoPE + KV write (double products, rounded once), the joins and the adds:
              the fp64 value rounded once to float, exactly (an add of two floats in double is exact
              or rounds innocuously; two adds are rounded one after the other).
Residual join in a GEMM epilogue: the GEMM's bound and one rounding per add at the magnitude of its
              result.
"""
from dataclasses import dataclass

import numpy as np

import attn_ref as A
import fast_ref as R
from vsim_amd import modelgen as mg

QK = 32
U = R.U
H16 = 2.0 ** -11
EPS = float(np.float32(1e-5))
LIP = 1.13
AMB_CAP = 0.02  # tests/test_gpu_fast_ops.py's cap on the share of ambiguous elements


# ------------------------------------------------------------------ configurations and inputs
@dataclass(frozen=True)
class Config:
    name: str
    arch: str  # modelgen's: gptj, gptneox, bloom
    E: int
    H: int
    n_rot: int
    parallel: int = 1
    seed: int = 11

    @property
    def d(self):
        return self.E // self.H

    @property
    def F(self):
        return 4 * self.E

    @property
    def style(self):  # vsim_op_rope's: 0 rotate-half, 1 GPT-J pairs
        return 1 if self.arch == "gptj" else 0

    @property
    def bias(self):  # Q, K, V and the out-projection carry biases
        return self.arch != "gptj"

    @property
    def two_norms(self):
        return self.arch != "gptj"

    @property
    def alibi(self):
        return self.arch == "bloom"

    @property
    def residual(self):
        if self.arch == "bloom":
            return "serial_joined"
        return "parallel" if self.arch == "gptj" or self.parallel else "serial_old"

    def hparams(self, n_layer, n_vocab=512):
        return mg.HParams(n_vocab, self.E, self.H, n_layer, self.n_rot, 1 if self.arch == "gptj" else self.parallel)


CONFIGS = [
    Config("gptj-d128", "gptj", 512, 4, 64),
    Config("gptj-d256", "gptj", 512, 2, 64),
    Config("gptj-d64", "gptj", 512, 8, 32),
    Config("gptj-e384", "gptj", 384, 3, 64),
    Config("neox-par", "gptneox", 512, 8, 32, 1),
    Config("neox-ser", "gptneox", 512, 8, 32, 0),
    Config("bloom", "bloom", 512, 8, 0, 0),
]
PAIRS = [(37, 300), (256, 9), (72, 72), (72, 3)]
STD = 0.05  # the suite's weight and bias spread


def resid_rows(cfg, N, n_past):
    """The stage input of one eval: N(0, 1) rows, seeded by the configuration and the batch, with
    three crafted rows: all zeros, one row scaled by 1e4, one row with a single non-zero element."""
    rng = np.random.default_rng([cfg.seed, cfg.E, cfg.H, N, n_past])
    x = rng.standard_normal((N, cfg.E)).astype(np.float32)
    zero, big, single = sorted({N // 4, N // 2, N - 1}) if N >= 3 else (0, 0, 0)
    if N >= 3:
        x[zero] = 0.0
        x[big] *= np.float32(1e4)
        keep = x[single, 7]
        x[single] = 0.0
        x[single, 7] = keep if keep != 0 else np.float32(1.0)
    return x


@dataclass(frozen=True)
class Plan:
    """Which launches run_layer takes for N rows (include/vsim_hip.h, the fast-mode prompt layer)."""
    pf: bool        # the activations are the GEMMs' fp16 operand (else f32 / Q4 rows)
    g2: bool        # the 256-wide-tile GEMM with its epilogues
    rope_epi: bool  # RoPE and the cache write in the Q / K / V GEMMs' epilogues
    attn16: bool    # the fp16 MFMA attention
    kv16: bool      # ... with the new keys' fp16 copies made by the K and V GEMMs
    attn_q16: bool  # ... writing the out-projection's fp16 operand itself
    pair: bool      # Q and K as one launch
    join_epi: bool  # the residual join in fc_out's epilogue


def plan(cfg, N):
    pf = N >= 8
    g2 = pf and N >= 256 and cfg.E % 64 == 0
    rope_epi = g2 and cfg.arch == "gptj"
    attn16 = not cfg.alibi and N >= 8 and cfg.d in (64, 96, 128, 256) and cfg.E % 64 == 0
    return Plan(pf, g2, rope_epi, attn16, rope_epi and attn16, attn16 and pf and cfg.d == 256,
                rope_epi and cfg.E % 256 == 0, g2 and cfg.residual != "serial_joined")


# ------------------------------------------------------------------ weights
_LAYER_NAMES = {
    "gptj": ("transformer.h.{}.", dict(
        ln1_w="ln_1.weight", ln1_b="ln_1.bias", wq="attn.q_proj.weight", wk="attn.k_proj.weight",
        wv="attn.v_proj.weight", wo="attn.out_proj.weight", wfc="mlp.fc_in.weight", bfc="mlp.fc_in.bias",
        wproj="mlp.fc_out.weight", bproj="mlp.fc_out.bias")),
    "gptneox": ("gpt_neox.layers.{}.", dict(
        ln1_w="input_layernorm.weight", ln1_b="input_layernorm.bias", ln2_w="post_attention_layernorm.weight",
        ln2_b="post_attention_layernorm.bias", wq="attention.query.weight", bq="attention.query.bias",
        wk="attention.key.weight", bk="attention.key.bias", wv="attention.value.weight", bv="attention.value.bias",
        wo="attention.dense.weight", bo="attention.dense.bias", wfc="mlp.dense_h_to_4h.weight",
        bfc="mlp.dense_h_to_4h.bias", wproj="mlp.dense_4h_to_h.weight", bproj="mlp.dense_4h_to_h.bias")),
    "bloom": ("layers.{}.", dict(
        ln1_w="attention_norm.weight", ln1_b="attention_norm.bias", ln2_w="ffn_norm.weight", ln2_b="ffn_norm.bias",
        wqkv="attention.query_key_value.weight", bqkv="attention.query_key_value.bias", wo="attention.wo.weight",
        bo="attention.wo.bias", wfc="feed_forward.w1.weight", bfc="feed_forward.w1.bias",
        wproj="feed_forward.w2.weight", bproj="feed_forward.w2.bias")),
}
_GLOBAL_NAMES = {
    "gptj": dict(wte="transformer.wte.weight", lnf_w="transformer.ln_f.weight", lnf_b="transformer.ln_f.bias",
                 lmh="lm_head.weight", lmh_b="lm_head.bias"),
    "gptneox": dict(wte="gpt_neox.embed_in.weight", lnf_w="gpt_neox.final_layer_norm.weight",
                    lnf_b="gpt_neox.final_layer_norm.bias", lmh="embed_out.weight"),
    "bloom": dict(wte="tok_embeddings.weight", emb_w="norm.weight", emb_b="norm.bias", lnf_w="output_norm.weight",
                  lnf_b="output_norm.bias", lmh="output.weight"),
}


class Weights:
    """Tensors by role: .aos[role] the Q4_0 file bytes of a matrix [M][K] (with .shape[role] = (M, K)),
    .f[role] a float32 vector; .W(role) / .W16(role) the matrix's values d*(q-8) in float64, exact and
    rounded once to fp16."""

    def __init__(self):
        self.aos, self.shape, self.f, self._w, self._w16 = {}, {}, {}, {}, {}

    def add(self, role, rec):
        ne, ftype, raw = rec
        if ftype == 2:
            self.aos[role] = np.frombuffer(raw, np.uint8)
            self.shape[role] = (int(ne[1]), int(ne[0]))
        else:
            self.f[role] = np.frombuffer(raw, np.float32)

    def W(self, role):
        if role not in self._w:
            self._w[role] = mg.dequantize_q4_0(self.aos[role], self.shape[role][1]).astype(np.float64)
        return self._w[role]

    def W16(self, role):
        if role not in self._w16:
            self._w16[role] = R.w16_of(self.aos[role], self.shape[role][1]).astype(np.float64)
        return self._w16[role]


def read_weights(path, arch, layers):
    """(hparams, globals, {il: layer}) of a model file; BLOOM's fused q | k | v rows split in thirds."""
    hp, T = mg.read_model(path, arch)
    g = Weights()
    for role, name in _GLOBAL_NAMES[arch].items():
        g.add(role, T[name])
    out = {}
    prefix, names = _LAYER_NAMES[arch]
    for il in layers:
        L = Weights()
        for role, name in names.items():
            ne, ftype, raw = T[prefix.format(il) + name]
            if role == "wqkv":
                n = len(raw) // 3
                for i, r in enumerate(("wq", "wk", "wv")):
                    L.add(r, ([ne[0], ne[1] // 3], ftype, raw[i * n:(i + 1) * n]))
            elif role == "bqkv":
                n = len(raw) // 3
                for i, r in enumerate(("bq", "bk", "bv")):
                    L.add(r, ([ne[0] // 3], ftype, raw[i * n:(i + 1) * n]))
            else:
                L.add(role, (ne, ftype, raw))
        out[il] = L
    return hp, g, out


def alibi_slopes(n_head):
    """ggml_alibi's head slopes (ggml.c:6217-6232): m0 = (float)2^(-8 / n), m1 = (float)2^(-4 / n), n the
    largest power of two <= n_head; head k < n: (float)m0^(k + 1), else (float)m1^(2 (k - n) + 1)."""
    n = 1 << int(np.floor(np.log2(n_head)))
    m0 = float(np.float32(2.0 ** (-8.0 / n)))
    m1 = float(np.float32(2.0 ** (-4.0 / n)))
    return np.array([m0 ** (k + 1) if k < n else m1 ** (2 * (k - n) + 1) for k in range(n_head)]).astype(np.float32)


# ------------------------------------------------------------------ stage arithmetic in fp64
def layernorm(x, w, b):
    """ggml_norm + affine (vsim.cpp:526-533) of the rows x [N][E]; value and bound."""
    x = np.asarray(x, np.float64)
    mean = x.mean(axis=1, keepdims=True)
    var = ((x - mean) ** 2).mean(axis=1, keepdims=True)
    t = np.asarray(w, np.float64)[None, :] * ((x - mean) / np.sqrt(var + EPS))
    y = t + np.asarray(b, np.float64)[None, :]
    return y, 4.5 * U * np.abs(t) + U * np.abs(y)


def gemm16(x16, W16, bias):
    """The fp16 MFMA GEMMs: x16 [N][K] (the device's fp16 operand) times W16 [M][K], + bias."""
    X = np.asarray(x16).astype(np.float64)
    y = X @ W16.T
    ab = np.abs(X) @ np.abs(W16).T
    if bias is not None:
        y = y + np.asarray(bias, np.float64)[None, :]
    return y, R.gemm_f16_tol(W16.shape[1], ab, None if bias is None else np.asarray(bias)[None, :])


def gemv_q4(xq, W, bias):
    """The fast GEMV on Q4 rows xq = (d [N][nb], q [N][nb][32]) times the Q4_0 weight values W [M][K]."""
    d, q = xq
    X = (np.asarray(d, np.float64)[:, :, None] * np.asarray(q, np.float64)).reshape(d.shape[0], -1)
    y = X @ W.T
    tol = 4.0 * W.shape[1] * U * (np.abs(X) @ np.abs(W).T)
    if bias is not None:
        y = y + np.asarray(bias, np.float64)[None, :]
        tol = tol + U * np.abs(y)
    return y, tol


def rope(y, pos, cs, d, n_rot, style, tol=None):
    """ggml_rope (style 1: pairs 2j, 2j + 1; ggml.c:5919-5974) / ggml_gptneox_rope (style 0: j, j + n_rot / 2;
    ggml.c:6086-6153) of the rows y [N][H d] at positions pos [N], the first n_rot dims of every
    head, angle pos * 10000^(-2j / n_rot) (cs = fast_ref.rope_table).  With tol also the bound."""
    y = np.asarray(y, np.float64)
    N, E = y.shape
    v = y.reshape(N, E // d, d)
    out = v.copy()
    t = None if tol is None else np.asarray(tol, np.float64).reshape(N, E // d, d).copy()
    if n_rot > 0:
        half = n_rot // 2
        c = cs[np.asarray(pos), :half, 0][:, None, :]
        s = cs[np.asarray(pos), :half, 1][:, None, :]
        ia, ib = (slice(0, n_rot, 2), slice(1, n_rot, 2)) if style == 1 else (slice(0, half), slice(half, n_rot))
        a, b = v[:, :, ia], v[:, :, ib]
        out[:, :, ia] = a * c - b * s
        out[:, :, ib] = a * s + b * c
        if t is not None:
            ta, tb = t[:, :, ia].copy(), t[:, :, ib].copy()
            t[:, :, ia] = ta + tb
            t[:, :, ib] = ta + tb
    out = out.reshape(N, E)
    if t is None:
        return out
    return out, t.reshape(N, E) + U * np.abs(out)


def gelu(s):
    s = np.asarray(s, np.float64)
    return 0.5 * s * (1.0 + np.tanh(0.79788456 * s * (1.0 + 0.044715 * s * s)))


def gelu_tol(s, tol_s):
    s = np.asarray(s, np.float64)
    g = gelu(s)
    return g, LIP * (tol_s + H16 * np.abs(s) + 2.0 ** -25) + H16 * (1 + 2.0 ** -12) * np.abs(g) + 2.0 ** -25


def attn_exact(Q, kc, vc, d, n_past, scale, slopes=None, mask_shift=0, zero_cached=False, slope_shift=0):
    """The three exact attention kernels (KQ, scale -> ALiBi -> mask -> softmax, KQV: vsim.cpp:583-616,
    eval_bloom) in fp64: out[j][h d + c] = sum_k p_jk v_kc, p = softmax over the keys k <= n_past + j of
    scale q_j . k_k (+ (j + 1) m_h, ggml_alibi's per-row term).  Returns out, tol [N][H d].

    The bound, first order, per head and query row (nv visible keys; p normalized, A_c = sum p |v_c|):
      score   every product q_i k_i rounded to float (u sum |q_i k_i|, the sum itself in double), the
              sum rounded to float, times scale, plus the ALiBi term (itself a float product):
              ts_k = u (scale sum |q_i k_i| + 2 |scale q.k| + |s_k| + |(j + 1) m_h|)
      weight  e^(s_k - max) through the fp16 tables: the argument moves by ts_k + max ts, its
              float difference and its fp16 rounding by (u + h) |s_k - max| (2^-25 for a denormal),
              the table entry is fp16 of a float exp: h (1 + 2^-12) relative, or 2^-25 absolute
              below 2^-14.  Relative e_k = ts_k + max ts + (u + h) |x_k| + h (1 + 2^-12) + 2^-24,
              absolute a = 2^-25 (of a sum of weights >= 1).
      out     sum w v / sum w with w_k = p_k (1 + e_k) + a: |d out_c| <= sum p e |v_c| + A_c sum p e
              + a (sum |v_kc| + nv A_c); the float 1 / sum, the products by it and KQV's float chain
              of nv products and adds: (2 nv + 4) u A_c.  The total times 1.02 for second order.
    mask_shift, zero_cached, slope_shift: the CPU tests' wrong variants."""
    Q = np.asarray(Q, np.float64)
    K = np.asarray(kc, np.float64).copy()
    V = np.asarray(vc, np.float64).copy()
    if zero_cached:
        K[:n_past] = 0.0
        V[:n_past] = 0.0
    N, E = Q.shape
    nk = K.shape[0]
    Hh = E // d
    sc = float(np.float32(scale))
    vis = np.arange(nk)[None, :] <= (n_past + np.arange(N) + mask_shift)[:, None]
    out, tol = np.empty((N, E)), np.empty((N, E))
    for h in range(Hh):
        sl = slice(h * d, (h + 1) * d)
        raw = (Q[:, sl] @ K[:, sl].T) * sc
        S = (np.abs(Q[:, sl]) @ np.abs(K[:, sl]).T) * sc
        ab = np.zeros(N) if slopes is None else (np.arange(N) + 1.0) * float(slopes[(h + slope_shift) % Hh])
        s = raw + ab[:, None]
        ts = U * (S + 2 * np.abs(raw) + np.abs(s) + np.abs(ab)[:, None])
        s = np.where(vis, s, -np.inf)
        x = s - s.max(axis=1, keepdims=True)
        p = np.where(vis, np.exp(x), 0.0)
        p /= p.sum(axis=1, keepdims=True)
        tmx = np.where(vis, ts, 0.0).max(axis=1, keepdims=True)
        e = np.where(vis, ts + tmx + (U + H16) * np.abs(np.where(vis, x, 0.0)) + H16 * (1 + 2.0 ** -12) + 2.0 ** -24, 0.0)
        av = np.abs(V[:, sl])
        Ac = p @ av
        nv = vis.sum(axis=1, keepdims=True)
        out[:, sl] = p @ V[:, sl]
        tol[:, sl] = 1.02 * ((p * e) @ av + Ac * (p * e).sum(axis=1, keepdims=True) +
                             2.0 ** -25 * (vis.astype(np.float64) @ av + nv * Ac) + (2 * nv + 4) * U * Ac)
    return out, tol


def attn_wrong(Q, kc, vc, d, n_past, scale, **kw):
    """What an attention with a wrong mask or zeroed cached keys would give (the CPU tests' variants)."""
    return attn_exact(Q, kc, vc, d, n_past, scale, **kw)[0]


# ------------------------------------------------------------------ checkers
def q4_f16_ref(y):
    return R.q4_f16_ref(np.asarray(y, np.float32))


def q4_rows(y):
    """quantize_row_q4_0 of the f32 rows y [N][K]: (d [N][nb], q [N][nb][32] signed)."""
    y = np.ascontiguousarray(y, np.float32)
    d, q = R.q4_quantize_ref(y)
    return d.reshape(y.shape[0], -1), q.reshape(y.shape[0], -1, QK)


def q4_f16_check(x16, y_ref, tol):
    """fast_ref.q4_check for a quantized fp16 operand x16 = fp16(d (q - 8)) of rows y with |y - y_ref| <=
    tol.  The codes are read back from the values: a block's largest |value| is 7 d (quantize_row_q4_0
    maps amax to +-7), and fp16's 2^-11 cannot move value / d across a half.  Unambiguous codes must
    equal the reference's, ambiguous ones may differ by one step; every value must be a code times a
    scale within the amax tolerance, rounded to fp16.  Returns the ambiguous share."""
    y_ref = np.asarray(y_ref, np.float64)
    q_e, d64, dtol, amb = R._q4_expect(y_ref.reshape(-1), np.broadcast_to(np.asarray(tol, np.float64), y_ref.shape).reshape(-1))
    v = np.asarray(x16, np.float16).astype(np.float64).reshape(-1, QK)
    assert np.isfinite(v).all(), "a quantized operand holds a NaN or an Inf"
    dd = np.abs(v).max(axis=1) / 7.0
    q = np.rint(v / np.where(dd > 0, dd, 1.0)[:, None]).astype(np.int64)
    diff = np.abs(q - q_e)
    bad = np.where(amb, diff > 1, diff != 0)
    assert not bad.any(), (f"{int(bad.sum())} quantized value(s) off: first at {tuple(np.argwhere(bad)[0])}, "
                           f"device code {q[bad][0]} expected {q_e[bad][0]}")
    want = d64[:, None] * q
    lim = np.abs(q) * dtol[:, None] + H16 * (1 + H16) * np.abs(want) + 2.0 ** -25
    bad = np.abs(v - want) > lim
    assert not bad.any(), f"{int(bad.sum())} value(s) outside the block scale's tolerance: first at {tuple(np.argwhere(bad)[0])}"
    return float(amb.mean())


class Stage:
    """One step of the layer: `fn(mut)` gives its fp64 value and bound from the device's input
    (mut: the CPU tests' wrong variant of this step, else empty); `kind` says how the device output
    st[key] is held to it:
      f32     |dev - ref| <= tol
      exact   dev == float32(ref)  (ref already holds the float steps where there are two)
      q16     q4_f16_check(dev, ref, tol)
      q4      the Q4 rows (d, q) of ref, exactly
      bits    dev and ref (another device array) are the same fp16 bits
      attn16  attn_ref.Ref(...).check(dev)  (fn returns the Ref)"""

    def __init__(self, name, kind, key, fn):
        self.name, self.kind, self.key, self.fn = name, kind, key, fn

    def device(self, mut=frozenset()):
        """The output of a device that computes the reference's fp64 value (of variant mut) and rounds
        it as the kernel does."""
        ref, _ = self.fn(mut)
        if self.kind in ("f32", "exact"):
            return np.asarray(ref, np.float64).astype(np.float32)
        if self.kind == "q16":
            return q4_f16_ref(np.asarray(ref, np.float64).astype(np.float32))
        if self.kind == "q4":
            return q4_rows(ref)
        if self.kind == "bits":
            return np.array(ref, copy=True)
        return np.asarray(ref if mut else ref.ref16, np.float64).astype(np.float32)

    def check(self, dev):
        """(worst error / bound, ambiguous share or None); AssertionError when the stage misses."""
        ref, tol = self.fn(frozenset())
        if self.kind == "f32":
            r = R.bound_ratio(dev, ref, tol)
            assert r <= 1.0, f"{self.name}: |dev - fp64| reaches {r:.3g} x its bound"
            return r, None
        if self.kind == "exact":
            want = np.asarray(ref, np.float64).astype(np.float32)
            bad = ~(np.asarray(dev) == want)
            assert not bad.any(), f"{self.name}: {int(bad.sum())} value(s) are not the fp64 value rounded to float"
            return 0.0, None
        if self.kind == "q16":
            try:
                return 0.0, q4_f16_check(dev, ref, tol)
            except AssertionError as e:
                raise AssertionError(f"{self.name}: {e}") from None
        if self.kind == "q4":
            d, q = q4_rows(ref)
            ok = np.array_equal(np.asarray(dev[0], np.float32).view(np.uint32), d.view(np.uint32)) and \
                np.array_equal(np.asarray(dev[1]).astype(np.int64), q)
            assert ok, f"{self.name}: not quantize_row_q4_0 of the f32 rows"
            return 0.0, None
        if self.kind == "bits":
            a, b = np.ascontiguousarray(dev), np.ascontiguousarray(ref)
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint16), b.view(np.uint16)), \
                f"{self.name}: the fused launch's operand is not the two-launch form's, bit for bit"
            return 0.0, None
        return ref.check(dev, self.name), None


def walk(cfg, L, st, n_past, cs, slopes=None):
    """The stages of one layer on the intermediates st (filled by the caller as the walk goes, or
    complete), in the layer's order.  st keys: inpL [N][E]; xa (fp16) or cur1 / xq1; Qb, Kb, Vb where
    RoPE is a launch of its own; Q, Knew, Vnew (the new cache rows), kc_old (the cache rows before
    n_past as this eval finds them) and kc_prev / vc_prev (as the earlier eval left them); attn_in;
    xb_a (fp16) or xq2; attn; joined; xa2 or cur2 / xqn; fch; g; xb_g or xq3; ff; out."""
    N = st["inpL"].shape[0]
    p = plan(cfg, N)
    E, d, f = cfg.E, cfg.d, L.f
    pos = n_past + np.arange(N)
    sc = float(np.float32(1.0 / np.sqrt(float(np.float32(E) / np.float32(cfg.H)))))

    def product(role, bias, k16, kq4, drop_bias=False):
        b = None if bias is None or drop_bias else f[bias]
        return gemm16(st[k16], L.W16(role), b) if p.pf else gemv_q4(st[kq4], L.W(role), b)

    def norm_stages(tag, src, wk, bk, k16, kf, kq, wrong_gain=None):
        def fn(mut):
            return layernorm(st[src], f[wrong_gain] if wrong_gain and "norm2_gain1" in mut else f[wk], f[bk])
        if p.pf:
            yield Stage(tag, "q16", k16, fn)
        else:
            yield Stage(tag, "f32", kf, fn)
            yield Stage(tag + ".q4", "q4", kq, lambda mut: (st[kf], None))

    yield from norm_stages("ln1", "inpL", "ln1_w", "ln1_b", "xa", "cur1", "xq1")

    # Q, K, V (+ bias) and RoPE at positions n_past + i
    def roped(yt, mut):
        y, t = yt
        n_rot, style, ps, tab = cfg.n_rot, cfg.style, pos, cs
        if "rope_pos_plus1" in mut:
            ps = pos + 1
        if "rope_full" in mut:
            n_rot, tab = d, R.rope_table(n_past + N + 1, d)
        if "rope_style_swapped" in mut:
            style = 1 - style
        return rope(y, ps, tab, d, n_rot, style, tol=t)

    bq, bk, bv = ("bq", "bk", "bv") if cfg.bias else (None, None, None)
    if p.rope_epi:
        yield Stage("Q", "f32", "Q", lambda mut: roped(product("wq", bq, "xa", "xq1"), mut))
        yield Stage("K", "f32", "Knew", lambda mut: roped(product("wk", bk, "xa", "xq1", "k_bias_dropped" in mut), mut))
        yield Stage("V", "f32", "Vnew", lambda mut: product("wv", bv, "xa", "xq1"))
    else:
        yield Stage("Qb", "f32", "Qb", lambda mut: product("wq", bq, "xa", "xq1"))
        yield Stage("Kb", "f32", "Kb", lambda mut: product("wk", bk, "xa", "xq1", "k_bias_dropped" in mut))
        yield Stage("Vb", "f32", "Vb", lambda mut: product("wv", bv, "xa", "xq1"))
        yield Stage("Q", "exact", "Q", lambda mut: (roped((st["Qb"], np.zeros_like(st["Qb"], np.float64)), mut)[0], None))
        yield Stage("K", "exact", "Knew", lambda mut: (roped((st["Kb"], np.zeros_like(st["Kb"], np.float64)), mut)[0], None))
        yield Stage("V", "exact", "Vnew", lambda mut: (st["Vb"], None))
    if n_past:
        yield Stage("cache.k", "exact", "kc_old", lambda mut: (st["kc_prev"], None))
        yield Stage("cache.v", "exact", "vc_old", lambda mut: (st["vc_prev"], None))

    def caches():
        if n_past:
            return np.concatenate([st["kc_old"], st["Knew"]]), np.concatenate([st["vc_old"], st["Vnew"]])
        return st["Knew"], st["Vnew"]

    # attention over the keys k <= n_past + j
    def attention(mut):
        kc, vc = caches()
        kw = dict(mask_shift=1 if "mask_plus1" in mut else 0, zero_cached="cached_keys_zeroed" in mut,
                  slope_shift=1 if "alibi_neighbour" in mut else 0)
        if p.attn16:
            if mut:
                return attn_wrong(st["Q"], kc, vc, d, n_past, sc, **kw), None
            return A.Ref(st["Q"], kc, vc, d, n_past, sc), None
        return attn_exact(st["Q"], kc, vc, d, n_past, sc, slopes if cfg.alibi else None, **kw)

    if p.attn_q16:
        # (attn_in, xb_a_side: the side launches of the module docstring's "Fused quantizers")
        yield Stage("attn", "attn16", "attn_in", attention)
        yield Stage("attn.q16", "q16", "xb_a_side", lambda mut: (st["attn_in"], np.zeros_like(st["attn_in"], np.float64)))
        yield Stage("attn.fused", "bits", "xb_a", lambda mut: (st["xb_a_side"], None))
    else:
        yield Stage("attn", "attn16" if p.attn16 else "f32", "attn_in", attention)
        if p.pf:
            yield Stage("attn.q16", "q16", "xb_a", lambda mut: (st["attn_in"], np.zeros_like(st["attn_in"], np.float64)))
        else:
            yield Stage("attn.q4", "q4", "xq2", lambda mut: (st["attn_in"], None))
    yield Stage("oproj", "f32", "attn", lambda mut: product("wo", "bo" if cfg.bias else None, "xb_a", "xq2"))

    # the MLP's input
    serial = cfg.residual != "parallel"
    fc16, fcq4 = "xa", "xq1"
    if cfg.two_norms:
        if serial:
            def joined(mut):
                if "ser_join_from_inpL" in mut:
                    return st["inpL"], None
                return np.asarray(st["attn"], np.float64) + np.asarray(st["inpL"], np.float64), None
            yield Stage("joined", "exact", "joined", joined)
        yield from norm_stages("ln2", "joined" if serial else "inpL", "ln2_w", "ln2_b", "xa2", "cur2", "xqn", "ln1_w")
        fc16, fcq4 = "xa2", "xqn"

    # fc_in + bias + GELU
    def act(s, tol_s, mut):
        if "fcin_bias_missing" in mut:
            s = s - np.asarray(f["bfc"], np.float64)[None, :]
        return gelu_tol(s, tol_s)

    yield Stage("fc_in", "f32", "fch", lambda mut: product("wfc", None, fc16, fcq4))

    def biased_gelu(mut):
        s = np.asarray(st["fch"], np.float64) + np.asarray(f["bfc"], np.float64)[None, :]
        return act(s, U * np.abs(s), mut)
    if p.g2:  # (fch, xb_g_side: the side launches of the module docstring's "Fused quantizers")
        yield Stage("gelu", "q16", "xb_g_side", biased_gelu)
        yield Stage("gelu.fused", "bits", "xb_g", lambda mut: (st["xb_g_side"], None))
    elif p.pf:
        yield Stage("gelu", "q16", "xb_g", biased_gelu)
    else:
        yield Stage("gelu", "f32", "g", biased_gelu)
        yield Stage("gelu.q4", "q4", "xq3", lambda mut: (st["g"], None))

    # fc_out + bias and the residual
    x, a = np.asarray(st["inpL"], np.float64), None
    if p.join_epi:
        def join(mut):
            y, t = product("wproj", "bproj", "xb_g", "xq3")
            if serial:  # inpL = inpFF + inpL (vsim.cpp:657)
                out = y + x
                return out, t + U * np.abs(out)
            a = np.asarray(st["attn"], np.float64)
            inner = y if "par_join_no_attn" in mut else a + y  # inpL + (cur + inpFF) (vsim.cpp:694-695)
            out = x + inner
            return out, t + U * (np.abs(inner) + np.abs(out))
        yield Stage("out", "f32", "out", join)
    else:
        yield Stage("fc_out", "f32", "ff", lambda mut: product("wproj", "bproj", "xb_g", "xq3"))

        def final(mut):
            ff = np.asarray(st["ff"], np.float64)
            if cfg.residual == "serial_joined":  # inpL = ff + inpFF (eval_bloom)
                base = x if "bloom_final_from_inpL" in mut else np.asarray(st["joined"], np.float64)
                return ff + base, None
            if serial:
                return ff + x, None
            inner = ff if "par_join_no_attn" in mut else (np.asarray(st["attn"], np.float64) + ff).astype(np.float32)
            return x + np.asarray(inner, np.float64), None
        yield Stage("out", "exact", "out", final)


# the wrong variants of tests/test_fast_prompt_ref_cpu.py: name -> (stages that must reject it, the
# configurations that have it)
VARIANTS = {
    "k_bias_dropped": (("Kb|K",), lambda c: c.bias),  # (a|b: the first of the two that the walk has)
    "rope_pos_plus1": (("Q", "K"), lambda c: c.n_rot > 0),
    "rope_full": (("Q", "K"), lambda c: 0 < c.n_rot < c.d),
    "rope_style_swapped": (("Q", "K"), lambda c: c.arch == "gptj"),
    "mask_plus1": (("attn",), lambda c: True),
    "cached_keys_zeroed": (("attn",), lambda c: True),
    "norm2_gain1": (("ln2",), lambda c: c.two_norms),
    "fcin_bias_missing": (("gelu",), lambda c: True),
    "par_join_no_attn": (("out",), lambda c: c.residual == "parallel"),
    "ser_join_from_inpL": (("joined",), lambda c: c.residual != "parallel"),
    "bloom_final_from_inpL": (("out",), lambda c: c.residual == "serial_joined"),
}


def simulate(cfg, L, inpL, n_past, cs, slopes=None, kc_prev=None, vc_prev=None):
    """The intermediates of a device that computes every stage's fp64 value from its own rounded
    inputs: the reference's stage outputs rounded to fp32 / fp16."""
    st = {"inpL": np.asarray(inpL, np.float32)}
    if n_past:
        st["kc_prev"], st["vc_prev"] = kc_prev, vc_prev
    for stg in walk(cfg, L, st, n_past, cs, slopes):
        st[stg.key] = stg.device()
    return st


def check(cfg, L, st, n_past, cs, slopes=None):
    """Every stage of st against its bound.  Returns {stage: worst error / bound}, {stage: ambiguous
    share}; AssertionError naming the first stage that misses."""
    ratios, shares = {}, {}
    for stg in walk(cfg, L, st, n_past, cs, slopes):
        r, s = stg.check(st[stg.key])
        ratios[stg.name] = r
        if s is not None:
            shares[stg.name] = s
    return ratios, shares
