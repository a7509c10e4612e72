"""numpy restatement of the weight-only mode (VSIM_MODE_W4A16, vsim_amd/csrc/gemm_w4a16_rows.hip):
the row operand bit for bit, the product in fp64 with its derived bound, and a small fp64 forward of
GPT-NeoX (parallel residual) built from the oracle's table ops (tests/oracle_py.py) for the quality
check.  The checkers' teeth are shown on the CPU by tests/test_w4a16_ref_cpu.py.

Conventions as tests/fast_ref.py: a Q4_0 row is (d [nb] float32, q [nb][32] signed = nibble - 8);
u = 2^-24 is the unit roundoff of one float operation.
"""
import functools

import numpy as np

import fast_ref as R

QK = 32
U = 2.0 ** -24
P = 16                      # partials of k_gemm_w4a16_rows (one per wave)
NONFINITE = -2 ** 31        # VSIM_W4A16_NONFINITE
QNAN_BITS = 0x7FC00000      # every output of a row that holds a NaN or an Inf
# gfx950's v_mfma_f32_16x16x32_f16 takes fp16 subnormal A / B inputs at their value (measured:
# tests/test_gpu_w4a16_ops.py::test_subnormal_operands_count, which fails if the matrix core flushed
# them).  False would restate a flushing matrix core: subnormal h count as zero in the product.
MFMA_KEEPS_F16_SUBNORMALS = True


# ------------------------------------------------------------------ the row operand
def row_operand(x):
    """x [n][K] float32 -> (h [n][K] float16, e [n] int32), the operand of vsim_op_w4a16_rows:
    amax = the row's largest finite |x|; e = 14 - floor(log2(amax)) (0 for amax == 0), so that
    amax * 2^e lies in [2^14, 2^15); h = fp16_rn(x * 2^e), the scaling exact (ldexp), fp16
    subnormals kept.  A row with a NaN or an Inf: e = NONFINITE, h = +0 throughout."""
    x = np.ascontiguousarray(x, np.float32)
    n, K = x.shape
    h = np.zeros((n, K), np.float16)
    e = np.zeros(n, np.int32)
    for j in range(n):
        row = x[j]
        if not np.isfinite(row).all():
            e[j] = NONFINITE
            continue
        amax = float(np.abs(row).max())
        if amax > 0.0:
            _, ex = np.frexp(amax)          # amax = f * 2^ex, f in [0.5, 1): floor(log2) = ex - 1
            e[j] = 14 - (int(ex) - 1)
        with np.errstate(under="ignore"):
            # float64 holds x * 2^e exactly (|e| <= 163): one rounding, to fp16
            h[j] = np.ldexp(row.astype(np.float64), int(e[j])).astype(np.float16)
    return h, e


# ------------------------------------------------------------------ the product
def c_of_k(K):
    """The bound's constant.  Per (weight row, activation row), with nb = K / 32 blocks and every
    product (q - 8) * h exact in fp32 (4 bits by 11 bits):
      * dot_b is a sum of 32 exact terms formed by at most 32 fp32 additions in some fixed order
        (the matrix core's, starting from C = 0), so fl(dot_b) = sum_i t_i (1 + th_i), |th_i| <=
        (1 + u)^32 - 1;
      * part[p] takes its blocks by one fma each, ceil(nb / P) of them at most: a term meets at most
        that many further roundings;
      * the P partials are added in order from 0.0f: at most P further roundings per term.
    A term therefore carries at most c = 32 + ceil(nb / P) + P factors (1 + delta), |delta| <= u, and
    |y - y64| <= ((1 + u)^c - 1) sum |terms| <= c u (1 + c u) sum |terms| (c u < 2^-17 for K up to
    2^20).  The second-order factor is folded into the constant as one more unit: c(K) = 32 +
    ceil(nb / P) + P + 1.  The multiply by 2^-e is exact (or adds 2^-149 where the result is an f32
    subnormal); the bias add is one more rounding of its result."""
    nb = K // QK
    return 32 + -(-nb // P) + P + 1


def _hvals(h):
    hv = np.asarray(h, np.float16).astype(np.float64)
    if not MFMA_KEEPS_F16_SUBNORMALS:
        hv = np.where(np.abs(hv) < 2.0 ** -14, 0.0, hv)
    return hv


def product64(wd, wq, h, e, bias=None):
    """The product's formula in fp64 on the operand (h, e): y64 [n][M] = sum_b d_w[b] sum_i q_i h_i
    2^-e (+ bias), and the absolute bound tol [n][M] of the docstring above.  wd [M][nb], wq
    [M][nb][32].  Rows with e == NONFINITE: y64 = NaN, tol = 0 (checked bitwise by the caller)."""
    wd = np.asarray(wd, np.float32).astype(np.float64)
    wq = np.asarray(wq).astype(np.float64)
    M, nb = wd.shape
    hv = _hvals(h).reshape(len(e), nb, QK)
    n = hv.shape[0]
    y = np.empty((n, M))
    tol = np.empty((n, M))
    c = c_of_k(nb * QK)
    for j in range(n):
        if e[j] == NONFINITE:
            y[j], tol[j] = np.nan, 0.0
            continue
        sc = 2.0 ** -float(e[j])
        dots = np.einsum("mbi,bi->mb", wq, hv[j])
        mags = np.einsum("mbi,bi->mb", np.abs(wq), np.abs(hv[j]))
        s = (wd * dots).sum(axis=1) * sc
        mag = (np.abs(wd) * mags).sum(axis=1) * sc
        t = c * U * mag + 2.0 ** -149
        if bias is not None:
            s = s + np.asarray(bias, np.float64)
            t = t + U * (np.abs(s) + t)
        y[j], tol[j] = s, t
    return y, tol


def product32_reversed(wd, wq, h, e):
    """The same formula in fp32 with another legitimate order: each block's 32 products added
    sequentially from the last element to the first, the blocks by one chain from the last block to
    the first (product rounded, then added), then the scaling.  No bias.  float32 [n][M]."""
    wd = np.asarray(wd, np.float32)
    M, nb = wd.shape
    wq32 = np.asarray(wq).astype(np.float32)
    hv = _hvals(h).astype(np.float32).reshape(len(e), nb, QK)
    n = hv.shape[0]
    out = np.empty((n, M), np.float32)
    for j in range(n):
        if e[j] == NONFINITE:
            out[j] = np.nan
            continue
        prod = wq32 * hv[j][None]                  # exact
        dot = np.zeros((M, nb), np.float32)
        for i in range(QK - 1, -1, -1):
            dot = dot + prod[:, :, i]
        acc = np.zeros(M, np.float32)
        for b in range(nb - 1, -1, -1):
            acc = acc + wd[:, b] * dot[:, b]
        out[j] = np.ldexp(acc, -int(e[j])).astype(np.float32)
    return out


def subnormal_case():
    """An operand whose fp16 subnormals matter: weight (d, q) [M][nb], x [1][K] with one 2^20 outlier
    among values of about 2^-16 -- after the scaling every other element is an fp16 subnormal of 4
    to 7 bits -- and the outlier's own weights set to zero (q = 0), so that the subnormals alone
    make the product.  Returns (wd, wq, x, outlier index)."""
    from vsim_amd import modelgen as mg
    Ms, Ks = 16, 64
    rng = np.random.default_rng(17)
    wd, wq = R.q4_parse(mg.quantize_q4_0(rng.standard_normal(Ms * Ks).astype(np.float32) * np.float32(0.02)), Ks)
    wq = wq.copy()
    x = (rng.uniform(1.0, 2.0, (1, Ks)) * rng.choice([-1.0, 1.0], (1, Ks)) * 2.0 ** -16).astype(np.float32)
    x[0, 5] = 2.0 ** 20
    wq[:, 0, 5] = 0
    return wd, wq, x, 5


def bound_ratio(y, y64, tol):
    """max |y - y64| / tol over the finite reference entries."""
    return float(np.max(np.abs(np.asarray(y, np.float64) - y64) / tol))


# ------------------------------------------------------------------ a small fp64 forward (GPT-NeoX)
# The quality case: a two-layer parallel-residual GPT-NeoX at the executor's smallest width (n_embd
# must be a multiple of 128) with head dim 32, std 0.1 so that the logits are O(1), a 24-token
# prompt.  Seed chosen so that the oracle alone shows exact mode well clear of the ideal (below).
QUALITY_HP = dict(n_vocab=128, n_embd=128, n_head=4, n_layer=2, n_rot=8)
QUALITY_SEED, QUALITY_STD, QUALITY_TOKENS_SEED, QUALITY_N = 31, 0.1, 7, 24
N_CTX = 96

# Recorded on the CPU by tests/test_w4a16_ref_cpu.py::test_quality_distances_recorded (which recomputes
# and compares them), model seed 31, token seed 7, all 24 x 128 logits, RMS:
#   EXACT_TO_IDEAL   the oracle's exact mode (Q4_0 activations) against the ideal forward;
#   REST_ORDER_DIST  the h(x) restatement with fp64 products against the same with fp32 products
#                    summed in reversed block order: what a legitimate change of order moves.
# REST_TOL = 4 x REST_ORDER_DIST is the device's allowance against the fp64 restatement (k = 4: the
# matrix core's internal order is a third legitimate order).
EXACT_TO_IDEAL = 0.26289113046619356      # (logits RMS 1.16; the restatement's distance to the ideal: 5.67e-4)
REST_ORDER_DIST = 1.2539313737148223e-04
REST_TOL = 4.0 * REST_ORDER_DIST          # 5.0157e-04
QUALITY_FLOOR = 8.0  # 2^-5 of the block maximum (Q4_0) against 2^-11 of the element (fp16): at least 8


def rms(a, b):
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    return float(np.sqrt(np.mean(d * d)))


def quality_model_file(path):
    """Writes the quality case's model file; returns (hparams, tokens)."""
    from vsim_amd import modelgen as mg
    hp = mg.HParams(**QUALITY_HP)
    mg.write_model(path, "gptneox", hp, seed=QUALITY_SEED, std=QUALITY_STD)
    rng = np.random.default_rng(QUALITY_TOKENS_SEED)
    return hp, [int(t) for t in rng.integers(0, hp.n_vocab, QUALITY_N)]


def mm_ideal(w, x):
    """Dequantized weights times the unrounded activations, in fp64."""
    wd, wq = w
    W = wd.astype(np.float64)[:, :, None] * wq.astype(np.float64)
    return (x.astype(np.float64) @ W.reshape(W.shape[0], -1).T).astype(np.float32)


def mm_rest64(w, x):
    """The mode's restatement: the operand h(x), the product in fp64."""
    h, e = row_operand(x)
    return product64(w[0], w[1], h, e)[0].astype(np.float32)


def mm_rest32(w, x):
    h, e = row_operand(x)
    return product32_reversed(w[0], w[1], h, e)


def neox_forward(path, tokens, mm):
    """All rows' logits [N][n_vocab] of a prompt from position 0: the graph of the oracle's eval
    (vsim.cpp:470-747, parallel residual) with its own table ops through oracle_py -- LayerNorm,
    RoPE, KQ, the fp16-table softmax, KQV, the table GELU, the float32 joins -- and every product
    through `mm` ((d, q) of the weight, x [N][K] float32) -> float32 [N][M]; biases are added in
    float32 afterwards, as the kernels do."""
    import oracle_py as O
    from vsim_amd import modelgen as mg
    hp, T = mg.read_model(path, "gptneox")
    E, H, V, F = hp.n_embd, hp.n_head, hp.n_vocab, hp.n_ff
    d, N = E // H, len(tokens)

    def q(name):
        ne, _, raw = T[name]
        return R.q4_parse(np.frombuffer(raw, np.uint8), ne[0])

    def f(name):
        return np.frombuffer(T[name][2], np.float32)

    def ln(x, w, b):
        return (f(w)[None] * O.norm(x, E, N).reshape(N, E)).astype(np.float32) + f(b)[None]

    inp = O.get_rows(np.frombuffer(T["gpt_neox.embed_in.weight"][2], np.uint8), E, tokens).reshape(N, E)
    scale = np.float32(1.0 / np.sqrt(np.float64(np.float32(E) / np.float32(H))))
    for i in range(hp.n_layer):
        p = f"gpt_neox.layers.{i}."
        cur = ln(inp, p + "input_layernorm.weight", p + "input_layernorm.bias")
        Q = mm(q(p + "attention.query.weight"), cur) + f(p + "attention.query.bias")[None]
        K = mm(q(p + "attention.key.weight"), cur) + f(p + "attention.key.bias")[None]
        Vv = mm(q(p + "attention.value.weight"), cur) + f(p + "attention.value.bias")[None]
        Q = O.rope("neox", Q, d, H, N, 0, hp.n_rot, 0).reshape(N, E)
        K = O.rope("neox", K, d, H, N, 0, hp.n_rot, 0).reshape(N, E)
        S = O.attn_softmax(O.kq(K, Q, d, H, N, N), N, N, H, 0, float(scale))
        kqv = O.kqv(Vv, S, d, H, N, N).reshape(H, N, d)
        att_in = np.ascontiguousarray(kqv.transpose(1, 0, 2)).reshape(N, E)
        attn = mm(q(p + "attention.dense.weight"), att_in) + f(p + "attention.dense.bias")[None]
        cur2 = ln(inp, p + "post_attention_layernorm.weight", p + "post_attention_layernorm.bias")
        hid = mm(q(p + "mlp.dense_h_to_4h.weight"), cur2) + f(p + "mlp.dense_h_to_4h.bias")[None]
        hid = O.gelu(hid).reshape(N, F)
        ff = mm(q(p + "mlp.dense_4h_to_h.weight"), hid) + f(p + "mlp.dense_4h_to_h.bias")[None]
        inp = inp + (attn + ff)
    cur = ln(inp, "gpt_neox.final_layer_norm.weight", "gpt_neox.final_layer_norm.bias")
    return mm(q("embed_out.weight"), cur)


def oracle_exact_rows(path, tokens):
    """Row i: the oracle's exact-mode logits (the reference's arithmetic) of the prefix ending at i."""
    import oracle_py as O
    om = O.Model(path, 0, n_ctx=N_CTX)
    return np.stack([om.eval(0, tokens[:i + 1]) for i in range(len(tokens))])


@functools.lru_cache(maxsize=None)
def quality_case(tmpdir):
    """(path, tokens, ideal [N][V], rest64 [N][V]) of the quality case, computed once."""
    import os
    path = os.path.join(tmpdir, "w4a16_quality.bin")
    _, tokens = quality_model_file(path)
    return path, tokens, neox_forward(path, tokens, mm_ideal), neox_forward(path, tokens, mm_rest64)
