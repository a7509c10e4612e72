"""fp64 restatement of the fast-mode prompt attention (vsim_amd/csrc/attn_prefill.hip) and of the
fp16 K / V^T copies it reads, with the checker the GPU tests use (tests/test_gpu_attn_prefill.py;
its teeth are shown on the CPU by tests/test_attn_ref_cpu.py).  numpy only.

The kernel's operands, as it rounds them (one head, D dims, queries at positions n_past + q):
    q16 = fp16(float32(q) * qs),  qs = float32(scale) * float32(log2 e)   (one float product each)
    k16 = fp16(k),  v16 = fp16(v)
    s_k = sum_i q16_i k16_i  (fp32 MFMA),  masked for k > n_past + q
    per 64-key block: m' = max(m, block max), alpha = exp2(m - m'), p_k = exp2(s_k - m') (fp32),
    l = l alpha + sum p_k (fp32),  O = O alpha + sum fp16(p_k) v16_k (fp32 MFMA),  y = O / l.
`attention` computes y from the same q16 / k16 / v16 in float64 (base-2 softmax): ref16.

The bound.  Per output element, with p^_k = exp2(s_k - max_k s_k), l = sum p^_k (float64):
    A = sum_k p^_k |v16_k| / l
    T = sum_{k : p^_k < 2^-14} p^_k |v16_k| / l
    S = max over the query's visible keys of sum_i |q16_i k16_i|
    |y - ref16| <= c 2^-11 A + T,   c = min(4, 1.25 + ln2 D S 2^-11).
Derivation (u = 2^-24; first order; e_k a relative error of key k's weight):
  * fp16(p_k) enters O only: |fp16(p) - p| <= 2^-11 p for a normal result, so the sum moves by
    at most 2^-11 A.  This is the 1 of c.
  * A probability below 2^-14 relative to the running maximum m' is an fp16 denormal.  Rounded
    to a denormal or flushed to zero (whichever the MFMA does), it loses at most itself.  m' never
    exceeds the row's final maximum, so such a key has p^_k < 2^-14: T covers it.
  * s_k: the products of two fp16 are exact in fp32; D additions, each within 2^-23 of the
    running sum (one ulp: true whether the unit's adder rounds to nearest or truncates), so
    |ds| <= 2 D u S and the weight 2^s moves by e_k <= ln2 2 D u S.  The same p_k enters O and l:
    y = sum w v / sum w with w_k = p_k (1 + e_k) is within 2 max|e_k| A of sum p v / sum p.
    2 ln2 2 D u S = ln2 D S 2^-11 2^-11: the second term of c.
  * the rest, in units of 2^-11 A, for up to 32 key blocks (nk <= 2048): exp2f within 2 ulp and
    the rounding of s - m' (|s - m'| <= 14 above the denormal range), both in O and l:
    2 (2^-22 + 14 ln2 u) < 0.004; alpha the same per block, 32 blocks: 2 * 32 * 1.1 * 2^-22 <
    0.04; l's fp32 sum (each term through at most 34 + 2 * 32 adds / multiplies) < 0.012; O's
    fp32 MFMA accumulation and rescales (32 + 10 * 32 roundings at most) < 0.05; 1 / l and the
    final product, 4 u, < 0.001; second-order products of the above < 0.02.  Sum < 0.13: 0.25.
  * the cap.  The s_k term is a worst case: all D roundings a full ulp, all in one direction.
    It passes 2.75 only for long, large dot products (D = 256 with Q x 8: up to 15).  There c is
    held at 4, the figure the bound was proposed with.  That still admits a score error of
    2.75 2^-11 / (2 ln2) = 2^-10: at S = 140 (the largest here) 117 u S, where D = 256 roundings
    to nearest that are not aligned reach about sqrt(D) u S = 16 u S and the worst case is
    2 D u S = 512 u S.  A mask, key-order or rescale mistake misses the bound by factors of
    hundreds (tests/test_attn_ref_cpu.py), so the cap costs the check nothing it could catch.
No constant here is fitted to a device run; the tests print the measured maximum of
|y - ref16| / (c 2^-11 A + T) and the range of c.

The second tier holds y to the unrounded float64 attention (`attention_exact`) within
2e-2 max|V|: it bounds what rounding the operands to fp16 costs.
"""
import numpy as np

AP_BK = 64          # keys per block (AP_BK of attn_prefill.hip)
LOG2E_F32 = np.float32(1.4426950408889634)
DENORM = 2.0 ** -14  # smallest normal fp16
C0, C_CAP = 1.25, 4.0


def vt_pos(k):
    """Position of key k in a V^T row: bits 2 and 3 swapped (of each 16 keys: 0-3, 8-11, 4-7, 12-15)."""
    k = np.asarray(k)
    return (k & ~12) | ((k & 4) << 1) | ((k & 8) >> 1)


def ldt_of(nk):
    return (nk + AP_BK - 1) // AP_BK * AP_BK


def kv_images(K, V, d, ldt=None, swap=True):
    """The scratch images of a cache K, V [nk][E] (float32): K16 [nk][E] = fp16(K) and
    Vt16 [H][d][ldt] with Vt16[h][dim][vt_pos(key)] = fp16(V[key][h d + dim]), columns of keys
    >= nk zero.  (The K16 area has ldt rows; the kernels neither write nor read rows >= nk.)"""
    nk, E = K.shape
    H = E // d
    ldt = ldt_of(nk) if ldt is None else ldt
    K16 = np.ascontiguousarray(K, np.float32).astype(np.float16)
    Vt = np.zeros((H, d, ldt), np.float16)
    pos = vt_pos(np.arange(nk)) if swap else np.arange(nk)
    Vt[:, :, pos] = np.ascontiguousarray(V, np.float32).astype(np.float16).reshape(nk, H, d).transpose(1, 2, 0)
    return K16, Vt


def images_mismatch(k16, vt16, K, V, d):
    """None when the scratch images k16 [>= nk][E], vt16 [H][d][ldt] (fp16) are bit for bit
    kv_images(K, V), zero padding included; else what differs."""
    nk = K.shape[0]
    wk, wv = kv_images(K, V, d, ldt=vt16.shape[2])
    if not np.array_equal(np.asarray(k16)[:nk].view(np.uint16), wk.view(np.uint16)):
        return "K16 rows"
    bad = np.asarray(vt16).view(np.uint16) != wv.view(np.uint16)
    if bad.any():
        h, dim, pos = (int(v) for v in np.argwhere(bad)[0])
        return f"{int(bad.sum())} V^T halves, first at head {h} dim {dim} position {pos}" + (" (padding)" if vt_pos(pos) >= nk else "")
    return None


def q16_of(Q, scale):
    qs = np.float32(scale) * LOG2E_F32
    return (np.ascontiguousarray(Q, np.float32) * qs).astype(np.float16)


def attention(Q, K, V, d, n_past, scale):
    """ref16, A, T [N][E] and S [N][H] (module docstring) of queries Q [N][E] over K, V [nk][E]."""
    N, E = Q.shape
    nk = K.shape[0]
    H = E // d
    q16 = q16_of(Q, scale).astype(np.float64)
    k16 = np.ascontiguousarray(K, np.float32).astype(np.float16).astype(np.float64)
    v16 = np.ascontiguousarray(V, np.float32).astype(np.float16).astype(np.float64)
    mask = np.arange(nk)[None, :] > (n_past + np.arange(N))[:, None]
    ref, A, T = (np.empty((N, E)) for _ in range(3))
    S = np.empty((N, H))
    for h in range(H):
        sl = slice(h * d, (h + 1) * d)
        s = q16[:, sl] @ k16[:, sl].T
        s[mask] = -np.inf
        p = np.exp2(s - s.max(axis=1, keepdims=True))
        l = p.sum(axis=1, keepdims=True)
        av = np.abs(v16[:, sl])
        ref[:, sl] = (p @ v16[:, sl]) / l
        A[:, sl] = (p @ av) / l
        T[:, sl] = (np.where(p < DENORM, p, 0.0) @ av) / l
        sa = np.abs(q16[:, sl]) @ np.abs(k16[:, sl]).T
        sa[mask] = 0.0
        S[:, h] = sa.max(axis=1)
    return ref, A, T, S


def attention_exact(Q, K, V, d, n_past, scale):
    """Causal softmax attention of the unrounded operands in float64 (the second tier's reference)."""
    N, E = Q.shape
    nk = K.shape[0]
    mask = np.arange(nk)[None, :] > (n_past + np.arange(N))[:, None]
    ref = np.empty((N, E))
    for h in range(E // d):
        sl = slice(h * d, (h + 1) * d)
        s = (Q[:, sl].astype(np.float64) @ K[:, sl].astype(np.float64).T) * scale
        s[mask] = -np.inf
        p = np.exp(s - s.max(axis=1, keepdims=True))
        p /= p.sum(axis=1, keepdims=True)
        ref[:, sl] = p @ V[:, sl].astype(np.float64)
    return ref


class Ref:
    """The references of one (Q, K, V) case, computed once and shared by the tests that check
    several runs against it."""

    def __init__(self, Q, K, V, d, n_past, scale):
        assert K.shape[0] == n_past + Q.shape[0] <= 32 * AP_BK, "the bound's constant covers 32 key blocks"
        self.d, self.V = d, V
        self.ref16, self.A, self.T, self.S = attention(Q, K, V, d, n_past, scale)
        self.c = np.minimum(C_CAP, C0 + np.log(2.0) * d * self.S * 2.0 ** -11)  # [N][H]
        self.bound = np.repeat(self.c, d, axis=1) * 2.0 ** -11 * self.A + self.T
        self.exact = attention_exact(Q, K, V, d, n_past, scale)

    def ratio(self, y):
        """max |y - ref16| / bound (inf for a NaN or where a zero bound is missed)."""
        err = np.abs(np.asarray(y, np.float64) - self.ref16)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(err == 0.0, 0.0, err / self.bound)
        r = np.where(np.isnan(r), np.inf, r)
        return float(r.max())

    def check(self, y, what=""):
        """Both tiers; returns the first tier's measured maximum ratio."""
        y = np.asarray(y, np.float64).reshape(self.ref16.shape)
        r = self.ratio(y)
        assert r <= 1.0, f"{what}: |y - ref16| reaches {r:.3g} x (c 2^-11 A + T), c up to {self.c.max():.2f}"
        e2 = float(np.max(np.abs(y - self.exact)))
        assert e2 <= 2e-2 * np.max(np.abs(self.V)), f"{what}: |y - fp64| = {e2:.3g}"
        return r
