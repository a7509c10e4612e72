"""Inputs, a numpy restatement and the row-independence comparator for weight-only mode's fp16
attention (vsim_amd/csrc/attn_w4a16.hip), shared by tests/test_gpu_w4a16_attn_ops.py (the device's two
forms against each other, bit for bit, and against tests/attn_ref.py's bound) and
tests/test_w4a16_attn_cpu.py (the inputs have teeth: six plausible kernel shortcuts are rejected on
them, the first four by the comparator, the last two by attn_ref.Ref.check).

The contract per row (one head, D dims, query at absolute position p, keys 0..p of the fp32 cache):
    q16 = fp16(float32(q) * qs), qs = float32(scale) * float32(log2 e); k16 = fp16(k), v16 = fp16(v)
    key blocks of 64 aligned to key 0, visited 0 .. p / 64 and no others
    S = K16 . q16 (the matrix core, from C = 0); keys past p: out of the maximum, p_k = 0 exactly
    m' = max(m, block max), alpha = exp2f(m - m'), p_k = exp2f(s_k - m')
    l = l alpha + sum p_k  (the half-wave's 32 keys in register order, then the two halves added)
    O = O alpha, then O += V16^T . fp16(P)^T (the matrix core); V of keys past the last key is zero
    y = O / l + 0.0f
numpy cannot restate the matrix core's inner order, so both products here are a stand-in shared by
every variant: the exact sum (float64) rounded once to fp32, with IEEE's sign for a zero result of
adding C (minus zero only when C and every product are minus zero).  Everything else is restated in
float32.  `emulate_prompt` and `emulate_rows` model the two launch forms: what a kernel built with
shortcut `variant` would give for each row *in that launch*; with variant None neither depends on
the launch.
"""
import numpy as np

import attn_ref as R

F32 = np.float32
BK = R.AP_BK
H = 2
N_CTX = 256
DS = (64, 96, 128, 256)
PROMPTS = ((1, 0), (7, 0), (33, 0), (130, 0), (5, 62), (130, 61))
SEAMS = (0, 1, 31, 32, 62, 63, 64, 65, 127, 128, 129, 191, 255)
VARIANTS = ("shared_max", "npast_blocks", "v_tail", "visit_no_rule", "p_rtz", "mask_value")
ROW_VARIANTS = VARIANTS[:4]   # rejected by the row-independence comparator
REF_VARIANTS = VARIANTS[4:]   # rejected by attn_ref.Ref.check
MASK_VALUE = F32(-1.0e4)      # variant mask_value: what a masked score is set to, instead of exclusion
# (style, n_rot) per head dim of the random family: GPT-J pairs (1) and rotate-half (0) at two dims
# each; n_rot = 0 once more at d = 64 (ROPE_NONE) and in the zero family
ROPE = {64: (1, 32), 96: (0, 24), 128: (1, 128), 256: (0, 64)}
ROPE_NONE = (64, 0, 0)
# the sign-of-zero family: the prompt (N, n_past) and the row whose bits the shortcut flips
ZERO_PROMPT, ZERO_POS = (126, 5), 127


def head_scale(d):
    return float(F32(1.0) / np.sqrt(F32(d)))


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ------------------------------------------------------------------ inputs
def random_world(d, seed=0, qmul=1.0):
    """q, k, v [N_CTX][H d] float32 before RoPE: one sequence of N_CTX tokens."""
    rng = np.random.default_rng(7000 + 13 * d + seed)
    E = H * d
    q = (rng.standard_normal((N_CTX, E)) * qmul).astype(F32)
    k = rng.standard_normal((N_CTX, E)).astype(F32)
    v = rng.standard_normal((N_CTX, E)).astype(F32)
    return q, k, v


def zero_world(d, seed):
    """The sign-of-zero family (n_rot = 0).  Per head: q = 8 sqrt(d) on dims 0..3 and 0 elsewhere; key
    j < 100 has k = -(400 + r_j) on dims 0..3 (r_0 = 0, else r_j an integer in 1..8; every score is then
    exact in fp32, -4 c (400 + r_j) with c = fp16(8 sqrt(d) qs) = 11.54: about -18,500, and key 0 holds
    block 0's maximum), key 100 and the keys after it have k = 0 there (score 0): at a row's block 1
    the maximum rises by thousands and alpha underflows to 0.  (Rows before key 100 see only scores
    below -1e4: a kernel that masks with such a value instead of excluding gives them to masked keys.)  V's dimension 0 is
    negative at key 0, so O[0] < 0 after block 0 and -0 after the rescale; afterwards it is -0.0 or 0:
    seeds = 0 mod 2 make it -0.0 at every key from 64 on (block 1 then adds only -0 products and O[0]
    stays -0 for the row at position 127, which sees the whole block), odd seeds draw the sign per
    key.  The other dims of V are random."""
    rng = np.random.default_rng(9000 + 17 * d + seed)
    E = H * d
    q = np.zeros((N_CTX, E), F32)
    k = rng.standard_normal((N_CTX, E)).astype(F32)
    v = rng.standard_normal((N_CTX, E)).astype(F32)
    for h in range(H):
        q[:, h * d:h * d + 4] = F32(8.0 * np.sqrt(d))
        r = rng.integers(1, 9, (100, 1))
        r[0] = 0
        k[:100, h * d:h * d + 4] = -(400.0 + r)
        k[100:, h * d:h * d + 4] = 0.0
        v[0, h * d] = -1.5
        sign = rng.integers(0, 2, N_CTX - 1).astype(bool)
        v[1:, h * d] = np.where(sign, F32(-0.0), F32(0.0))
        if seed % 2 == 0:
            v[64:, h * d] = F32(-0.0)
    return q, k, v


PAIR_PROMPT = (4, 0)


def pair_world(d, seed):
    """The two-key family (n_rot = 0).  Per head q = 8 sqrt(d) on dimension 0 and 0 elsewhere, so a score
    is one exact product c k_0 (c = 11.54) and the bound's S is the score itself; key 1 has k_0 = 0
    (score 0), key 0 has k_0 in (-0.087, -0.05) (score in (-1, -0.58)), the later keys lie between.
    V = 1 at key 0 and 0 at key 1 in every dimension.  Row 1 sees those two keys only: its output is
    p_0 / (1 + p_0) with p_0 anywhere in (0.5, 0.67), where fp16's relative step is widest and the
    bound's c is near its floor of 1.25 -- an error in the direction fp16(P) is rounded shows undiluted."""
    rng = np.random.default_rng(11000 + 19 * d + seed)
    E = H * d
    q = np.zeros((N_CTX, E), F32)
    k = rng.standard_normal((N_CTX, E)).astype(F32)
    v = rng.standard_normal((N_CTX, E)).astype(F32)
    for h in range(H):
        q[:, h * d] = F32(8.0 * np.sqrt(d))
        k[:, h * d] = -rng.uniform(0.0, 0.087, N_CTX)
        k[0, h * d] = -rng.uniform(0.05, 0.087)
        k[1, h * d] = 0.0
    v[0, :] = 1.0
    v[1, :] = 0.0
    return q, k, v


def pair_search(d, max_seeds=32):
    """The first seed of pair_world(d, seed) on which shortcut p_rtz misses attn_ref's bound (the
    emulation decides): (seed, q, k, v, Ref).  None if none does."""
    N, n_past = PAIR_PROMPT
    scale = head_scale(d)
    for seed in range(max_seeds):
        q, k, v = pair_world(d, seed)
        ref = R.Ref(q[:N], k[:N], v[:N], d, n_past, scale)
        if ref.ratio(emulate_prompt(q[:N], k, v, d, n_past, scale, "p_rtz")) > 1.0:
            return seed, q, k, v, ref
    return None


def stale_rows(n, E, kind, seed=0, row0=0):
    """Cache rows row0 .. row0 + n - 1 as an earlier sequence may have left them (a function of the
    row's own index, so that two caches of one kind agree wherever both are stale).  nan: all NaN;
    mixed: NaN, +Inf, -Inf and 6e4 by turns along both axes; finite: random finite values (another
    legitimate tail)."""
    if kind == "nan":
        return np.full((n, E), np.nan, F32)
    if kind == "finite":
        return np.random.default_rng(31 + seed).standard_normal((row0 + n, E)).astype(F32)[row0:]
    pat = np.array([np.nan, np.inf, -np.inf, 6.0e4], F32)
    return pat[(seed + row0 + np.arange(n)[:, None] + np.arange(E)[None, :]) % 4]


def rope_np(x, pos, d, n_rot, style):
    """RoPE of rows x [n][H d] at positions pos (float64 angles, one rounding): the arithmetic of
    vsim_op_rope_kv_write, for the CPU test's inputs (the GPU test takes the device's own rows)."""
    x = np.array(x, F32)
    if n_rot == 0:
        return x
    half = n_rot // 2
    theta = np.power(10000.0, 2.0 * (-np.arange(half, dtype=np.float64)) / n_rot)
    ang = np.asarray(pos, np.float64)[:, None] * theta[None, :]
    c, s = np.cos(ang), np.sin(ang)
    for h in range(x.shape[1] // d):
        b = x[:, h * d:(h + 1) * d]
        i0 = np.arange(half) if style == 0 else 2 * np.arange(half)
        i1 = i0 + half if style == 0 else i0 + 1
        x0, x1 = b[:, i0].astype(np.float64), b[:, i1].astype(np.float64)
        b[:, i0] = (c * x0 - s * x1).astype(F32)
        b[:, i1] = (c * x1 + s * x0).astype(F32)
    return x


def ragged_positions(seed=0):
    """32 positions for one rows call: the seams, then random ones, in a permuted order."""
    rng = np.random.default_rng(500 + seed)
    pos = list(SEAMS) + [int(p) for p in rng.integers(0, N_CTX, 32 - len(SEAMS))]
    return [pos[i] for i in rng.permutation(32)]


# ------------------------------------------------------------------ the restatement
def _acc(C, A, B):
    """The stand-in for C + A . B on the matrix core: float64, rounded once; a zero result is -0
    only when C is -0 and every product is a minus zero (IEEE round-to-nearest)."""
    with np.errstate(invalid="ignore", over="ignore"):
        r = (C.astype(np.float64) + A.astype(np.float64) @ B.astype(np.float64)).astype(F32)
        zero = r == 0
        if zero.any():
            negc = np.signbit(C)
            for g, c in np.argwhere(zero):
                prod = A[g].astype(np.float64) * B[:, c].astype(np.float64)
                allneg = bool(np.all(np.signbit(prod) & (prod == 0)))
                r[g, c] = F32(-0.0) if (negc[g, c] and allneg) else F32(0.0)
    return r


def _rtz16(p):
    """p >= 0 cut off to fp16 toward zero (what a packing convert without rounding gives), as float32."""
    h = p.astype(np.float16)
    h = np.where(h.astype(F32) > p, np.nextafter(h, np.float16(0)), h)
    return h.astype(F32)


def _lane_sum(p):
    """sum of a block's 64 probabilities per row as the wave adds them: each half-wave (hl) its 32
    keys 32 t + (g & 3) + 8 (g >> 2) + 4 hl in the order t = 0, 1; g = 0..15, then the two halves."""
    halves = []
    for hl in range(2):
        s = np.zeros(p.shape[0], F32)
        for t in range(2):
            for g in range(16):
                s = s + p[:, 32 * t + (g & 3) + 8 * (g >> 2) + 4 * hl]
        halves.append(s)
    return halves[0] + halves[1]


def _group(q16, qpos, K16, V16, first, last_key, variant):
    """One query group (rows that share key blocks, as a wave's 32 queries do; one row in the rows
    form) of one head: q16 [G][d] float32 values of fp16, qpos [G], K16 / V16 [n][d] float32 values
    of fp16(cache) with whatever the tail holds.  first: the first block's first key (0; variant
    npast_blocks: aligned to n_past).  last_key: the launch's last key -- V of keys past it is zero
    (not with variant v_tail), K rows are clamped to it."""
    G, d = q16.shape
    n = K16.shape[0]
    m = np.full(G, -np.inf, F32)
    l = np.zeros(G, F32)
    O = np.zeros((G, d), F32)
    pmax = int(qpos.max())
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for k0 in range(first, pmax + 1, BK):
            keys = k0 + np.arange(BK)
            kidx = np.clip(keys, 0, last_key)
            s = (q16.astype(np.float64) @ K16[kidx].astype(np.float64).T).astype(F32)
            masked = (keys[None, :] > qpos[:, None]) | (keys[None, :] < 0)
            sees = ~masked.all(axis=1)
            if variant == "mask_value":
                s = np.where(masked, MASK_VALUE, s)
            else:
                s = np.where(masked, F32(-np.inf), s)
            bm = s.max(axis=1)
            if variant == "shared_max":
                bm = np.full(G, bm.max(), F32)
            mnew = np.maximum(m, bm)
            alpha = np.exp2(m - mnew).astype(F32)
            p = np.exp2(s - mnew[:, None]).astype(F32)
            if variant != "mask_value":
                p = np.where(masked, F32(0), p)
            lnew = l * alpha + _lane_sum(p)
            P = _rtz16(p) if variant == "p_rtz" else p.astype(np.float16).astype(F32)
            Vb = V16[np.clip(keys, 0, n - 1)].copy()
            dead = (keys < 0) | (keys > n - 1)
            if variant != "v_tail":
                dead |= keys > last_key
            Vb[dead] = 0
            Onew = _acc(O * alpha[:, None], P, Vb)
            if variant == "visit_no_rule":
                m, l, O = mnew, lnew, Onew  # (every row of the group goes through every block)
            else:
                m = np.where(sees, mnew, m)
                l = np.where(sees, lnew, l)
                O = np.where(sees[:, None], Onew, O)
        y = O / l[:, None]
        if variant != "visit_no_rule":
            y = y + F32(0.0)
    return y.astype(F32)


def _halves(Kc, Vc, h, d):
    sl = slice(h * d, (h + 1) * d)
    with np.errstate(over="ignore", invalid="ignore"):
        return Kc[:, sl].astype(np.float16).astype(F32), Vc[:, sl].astype(np.float16).astype(F32)


def emulate_prompt(Q, Kc, Vc, d, n_past, scale, variant=None):
    """The prompt form: Q [N][E] (after RoPE) at positions n_past.. over the cache Kc, Vc [n_ctx][E],
    whose rows from n_past + N on are stale.  Queries in groups of 32 from the prompt's first."""
    assert variant is None or variant in VARIANTS
    N, E = Q.shape
    q16 = R.q16_of(Q, scale).astype(F32)
    out = np.empty((N, E), F32)
    first = n_past % BK - BK if (variant == "npast_blocks" and n_past % BK) else 0
    for h in range(E // d):
        K16, V16 = _halves(Kc, Vc, h, d)
        for g0 in range(0, N, 32):
            g1 = min(N, g0 + 32)
            # (a 128-query block clamps K to its own last key; any in-range row serves a masked score)
            out[g0:g1, h * d:(h + 1) * d] = _group(q16[g0:g1, h * d:(h + 1) * d], n_past + np.arange(g0, g1), K16, V16,
                                                   first, n_past + N - 1, variant)
    return out


def emulate_rows(Q, caches, pos, d, scale, variant=None):
    """The single-query form: row b's query Q[b] (after RoPE) at pos[b] on caches[b] = (Kc, Vc)
    [n_ctx][E] holding its keys 0..pos[b] and a stale tail."""
    assert variant is None or variant in VARIANTS
    B, E = Q.shape
    q16 = R.q16_of(Q, scale).astype(F32)
    out = np.empty((B, E), F32)
    for b in range(B):
        p = int(pos[b])
        first = p % BK - BK if (variant == "npast_blocks" and p % BK) else 0
        for h in range(E // d):
            K16, V16 = _halves(caches[b][0], caches[b][1], h, d)
            out[b, h * d:(h + 1) * d] = _group(q16[b:b + 1, h * d:(h + 1) * d], np.array([p]), K16, V16, first, p,
                                               variant)[0]
    return out


# ------------------------------------------------------------------ the comparator
def rows_differ(a, b):
    """Rows whose bits differ between two evaluations of the same rows (uint32, so -0 != +0 and a
    NaN equals itself only bit for bit): the row-independence comparator.  [] when independent."""
    a, b = bits(a), bits(b)
    assert a.shape == b.shape
    return [int(i) for i in np.nonzero((a != b).reshape(a.shape[0], -1).any(axis=1))[0]]


def zero_search(d, emulate_p=emulate_prompt, emulate_r=emulate_rows, max_seeds=8):
    """The first seed of zero_world(d, seed) on which shortcut visit_no_rule flips a bit of the row
    at ZERO_POS between the two forms (the emulation decides): (seed, q, k, v).  None if none does."""
    N, n_past = ZERO_PROMPT
    scale = head_scale(d)
    i = ZERO_POS - n_past
    for seed in range(max_seeds):
        q, k, v = zero_world(d, seed)
        yp = emulate_p(q[n_past:n_past + N], k, v, d, n_past, scale, "visit_no_rule")[i:i + 1]
        yr = emulate_r(q[ZERO_POS:ZERO_POS + 1], [(k, v)], [ZERO_POS], d, scale, "visit_no_rule")
        if rows_differ(yp, yr):
            return seed, q, k, v
    return None
