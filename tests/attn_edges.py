"""Adversarial single-query attention rows for the exact decode heads (attn.hpp attn_body).

Every generator is numpy only, seeded, and returns rows (q, k, v, kc, vc, pos) for
vsim_op_attn_decode_batch / vsim_op_tail_attn: q, k, v [E] before RoPE, the caches [n_ctx][E]
with every row at or past pos NaN, and the position.  reference_row() composes the oracle's ops
for such a row (tests/test_gpu_batch_ops.py composes with it too), optionally with the raw KQ
scores replaced, which is how the CPU test shows that a row bites.

Finite inputs only: NaN and Inf scores stay out, because the reference's soft_max takes its
maximum in an order-dependent way there (a NaN compares false either way), so no single answer
exists to be bit-exact with.

Families
  cert_gross    keys with q[a] = q[b] = 1, k[a] = 2^52, k[b] = -2^52 (a < b): the reference's
                sequential double sum rounds every product between a and b to an integer, the
                exactly rounded sum does not, and the kernel's certificate must send the key to
                its sequential redo.  a, b sit at dims >= n_rot, so RoPE leaves them alone.
  cert_one_ulp  a seeded search for rows whose sequential sum and exactly rounded sum differ by
                one float ulp, at scores of 4096 / scale, where one ulp of the score is one fp16
                ulp of (score - max) and so another exp table entry.
  softmax_*     score spreads at the fp16 exp table's edges.
  quant_*       one-hot probabilities that hand the quantizer a chosen V row.
"""
import functools
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# (style, d, H, n_rot, alibi, kqv_nth): the cases of tests/test_gpu_batch_ops.py with a dimension
# RoPE leaves alone (n_rot < d), which the certificate and softmax rows need; those of E = 192 for
# the quantizer rows
CASES = [(0, 64, 2, 32, False, 1), (0, 96, 3, 24, False, 3), (0, 256, 3, 64, False, 1), (1, 256, 2, 64, False, 3),
         (1, 96, 2, 32, False, 1), (0, 64, 3, 0, True, 3), (0, 96, 2, 0, True, 1), (0, 256, 2, 0, True, 1)]
QUANT_CASES = [(0, 64, 3, 0, True, 3), (1, 96, 2, 32, False, 1), (0, 96, 2, 0, True, 1)]


def case_id(c):
    return "-".join(str(int(v)) for v in c)


def f32(x):
    return np.asarray(x, np.float32)


def head_scale(d):
    return np.float32(1.0 / np.sqrt(np.float64(np.float32(d))))


# ------------------------------------------------------------------ the reference composition
def kqv_runs(V, p, d, H, nth):
    """ggml.c:4535-4581 + 4469-4493 for one query at --threads nth: pool thread t mads keys
    [t dc, t dc + dc) in order in float32 from 0, FINALIZE adds the partial rows in thread order."""
    nk = V.shape[0]
    Vr = V.reshape(nk, H, d)
    dc = (nk + nth - 1) // nth
    out = None
    with np.errstate(over="ignore", invalid="ignore"):
        for t in range(nth):
            part = np.zeros((H, d), np.float32)
            for ic in range(dc * t, min(dc * t + dc, nk)):
                part = (part + (Vr[ic] * p[:, ic:ic + 1]).astype(np.float32)).astype(np.float32)
            out = part if out is None else (out + part).astype(np.float32)
    return out


def slopes(H):
    """ggml_alibi's head slopes, read off the oracle: alibi of a zero score in row 0 is 1 * m_h."""
    import oracle_py as O
    z = np.zeros(H, np.float32)
    O.lib().vo_alibi_f32(O.p(z), 1, 1, H, H)
    return z


def reference_row(case, row, scores=None, want_p=False):
    """One row's step from the oracle's ops: (out [E], its Q4_0 AoS bytes, the K and V cache rows
    it writes).  case = (style, d, H, n_rot, alibi, nth).  scores: raw KQ [H][nk] used instead of
    O.kq's.  want_p: also the raw scores and the probabilities, [H][nk] each."""
    import oracle_py as O
    style, d, H, n_rot, alibi, nth = case
    q, k, v, kc, vc, pos = row
    E = d * H
    if n_rot:
        name = "neox" if style == 0 else "gptj"
        q = O.rope(name, q, d, H, 1, pos, n_rot, 0)
        k = O.rope(name, k, d, H, 1, pos, n_rot, 0)
    nk, scale = pos + 1, float(head_scale(d))
    K = np.concatenate([kc[:pos], k.reshape(1, E)]).astype(np.float32)
    V = np.concatenate([vc[:pos], v.reshape(1, E)]).astype(np.float32)
    s = O.kq(K, q, d, H, nk, 1) if scores is None else f32(scores).reshape(-1).copy()
    if alibi:
        p = O.attn_softmax_alibi(s, nk, 1, H, pos, H, scale)
    else:
        p = O.attn_softmax(s, nk, 1, H, pos, scale)
    if nth == 1:
        out = O.kqv(V, p, d, H, nk, 1).reshape(E)
    else:
        out = kqv_runs(V, p.reshape(H, nk), d, H, nth).reshape(E)
    res = (out, O.quantize(out), k.reshape(E), v.reshape(E))
    if want_p:
        res += (s.reshape(H, nk), p.reshape(H, nk), q.reshape(E), K)
    return res


def seq_dot(k, q):
    """The reference's f32 dot (ggml.c:4760-4800): float products, summed in order in double."""
    prod = (f32(k) * f32(q)).astype(np.float32).astype(np.float64)
    return np.float32(np.add.accumulate(prod)[-1])


def exact_dot(k, q):
    """The same float products, summed exactly and rounded once."""
    prod = (f32(k) * f32(q)).astype(np.float32).astype(np.float64)
    return np.float32(math.fsum(prod.tolist()))


def exact_scores(case, row):
    """[H][nk] raw scores from the exactly rounded sums, for reference_row(scores=...)."""
    _, d, H, _, _, _ = case
    pos = row[5]
    qr, K = reference_row(case, row, want_p=True)[6:8]
    out = np.empty((H, pos + 1), np.float32)
    for h in range(H):
        for j in range(pos + 1):
            out[h, j] = exact_dot(K[j, h * d:(h + 1) * d], qr[h * d:(h + 1) * d])
    return out


def _blank(rng, E, n_ctx, pos, kstd=1.0):
    q, k, v = (rng.standard_normal(E).astype(np.float32) for _ in range(3))
    kc = (rng.standard_normal((n_ctx, E)) * kstd).astype(np.float32)
    vc = rng.standard_normal((n_ctx, E)).astype(np.float32)
    k *= np.float32(kstd)
    return q, k, v, kc, vc


def _seal(q, k, v, kc, vc, pos):
    kc[pos:] = np.nan  # nothing at or past the position may be read before it is written
    vc[pos:] = np.nan
    return f32(q), f32(k), f32(v), kc, vc, int(pos)


def gaussian_row(case, n_ctx, pos, seed):
    _, d, H, _, _, _ = case
    rng = np.random.default_rng(seed)
    return _seal(*_blank(rng, d * H, n_ctx, pos), pos)


# ------------------------------------------------------------------ certificate rows (gross)
def cert_ab(d, n_rot, same_lane):
    """(a, b) at dims >= n_rot.  Lane l16 of a key's 16 holds the float4s at 4 l16 + 64 e, so b =
    a + 64 is the same lane (d >= 128, or d = 96 with a < 32); a just above n_rot (lane 0, 6 or 8)
    and b = d - 4 (lane 15 or 7) are two lanes.  None when no same-lane pair lies above n_rot."""
    a = n_rot + 1
    if same_lane:
        return (a, a + 64) if a + 64 < d else None
    return a, d - 4


def _craft(krow, q, h, d, a, b, big=52):
    krow[h * d + a] = np.float32(2.0 ** big)
    krow[h * d + b] = -np.float32(2.0 ** big)
    q[h * d + a] = q[h * d + b] = np.float32(1.0)


# crafted cached keys: waves 0, 5, 10 and 15 of the 16-wave kernel (key / 16 % 16; with the tail's
# 11 waves, key / 16 % 11: waves 0, 5, 10 and 4), each of the ATT_KB = 4 steps, each 16-lane row
CERT_KEYS = [16 * w + 4 * j + (j + w) % 4 for w in (0, 5, 10, 15) for j in range(4)]


def cert_gross(case, n_ctx, seed=0):
    """Four rows (each with (a, b) in every head; the crafted keys listed per row):
    0: pos 300, CERT_KEYS crafted in the cache, (a, b) in different lanes
    1: pos 300, the new key crafted: the only valid key of its step (rows 1-3 clamped), read back
       after the barrier
    2: pos 301, cached key 300 and the new key 301 crafted, keys 302, 303 of the step clamped
    3: pos 300, CERT_KEYS crafted with a and b in one lane where d allows (else as row 0 at
       another seed)
    Returns [(row, crafted key indices)]."""
    _, d, H, n_rot, _, _ = case
    E = d * H
    rows = []
    ab_same = cert_ab(d, n_rot, True) or cert_ab(d, n_rot, False)
    for i, (pos, keys, ab) in enumerate([(300, CERT_KEYS, cert_ab(d, n_rot, False)), (300, [300], cert_ab(d, n_rot, False)),
                                         (301, [300, 301], ab_same), (300, CERT_KEYS, ab_same)]):
        rng = np.random.default_rng(7000 + 100 * seed + 10 * d + i)
        q, k, v, kc, vc = _blank(rng, E, n_ctx, pos, kstd=0.25)
        for h in range(H):
            for key in keys:
                _craft(k if key == pos else kc[key], q, h, d, *ab)
        rows.append((_seal(q, k, v, kc, vc, pos), list(keys)))
    return rows


# ------------------------------------------------------------------ certificate rows (one ulp)
ONE_ULP_SEED = 20240
ONE_ULP_TRIALS = 600
ONE_ULP_ROWS = 12  # kept per case (the search finds about 55 hits per 600 trials; the first 12 that bite)
ONE_ULP_POS = 37


def _one_ulp_candidates(d, n_rot):
    """(q_head, k_head, a, b, m) with float(sequential sum) one ulp from float(fsum)."""
    rng = np.random.default_rng(ONE_ULP_SEED + d)
    # k = alpha q + noise over the unrotated dims: raw score ~ alpha (d - n_rot) = 4096 / scale
    alpha = np.float32(4096.0 / float(head_scale(d)) / (d - n_rot))
    out = []
    for _ in range(ONE_ULP_TRIALS):
        q = rng.standard_normal(d).astype(np.float32)
        q[:n_rot] = 0.0  # the kernel rotates q there; zeros stay zeros
        k = (alpha * q + rng.standard_normal(d).astype(np.float32)).astype(np.float32)
        a = int(rng.integers(n_rot, d - 8))
        b = int(rng.integers(a + 4, d))
        m = int(rng.integers(30, 45))
        q[a] = q[b] = np.float32(1.0)
        k[a], k[b] = np.float32(2.0 ** m), -np.float32(2.0 ** m)
        s, e = seq_dot(k, q), exact_dot(k, q)
        if abs(int(s.view(np.int32)) - int(e.view(np.int32))) == 1:
            out.append((q, k, a, b, m))
    return out


@functools.lru_cache(maxsize=None)
def cert_one_ulp(case, n_ctx, limit=ONE_ULP_ROWS):
    """Rows at pos 37 whose head 0 holds one search hit as cached key 20 and, as key 9, the same key
    without the cancelling pair and 0.7 / scale lower, so the two lead the softmax 0.7 apart at
    4096; all other keys are small.  Only rows whose composed reference output changes when the
    hit's score is replaced by the exactly rounded one are kept (at most `limit`)."""
    _, d, H, n_rot, _, _ = case
    E, pos, scale = d * H, ONE_ULP_POS, float(head_scale(d))
    rows = []
    for i, (qh, kh, a, b, m) in enumerate(_one_ulp_candidates(d, n_rot)):
        rng = np.random.default_rng(ONE_ULP_SEED + 31 * i + d)
        q, k, v, kc, vc = _blank(rng, E, n_ctx, pos, kstd=0.05)
        q[:d] = qh
        kc[20, :d] = kh
        k2 = kh.copy()
        k2[a] = k2[b] = 0.0
        c = int(np.argmax(np.abs(qh[n_rot:]) * (np.arange(n_rot, d) != a) * (np.arange(n_rot, d) != b))) + n_rot
        k2[c] -= np.float32(0.7 / scale / float(qh[c]))
        kc[9, :d] = k2
        row = _seal(q, k, v, kc, vc, pos)
        s, e = seq_dot(kh, qh), exact_dot(kh, qh)
        ref = reference_row(case, row, want_p=True)
        sc = ref[4].copy()
        assert sc[0, 20].view(np.uint32) == s.view(np.uint32)  # seq_dot restates the oracle's dot
        sc[0, 20] = e
        alt = reference_row(case, row, scores=sc)
        if np.array_equal(ref[0].view(np.uint32), alt[0].view(np.uint32)):
            continue
        rows.append(row)
        if len(rows) == limit:
            break
    return tuple(rows)


# ------------------------------------------------------------------ softmax extremes
def _score_row(case, n_ctx, pos, targets, seed, new_target):
    """A row whose scaled scores are targets[j] (float32(t / scale) * scale, to rounding): q is 1 at
    one unrotated dim c per head and Gaussian elsewhere, key j is targets[j] / scale at c, zero
    elsewhere.  targets has pos entries (the cache) and new_target is the new key's."""
    _, d, H, n_rot, _, _ = case
    E, scale = d * H, float(head_scale(d))
    if n_rot >= d:
        raise ValueError("needs an unrotated dim")
    rng = np.random.default_rng(seed)
    q, k, v, kc, vc = _blank(rng, E, n_ctx, pos)
    kc[:] = 0.0
    k[:] = 0.0
    for h in range(H):
        c = h * d + n_rot + (3 * h + 2) % (d - n_rot)
        q[c] = 1.0
        kc[:pos, c] = f32(np.asarray(targets, np.float64) / scale)
        k[c] = np.float32(new_target / scale)
    return _seal(q, k, v, kc, vc, pos)


def softmax_rows(case, n_ctx):
    """{family: [rows]}; the property each family must show on the oracle's own probabilities is
    checked by tests/test_attn_edges_cpu.py:
      overflow   differences past -65504: f2h gives -inf, probability exactly 0
      denormal   differences of -10 .. -17: the exp table's entries are fp16 denormals
      tiny       differences below 6.1e-5 (an fp16-denormal argument) and below 3e-8 (+-0)
      tie        two keys share the maximum exactly
      equal      all keys equal, nk = 1, 17 and 300
      onehot     one key at the top, every other one past -65504"""
    rng = np.random.default_rng(99)
    fam = {}
    pos = 41
    t = np.zeros(pos)
    t[:] = -rng.uniform(66000.0, 200000.0, pos)
    t[5], t[17], t[30] = 0.0, -1.5, -65400.0
    fam["overflow"] = [_score_row(case, n_ctx, pos, t, 1, new_target=-70000.0)]
    t = -rng.uniform(10.0, 17.0, pos)
    t[11] = 0.0
    fam["denormal"] = [_score_row(case, n_ctx, pos, t, 2, new_target=-16.5)]
    t = -rng.uniform(1e-6, 6.0e-5, pos)
    t[::3] = -rng.uniform(1e-10, 2.9e-8, t[::3].size)
    t[7] = 0.0
    fam["tiny"] = [_score_row(case, n_ctx, pos, t, 3, new_target=-2e-8)]
    t = -rng.uniform(0.5, 6.0, pos)
    t[4] = t[33] = 0.25
    fam["tie"] = [_score_row(case, n_ctx, pos, t, 4, new_target=-1.0),
                  _score_row(case, n_ctx, pos, t, 5, new_target=0.25)]
    fam["equal"] = [_score_row(case, n_ctx, p, np.full(p, 1.75), 6 + p, new_target=1.75) for p in (0, 16, 299)]
    t = -rng.uniform(66000.0, 200000.0, pos)
    t[23] = 3.0
    fam["onehot"] = [_score_row(case, n_ctx, pos, t, 7, new_target=-90000.0)]
    return fam


# ------------------------------------------------------------------ quantizer edges
def qrow_edges():
    """(x [192], y bytes [120]): the six hand-built edge blocks of the golden quantize_row_q4_0
    case (zeros, ties, subnormals, 1e30, constant -5, a ramp) and the reference's Q4_0 bytes."""
    z = np.load(os.path.join(GOLDEN, "ops_qrow.npz"))
    return f32(z["x"][-192:]), np.asarray(z["y"][-120:], np.uint8)


def quant_rows(case, n_ctx):
    """[cached, newest, zeros] for E = 192: a one-hot softmax (p exactly 1.0 on one key, 0 on the
    rest) whose key's V row is the edge blocks, as cached key 19 and as the new key; and an
    all-zero V cache.  The head outputs are then that row exactly."""
    _, d, H, _, _, _ = case
    assert d * H == 192
    x, _ = qrow_edges()
    pos = 41
    rows = []
    for hot in (19, pos):
        t = np.full(pos, -90000.0)
        if hot < pos:
            t[hot] = 2.0
        q, k, v, kc, vc, _ = _score_row(case, n_ctx, pos, t, 50 + hot, new_target=2.0 if hot == pos else -80000.0)
        if hot < pos:
            vc[hot] = x
        else:
            v = x.copy()
        rows.append((q, k, v, kc, vc, pos))
    q, k, v, kc, vc, _ = gaussian_row(case, n_ctx, pos, 77)
    vc[:pos] = 0.0
    rows.append((q, k, np.zeros_like(v), kc, vc, pos))
    return rows
