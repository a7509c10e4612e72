"""fp64 restatement of the fast decode step's kernels (vsim_amd/csrc/fast_decode.hip) and the
checkers the per-kernel tests use (tests/test_gpu_fast_ops.py; their teeth are shown on the CPU
by tests/test_fast_ref_cpu.py).  numpy only.

Conventions: a Q4_0 row is (d [nb] float32, q [nb][32] int, the signed value nibble - 8); u =
2^-24 is the unit roundoff of one float operation.  A "tolerance" is an absolute bound per
element on |device - fp64|.
"""
import itertools
import math

import numpy as np

QK = 32
U = 2.0 ** -24


# ------------------------------------------------------------------ Q4_0 rows
def q4_quantize_ref(y):
    """quantize_row_q4_0 (ggml.c:209-251) per 32-block, in the reference's float steps:
    d = amax / 7, id = 1 / d (0 for d = 0), q = round-half-away(y * id).  Returns d [nb], q [nb][32]."""
    b = np.ascontiguousarray(y, np.float32).reshape(-1, QK)
    amax = np.abs(b).max(axis=1).astype(np.float32)
    d = (amax / np.float32(7.0)).astype(np.float32)
    with np.errstate(divide="ignore"):
        idv = np.where(d != 0, np.float32(1.0) / d, np.float32(0.0)).astype(np.float32)
    t = (b * idv[:, None]).astype(np.float32)
    q = np.where(t >= 0, np.floor(t + 0.5), -np.floor(-t + 0.5))  # (exact in float64: |t| <= 7)
    return d, q.astype(np.int64)


def q4_f16_ref(y):
    """The prompt GEMMs' operand: quantize_row_q4_0 of the f32 rows y, the values d*(q-8) rounded
    once to fp16."""
    d, q = q4_quantize_ref(y)
    return (d[:, None].astype(np.float64) * q).astype(np.float16).reshape(np.shape(y))


def w16_of(w_aos, K):
    """The fp16 weight operand of the prompt GEMMs: each Q4_0 value d*(q-8) rounded ONCE to
    fp16 from its exact value (gemm_f16.hip deq_word_f16: one v_fma_mix; the product d*(q-8)
    is exact in fp64 and numpy's fp64 -> fp16 conversion rounds to nearest even directly)."""
    blk = np.asarray(w_aos, dtype=np.uint8).reshape(-1, 20)
    d = blk[:, :4].copy().view(np.float32).reshape(-1).astype(np.float64)
    q = np.empty((blk.shape[0], 32), dtype=np.float64)
    q[:, 0::2] = (blk[:, 4:] & 0xF).astype(np.float64) - 8
    q[:, 1::2] = (blk[:, 4:] >> 4).astype(np.float64) - 8
    return (q * d[:, None]).astype(np.float16).reshape(-1, K)


def gemm_f16_tol(K, abs16, bias=None):
    """The fp16 MFMA GEMMs' per-element bound against the fp64 product of the fp16-rounded operands
    (tests/test_gpu_ops.py test_prefill_gemm_f16): products of two fp16 are exact in fp32, the fp32
    accumulation of K of them in any order stays within 4 K 2^-24 sum |w16 x16| (abs16), and the
    bias add within 1e-6 |b|."""
    t = 4.0 * K * 2.0 ** -24 * np.asarray(abs16, np.float64)
    return t if bias is None else t + 1e-6 * np.abs(np.asarray(bias, np.float64))


def q4_parse(aos, k):
    """ggml AoS blocks (fp32 d + 16 nibble bytes: lo = element 2l, hi = 2l+1) of rows of k values ->
    d [rows][nb] float32, q [rows][nb][32] signed."""
    blk = np.asarray(aos, np.uint8).reshape(-1, 20)
    d = blk[:, :4].copy().view(np.float32).reshape(-1)
    q = np.empty((blk.shape[0], QK), np.int8)
    q[:, 0::2] = blk[:, 4:] & 0xF
    q[:, 1::2] = blk[:, 4:] >> 4
    q -= 8
    nb = k // QK
    return d.reshape(-1, nb), q.reshape(-1, nb, QK)


def q4_pack(d, q):
    """The inverse of q4_parse: AoS bytes of the blocks (d, q signed)."""
    d = np.ascontiguousarray(d, np.float32).reshape(-1)
    n = (np.asarray(q).reshape(-1, QK) + 8).astype(np.uint8)
    out = np.empty((d.size, 20), np.uint8)
    out[:, :4] = d.view(np.uint8).reshape(-1, 4)
    out[:, 4:] = n[:, 0::2] | (n[:, 1::2] << 4)
    return out.reshape(-1)


def q4_dot(wd, wq, xd, xq, b0=0, b1=None):
    """Rows of W . x over blocks [b0, b1): sum_b d_w d_x s_b with s_b the exact integer block dot,
    in fp64, and the sum of the terms' magnitudes.  wd [M][nb], wq [M][nb][32], xd [nb], xq [nb][32]."""
    xf = np.asarray(xq)[b0:b1].astype(np.float32)
    dx = np.asarray(xd, np.float32)[b0:b1].astype(np.float64)
    y, a = np.empty(wq.shape[0]), np.empty(wq.shape[0])
    for r0 in range(0, wq.shape[0], 512):  # (row chunks: the integer dots are exact in float32, |s_b| <= 2048)
        s = (wq[r0:r0 + 512, b0:b1].astype(np.float32) * xf[None]).sum(axis=2)
        t = wd[r0:r0 + 512, b0:b1].astype(np.float64) * dx[None, :] * s
        y[r0:r0 + 512], a[r0:r0 + 512] = t.sum(axis=1), np.abs(t).sum(axis=1)
    return y, a


def gemv_tol(nb, absum):
    """|y - y64| <= (nb + 8) u sum_b |d_w d_x s_b| for a row of nb blocks (derivation:
    tests/test_gpu_fast_ops.py)."""
    return (nb + 8) * U * np.asarray(absum, np.float64)


def q4_margin(y):
    """Distance of the reference's y * id from the nearest rounding boundary (a half-integer), the
    smallest over the row."""
    d, _ = q4_quantize_ref(y)
    b = np.ascontiguousarray(y, np.float32).reshape(-1, QK)
    with np.errstate(divide="ignore"):
        idv = np.where(d != 0, np.float32(1.0) / d, np.float32(0.0)).astype(np.float32)
    t = np.abs((b * idv[:, None]).astype(np.float32).astype(np.float64))
    return float(np.abs(t - np.floor(t) - 0.5).min())


def _q4_expect(y_ref, tol):
    y_ref = np.asarray(y_ref, np.float64).reshape(-1, QK)
    tol = np.broadcast_to(np.asarray(tol, np.float64), y_ref.size).reshape(-1, QK)
    _, q_e = q4_quantize_ref(y_ref.astype(np.float32))
    amax = np.abs(y_ref).max(axis=1)
    ta = tol.max(axis=1)
    d64 = amax / 7.0
    dtol = ta / 7.0 + 2.0 * U * d64
    safe = np.where(d64 > 0, d64, 1.0)
    t = np.abs(y_ref) / safe[:, None]
    dt = tol / safe[:, None] + t * (ta / np.where(amax > 0, amax, 1.0) + 4.0 * U)[:, None]
    amb = np.abs(t - np.floor(t) - 0.5) <= dt
    return q_e, d64, dtol, amb


def q4_ambiguous_share(y_ref, tol):
    """The share of q4_check's ambiguous elements: a property of the reference and its bound
    alone, so a test can choose inputs that keep it small before anything runs."""
    return float(_q4_expect(y_ref, tol)[3].mean())


def q4_check(qs, d, y_ref, tol):
    """Is the device block (d [nb], qs [nb][32] signed) a quantization of some y with |y - y_ref| <=
    tol?  Expected (d, q): q4_quantize_ref(y_ref).  The device's amax lies within ta = max tol of
    the block of the reference's, so d within ta / 7 (+ its two float roundings); an element's
    y / d moves by at most tol / d + |y / d| (ta / amax + 4u): it is *ambiguous* when that reaches
    a rounding boundary, and may then differ by one step; every other element must match exactly.
    Returns the ambiguous share; raises AssertionError otherwise."""
    q_e, d64, dtol, amb = _q4_expect(y_ref, tol)
    qs = np.asarray(qs).reshape(-1, QK).astype(np.int64)
    d = np.asarray(d, np.float32).reshape(-1).astype(np.float64)
    bad = np.abs(d - d64) > dtol
    assert not bad.any(), (f"block scale outside the amax tolerance: block {int(np.argmax(bad))}, "
                           f"d {d[np.argmax(bad)]!r} vs {d64[np.argmax(bad)]!r} +- {dtol[np.argmax(bad)]!r}")
    diff = np.abs(qs - q_e)
    bad = np.where(amb, diff > 1, diff != 0)
    assert not bad.any(), (f"{int(bad.sum())} quantized value(s) off: first at {tuple(np.argwhere(bad)[0])}, "
                           f"device {qs[bad][0]} expected {q_e[bad][0]}")
    return float(amb.mean())


# ------------------------------------------------------------------ LayerNorm prologue
def layernorm_ref(x, w, b):
    """LnStage::finish: both moments in double (one pass: var = E[x^2] - mean^2), scale =
    (float)(1 / sqrt(var + (double)1e-5f)), y = w * ((float)(x - mean) * scale) + b in float steps."""
    x = np.ascontiguousarray(x, np.float32)
    xd = x.astype(np.float64)
    mean = xd.sum() / x.size
    var = (xd * xd).sum() / x.size - mean * mean
    scale = np.float32(1.0 / math.sqrt(var + float(np.float32(1e-5))))
    t = ((xd - mean).astype(np.float32) * scale).astype(np.float32)
    return ((np.asarray(w, np.float32) * t).astype(np.float32) + np.asarray(b, np.float32)).astype(np.float32)


# ------------------------------------------------------------------ GELU epilogue
def f2h_bits(x):
    return np.asarray(x, np.float64).astype(np.float16).view(np.uint16)


def gelu_candidates(s64, tol, gelu_tab):
    """The values the GELU epilogue may produce for a row whose float s + bias lies in s64 +- tol:
    h2f(table[h]) over the fp16 values h between f2h(s64 - tol) and f2h(s64 + tol) (f2h is
    monotone).  Near zero fp16 is far finer than any bound and the range holds many values: such
    a row keeps only its smallest and its largest table value (quantization is monotone in the
    value, and a range that narrow spans at most one rounding boundary) and is marked wide.
    Returns a list of float32 arrays, one per row, and the wide mask."""
    lo = np.asarray(s64 - tol, np.float64).astype(np.float16)
    hi = np.asarray(s64 + tol, np.float64).astype(np.float16)
    tab = np.asarray(gelu_tab, np.uint16)
    out, wide = [], []
    for a, z in zip(lo.reshape(-1), hi.reshape(-1)):
        c = [a]
        while c[-1] < z:
            c.append(np.nextafter(c[-1], np.float16(np.inf)))
            assert len(c) <= 4096, "the row tolerance spans more than 4096 fp16 values"
        bits = np.array(c, np.float16).view(np.uint16)
        v = np.unique(tab[bits].view(np.float16).astype(np.float32))
        wide.append(v.size > 2)
        out.append(v[[0, -1]] if v.size > 2 else v)
    return out, np.array(wide)


def gelu_q4_check(qs, d, s64, tol, gelu_tab):
    """The GELU-quantize epilogue's output blocks (d [nb], qs [nb][32] signed) for rows whose
    s + bias is s64 +- tol.  The fp16 conversion is a second discontinuity, so each 32-row block
    must equal q4_quantize_ref of some admissible combination of table values, exactly (the
    quantization of fixed float inputs is exact float arithmetic).  Returns the share of rows
    with more than one admissible value."""
    cand, wide = gelu_candidates(s64, tol, gelu_tab)
    qs = np.asarray(qs).reshape(-1, QK).astype(np.int64)
    d = np.asarray(d, np.float32).reshape(-1)
    n_amb = 0
    for blk in range(qs.shape[0]):
        cs = cand[blk * QK:(blk + 1) * QK]
        # a wide row's two ends stand for its range only while it cannot set the block's scale
        big = max(float(np.abs(c).min()) for c in cs)
        assert all(float(np.abs(c).max()) < 0.25 * big for c, w in zip(cs, wide[blk * QK:(blk + 1) * QK]) if w), \
            f"GELU block {blk}: a row near zero could be the block's maximum"
        n_amb += sum(len(c) > 1 for c in cs)
        combos = int(np.prod([len(c) for c in cs]))
        assert combos <= 4096, "too many admissible fp16 combinations in one block"
        ok = False
        for pick in itertools.product(*cs):
            de, qe = q4_quantize_ref(np.array(pick, np.float32))
            if de[0].view(np.uint32) == d[blk].view(np.uint32) and np.array_equal(qe[0], qs[blk]):
                ok = True
                break
        assert ok, f"GELU block {blk}: the device block is the quantization of no admissible input"
    return n_amb / max(1, len(cand))


# ------------------------------------------------------------------ RoPE epilogues
def rope_table(n_pos, n_rot):
    """cs [pos][n_rot/2][2] = {cos, sin}(pos * 10000^(-2j/n_rot)) with the C library's pow, cos and
    sin (math.*), as the model builds its table (rope_table_host)."""
    half = n_rot // 2
    cs = np.empty((n_pos, half, 2), np.float64)
    for j in range(half):
        theta = math.pow(10000.0, 2 * (-float(j)) / n_rot)
        for p in range(n_pos):
            cs[p, j, 0] = math.cos(p * theta)
            cs[p, j, 1] = math.sin(p * theta)
    return cs


def rope_ref(v, pos, cs, d, n_rot, style, tol=None, shift=0):
    """The RoPE epilogue on the row v [H d] at position pos, in double: style 0 rotate-half (head
    dim i pairs with i + n_rot/2), style 1 GPT-J pairs (2j, 2j + 1); dims >= n_rot pass through.
    The kernel rounds each double result once to float: rope_ref(...).astype(float32) of its float
    input.  With tol (the bound on v) also returns the bound on the result: |c| tol_self +
    |s| tol_partner <= tol_self + tol_partner, and one rounding of the result.  shift: the
    partner taken `shift` pairs further (the checkers' mutation)."""
    v = np.asarray(v, np.float64)
    y = v.copy()
    t = None if tol is None else np.asarray(tol, np.float64).copy()
    half = n_rot // 2
    for h0 in range(0, v.size, d):
        for j in range(half):
            a, b = (h0 + j, h0 + j + half) if style == 0 else (h0 + 2 * j, h0 + 2 * j + 1)
            if shift:
                b = h0 + (b - h0 + (1 if style == 0 else 2) * shift) % d
            c, s = cs[pos, j]
            y[a] = v[a] * c - v[b] * s
            y[b] = v[a] * s + v[b] * c
            if t is not None:
                t[a] = t[b] = tol[a] + tol[b]
    if t is None:
        return y
    return y, t + U * np.abs(y)


# ------------------------------------------------------------------ attention
def attn_ref(q, kc, vc, n_past, d, H, nchunk, scale, chunk=64, drop_last_key=False, own_max_chunk=None):
    """Causal single-query attention over the cache rows 0 .. n_past in fp64, as flash-decoding
    partials per (head, 64-position chunk) -- m = max score, l = sum e^(s - m), o = sum e^(s - m) v
    (a chunk past n_past: m = -inf, l = 0) -- and their merge sum_c o_c w_c / sum_c l_c w_c with
    w_c = e^(m_c - M).  Also returns the magnitudes the bounds need.  drop_last_key /
    own_max_chunk: the checkers' mutations (the key at n_past left out; chunk c weighed against
    its own maximum)."""
    E = d * H
    nk = n_past + (0 if drop_last_key else 1)
    q = np.asarray(q, np.float64).reshape(H, d)
    K = np.asarray(kc, np.float64)[:nk].reshape(nk, H, d)
    V = np.asarray(vc, np.float64)[:nk].reshape(nk, H, d)
    sc = float(np.float32(scale))
    s = np.einsum("hd,phd->hp", q, K) * sc
    sabs = np.einsum("hd,phd->hp", np.abs(q), np.abs(K)) * sc
    r = {"s": s, "sabs": sabs, "m": np.full((H, nchunk), -np.inf), "l": np.zeros((H, nchunk)),
         "o": np.zeros((H, nchunk, d)), "oabs": np.zeros((H, nchunk, d)), "p": [None] * nchunk, "nk": nk}
    for c in range(nchunk):
        p0, p1 = c * chunk, min((c + 1) * chunk, nk)
        if p0 >= nk:
            continue
        m = s[:, p0:p1].max(axis=1)
        e = np.exp(s[:, p0:p1] - m[:, None])
        r["m"][:, c], r["l"][:, c], r["p"][c] = m, e.sum(axis=1), e
        r["o"][:, c] = np.einsum("hp,phd->hd", e, V[p0:p1])
        r["oabs"][:, c] = np.einsum("hp,phd->hd", e, np.abs(V[p0:p1]))
    M = r["m"].max(axis=1)
    w = np.exp(r["m"] - M[:, None])
    if own_max_chunk is not None:
        w[:, own_max_chunk] = np.where(np.isfinite(r["m"][:, own_max_chunk]), 1.0, 0.0)
    L = (r["l"] * w).sum(axis=1)
    r["w"], r["L"] = w, L
    r["out"] = (np.einsum("hcd,hc->hd", r["o"], w) / L[:, None]).reshape(E)
    return r


def attn_tols(r, d, eps_p, chunk=64):
    """Bounds for attn_ref's quantities as the kernel computes them (u = 2^-24):
      score      ts = (d + 2) u sum_i |q_i k_i| scale   (d products and sums, the scale)
      max        tm = max ts over the chunk
      e^(s - m)  relative rp = ts + tm + eps_p   (eps_p: the allowance for __expf, the caller's)
      l          sum_j e_j rp_j + (n + 8) u l
      o_i        sum_j e_j rp_j |v_ji| + (n + 8) u sum_j e_j |v_ji|
      merge      weight e^(m_c - M): relative rc = tm_c + tM + eps_p;  L: sum_c (tl_c + l_c rc) w_c +
                 (nch + 8) u L;  out_i: sum_c w_c / L (to_ci + |o_ci| (rc + tL / L + 2u)) +
                 (nch + 8) u sum_c |o_ci| w_c / L
    Returns dict of arrays shaped like r's: m, l, o, out."""
    H, nch = r["m"].shape
    ts = (d + 2) * U * r["sabs"]
    t = {"m": np.zeros((H, nch)), "l": np.zeros((H, nch)), "o": np.zeros((H, nch, d))}
    for c in range(nch):
        e = r["p"][c]
        if e is None:
            continue
        n = e.shape[1]
        tsc = ts[:, c * chunk:c * chunk + n]
        tm = tsc.max(axis=1)
        rp = tsc + tm[:, None] + eps_p
        t["m"][:, c] = tm
        t["l"][:, c] = (e * rp).sum(axis=1) + (n + 8) * U * r["l"][:, c]
        # |v| enters only through sum e |v| (oabs): bound e rp |v| by max rp
        t["o"][:, c] = (rp.max(axis=1)[:, None] + (n + 8) * U) * r["oabs"][:, c]
    tM = t["m"].max(axis=1)
    rc = t["m"] + tM[:, None] + eps_p
    w, L = r["w"], r["L"]
    tL = ((t["l"] + r["l"] * rc) * w).sum(axis=1) + (nch + 8) * U * L
    wl = w / L[:, None]
    rel = rc + (tL / L)[:, None] + 2 * U
    t["out"] = (np.einsum("hcd,hc->hd", t["o"], wl) + np.einsum("hcd,hc->hd", r["oabs"], wl * rel) +
                (nch + 8) * U * np.einsum("hcd,hc->hd", r["oabs"], wl)).reshape(-1)
    return t


def attn_part_check(part, r, t):
    """The device's chunk partials part [H][nchunk][d + 2] against attn_ref / attn_tols: every
    chunk up to n_past within its bounds, every later chunk (m, l) = (-inf, 0).  Returns the worst
    error as a fraction of its bound."""
    H, nch = r["m"].shape
    part = np.asarray(part, np.float64).reshape(H, nch, -1)
    worst = 0.0
    for c in range(nch):
        m, l, o = part[:, c, 0], part[:, c, 1], part[:, c, 2:]
        if r["p"][c] is None:
            assert np.all(np.isneginf(m)) and np.all(l == 0.0), f"chunk {c} past n_past: m {m}, l {l}"
            continue
        for name, got, ref, tol in (("m", m, r["m"][:, c], t["m"][:, c]), ("l", l, r["l"][:, c], t["l"][:, c]),
                                    ("o", o, r["o"][:, c], t["o"][:, c])):
            err = np.abs(got - ref)
            assert np.all(err <= tol), f"chunk {c} {name}: worst error {float((err / (tol + 1e-300)).max()):.3g} x bound"
            worst = max(worst, float((err / (tol + 1e-300)).max()))
    return worst


# ------------------------------------------------------------------ join
def join_ref(x, attn, bo, ffp, bproj):
    """x + ((attn + b_o) + (sum_s ffp[s] + b_proj)) in fp64 (vsim.cpp:694-695)."""
    a = np.asarray(attn, np.float64) + (0.0 if bo is None else np.asarray(bo, np.float64))
    f = np.asarray(ffp, np.float64).sum(axis=0) + np.asarray(bproj, np.float64)
    return np.asarray(x, np.float64) + (a + f)


def bound_ratio(y, y64, tol):
    """The worst |y - y64| as a fraction of its bound (<= 1 passes); NaN counts as infinite."""
    err = np.abs(np.asarray(y, np.float64) - np.asarray(y64, np.float64))
    r = err / (np.asarray(tol, np.float64) + 1e-300)
    return float("inf") if np.isnan(r).any() else float(r.max())
