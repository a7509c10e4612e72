"""Adversarial joined rows for the layer tail's LayerNorm (gemv_chain.hip lnt_owner), and a numpy
restatement of its arithmetic.  No GPU code here; tests/test_tail_ln_cpu.py shows on the CPU that
the rows bite, tests/test_gpu_tail_ln.py runs them through vsim_op_tail_ln.

restate(v) follows lnt_owner in doubles, in the kernel's own orders:
  * per 32-row tile the half-wave sums of v, |v| and v^2 (a butterfly: the pairwise tree over
    adjacent lanes), the tile's smallest ulp exponent, sum |v| rounded up to a float;
  * the partial poll: lane l adds granules l, l + 64, ... in turn (even granules {sum, umin}, odd
    ones {sum v^2, sum |v|}), then the wave reduction (again the pairwise tree over 64 lanes);
  * the mean certificate A (1 + 2^-30) < 2^(53 + U);
  * the moments scale s2 = (Q - 2 m S) + n m^2 and its interval B = ((2n + 64) s2 + 64 M) 2^-53
    (1 + 2^-20), accepted when r - dr and r + dr round to one float;
  * the fallback: the sequential mean sum when the mean was not certified, the tree s2 (lane l
    adds elements l, l + 64, ... in turn, then the wave tree), sc_lo / sc_hi, and lane 0's
    sequential s2 when they differ.
Each certificate can be switched off (accept_moments, always_sc_lo, any_order_mean): the rows below
are kept only where that changes the bits the kernel hands on.

The rows are the joined row v itself: the GPU test steers them in exactly with zero-scale
out-projection and fc_out weights and zero biases (v = x + ((0 + 0) + (0 + 0)) = x).  Every row
comes with the affine of norm 1 that the test applies: ones and zeros, except that the elements a
mean error moves (the tiny ones, whose y is about -mean * scale) get a power-of-two weight that
lifts them to the top of their Q4_0 block, where the block scale d = amax / 7 shows their bits.

Families (rows(E) -> {family: [Row]}, at least MIN_ROWS each, seeded, cached):
  certified          both certificates pass: the fast path, no counter moves
  mean_uncertified   the families of test_norm_sequential_mean_sum_cases on a base of cancelling
                     pairs (so the mean is small and its rounding shows): tiny elements, more than
                     32 roundings in one 256-chunk, 1e30 / 1e-30 in a chunk, denormals and zeros, a
                     growing running sum, cancellation pairs; kept where the any-order (tree) sum
                     gives other Q4 bytes than the sequential one
  moments_wrong      mean 1e3, spread 1e-2: the float scale from the moments differs from the
                     sequential one, so the interval check has to reject it
  scale_ambiguous    a directed search (one element of a Gaussian row swept over the floats of a
                     binade, candidates located in float64, confirmed with restate) for rows whose
                     exact scale lies within the fallback's interval of a float midpoint
                     (sc_lo != sc_hi); some whose sequential scale is sc_lo and some sc_hi
The search finds scale-ambiguous rows at all six sizes; none is skipped.
"""
import functools
import math
from dataclasses import dataclass, field

import numpy as np

from vsim_amd import modelgen as mg

SIZES = [(32, 32, 1), (64, 64, 1), (1024, 256, 4), (1056, 96, 11), (2048, 128, 16), (6144, 256, 24)]  # (E, d, H)
MIN_ROWS = 4
FAMILIES = ("certified", "mean_uncertified", "moments_wrong", "scale_ambiguous")
EPS = np.float64(np.float32(1e-5))
NOCERT = 1 << 30
f32, f64 = np.float32, np.float64


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def ulp_exp(v):
    """kern.hpp ulp_exp: the exponent of the float's last bit; NOCERT for zeros."""
    b = bits(v) & np.uint32(0x7FFFFFFF)
    e = (b >> np.uint32(23)).astype(np.int64)
    return np.where(b == 0, NOCERT, np.where(e == 0, -149, e - 150))


def tree(a):
    """The DPP butterflies (half_sum_d, wave_sum_d): the pairwise tree over adjacent lanes."""
    a = np.asarray(a, f64)
    while a.shape[-1] > 1:
        a = a[..., 0::2] + a[..., 1::2]
    return a[..., 0]


def seq_sum(a):
    """((0 + a0) + a1) + ... in double."""
    return f64(np.add.accumulate(np.asarray(a, f64))[-1])


def lane_strided(a):
    """Lane l adds a[l], a[l + 64], ... in turn from 0.0: the 64 lane sums."""
    a = np.asarray(a, f64)
    pad = (-a.size) % 64
    a = np.concatenate([a, np.zeros(pad)]).reshape(-1, 64)
    s = np.zeros(64)
    for r in a:
        s = s + r
    return s


def rscale(s2, n):
    return f64(1.0) / np.sqrt(s2 / n + EPS)


@dataclass
class Stats:
    y: np.ndarray            # the normalized row before the affine, float32
    mean: float
    scale: np.float32
    counters: tuple          # what the launch adds to vsim_norm_fallbacks
    mean_ok: bool
    moments_ok: bool         # the moments scale was accepted
    sc_moments: object = None  # float of the moments scale (mean_ok only)
    sc_lo: object = None
    sc_hi: object = None


def restate(v, accept_moments=False, always_sc_lo=False, any_order_mean=False):
    """lnt_owner's statistics of the joined row v (float32 [n], n % 32 == 0): Stats."""
    v = np.ascontiguousarray(v, f32)
    n = v.size
    assert n % 32 == 0
    with np.errstate(all="ignore"):
        vd = v.astype(f64).reshape(-1, 32)
        s_t, sa_t, q_t = tree(vd), tree(np.abs(vd)), tree(vd * vd)
        um_t = ulp_exp(v).reshape(-1, 32).min(axis=1)
        au = sa_t.astype(f32)
        up = au.astype(f64) < sa_t
        au = np.where(up, (bits(au) + np.uint32(1)).view(f32), au)
        # granule g = 2 t (+ 1) lands in lane g % 64, in the order of k = g / 64
        def granules(vals, odd):
            g = np.zeros(2 * vals.size)
            g[odd::2] = vals
            return g

        S = tree(lane_strided(granules(s_t, 0)))
        Q = tree(lane_strided(granules(q_t, 1)))
        A = tree(lane_strided(granules(au.astype(f64), 1)))
        U = int(um_t.min())
        mean_ok = bool(any_order_mean or U == NOCERT or A * (1.0 + 2.0 ** -30) < np.ldexp(1.0, 53 + U))
        fallback = not mean_ok
        mean, scale, sc_m, moments_ok = f64(0.0), f32(0.0), None, False
        if mean_ok:
            mean = S / n
            t1, t3 = mean * S, (mean * mean) * n
            s2 = (Q - 2.0 * t1) + t3
            M = Q + 2.0 * np.abs(t1) + t3
            s2c = s2 if s2 > 0.0 else f64(0.0)
            B = ((2.0 * n + 64.0) * s2c + 64.0 * M) * 2.0 ** -53 * (1.0 + 2.0 ** -20)
            r = rscale(s2, n)
            dr = r * (B / ((s2c - B if s2c - B > 0.0 else 0.0) + n * EPS) + 2.0 ** -48)
            sc_m = f32(r)
            if accept_moments or (f32(r - dr) == sc_m and f32(r + dr) == sc_m):
                scale, moments_ok = sc_m, True
            else:
                fallback = True
        c0 = c1 = 0
        sc_lo = sc_hi = None
        if fallback:
            m = S if mean_ok else seq_sum(v)
            mean = m / n
            d = v.astype(f64) - mean
            s2 = tree(lane_strided(d * d))
            B = (2.0 * n + 64.0) * 2.0 ** -53 * s2
            sc_lo = f32(rscale(s2 + B, n))
            sc_hi = f32(rscale(s2 - B if s2 - B > 0.0 else f64(0.0), n))
            scale = sc_lo
            if sc_lo != sc_hi and not always_sc_lo:
                scale = f32(rscale(seq_sum(d * d), n))
                c1 = 1
            if not mean_ok:
                c0 = 1
        y = (v.astype(f64) - mean).astype(f32) * f32(scale)
    return Stats(y.astype(f32), float(mean), f32(scale), (c0, c1), mean_ok, moments_ok, sc_m, sc_lo, sc_hi)


def seq_norm(v):
    """ggml_compute_forward_norm_f32 in numpy: sequential double sums (what the oracle's vo_norm_f32 runs)."""
    v = np.ascontiguousarray(v, f32)
    n = v.size
    with np.errstate(all="ignore"):
        mean = seq_sum(v) / n
        d = v.astype(f64) - mean
        scale = f32(rscale(seq_sum(d * d), n))
        return (d.astype(f32) * scale).astype(f32), scale


def affine(w, y, b):
    """w * y + b with two float32 roundings."""
    with np.errstate(all="ignore"):
        return ((f32(w) * f32(y)).astype(f32) + f32(b)).astype(f32)


def q4_bytes(z):
    """quantize_row_q4_0's AoS bytes (the MAX macro's NaN rule) in numpy."""
    return mg.quantize_q4_0_w(z, nan_as_max=True)[0]


@dataclass
class Row:
    family: str
    v: np.ndarray
    w1: np.ndarray
    b1: np.ndarray
    counters: tuple          # restate's prediction of the fallback-counter deltas
    seq_is: str = ""         # scale_ambiguous: which end of the interval the sequential scale equals
    note: str = ""
    stats: Stats = field(default=None, repr=False)

    def out(self, **sw):
        """The Q4 bytes of norm 1 under restate(**sw)."""
        return q4_bytes(affine(self.w1, restate(self.v, **sw).y, self.b1))


def _plain(family, v, st, **kw):
    return Row(family, v, np.ones(v.size, f32), np.zeros(v.size, f32), st.counters, stats=st, **kw)


# ------------------------------------------------------------------ certified
def _certified(n):
    rng = np.random.default_rng(1000 + n)
    out = []
    for k in range(64):
        v = (rng.standard_normal(n) * [0.05, 1.0, 40.0][k % 3] + [0.0, 0.3][k % 2]).astype(f32)
        st = restate(v)
        if st.mean_ok and st.moments_ok:
            out.append(_plain("certified", v, st))
        if len(out) == MIN_ROWS + 2:
            break
    return out


# ------------------------------------------------------------------ mean-uncertified
MEAN_CANDIDATES = 64


def _mean_candidate(n, k, rng):
    r = (rng.standard_normal(n) * rng.choice([0.05, 1.0, 40.0])).astype(f32)
    kind = k % 8
    if kind != 5:
        r[1::2] = -r[0::2]  # cancelling pairs: the mean is what the tiny elements leave
    npair = n // 2

    def pairs(m):
        return rng.choice(npair, min(m, npair - 2), replace=False)

    def put(p, vals):  # both elements of pair p
        r[2 * p], r[2 * p + 1] = vals

    if kind == 0:  # one tiny pair
        put(pairs(1)[0], np.float32(3e-7) * rng.standard_normal(2).astype(f32))
    elif kind == 1:  # a few tinier ones
        for p in pairs(5):
            put(p, (rng.standard_normal(2) * 1e-9).astype(f32))
    elif kind == 2:  # more roundings in one 256-chunk than the restart cap
        c = int(rng.integers(0, max(n // 256, 1))) * 128
        for p in c + rng.choice(min(128, npair), min(100, npair - 2), replace=False):
            put(p, (rng.standard_normal(2) * 1e-12).astype(f32))
    elif kind == 3:  # a huge dynamic range inside a chunk
        ps = pairs(4)
        put(ps[0], (np.float32(1e30), np.float32(-1e30)))
        for p in ps[1:]:
            put(p, (np.float32(1e-30), np.float32(1e-30)))
    elif kind == 4:  # denormals and zeros
        ps = pairs(12)
        for p in ps[:4]:
            put(p, (np.float32(1e-41), np.float32(3e-41)))
        for p in ps[4:]:
            put(p, (np.float32(0.0), np.float32(0.0)))
        put(ps[-1], (rng.standard_normal(2) * 1e-11).astype(f32))
    elif kind == 5:  # a growing running sum
        r = (np.abs(r) * 1000 + 1e-4 * rng.standard_normal(n)).astype(f32)
    elif kind == 6:  # exact cancellation and one tiny element
        r[int(rng.integers(0, n))] = np.float32(1e-8)
    else:  # scaled-down pairs
        for p in pairs(20):
            put(p, (r[2 * p:2 * p + 2] * np.float32(1e-7) * rng.standard_normal(2).astype(f32)).astype(f32))
    return r, kind


def _boost(y_ref, y_alt):
    """Norm 1's weights: 1, and a power of two that lifts every element the two statistics disagree
    on to [2, 4) times the row's largest |y|."""
    w = np.ones(y_ref.size, f32)
    fin = np.isfinite(y_ref)
    if not fin.any():
        return w
    amax = float(np.abs(y_ref[fin]).max())
    for i in np.nonzero(bits(y_ref) != bits(y_alt))[0]:
        a = abs(float(y_ref[i])) or abs(float(y_alt[i]))
        if not (amax > 0 and a > 0 and math.isfinite(a)):
            continue
        p = math.ceil(math.log2(2 * amax / a))
        if 2.0 ** p * a >= 4 * amax:
            p -= 1
        w[i] = f32(2.0 ** max(min(p, 100), -100))
    return w


def _mean_uncertified(n):
    """(the rows that bite, one more row per candidate kind whether it bites or not: the latter only
    walk seq_sum_exact_inl's paths -- the restart cap, a failed chunk certificate, lane 0's loop)"""
    rng = np.random.default_rng(2000 + n)
    out, kinds, paths = [], set(), {}
    for k in range(MEAN_CANDIDATES):
        v, kind = _mean_candidate(n, k, rng)
        st = restate(v)
        if st.mean_ok or st.counters[0] != 1:
            continue
        alt = restate(v, any_order_mean=True)
        w = _boost(st.y, alt.y)
        row = Row("mean_uncertified", v, w, np.zeros(n, f32), st.counters, note=f"kind {kind}", stats=st)
        if kind not in paths:
            paths[kind] = Row("mean_paths", v, w, np.zeros(n, f32), st.counters, note=f"kind {kind}", stats=st)
        if st.counters != (1, 0) or np.array_equal(q4_bytes(affine(w, st.y, 0)), q4_bytes(affine(w, alt.y, 0))):
            continue
        if kind in kinds and len(out) >= MIN_ROWS:
            continue
        kinds.add(kind)
        out.append(row)
    return out, [paths[k] for k in sorted(paths)]


# ------------------------------------------------------------------ moments-wrong
def _moments_wrong(n):
    rng = np.random.default_rng(3000 + n)
    out = []
    for _ in range(64):
        v = (1000.0 + 0.01 * rng.standard_normal(n)).astype(f32)
        st = restate(v)
        if st.mean_ok and not st.moments_ok and bits(st.sc_moments) != bits(seq_norm(v)[1]):
            dv = (v.astype(f64) - st.mean).astype(f32)
            if np.array_equal(q4_bytes(dv * st.sc_moments), q4_bytes(st.y)):
                continue  # (the two scales give one Q4 row: not a row that shows)
            out.append(_plain("moments_wrong", v, st))
        if len(out) == MIN_ROWS + 2:
            break
    return out


# ------------------------------------------------------------------ scale-ambiguous
SWEEP_CHUNK = 1 << 21


def _scale_ambiguous(n, want=3, max_binades=16):
    """Rows with sc_lo != sc_hi: element j of a Gaussian row swept over the floats of the binades
    [2^-k, 2^(1-k)), k = 1, 2, ...  s2 as a function of the swept x from the other elements' exact
    sums, r = 1/sqrt(s2/n + eps) in float64, candidates where r lies within three half-widths of the
    fallback's interval of a float midpoint, confirmed by restate.  Stops once `want` rows of either
    kind (sequential scale = sc_lo, = sc_hi) are found."""
    rng = np.random.default_rng(4000 + n)
    base = rng.standard_normal(n).astype(f32)
    j = n // 2 + 1
    rest = np.delete(base.astype(f64), j)
    S_r, Q_r = math.fsum(rest.tolist()), math.fsum((rest * rest).tolist())
    hw = 3.0 * 0.5 * (2.0 * n + 64.0) * 2.0 ** -53 * 2.0 ** 24 + 2.0 ** -26  # in float ulps of r
    found = {"lo": [], "hi": []}
    for k in range(1, max_binades + 1):
        for c0 in range(0, 1 << 23, SWEEP_CHUNK):
            m = np.arange((1 << 23) + c0, (1 << 23) + c0 + SWEEP_CHUNK, dtype=np.int64)
            x = np.ldexp(m.astype(f64), -k - 23)
            s2 = (Q_r + x * x) - (S_r + x) * (S_r + x) / n
            mant, _ = np.frexp(1.0 / np.sqrt(s2 / n + EPS))
            fr = mant * 2.0 ** 24
            dist = np.abs(fr - np.floor(fr) - 0.5)
            for i in np.nonzero(dist < hw)[0]:
                v = base.copy()
                v[j] = f32(x[i])
                st = restate(v)
                if not (st.mean_ok and st.counters == (0, 1)):
                    continue
                dv = (v.astype(f64) - st.mean).astype(f32)
                if np.array_equal(q4_bytes(dv * st.sc_lo), q4_bytes(dv * st.sc_hi)):
                    continue  # (one ulp of the scale can vanish in the products' rounding: not a row that shows)
                sq = seq_norm(v)[1]
                kind = "lo" if bits(sq) == bits(st.sc_lo) else "hi"
                assert bits(sq) == bits(st.sc_lo if kind == "lo" else st.sc_hi)
                if len(found[kind]) < want:
                    found[kind].append(_plain("scale_ambiguous", v, st, seq_is=kind, note=f"x = {float(x[i])!r}"))
            if len(found["lo"]) >= want and len(found["hi"]) >= want:
                return found["lo"] + found["hi"]
    return found["lo"] + found["hi"]


@functools.lru_cache(maxsize=None)
def rows(E):
    """{family: [Row]} for the joined-row width E: FAMILIES, and "mean_paths" (see _mean_uncertified)."""
    bite, paths = _mean_uncertified(E)
    return {"certified": _certified(E), "mean_uncertified": bite, "moments_wrong": _moments_wrong(E),
            "scale_ambiguous": _scale_ambiguous(E), "mean_paths": paths}


def nonfinite_rows(E):
    """[(name, v)]: a Gaussian row with one +inf, and one with a NaN."""
    rng = np.random.default_rng(6000 + E)
    a, b = rng.standard_normal(E).astype(f32), rng.standard_normal(E).astype(f32)
    a[E // 3] = np.inf
    b[(2 * E) // 3 + 1] = np.nan
    return [("inf", a), ("nan", b)]
