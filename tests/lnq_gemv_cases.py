"""Inputs and numpy restatements shared by tests/test_gpu_ln_quant.py, tests/test_gpu_gemv_batch.py
and tests/test_ln_quant_gemv_cpu.py (which shows on the CPU that these inputs bite).  No GPU code.

  * the constants of the two launches the lists below are derived from (layer.hip, kern.hpp,
    gemv_chain.hip); the CPU test recomputes the lists from them;
  * the four residual-join forms of ln_exact_lds_t in float32, and other associations of the same
    sums (what a kernel that adds in another order would give);
  * lnq_restate: k_ln_quant's statistics (ln_exact_lds_t<512>) in doubles, in the kernel's own
    orders, for the vsim_norm_fallbacks deltas a call must cause;
  * the fp16 tie rows of the GEMV's GELU epilogue and three float -> half roundings;
  * Q4 helpers: the factors xd of a Q4_0 row in xd_slot order, the SoA image of AoS blocks.
"""
import numpy as np

f32, f64 = np.float32, np.float64
NOCERT = 1 << 30
EPS = f64(f32(1e-5))

# ------------------------------------------------------------------ k_ln_quant
LNQ_NT, LNQ_UP, LNQ_SPLIT = 512, 4, 8  # LNQ_THREADS, ln_exact_lds_t's UP, slice workgroups per norm
LNQ_ONE_PASS = 4 * LNQ_UP * LNQ_NT     # floats the single-pass load takes (n4 <= UP * NT)
# blocks: 1, 4, 7 (empty slices), 8, 9, 33 (uneven, odd slice lengths), 64, 192 (even), then the two
# sides of the single-pass load: n4 == UP * NT takes it, one block more runs the strided loop
LNQ_SIZES = [32, 128, 224, 256, 288, 1056, 2048, 6144, LNQ_ONE_PASS, LNQ_ONE_PASS + 32]
LNQ_MAX_N = 16320                      # the row and the kernel's static words within 64 KB of LDS
JOIN_FORMS = ("full", "a_f", "a_only", "f_only")


def slices(n):
    """[(b0, b1)] the blocks of each of k_ln_quant's LNQ_SPLIT slice workgroups."""
    nb = n // 32
    return [(p * nb // LNQ_SPLIT, (p + 1) * nb // LNQ_SPLIT) for p in range(LNQ_SPLIT)]


def join_operands(n, seed):
    """x, a, ab, f, fb: Gaussian rows of different scales, so that the sums round at every step."""
    rng = np.random.default_rng(seed)
    return tuple((rng.standard_normal(n) * s).astype(f32) for s in (1.0, 0.7, 0.13, 1.3, 0.09))


def _add(p, q):
    with np.errstate(all="ignore"):
        return (f32(p) + f32(q)).astype(f32)


def join(form, x, a, ab, f, fb):
    """The joined row of ln_exact_lds_t in float32 for the operands the form passes."""
    if form == "none":
        return np.ascontiguousarray(x, f32)
    if form == "full":
        return _add(x, _add(_add(a, ab), _add(f, fb)))
    if form == "a_f":
        return _add(x, _add(a, _add(f, fb)))
    if form == "a_only":
        return _add(x, _add(a, ab))
    if form == "f_only":
        return _add(x, _add(f, fb))
    raise ValueError(form)


def join_args(form, a, ab, f, fb):
    """(ja, jab, jf, jfb) the call passes for the form (None: NULL)."""
    return {"none": (None, None, None, None), "full": (a, ab, f, fb), "a_f": (a, None, f, fb),
            "a_only": (a, ab, None, None), "f_only": (None, None, f, fb)}[form]


def join_other_orders(form, x, a, ab, f, fb):
    """The same sum added in other orders: left to right, and the bias last."""
    if form == "full":
        return [_add(_add(_add(_add(x, a), ab), f), fb), _add(_add(x, _add(a, ab)), _add(f, fb)),
                _add(_add(x, _add(a, f)), _add(ab, fb))]
    if form == "a_f":
        return [_add(_add(_add(x, a), f), fb), _add(_add(x, a), _add(f, fb)), _add(x, _add(_add(a, f), fb))]
    if form == "a_only":
        return [_add(_add(x, a), ab), _add(_add(x, ab), a)]
    if form == "f_only":
        return [_add(_add(x, f), fb), _add(_add(x, fb), f)]
    raise ValueError(form)


def ulp_exp(v):
    """kern.hpp ulp_exp: the exponent of the float's last bit; NOCERT for zeros."""
    b = np.ascontiguousarray(v, f32).view(np.uint32) & np.uint32(0x7FFFFFFF)
    e = (b >> np.uint32(23)).astype(np.int64)
    return np.where(b == 0, NOCERT, np.where(e == 0, -149, e - 150))


def tree(a):
    """wave_sum_d: the DPP butterfly, a pairwise tree over adjacent lanes."""
    a = np.asarray(a, f64)
    while a.shape[-1] > 1:
        a = a[..., 0::2] + a[..., 1::2]
    return a[..., 0]


def seq_sum(a):
    """((0 + a0) + a1) + ... in double."""
    return f64(np.add.accumulate(np.asarray(a, f64))[-1])


def _workgroup_sum(vals, valid):
    """ln_exact_lds_t's sum of a per-element double: thread t adds the elements of float4 t, t + NT,
    ... in order from 0.0, wave_sum_d per wave, then the waves' sums in order from 0.0."""
    n = vals.size
    per = 4 * LNQ_NT
    pad = (-n) % per
    a = np.concatenate([np.where(valid, vals, 0.0), np.zeros(pad)]).reshape(-1, LNQ_NT, 4)
    s = np.zeros(LNQ_NT)
    for p in range(a.shape[0]):
        for j in range(4):
            s = s + a[p, :, j]  # (a padding element adds +0.0: no rounding)
    w = tree(s.reshape(LNQ_NT // 64, 64))
    t = f64(0.0)
    for x in w:
        t = t + x
    return t


def lnq_restate(v):
    """(counters, scale) of one k_ln_quant job on the joined row v: counters is what its slice 0 adds
    to vsim_norm_fallbacks ([0] the mean certificate failed, [1] sc_lo != sc_hi), scale the float
    the kernel multiplies with."""
    v = np.ascontiguousarray(v, f32)
    n = v.size
    with np.errstate(all="ignore"):
        vd = v.astype(f64)
        ok = np.ones(n, bool)
        s, sa = _workgroup_sum(vd, ok), _workgroup_sum(np.abs(vd), ok)
        um = int(ulp_exp(v).min())
        exact = um == NOCERT or bool(sa * (1.0 + 2.0 ** -30) < np.ldexp(1.0, 53 + um))
        if not exact:
            s = seq_sum(vd)
        mean = s / n
        d = vd - mean
        s2 = _workgroup_sum(d * d, ok)
        B = (2.0 * n + 64.0) * 2.0 ** -53 * s2
        sc_lo = f32(1.0 / np.sqrt((s2 + B) / n + EPS))
        sc_hi = f32(1.0 / np.sqrt((s2 - B if s2 - B > 0.0 else f64(0.0)) / n + EPS))
        amb = not (sc_lo == sc_hi)  # (NaN scales compare unequal, as in the kernel)
        scale = f32(1.0 / np.sqrt(seq_sum(d * d) / n + EPS)) if amb else sc_lo
    return (0 if exact else 1, 1 if amb else 0), scale


# ------------------------------------------------------------------ Q4 rows
def xd_slot(l):
    return (l & ~3) | ((l & 1) << 1) | ((l >> 1) & 1)


XD_SLOTS = np.array([xd_slot(l) for l in range(32)])


def q4_factors(aos):
    """The factors d * (q - 8) of Q4_0 AoS blocks, float32, each block in xd_slot order (the exact
    GEMV's activation operand, vsim_op_q4_quantize's xd)."""
    blk = np.asarray(aos, np.uint8).reshape(-1, 20)
    d = blk[:, :4].copy().view(f32).reshape(-1)
    q = np.empty((blk.shape[0], 32), f32)
    q[:, 0::2] = (blk[:, 4:] & 0xF).astype(f32) - 8
    q[:, 1::2] = (blk[:, 4:] >> 4).astype(f32) - 8
    with np.errstate(all="ignore"):
        val = (d[:, None] * q).astype(f32)
    out = np.empty_like(val)
    out[:, XD_SLOTS] = val
    return out.reshape(-1)


def q4_soa(aos):
    """Q4 SoA image of AoS blocks: the nibble plane [nb][16], then the scales [nb]."""
    blk = np.asarray(aos, np.uint8).reshape(-1, 20)
    return np.concatenate([blk[:, 4:].reshape(-1), blk[:, :4].reshape(-1)])


def q4_scales(aos):
    return np.asarray(aos, np.uint8).reshape(-1, 20)[:, :4].copy().view(f32).reshape(-1)


def rand_q4_aos(rng, M, K, std=0.02, zero_scale=False):
    """Random Q4_0 rows straight as AoS blocks: uniform nibbles, scales |N(0, 1)| * std / 3, or every
    scale +0 (then every product is a zero and the chain stays +0)."""
    nblk = M * K // 32
    out = np.empty((nblk, 20), np.uint8)
    sc = np.abs(rng.standard_normal(nblk, dtype=f32)) * f32(std / 3)
    if zero_scale:
        sc[:] = 0
    out[:, :4] = sc.view(np.uint8).reshape(-1, 4)
    out[:, 4:] = rng.integers(0, 256, (nblk, 16), dtype=np.uint8)
    return out.reshape(-1)


# ------------------------------------------------------------------ the GEMV batch
SOLO_CB, SOLO_PF, C5_RING, SOLO_MIN_GROUPS = 6, 3, 3, 192
C2_CB, C2_DEPTH = 8, 4  # C2Gemv: 8-block chunks, 4 in flight


def solo_seam_blocks():
    """K in 32-blocks for k_gemv_solo: one block, below one chunk, both sides of one chunk, of the
    prefetch depth (PF chunks), of the ring, of the nit round-up ((nch + 2 + PF) rounded up to a
    multiple of PF + 1 steps up where nch goes 2 -> 3 and 6 -> 7), and a ragged long row."""
    cb = SOLO_CB
    nb = {1, 2, cb - 1, cb, cb + 1}
    for chunks in (2, SOLO_PF, SOLO_PF + 1, 2 * C5_RING):  # nch = chunks | chunks + 1
        nb |= {chunks * cb, chunks * cb + 1}
    nb |= {7 * cb + 1}
    return sorted(nb)


def chain32_seam_blocks():
    """K in 32-blocks for k_gemv_chain32: both sides of 1 .. DEPTH chunks, below one, and a ragged row
    past the chunks in flight."""
    cb = C2_CB
    nb = {1, cb - 1}
    for chunks in range(1, C2_DEPTH + 1):
        nb |= {chunks * cb, chunks * cb + 1}
    nb |= {(C2_DEPTH + 1) * cb + 1}
    return sorted(nb)


SOLO_NB = [1, 2, 5, 6, 7, 12, 13, 18, 19, 24, 25, 36, 37, 43]
CHAIN32_NB = [1, 7, 8, 9, 16, 17, 24, 25, 32, 33, 41]


def solo_groups(Ms):
    """Groups of 64 rows over the jobs of a batch (gemv_chain.hip solo_groups)."""
    return sum(((M + 31) // 32 + 1) // 2 for M in Ms)


def picks_solo(Ms):
    return solo_groups(Ms) >= SOLO_MIN_GROUPS


# ------------------------------------------------------------------ the epilogue's domain
LAST_HALF = 0x7BFF  # 65504


def half_value(i):
    """float64 values of the non-negative finite half patterns i (arrays of ints)."""
    return np.asarray(i, np.uint16).view(np.float16).astype(f64)


def all_half_rows():
    """Sweep (a): every fp16 pattern widened to float32 (NaN patterns stay NaNs of their sign)."""
    with np.errstate(all="ignore"):
        return np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16).astype(f32)


def tie_rows():
    """Sweep (b): (rows float32 [2][3][31744], h uint16 [31744]).  For every finite half h >= 0 the
    float32 midpoint of h and its successor (past the largest half: 65520, the midpoint of 65504 and
    2^16) at index 1 of axis 1, the float32 just below it at 0 and just above it at 2; axis 0 is
    the sign (+, -).  Every midpoint is a float32: it needs one bit more than a half."""
    h = np.arange(LAST_HALF + 1, dtype=np.uint16)
    lo = half_value(h)
    hi = np.concatenate([half_value(h[1:]), [65536.0]])
    mid64 = (lo + hi) / 2
    mid = mid64.astype(f32)
    assert np.array_equal(mid.astype(f64), mid64)
    pos = np.stack([np.nextafter(mid, f32(-np.inf)), mid, np.nextafter(mid, f32(np.inf))])
    return np.stack([pos, -pos]).astype(f32), h


def half_binade(h):
    """0 for subnormal halves, else the biased exponent 1..30."""
    return (np.asarray(h, np.uint16) >> 10) & 0x1F


def f2h_rne(x):
    """float32 -> half bits, round to nearest even, overflow to inf (IEEE; what f2h implements)."""
    with np.errstate(all="ignore"):
        return np.ascontiguousarray(x, f32).astype(np.float16).view(np.uint16)


def _f2h_floor_mag(x):
    """(half bits of |x| truncated toward zero, whether |x| is exactly that half, the sign bits)."""
    x = np.ascontiguousarray(x, f32)
    a = np.abs(x).astype(f64)
    sign = ((x.view(np.uint32) >> 16) & 0x8000).astype(np.uint16)
    t = np.minimum(f2h_rne(np.abs(x)), np.uint16(0x7C00))
    over = half_value(np.minimum(t, np.uint16(LAST_HALF))) > a  # RNE went up: step back
    t = np.where((t == 0x7C00) | over, t - 1, t).astype(np.uint16)
    return t, half_value(t) == a, sign


def f2h_trunc(x):
    """float32 -> half bits, truncation toward zero (finite inputs)."""
    t, _, sign = _f2h_floor_mag(x)
    return (t | sign).astype(np.uint16)


def f2h_half_up(x):
    """float32 -> half bits, round to nearest with ties away from zero (finite inputs)."""
    t, _, sign = _f2h_floor_mag(x)
    a = np.abs(np.ascontiguousarray(x, f32)).astype(f64)
    lo = half_value(t)
    hi = np.where(t == LAST_HALF, 65536.0, half_value(np.minimum(t + 1, LAST_HALF)))
    up = (a - lo) >= (hi - a)
    return (np.where(up, t + 1, t).astype(np.uint16) | sign).astype(np.uint16)
