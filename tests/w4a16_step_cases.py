"""numpy restatements of the weight-only mode's two fused operand kernels (k_w4a16_ln, k_w4a16_gelu,
vsim_amd/csrc/w4a16_decode.hip) and the row families a wrong fusion gets wrong.  No GPU code here:
tests/test_w4a16_step_cpu.py shows on the CPU that every family bites (its named wrong variant
changes a bit of (h, e) on a row of the family), tests/test_gpu_w4a16_step_ops.py runs the rows
through the op entries.

The restatements are compositions of what already exists: the oracle's norm (ggml's sequential double
sums) and its GELU table, float32 adds and multiplies, and w4a16_ref.row_operand.

  ln_operand(x, w, b)      row_operand(w * norm(x) + b)
  gelu_operand(x, bias)    g = table[f2h(x + bias)] (the float32 add first), row_operand(g)
  join(v, res, res_a)      res + (res_a + v), or v + res without res_a

Wrong variants (the `wrong` argument), each what a plausible fusion would compute instead:
  "max_before_affine"   LN: the exponent from the largest |y| of the normalized row, not of w y + b
  "max_over_inputs"     GELU: the exponent from the largest |x + bias|, not from the largest |g|
  "zero_unhandled"      the all-zero row's exponent from the subnormal branch (clz of 0): 164, not 0
  "nonfinite_ignored"   the exponent from the finite elements alone, the others converted as they are
  "log2_rounded"        floor(log2(amax)) taken as the float32 log2 rounded to nearest
  "interval_closed_above"  amax 2^e put into (2^14, 2^15] instead of [2^14, 2^15)
  "field_only"          the exponent field alone: an f32 subnormal maximum counted as 2^-127
  "join_left_first"     (res + res_a) + v
"""
import numpy as np

import oracle_py as O
import w4a16_ref as W

f32, f64 = np.float32, np.float64
QK = 32


# ------------------------------------------------------------------ the operand, with the wrong exponents
def _lg(amax, wrong):
    """floor(log2(amax)) of a finite amax > 0, or what the wrong variant takes for it."""
    _, ex = np.frexp(f64(amax))
    lg = int(ex) - 1
    if wrong == "log2_rounded":
        return int(np.rint(np.log2(f32(amax), dtype=f32))) if amax >= 2.0 ** -126 else lg
    if wrong == "interval_closed_above":
        return lg - 1 if f64(amax) == 2.0 ** lg else lg
    if wrong == "field_only":
        return max(lg, -127)
    return lg


def operand(z, wrong=None, amax_of=None):
    """row_operand of one row z [K] -> (h [K] float16, e int); amax_of: the row the wrong variants
    "max_before_affine" / "max_over_inputs" take the maximum from."""
    z = np.ascontiguousarray(z, f32)
    if wrong is None:
        h, e = W.row_operand(z[None])
        return h[0], int(e[0])
    src = z if amax_of is None else np.ascontiguousarray(amax_of, f32)
    fin = np.isfinite(src)
    if not fin.all() and wrong != "nonfinite_ignored":
        return np.zeros(z.size, np.float16), W.NONFINITE
    amax = float(np.abs(src[fin]).max()) if fin.any() else 0.0
    if amax > 0.0:
        e = 14 - _lg(amax, wrong)
    else:
        e = 164 if wrong == "zero_unhandled" else 0
    with np.errstate(all="ignore"):
        h = np.ldexp(z.astype(f64), e).astype(np.float16)
    return h, e


# ------------------------------------------------------------------ the two fused kernels
def affine(w, y, b):
    """w * y + b with two float32 roundings (the norm kernel's)."""
    with np.errstate(all="ignore"):
        return ((f32(w) * f32(y)).astype(f32) + f32(b)).astype(f32)


def ln_operand(x, w, b, wrong=None):
    x = np.ascontiguousarray(x, f32)
    y = O.norm(x, x.size, 1)
    z = affine(w, y, b)
    return operand(z, wrong, amax_of=y if wrong == "max_before_affine" else None)


def gelu_rows(x, bias):
    """(x + bias in float32, g) of one row."""
    with np.errstate(all="ignore"):
        s = (np.ascontiguousarray(x, f32) + np.ascontiguousarray(bias, f32)).astype(f32)
    return s, O.gelu(s)


def gelu_operand(x, bias, wrong=None):
    s, g = gelu_rows(x, bias)
    return operand(g, wrong, amax_of=s if wrong == "max_over_inputs" else None)


def join(v, res, res_a=None, wrong=None):
    v, res = np.ascontiguousarray(v, f32), np.ascontiguousarray(res, f32)
    with np.errstate(all="ignore"):
        if res_a is None:
            return (v + res).astype(f32)
        res_a = np.ascontiguousarray(res_a, f32)
        if wrong == "join_left_first":
            return ((res + res_a).astype(f32) + v).astype(f32)
        return (res + (res_a + v).astype(f32)).astype(f32)


def same(a, b):
    """(h, e) pairs equal bit for bit."""
    return a[1] == b[1] and np.array_equal(np.asarray(a[0]).view(np.uint16), np.asarray(b[0]).view(np.uint16))


# ------------------------------------------------------------------ the families
def ln_family(n, seed=0):
    """[(x, w, b)]: rows whose largest |w y + b| sits at another index than the largest |y|."""
    rng = np.random.default_rng(4100 + n + seed)
    out = []
    for k in range(4):
        x = rng.standard_normal(n).astype(f32)
        x[(5 * k + 3) % n] = 6.0                       # the largest |y| ...
        w = (1.0 + 0.1 * rng.standard_normal(n)).astype(f32)
        b = (0.1 * rng.standard_normal(n)).astype(f32)
        j = (11 * k + 7) % n
        if k % 2:
            w[j] = [64.0, -300.0][k // 2]              # ... and the largest output elsewhere: a large gain
        else:
            b[j] = [-900.0, 40.0][k // 2]              # or a large shift
        w[(5 * k + 3) % n] = 2.0 ** -6
        out.append((x, w, b))
    return out


def gelu_negative_max(K, seed=0):
    """[(x, bias)]: the largest |x + bias| is a large negative, where g is +-0."""
    rng = np.random.default_rng(4200 + K + seed)
    out = []
    for k in range(3):
        x = (rng.standard_normal(K) * 0.5).astype(f32)
        bias = (rng.standard_normal(K) * 0.25).astype(f32)
        x[(3 * k + 1) % K] = [-40.0, -3000.0, -60000.0][k]
        out.append((x, bias))
    return out


def gelu_all_zero(K, seed=0):
    """[(x, bias)]: every g is +-0 (x + bias = +-0, or far enough below zero)."""
    rng = np.random.default_rng(4300 + K + seed)
    a = rng.uniform(1.0, 2.0, K).astype(f32)
    return [(a, -a), (np.zeros(K, f32), np.full(K, -0.0, f32)), (-(a * f32(30.0)), np.full(K, -20.0, f32))]


def gelu_beyond_f16(K, seed=0):
    """[(x, bias)]: one x + bias beyond fp16's range (f2h gives inf, and the table what GELU makes of it)."""
    rng = np.random.default_rng(4400 + K + seed)
    out = []
    for k, big in enumerate([7.0e4, 3.0e38, -7.0e4]):
        x = (rng.standard_normal(K) * 0.5).astype(f32)
        bias = (rng.standard_normal(K) * 0.25).astype(f32)
        x[(7 * k + 2) % K] = big
        out.append((x, bias))
    return out


def _gelu_fixed_points():
    """Table inputs s >= 4 whose output g == s (GELU is the identity in fp16 from there on), as floats."""
    _, gt = O.tables()
    i = np.arange(0x4400, 0x7C00, dtype=np.uint16)
    keep = gt[i] == i
    return i[keep].view(np.float16).astype(f32)


def power_of_two_rows(K, seed=0):
    """[(x, bias, kind)] for the GELU kernel whose largest g is exactly 2^k ("exact") or the fp16 one
    ulp below it ("below"): inputs in the range where the table is the identity."""
    rng = np.random.default_rng(4500 + K + seed)
    fix = set(_gelu_fixed_points().tolist())
    out = []
    for k in (3, 7, 12):
        for kind, top in (("exact", 2.0 ** k), ("below", float(np.nextafter(np.float16(2.0 ** k), np.float16(0))))):
            assert top in fix, top
            x = (rng.standard_normal(K) * 0.5).astype(f32)
            x[(k + 5) % K] = top
            out.append((x, np.zeros(K, f32), kind))
    return out


def power_of_two_ln_rows(n):
    """[(x, w, b, kind)] for the LN kernel: zero gain, so the output row is the shift b, whose largest
    element is exactly 2^k or one f32 ulp below it."""
    rng = np.random.default_rng(4600 + n)
    out = []
    for k in (-20, 0, 9):
        for kind, top in (("exact", f32(2.0 ** k)), ("below", np.nextafter(f32(2.0 ** k), f32(0)))):
            b = (rng.uniform(-0.5, 0.5, n) * 2.0 ** k).astype(f32)
            b[(k + 40) % n] = -top
            out.append((rng.standard_normal(n).astype(f32), np.zeros(n, f32), b, kind))
    return out


def subnormal_ln_rows(n):
    """[(x, w, b)]: zero gain and an f32-subnormal shift, so the output's maximum is an f32 subnormal."""
    rng = np.random.default_rng(4700 + n)
    out = []
    for top in (2.0 ** -128, 3.0 * 2.0 ** -140, 2.0 ** -149):
        b = (rng.integers(-3, 4, n) * 2.0 ** -149).astype(f32)
        b[n // 2] = f32(top)
        out.append((rng.standard_normal(n).astype(f32), np.zeros(n, f32), b))
    return out


def join_rows(M, seed=0):
    """(v, res, res_a) [M] each with res + (res_a + v) != (res + res_a) + v at most elements."""
    rng = np.random.default_rng(4800 + M + seed)
    res = rng.standard_normal(M).astype(f32)
    res_a = (rng.standard_normal(M) * 1e-3).astype(f32)
    v = (rng.standard_normal(M) * 1e-3).astype(f32)
    return v, res, res_a
