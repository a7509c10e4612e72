"""The kernels of the weight-only mode's single-token step through their op entries (vsim_op_w4a16_ln,
vsim_op_w4a16_gelu, vsim_op_w4a16_gemv), each bit for bit against the composition of entries that
already exist -- vsim_op_norm / vsim_op_gelu / vsim_op_w4a16_rows / vsim_op_q4_gemm_w4a16_rows and
float32 adds in torch -- on the row families of tests/w4a16_step_cases.py (shown to bite on the CPU
by tests/test_w4a16_step_cpu.py) and at every shape where a kernel takes another path.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import fast_ref as R  # noqa: E402
import tail_ln_edges as T  # noqa: E402
import w4a16_ref as W  # noqa: E402
import w4a16_step_cases as C  # noqa: E402
from vsim_amd import hip  # noqa: E402
from vsim_amd import modelgen as mg  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
EINVAL = -1
GUARD = 64  # canary elements behind every output


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def hbits(a):
    return np.ascontiguousarray(a, np.float16).view(np.uint16)


def out_operand(K):
    """An operand to be written: K halves and one exponent, each followed by canaries."""
    return (torch.full((K + GUARD,), 7.0, dtype=torch.float16, device=DEV),
            torch.full((1 + GUARD,), 12345, dtype=torch.int32, device=DEV))


def read_operand(x16, e, K):
    hh, eh = host(x16), host(e)
    assert (hh[K:] == 7.0).all() and (eh[1:] == 12345).all(), "written behind the operand"
    return hh[:K], int(eh[0])


def rows_operand(z, K):
    """vsim_op_w4a16_rows of the device row z."""
    x16, e = out_operand(K)
    hip.w4a16_rows(z, K, 1, x16, e)
    return read_operand(x16, e, K)


def norm_then_rows(x, w, b, n):
    y = torch.full((n,), float("nan"), dtype=torch.float32, device=DEV)
    hip.check(hip.lib().vsim_op_norm(x.data_ptr(), y.data_ptr(), n, 1, w.data_ptr(), b.data_ptr(), None), "norm")
    return rows_operand(y, n)


def fused_ln(x, n, w1, b1, w2=None, b2=None):
    o1, o2 = out_operand(n), out_operand(n)
    two = w2 is not None
    hip.w4a16_ln(x, n, w1, b1, o1[0], o1[1], w2, b2, o2[0] if two else None, o2[1] if two else None)
    r1, r2 = read_operand(*o1, n), read_operand(*o2, n) if two else None
    if not two:
        assert (host(o2[0]) == 7.0).all() and (host(o2[1]) == 12345).all()
    return r1, r2


def same_operand(got, want, what):
    assert got[1] == want[1], (what, got[1], want[1])
    assert np.array_equal(hbits(got[0]), hbits(want[0])), (what, np.argwhere(hbits(got[0]) != hbits(want[0]))[:4])


# ------------------------------------------------------------------ vsim_op_w4a16_ln
def ln_rows(n):
    """[(name, x, w, b)]: random rows, the CPU file's LN families, a NaN row."""
    rng = np.random.default_rng(50 + n)
    out = [("random", (rng.standard_normal(n) * s + m).astype(np.float32), (1 + 0.1 * rng.standard_normal(n)).astype(np.float32),
            (0.1 * rng.standard_normal(n)).astype(np.float32)) for s, m in ((1.0, 0.0), (30.0, 4.0))]
    out += [("max elsewhere", *r) for r in C.ln_family(n)]
    out += [("2^k " + r[3], *r[:3]) for r in C.power_of_two_ln_rows(n)]
    out += [("subnormal", *r) for r in C.subnormal_ln_rows(n)]
    x = rng.standard_normal(n).astype(np.float32)
    x[n // 3] = np.nan
    out.append(("nan", x, out[0][2], out[0][3]))
    return out


@pytest.mark.parametrize("n", [32, 128, 160, 4096, 16320])
def test_ln_equals_norm_then_rows(n):
    rows = ln_rows(n)
    rng = np.random.default_rng(n)
    w2, b2 = dev((1 + 0.2 * rng.standard_normal(n)).astype(np.float32)), dev(rng.standard_normal(n).astype(np.float32))
    for name, x, w, b in rows:
        xd, wd, bd = dev(x), dev(w), dev(b)
        want1 = norm_then_rows(xd, wd, bd, n)
        got1, _ = fused_ln(xd, n, wd, bd)
        same_operand(got1, want1, (n, name, "one norm"))
        if n <= 160 and not name.startswith("nan"):   # ... and the numpy restatement, where it is cheap
            same_operand(got1, C.ln_operand(x, w, b), (n, name, "restatement"))
        if name == "nan":
            assert got1[1] == W.NONFINITE and not hbits(got1[0]).any()
        got1, got2 = fused_ln(xd, n, wd, bd, w2, b2)
        same_operand(got1, want1, (n, name, "norm 1 of two"))
        same_operand(got2, norm_then_rows(xd, w2, b2, n), (n, name, "norm 2 of two"))


@pytest.mark.parametrize("E", [32, 1056, 6144])
def test_ln_fallback_rows_and_counters(E):
    """The mean-uncertified and scale-ambiguous rows of tests/tail_ln_edges.py: the operand's bits, and
    vsim_norm_fallbacks moving as vsim_op_norm moves it on the same rows (each norm on its own)."""
    fam = T.rows(E)
    rows = fam["mean_uncertified"][:T.MIN_ROWS] + fam["scale_ambiguous"][:T.MIN_ROWS] + fam["certified"][:1]
    moved = [0, 0]
    for r in rows:
        xd, wd, bd = dev(r.v), dev(r.w1), dev(r.b1)
        c0 = hip.norm_fallbacks()
        want = norm_then_rows(xd, wd, bd, E)
        c1 = hip.norm_fallbacks()
        got, _ = fused_ln(xd, E, wd, bd)
        c2 = hip.norm_fallbacks()
        d_ref, d_got = (c1[0] - c0[0], c1[1] - c0[1]), (c2[0] - c1[0], c2[1] - c1[1])
        assert d_got == d_ref, (r.family, r.note, d_ref, d_got)
        same_operand(got, want, (E, r.family, r.note))
        fused_ln(xd, E, wd, bd, wd, bd)
        c3 = hip.norm_fallbacks()
        assert (c3[0] - c2[0], c3[1] - c2[1]) == (2 * d_ref[0], 2 * d_ref[1]), (r.family, "two norms count twice")
        moved = [moved[0] + d_ref[0], moved[1] + d_ref[1]]
    print(f"w4a16_ln E={E}: fallbacks over {len(rows)} rows: mean {moved[0]}, variance {moved[1]}")
    assert moved[0] > 0   # the mean-uncertified rows take vsim_op_norm's sequential sum, so the check is not idle


# ------------------------------------------------------------------ vsim_op_w4a16_gelu
def gelu_rows(K):
    rng = np.random.default_rng(60 + K)
    out = [("random", (rng.standard_normal(K) * 2).astype(np.float32), rng.standard_normal(K).astype(np.float32))]
    out += [("negative max", *r) for r in C.gelu_negative_max(K)]
    out += [("all zero", *r) for r in C.gelu_all_zero(K)]
    out += [("beyond fp16", *r) for r in C.gelu_beyond_f16(K)]
    out += [("2^k " + r[2], r[0], r[1]) for r in C.power_of_two_rows(K)]
    return out


# (24,576 is the last row that stays in registers; 24,608 makes g twice)
@pytest.mark.parametrize("K", [32, 512, 16384, 16416, 24576, 24608])
def test_gelu_equals_add_gelu_rows(K):
    for name, x, bias in gelu_rows(K):
        xd, bd = dev(x), dev(bias)
        s = xd + bd                                   # the float32 add
        g = torch.empty_like(s)
        hip.check(hip.lib().vsim_op_gelu(s.data_ptr(), g.data_ptr(), K, None), "gelu")
        want = rows_operand(g, K)
        x16, e = out_operand(K)
        gout = torch.full((K + GUARD,), float("nan"), dtype=torch.float32, device=DEV)
        hip.w4a16_gelu(xd, bd, K, x16, e, gout)
        got = read_operand(x16, e, K)
        same_operand(got, want, (K, name))
        gh = host(gout)
        assert np.isnan(gh[K:]).all() and np.array_equal(bits(gh[:K]), bits(host(g))), (K, name, "g")
        x16b, eb = out_operand(K)
        hip.w4a16_gelu(xd, bd, K, x16b, eb, None)     # without the f32 output
        same_operand(read_operand(x16b, eb, K), want, (K, name, "no g"))
        if K <= 512:
            same_operand(got, C.gelu_operand(x, bias), (K, name, "restatement"))
        if name == "all zero":
            assert got[1] == 0 and not (hbits(got[0]) & 0x7FFF).any()
        if name == "beyond fp16":
            assert got[1] == W.NONFINITE
    # no bias: no add (x = -0.0 stays -0.0 on its way into the table)
    x = np.full(K, -0.0, np.float32)
    x[K // 2] = 3.0
    xd = dev(x)
    g = torch.empty_like(xd)
    hip.check(hip.lib().vsim_op_gelu(xd.data_ptr(), g.data_ptr(), K, None), "gelu")
    x16, e = out_operand(K)
    hip.w4a16_gelu(xd, None, K, x16, e, None)
    same_operand(read_operand(x16, e, K), rows_operand(g, K), (K, "no bias"))


# ------------------------------------------------------------------ vsim_op_w4a16_gemv
def repack(aos_np, rows, k, slack=0):
    src = dev(aos_np)
    dst = torch.full((hip.q4_bytes(rows, k) + slack,), 0xFF, dtype=torch.uint8, device=DEV)
    hip.check(hip.lib().vsim_op_q4_repack(src.data_ptr(), dst.data_ptr(), rows, k, None), "repack")
    return dst


def weights(M, K, seed):
    rng = np.random.default_rng(seed)
    return mg.quantize_q4_0(rng.standard_normal(M * K).astype(np.float32) * np.float32(0.02)), rng.standard_normal(M).astype(np.float32)


def make_operand(x, K):
    """vsim_op_w4a16_rows of the numpy row x -> (x16 device [K], e device [1])."""
    x16 = torch.empty(K, dtype=torch.float16, device=DEV)
    e = torch.empty(1, dtype=torch.int32, device=DEV)
    hip.w4a16_rows(dev(x), K, 1, x16, e)
    return x16, e


def rows_product(w, M, K, x16, e, bias):
    y = torch.full((M + GUARD,), float("nan"), dtype=torch.float32, device=DEV)
    hip.q4_gemm_w4a16_rows(w, M, K, x16, e, 1, bias, y)
    return y[:M].clone()


def ybuf(M):
    return torch.full((M + GUARD,), float("nan"), dtype=torch.float32, device=DEV)


def yread(y, M):
    out = host(y)
    assert np.isnan(out[M:]).all(), "written past M"
    return out[:M]


def act_row(K, seed):
    return (np.random.default_rng(seed).standard_normal(K) * 1.5).astype(np.float32)


# K in blocks: 1, 4, 15, 16, 17, 33, 65 and 512 -- waves without a block, both sides of one block per
# wave, a ragged second block, the second trip of the eight-block loop (more than 128 blocks)
@pytest.mark.parametrize("K", [32, 128, 480, 512, 544, 1056, 2080, 16384])
def test_gemv_equals_rows_product_and_joins(K):
    x16, e = make_operand(act_row(K, K), K)
    v, res, res_a = None, None, None
    for M in (1, 16, 17, 48, 130):
        aos, b = weights(M, K, 3 * M + K)
        w, bd = repack(aos, M, K), dev(b)
        v, res, res_a = C.join_rows(M, K)
        rd, rad = dev(res), dev(res_a)
        for bias in (None, bd):
            want = rows_product(w, M, K, x16, e, bias)
            y = ybuf(M)
            hip.w4a16_gemv([(w, M, K, x16, e, bias, None, None, y)])
            assert np.array_equal(bits(yread(y, M)), bits(host(want))), (M, K, "plain")
            y = ybuf(M)
            hip.w4a16_gemv([(w, M, K, x16, e, bias, rd, None, y)])
            assert np.array_equal(bits(yread(y, M)), bits(host(want + rd))), (M, K, "v + res")
            y = ybuf(M)
            hip.w4a16_gemv([(w, M, K, x16, e, bias, rd, rad, y)])
            assert np.array_equal(bits(yread(y, M)), bits(host(rd + (rad + want)))), (M, K, "res + (res_a + v)")
            # in place: y is res
            y = ybuf(M)
            y[:M] = rd
            hip.w4a16_gemv([(w, M, K, x16, e, bias, y, rad, y)])
            assert np.array_equal(bits(yread(y, M)), bits(host(rd + (rad + want)))), (M, K, "in place")
            y = ybuf(M)
            y[:M] = rd
            hip.w4a16_gemv([(w, M, K, x16, e, bias, y, None, y)])
            assert np.array_equal(bits(yread(y, M)), bits(host(want + rd))), (M, K, "in place, res alone")


def test_gemv_join_order_shows():
    """The join family: res + (res_a + v) and (res + res_a) + v differ, and the kernel gives the first."""
    M, K = 130, 512
    aos, _ = weights(M, K, 9)
    w = repack(aos, M, K)
    x16, e = make_operand(act_row(K, 5) * np.float32(0.02), K)
    v = rows_product(w, M, K, x16, e, None)
    rng = np.random.default_rng(3)
    rd, rad = dev(rng.standard_normal(M).astype(np.float32)), host(v) * np.float32(1.7)
    rad = dev(rad.astype(np.float32))
    right, left = host(rd + (rad + v)), host((rd + rad) + v)
    assert (bits(right) != bits(left)).any()
    y = ybuf(M)
    hip.w4a16_gemv([(w, M, K, x16, e, None, rd, rad, y)])
    assert np.array_equal(bits(yread(y, M)), bits(right))


def test_gemv_four_jobs_and_neighbours():
    """Four jobs of four (M, K) on two operands: each job's bits with its neighbours are its bits alone."""
    shapes = [(130, 512), (17, 1056), (48, 512), (1, 1056)]
    ops = {K: make_operand(act_row(K, 70 + K), K) for K in (512, 1056)}
    jobs, alone = [], []
    for i, (M, K) in enumerate(shapes):
        aos, b = weights(M, K, 100 + i)
        w, bd = repack(aos, M, K), dev(b)
        x16, e = ops[K]
        res = dev(np.random.default_rng(i).standard_normal(M).astype(np.float32)) if i % 2 else None
        y = ybuf(M)
        hip.w4a16_gemv([(w, M, K, x16, e, bd, res, None, y)])
        alone.append(yread(y, M))
        want = rows_product(w, M, K, x16, e, bd)
        assert np.array_equal(bits(alone[-1]), bits(host(want + res if i % 2 else want)))
        jobs.append((w, M, K, x16, e, bd, res, None))
    for order in ([0, 1, 2, 3], [3, 2, 1, 0], [1, 3], [2, 0, 1]):
        ys = [ybuf(shapes[i][0]) for i in order]
        hip.w4a16_gemv([jobs[i] + (ys[k],) for k, i in enumerate(order)])
        for k, i in enumerate(order):
            assert np.array_equal(bits(yread(ys[k], shapes[i][0])), bits(alone[i])), (order, i)


def test_gemv_nonfinite_and_subnormal_operands():
    M, K = 48, 544
    aos, b = weights(M, K, 21)
    w, bd = repack(aos, M, K), dev(b)
    x = act_row(K, 22)
    x[77] = np.inf
    x16, e = make_operand(x, K)
    assert int(host(e)[0]) == W.NONFINITE
    res = dev(act_row(M, 23))
    for args in ((None, None), (res, None), (res, res)):
        y = ybuf(M)
        hip.w4a16_gemv([(w, M, K, x16, e, bd, args[0], args[1], y)])
        got = yread(y, M)
        want = rows_product(w, M, K, x16, e, bd)
        assert (bits(host(want)) == W.QNAN_BITS).all()
        if args[0] is not None:
            want = args[0] + (args[1] + want) if args[1] is not None else want + args[0]
        assert np.isnan(got).all() and np.array_equal(bits(got), bits(host(want))), args
    # a finite job beside it is untouched
    x16f, ef = make_operand(act_row(K, 24), K)
    y0, y1 = ybuf(M), ybuf(M)
    hip.w4a16_gemv([(w, M, K, x16, e, bd, None, None, y0), (w, M, K, x16f, ef, bd, None, None, y1)])
    assert np.array_equal(bits(yread(y1, M)), bits(host(rows_product(w, M, K, x16f, ef, bd))))
    # the subnormal-only operand: the product is made of fp16 subnormals alone
    wd_, wq_, xs, _ = W.subnormal_case()
    Ms, Ks = wd_.shape[0], wd_.shape[1] * 32
    ws = repack(R.q4_pack(wd_, wq_), Ms, Ks)
    x16s, es = make_operand(xs[0], Ks)
    y = ybuf(Ms)
    hip.w4a16_gemv([(ws, Ms, Ks, x16s, es, None, None, None, y)])
    got = yread(y, Ms)
    assert np.array_equal(bits(got), bits(host(rows_product(ws, Ms, Ks, x16s, es, None)))) and np.abs(got).min() > 0


def test_gemv_reads_nothing_behind_its_operands():
    M, K = 40, 544
    aos, b = weights(M, K, 1)
    x = act_row(K, 2)
    x16, e = make_operand(x, K)
    rng = np.random.default_rng(4)
    res, res_a = rng.standard_normal(M).astype(np.float32), rng.standard_normal(M).astype(np.float32)
    y = ybuf(M)
    hip.w4a16_gemv([(repack(aos, M, K), M, K, x16, e, dev(b), dev(res), dev(res_a), y)])
    want = yread(y, M)
    # NaN patterns behind the weight, the operand, the exponent, the bias and both join rows
    nan = np.full(GUARD, np.nan, np.float32)
    x16g = torch.full((K + GUARD,), float("nan"), dtype=torch.float16, device=DEV)
    x16g[:K] = x16
    eg = torch.full((1 + GUARD,), W.NONFINITE, dtype=torch.int32, device=DEV)
    eg[:1] = e
    y = ybuf(M)
    hip.w4a16_gemv([(repack(aos, M, K, slack=4096), M, K, x16g, eg, dev(np.concatenate([b, nan])),
                     dev(np.concatenate([res, nan])), dev(np.concatenate([res_a, nan])), y)])
    assert np.array_equal(bits(yread(y, M)), bits(want))


def test_argument_errors():
    M, K, n = 32, 64, 128
    L = hip.lib()
    w = torch.zeros(hip.q4_bytes(M, K), dtype=torch.uint8, device=DEV)
    x = torch.zeros(n + 4, dtype=torch.float32, device=DEV)
    aff = torch.ones(n + 4, dtype=torch.float32, device=DEV)
    h = torch.zeros(n + 8, dtype=torch.float16, device=DEV)
    e = torch.zeros(4, dtype=torch.int32, device=DEV)
    y = torch.zeros(M, dtype=torch.float32, device=DEV)

    def ln(**kw):
        a = dict(x=x, n=n, w1=aff, b1=aff, x16_1=h, e1=e, w2=None, b2=None, x16_2=None, e2=None)
        a.update(kw)
        args = hip.W4a16LnArgs(hip.ptr(a["x"]), a["n"], hip.ptr(a["w1"]), hip.ptr(a["b1"]), hip.ptr(a["x16_1"]), hip.ptr(a["e1"]),
                               hip.ptr(a["w2"]), hip.ptr(a["b2"]), hip.ptr(a["x16_2"]), hip.ptr(a["e2"]))
        return L.vsim_op_w4a16_ln(args, None)

    assert ln() == 0 and ln(w2=aff, b2=aff, x16_2=h, e2=e) == 0
    for bad in (dict(n=0), dict(n=48), dict(n=16416), dict(x=None), dict(w1=None), dict(b1=None), dict(x16_1=None),
                dict(e1=None), dict(w2=aff), dict(w2=aff, b2=aff, x16_2=h), dict(e2=e), dict(x=x[1:]), dict(w1=aff[1:]),
                dict(x16_1=h[2:]), dict(w2=aff, b2=aff[1:], x16_2=h, e2=e)):
        assert ln(**bad) == EINVAL, bad
    assert L.vsim_op_w4a16_ln(None, None) == EINVAL

    g = L.vsim_op_w4a16_gelu
    X, B, H, Ex = x.data_ptr(), aff.data_ptr(), h.data_ptr(), e.data_ptr()
    assert g(X, B, 64, H, Ex, None, None) == 0 and g(X, None, 64, H, Ex, X, None) == 0
    for bad in ((None, B, 64, H, Ex, None), (X, B, 0, H, Ex, None), (X, B, 48, H, Ex, None), (X, B, 64, None, Ex, None),
                (X, B, 64, H, None, None), (X + 4, B, 64, H, Ex, None), (X, B + 4, 64, H, Ex, None), (X, B, 64, H + 2, Ex, None),
                (X, B, 64, H, Ex, X + 4)):
        assert g(*bad, None) == EINVAL, bad

    def gemv(nj=1, **kw):
        a = dict(w=w, M=M, K=K, x16=h, e=e, bias=None, res=None, res_a=None, y=y)
        a.update(kw)
        args = hip.w4a16_gemv_args([tuple(a[k] for k in ("w", "M", "K", "x16", "e", "bias", "res", "res_a", "y"))] * max(nj, 1))
        args.nj = nj
        return L.vsim_op_w4a16_gemv(args, None)

    assert gemv() == 0 and gemv(4) == 0 and gemv(res=y) == 0 and gemv(res=y, res_a=y) == 0
    for bad in (dict(nj=0), dict(nj=5), dict(K=0), dict(K=48), dict(M=0), dict(M=-3), dict(w=None), dict(x16=None),
                dict(e=None), dict(y=None), dict(res_a=y), dict(x16=h[2:]), dict(w=w[4:])):
        assert gemv(**bad) == EINVAL, bad
    assert L.vsim_op_w4a16_gemv(None, None) == EINVAL
    old = hip.w4a16_set_step(0)
    assert old == 1 and hip.w4a16_set_step(1) == 0 and hip.w4a16_set_step(1) == 1
    torch.cuda.synchronize()
