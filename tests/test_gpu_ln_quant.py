"""k_ln_quant (layer.hip: ln_quant_job over ln_exact_lds_t<512>, 8 slice workgroups per norm) through
vsim_op_ln_quant, bit for bit against the oracle's ops: the float32 join in numpy in the association
the call's operands select, O.norm, the affine of tail_ln_edges, O.quantize.  Compared: the Q4 SoA
row (nibbles and scale bits), the factors xd in xd_slot order, and jout.  Every output buffer is
poisoned before the call and followed by a guard region that must stay as it was.

Sizes (tests/lnq_gemv_cases.py LNQ_SIZES): 1, 4 and 7 blocks leave slices empty, 9 and 33 make them
uneven and odd (the ok = false half of quantize_half), 8, 64 and 192 even; 8192 is the last row
the single-pass load takes and 8224 the first the strided loop does.  The adversarial rows of
tests/tail_ln_edges.py must add to vsim_norm_fallbacks exactly what lnq_restate (this kernel's orders
in numpy) says; tests/test_ln_quant_gemv_cpu.py shows that this is (0, 0), (1, 0) or (0, 1) per
job by family.  No tolerance anywhere.
"""
import functools
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import lnq_gemv_cases as C  # noqa: E402
import tail_ln_edges as T  # noqa: E402
from vsim_amd import hip  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
OK, EINVAL = 0, -1
GUARD = 256  # bytes behind every output buffer
f32 = np.float32


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class Guarded:
    """An output buffer of nbytes (a multiple of 16) with GUARD bytes behind it."""

    def __init__(self, nbytes):
        self.nbytes = nbytes
        self.raw = torch.empty(nbytes + GUARD, dtype=torch.uint8, device=DEV)
        assert self.raw.data_ptr() % 16 == 0

    def poison(self):
        self.raw[:self.nbytes].fill_(0xFF)  # float32 NaNs, nibbles no quantizer leaves with these scales
        self.raw[self.nbytes:].fill_(0x5C)

    def ptr(self):
        return self.raw.data_ptr()

    def bytes(self):
        return host(self.raw)[:self.nbytes].copy()

    def floats(self):
        return self.bytes().view(f32)

    def untouched(self):
        return bool((host(self.raw)[:self.nbytes] == 0xFF).all())

    def guard_ok(self):
        return bool((host(self.raw)[self.nbytes:] == 0x5C).all())


class Rig:
    """One row width's output buffers, built once."""

    def __init__(self, n):
        self.n = n
        self.q = [Guarded(n // 32 * 20 + (-(n // 32 * 20)) % 16) for _ in range(2)]
        self.xd = [Guarded(4 * n) for _ in range(2)]
        self.jout = Guarded(4 * n)
        self.ep = torch.zeros(4, dtype=torch.int32, device=DEV)
        rng = np.random.default_rng(11 * n + 5)
        self.w = [(1.0 + 0.1 * rng.standard_normal(n)).astype(f32) for _ in range(2)]
        self.b = [(0.1 * rng.standard_normal(n)).astype(f32) for _ in range(2)]

    def run(self, x, w1, b1, w2=None, b2=None, join=(None, None, None, None), jout=True, epoch=False):
        """One call: (jout or None, [(SoA bytes, xd)] per norm, the vsim_norm_fallbacks deltas)."""
        n = self.n
        two = w2 is not None
        joined = any(j is not None for j in join)
        for g in self.q + self.xd + [self.jout]:
            g.poison()
        keep = [dev(a) if a is not None else None for a in (x, w1, b1, w2, b2) + tuple(join)]
        a = hip.LnQuantArgs(hip.ptr(keep[0]), n, hip.ptr(keep[1]), hip.ptr(keep[2]), self.q[0].ptr(), self.xd[0].ptr(),
                            hip.ptr(keep[3]), hip.ptr(keep[4]), self.q[1].ptr() if two else None,
                            self.xd[1].ptr() if two else None, hip.ptr(keep[5]), hip.ptr(keep[6]), hip.ptr(keep[7]),
                            hip.ptr(keep[8]), self.jout.ptr() if joined and jout else None,
                            self.ep.data_ptr() if epoch else None)
        torch.cuda.synchronize()
        nf0 = hip.norm_fallbacks()
        hip.ln_quant(a)
        torch.cuda.synchronize()
        nf1 = hip.norm_fallbacks()
        for g in self.q + self.xd + [self.jout]:
            assert g.guard_ok(), "a store behind an output buffer"
        if not two:
            assert self.q[1].untouched() and self.xd[1].untouched()
        if not (joined and jout):
            assert self.jout.untouched()
        nq = n // 32 * 20
        outs = [(self.q[i].bytes()[:nq], self.xd[i].floats()) for i in range(2 if two else 1)]
        return (self.jout.floats() if joined and jout else None), outs, (nf1[0] - nf0[0], nf1[1] - nf0[1])

    def check(self, got, v, norms, tag):
        """jout (when stored) and every norm's SoA row and factors equal the oracle's of the joined row v."""
        import oracle_py as O
        jout, outs, _ = got
        if jout is not None:
            assert np.array_equal(bits(jout), bits(v)), tag + ("jout",)
        y = O.norm(v, self.n, 1)
        assert len(outs) == len(norms)
        for i, (w, b) in enumerate(norms):
            ref = O.quantize(T.affine(w, y, b))
            soa, xd = outs[i]
            assert np.array_equal(soa[:self.n // 2], C.q4_soa(ref)[:self.n // 2]), tag + (f"norm {i + 1}: nibbles",)
            assert np.array_equal(soa[self.n // 2:], C.q4_soa(ref)[self.n // 2:]), tag + (f"norm {i + 1}: scale bits",)
            assert np.array_equal(bits(xd), bits(C.q4_factors(ref))), tag + (f"norm {i + 1}: factors",)


@functools.lru_cache(maxsize=None)
def rig(n):
    return Rig(n)


# ------------------------------------------------------------------ Gaussian rows, every join form
@pytest.mark.parametrize("n", C.LNQ_SIZES + [C.LNQ_MAX_N])
def test_join_forms_vs_oracle(n):
    """No join and the four join forms, each with one norm and with two; jout stored by the first
    job only (once without a jout at all), the epoch word given on some calls."""
    R = rig(n)
    ops = C.join_operands(n, n)
    R.ep.zero_()
    calls = 0
    for k, form in enumerate(("none",) + C.JOIN_FORMS):
        v = C.join(form, *ops)
        for two in (False, True):
            want_jout = not (form == "a_f" and two)
            epoch = (k + two) % 2 == 0
            got = R.run(ops[0], R.w[0], R.b[0], R.w[1] if two else None, R.b[1] if two else None,
                        join=C.join_args(form, *ops[1:]), jout=want_jout, epoch=epoch)
            calls += epoch
            R.check(got, v, [(R.w[0], R.b[0])] + ([(R.w[1], R.b[1])] if two else []), (n, form, two))
            assert (got[0] is not None) == (form != "none" and want_jout)
            assert got[2] == tuple((2 if two else 1) * c for c in C.lnq_restate(v)[0]), (n, form, two, got[2])
    assert host(R.ep).tolist() == [calls, 0, 0, 0]


# ------------------------------------------------------------------ certificate rows
EXPECT = {"certified": (0, 0), "moments_wrong": (0, 0), "mean_uncertified": (1, 0), "scale_ambiguous": (0, 1)}


@pytest.mark.parametrize("size", T.SIZES, ids=lambda s: f"E{s[0]}")
def test_certificate_rows(size):
    """Every family of tests/tail_ln_edges.py as x with no join, and through the join that reproduces
    it (ja = jf = 0, biases 0), with one norm and with two: outputs equal the oracle's, and the call
    adds jobs x the restatement's counts to vsim_norm_fallbacks (slice 0 of each job counts)."""
    n = size[0]
    R = rig(n)
    zeros = np.zeros(n, f32)
    seen = {}
    for name, rows in T.rows(n).items():
        if name in T.FAMILIES:
            assert len(rows) >= T.MIN_ROWS
        for i, r in enumerate(rows):
            want, _ = C.lnq_restate(r.v)
            if name in EXPECT:
                assert want == EXPECT[name], (n, name, i)
            for joined in (False, True):
                two = (i + joined) % 2 == 0
                jobs = 2 if two else 1
                jn = (zeros, zeros if i % 3 else None, zeros, zeros) if joined else (None,) * 4
                v = C.join("full" if jn[1] is not None else "a_f", r.v, *[zeros] * 4) if joined else r.v
                got = R.run(r.v, r.w1, r.b1, R.w[1] if two else None, R.b[1] if two else None, join=jn)
                R.check(got, v, [(r.w1, r.b1)] + ([(R.w[1], R.b[1])] if two else []), (n, name, i, joined, r.note))
                assert got[2] == (jobs * want[0], jobs * want[1]), (n, name, i, joined, got[2], want)
                seen.setdefault(name, set()).add((got[2][0] // jobs, got[2][1] // jobs))
    print(f"n = {n}: vsim_norm_fallbacks deltas per job:", {k: sorted(v) for k, v in seen.items()})
    assert all(c[0] == 1 for c in seen["mean_paths"])


# ------------------------------------------------------------------ quantizer wiring
def test_quantizer_sees_the_golden_row():
    """w1 = 0, b1 = the golden row of tests/golden/ops_qrow.npz (4288 values: 134 blocks over 8
    slices, odd slice lengths among them): z = 0 * y + b = b, so vsim_op_act_unpack of q1 is the
    fixture's quantize_row_q4_0 output byte for byte."""
    gold = np.load(os.path.join(os.path.dirname(__file__), "golden", "ops_qrow.npz"))
    b, n = gold["x"], gold["x"].size
    R = rig(n)
    rng = np.random.default_rng(3)
    x = rng.standard_normal(n).astype(f32)
    _, outs, _ = R.run(x, np.zeros(n, f32), b)
    aos = torch.empty(n // 32 * 20, dtype=torch.uint8, device=DEV)
    hip.check(hip.lib().vsim_op_act_unpack(R.q[0].ptr(), aos.data_ptr(), 1, n, None), "act_unpack")
    assert np.array_equal(host(aos), gold["y"])
    assert np.array_equal(bits(outs[0][1]), bits(C.q4_factors(gold["y"])))


# ------------------------------------------------------------------ the epoch word
def test_epoch_word_advances_by_one_per_call():
    n = 288
    R = rig(n)
    ops = C.join_operands(n, 1)
    R.ep.copy_(torch.tensor([0xFFFFFFFE - (1 << 32), 7, 7, 7], dtype=torch.int32))
    want = 0xFFFFFFFE
    for two in (False, True, True, False):
        R.run(ops[0], R.w[0], R.b[0], R.w[1] if two else None, R.b[1] if two else None,
              join=C.join_args("full", *ops[1:]), epoch=True)
        want = (want + 1) & 0xFFFFFFFF
        assert host(R.ep).view(np.uint32).tolist() == [want, 7, 7, 7]
    R.run(ops[0], R.w[0], R.b[0])  # no epoch given: the word stands
    assert host(R.ep).view(np.uint32).tolist() == [want, 7, 7, 7]


# ------------------------------------------------------------------ non-finite rows
@pytest.mark.parametrize("n", [32, 1056, 8224])
def test_nonfinite_rows(n):
    """A row with one +inf, and one with a NaN: the call returns VSIM_OK, the nibbles equal the
    oracle's, and the scales and factors are NaN exactly where the oracle's are.  The sign and
    payload of a NaN are not compared: x86 and the GPU propagate them differently."""
    import oracle_py as O
    R = rig(n)
    ones, zeros = np.ones(n, f32), np.zeros(n, f32)
    for name, x in T.nonfinite_rows(n):
        for joined in (False, True):
            jn = (zeros, None, zeros, zeros) if joined else (None,) * 4
            jout, outs, delta = R.run(x, ones, zeros, R.w[1], R.b[1], join=jn)
            v = C.join("a_f", x, zeros, zeros, zeros, zeros) if joined else x
            if joined:
                assert np.array_equal(np.isnan(jout), np.isnan(v))
                assert np.array_equal(bits(jout[~np.isnan(v)]), bits(v[~np.isnan(v)]))
            want, _ = C.lnq_restate(v)
            assert want == (1, 1) and delta == (2, 2), (n, name, delta)
            y = O.norm(v, n, 1)
            for i, (w, b) in enumerate(((ones, zeros), (R.w[1], R.b[1]))):
                ref = O.quantize(T.affine(w, y, b)).reshape(-1, 20)
                soa, xd = outs[i]
                assert np.array_equal(soa[:n // 2], ref[:, 4:].reshape(-1)), (n, name, i, "nibbles")
                d_got, d_ref = soa[n // 2:].copy().view(f32), C.q4_scales(ref)
                assert np.array_equal(np.isnan(d_got), np.isnan(d_ref)), (n, name, i, "scales")
                assert np.array_equal(bits(d_got[~np.isnan(d_ref)]), bits(d_ref[~np.isnan(d_ref)]))
                assert np.array_equal(np.isnan(xd).reshape(-1, 32), np.repeat(np.isnan(d_ref)[:, None], 32, axis=1))


# ------------------------------------------------------------------ argument errors
def test_ln_quant_argument_errors():
    n = 256
    R = rig(n)
    L = hip.lib()
    ops = [dev(o) for o in C.join_operands(n, 2)]
    w, b = dev(R.w[0]), dev(R.b[0])
    big = torch.zeros(2 * n + 8, dtype=torch.float32, device=DEV)

    def rc(**f):
        a = hip.ln_quant_args(ops[0], n, w, b, None, None, ja=ops[1], jab=ops[2], jf=ops[3], jfb=ops[4])
        a.q1, a.xd1, a.jout = R.q[0].ptr(), R.xd[0].ptr(), R.jout.ptr()
        for k, v in f.items():
            setattr(a, k, v)
        return L.vsim_op_ln_quant(a, None)

    assert L.vsim_op_ln_quant(None, None) == EINVAL and L.vsim_op_ln_quant(hip.LnQuantArgs(), None) == EINVAL
    for bad_n in (0, -32, 48, 16, C.LNQ_MAX_N + 32, 1 << 20):
        assert rc(n=bad_n) == EINVAL, bad_n
    for name in ("x", "w1", "b1", "q1", "xd1"):
        assert rc(**{name: None}) == EINVAL, name
    second = dict(w2=w.data_ptr(), b2=b.data_ptr(), q2=R.q[1].ptr(), xd2=R.xd[1].ptr())
    for name in second:  # an incomplete second norm: any three of the four, and any one alone
        assert rc(**{k: v for k, v in second.items() if k != name}) == EINVAL, name
        assert rc(**{name: second[name]}) == EINVAL, name
    assert rc(ja=None) == EINVAL and rc(jf=None) == EINVAL  # a bias without its operand
    assert rc(ja=None, jab=None, jf=None, jfb=None) == EINVAL  # jout with nothing to join
    for name in ("x", "w1", "b1", "ja", "jab", "jf", "jfb"):  # jout aliasing, whole and partial
        assert rc(jout=getattr(hip.ln_quant_args(ops[0], n, w, b, None, None, ja=ops[1], jab=ops[2], jf=ops[3],
                                                 jfb=ops[4]), name)) == EINVAL, name
    assert rc(x=big.data_ptr(), jout=big.data_ptr() + 4 * n - 16) == EINVAL
    assert rc(x=big.data_ptr(), jout=big.data_ptr() + 4 * n) == OK  # back to back is no overlap
    assert rc(**second, jout=w.data_ptr()) == EINVAL
    for name in ("x", "w1", "b1", "ja", "jab", "jf", "jfb"):
        for off in (4, 8):  # not aligned for float4
            assert rc(**{name: big.data_ptr() + off}) == EINVAL, (name, off)
    assert rc(jout=big.data_ptr() + 8) == EINVAL
    assert rc(**dict(second, w2=big.data_ptr() + 4)) == EINVAL and rc(**dict(second, b2=big.data_ptr() + 8)) == EINVAL
    assert rc(q1=R.q[0].ptr() + 2) == EINVAL and rc(xd1=R.xd[0].ptr() + 2) == EINVAL
    assert rc(epoch=R.ep.data_ptr() + 2) == EINVAL
    assert rc() == OK and rc(**second) == OK and rc(epoch=R.ep.data_ptr() + 4) == OK
    assert rc(ja=None, jab=None) == OK and rc(jf=None, jfb=None) == OK and rc(jab=None) == OK
    assert rc(ja=None, jab=None, jf=None, jfb=None, jout=None) == OK
    torch.cuda.synchronize()
