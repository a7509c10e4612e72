"""The fused layer tail with its LayerNorm (k_layer_tail with TailLn: lnt_oproj, lnt_prefetch,
lnt_owner) through vsim_op_tail_ln, bit for bit against the oracle's ops: the whole tail on random
Q4_0 weights, and the adversarial joined rows of tests/tail_ln_edges.py with the exact
vsim_norm_fallbacks deltas each must cause.  tests/test_tail_ln_cpu.py shows on the CPU that those
rows bite.  No tolerance anywhere; every call also asserts that vsim_spin_timeouts stood still.

Sizes (E, d, H) give 2, 4, 64, 66, 128 and 384 partial granules for the owners' poll: below one wave,
exactly one, one over, several rounds; 6144 is the widest model width, and nothing wider is tried.
A size whose E/32 is not below the device's CU count is refused by the entry and skipped here.
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import attn_edges as A  # noqa: E402
import tail_ln_edges as T  # noqa: E402
from vsim_amd import hip  # noqa: E402
from vsim_amd import modelgen as mg  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
OK, EINVAL = 0, -1
N_CTX = 64
DEEP_POS = 37
SIZES = T.SIZES
BOTH_SPLITS = 1024  # the size that runs with one and with two workgroups per head


def size_id(s):
    return f"E{s[0]}"


f32 = np.float32


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def repack(aos_np, rows, k):
    src = dev(aos_np)
    dst = torch.empty(hip.q4_bytes(rows, k), dtype=torch.uint8, device=DEV)
    hip.check(hip.lib().vsim_op_q4_repack(src.data_ptr(), dst.data_ptr(), rows, k, None), "repack")
    return dst


def splits(d):
    """nsplit = 2 wherever the column parts are whole 32-blocks."""
    return 2 if (d // 2) % 32 == 0 else 1


def random_q4(rng, rows, k, zero_scale=False):
    """Q4_0 AoS bytes of a random [rows][k] weight from modelgen's quantizer; a K past 2048 repeats
    its first 2048 columns (quantizing 150 M values would take the test's time for nothing).
    zero_scale: every block scale +0 under the random nibbles, so every product is +0."""
    kb = min(k, 2048)
    aos = mg.quantize_q4_0(rng.standard_normal(rows * kb).astype(f32) * f32(0.02)).reshape(rows, kb // 32, 20)
    if k > kb:
        aos = np.tile(aos, (1, (k + kb - 1) // kb, 1))[:, :k // 32]
    aos = np.ascontiguousarray(aos)
    if zero_scale:
        aos[:, :, :4] = 0
    return aos.reshape(-1)


class Rig:
    """One size's device buffers, built once: the attention row at position 0 and at DEEP_POS with the
    oracle's head outputs, zero-scale weights (K = 32) for the crafted rows, outputs, a workspace."""

    def __init__(self, E, d, H):
        self.E, self.d, self.H = E, d, H
        n_rot = 16 if d == 32 else 32
        self.case = (H % 2, d, H, n_rot, False, 1)  # (style, d, H, n_rot, alibi, kqv_nth)
        rng = np.random.default_rng(7 * E + 1)
        self.rng = rng
        self.attn = {}
        for pos in (0, DEEP_POS):
            row = A.gaussian_row(self.case, N_CTX, pos, 300 + E + pos)
            ref = A.reference_row(self.case, row)
            q, k, v, kc, vc = (dev(row[i]) for i in range(5))
            kp = torch.tensor([kc.data_ptr()], dtype=torch.int64, device=DEV)
            vp = torch.tensor([vc.data_ptr()], dtype=torch.int64, device=DEV)
            self.attn[pos] = dict(t=(q, k, v, kc, vc, kp, vp, dev(np.asarray([pos], np.int32))), out=ref[0], aos=ref[1])
        self.oq = torch.zeros(E // 32 * 20, dtype=torch.uint8, device=DEV)
        self.oxd = torch.zeros(E, dtype=torch.float32, device=DEV)
        self.aout = torch.zeros(E, dtype=torch.float32, device=DEV)
        self.jout = torch.zeros(E, dtype=torch.float32, device=DEV)
        self.q = [torch.zeros(E // 32 * 20, dtype=torch.uint8, device=DEV) for _ in range(2)]
        self.xd = [torch.zeros(E, dtype=torch.float32, device=DEV) for _ in range(2)]
        self.zero_wo = repack(random_q4(rng, E, E, zero_scale=True), E, E)
        self.zero_wf = repack(random_q4(rng, E, 32, zero_scale=True), E, 32)
        xf = rng.standard_normal(32).astype(f32)
        self.xf32 = self.factors(xf)
        self.zeros = dev(np.zeros(E, f32))
        # norm 2 of the crafted rows: an ordinary affine
        self.w2 = (1.0 + 0.1 * rng.standard_normal(E)).astype(f32)
        self.b2 = (0.1 * rng.standard_normal(E)).astype(f32)
        self.ws = torch.zeros(hip.tail_ln_ws_bytes(E) + 256, dtype=torch.uint8, device=DEV)
        off = (-self.ws.data_ptr()) % 256
        self.ws = self.ws[off:off + hip.tail_ln_ws_bytes(E)]

    def factors(self, x):
        """vsim_op_q4_quantize's factors of the float row x."""
        k = x.size
        xq = torch.empty(k // 32 * 20, dtype=torch.uint8, device=DEV)
        xd = torch.empty(k, dtype=torch.float32, device=DEV)
        hip.check(hip.lib().vsim_op_q4_quantize(dev(x).data_ptr(), k, 1, xq.data_ptr(), xd.data_ptr(), None), "quantize")
        return xd

    def args(self, x, w1, b1, w2=None, b2=None, ab=None, fb=None, wo=None, wf=None, xd=None, K=32, nsplit=None,
             epoch=1, il=0, ws=None, pos=0):
        """(vsim_tail_ln_args, the tensors it points to)."""
        style, d, H, n_rot, _, nth = self.case
        q, k, v, kc, vc, kp, vp, npd = self.attn[pos]["t"]
        a = hip.AttnBatchArgs(hip.ptr(q), hip.ptr(k), hip.ptr(v), hip.ptr(kp), hip.ptr(vp), hip.ptr(npd), None, None, 1,
                              d, H, n_rot, style, N_CTX, nth, float(A.head_scale(d)), hip.ptr(self.aout),
                              hip.ptr(self.oq), hip.ptr(self.oxd))
        two = w2 is not None
        keep = [dev(x), None if ab is None else dev(ab), self.zeros if fb is None else dev(fb), dev(w1), dev(b1),
                dev(w2) if two else None, dev(b2) if two else None]
        t = hip.tail_ln_args(a, splits(d) if nsplit is None else nsplit, self.zero_wo if wo is None else wo,
                             self.zero_wf if wf is None else wf, self.xf32 if xd is None else xd, K, keep[0], keep[1],
                             keep[2], keep[3], keep[4], keep[5], keep[6], self.jout, self.q[0], self.xd[0],
                             self.q[1] if two else None, self.xd[1] if two else None, epoch, il, ws)
        return t, keep

    def run(self, **kw):
        """One call: (jout, [(Q4 SoA bytes, Q4 AoS bytes, xd)] per norm, the norm_fallbacks deltas).
        The outputs are poisoned first; the spin counter must stand still."""
        two = kw.get("w2") is not None
        self.jout.fill_(float("nan"))
        for i in range(2):
            self.q[i].fill_(0xA5)
            self.xd[i].fill_(float("nan"))
        t, keep = self.args(**kw)
        torch.cuda.synchronize()
        spin0, nf0 = hip.spin_timeouts(), hip.norm_fallbacks()
        hip.tail_ln(t)
        nf1 = hip.norm_fallbacks()
        assert hip.spin_timeouts() == spin0
        outs = []
        for i in range(2 if two else 1):
            aos = torch.empty_like(self.q[i])
            hip.check(hip.lib().vsim_op_act_unpack(self.q[i].data_ptr(), aos.data_ptr(), 1, self.E, None), "act_unpack")
            outs.append((host(self.q[i]).copy(), host(aos), host(self.xd[i]).copy()))
        if not two:  # the second norm's buffers are not touched
            assert (host(self.q[1]) == 0xA5).all() and np.isnan(host(self.xd[1])).all()
        return host(self.jout).copy(), outs, (nf1[0] - nf0[0], nf1[1] - nf0[1])

    def requant(self, z):
        """vsim_op_q4_quantize of the float row z: (Q4 SoA bytes, factors)."""
        xq = torch.empty(self.E // 32 * 20, dtype=torch.uint8, device=DEV)
        xd = torch.empty(self.E, dtype=torch.float32, device=DEV)
        hip.check(hip.lib().vsim_op_q4_quantize(dev(z).data_ptr(), self.E, 1, xq.data_ptr(), xd.data_ptr(), None), "quantize")
        return host(xq), host(xd)

    def check(self, got, v, norms, tag):
        """jout and every norm's nibbles, scales and factors equal the oracle's of the joined row v."""
        import oracle_py as O
        jout, outs, _ = got
        assert np.array_equal(bits(jout), bits(v)), tag + ("jout",)
        y = O.norm(v, self.E, 1)
        for i, (w, b) in enumerate(norms):
            z = T.affine(w, y, b)
            soa, aos, xd = outs[i]
            assert np.array_equal(aos, O.quantize(z)), tag + (f"norm {i + 1}: Q4 nibbles and scales",)
            rq, rxd = self.requant(z)
            assert np.array_equal(soa, rq) and np.array_equal(bits(xd), bits(rxd)), tag + (f"norm {i + 1}: SoA row, factors",)


@functools.lru_cache(maxsize=None)
def _rig(size):
    return Rig(*size)


def rig(size):
    """The size's Rig; where E/32 is not below the CU count the entry must refuse, and the test skips."""
    E = size[0]
    if E // 32 >= torch.cuda.get_device_properties(0).multi_processor_count:
        small = _rig(SIZES[0])
        t, keep = small.args(x=np.zeros(32, f32), w1=np.ones(32, f32), b1=np.zeros(32, f32), nsplit=1)
        t.attn.d, t.attn.H = size[1], size[2]  # the width alone is what is refused, before any buffer is read
        assert hip.lib().vsim_op_tail_ln(t, None) == EINVAL
        pytest.skip(f"E/32 = {E // 32} out-projection tiles do not fit this device's CUs at once")
    return _rig(size)


def join(x, a, ab, f, fb):
    """v = x + ((a + ab) + (f + fb)) in float32 (ab None: a alone)."""
    with np.errstate(all="ignore"):
        t = f32(a) if ab is None else (f32(a) + f32(ab)).astype(f32)
        return (f32(x) + (t + (f32(f) + f32(fb)).astype(f32)).astype(f32)).astype(f32)


# ------------------------------------------------------------------ the whole tail
@pytest.mark.parametrize("size", SIZES, ids=size_id)
def test_whole_tail_vs_oracle(size):
    """Random Q4_0 weights: a = O.mul_mat(wo, attention out), f = O.mul_mat(wf, xf), the float32 join,
    O.norm, the affine, O.quantize.  fc_out K: one block; one full 16-block chunk; two chunks with a
    ragged second (the epilogue's prefetch in chunk 0); the model's 4E.  ab NULL and given, one and
    two norms, position 0 and DEEP_POS, one and two workgroups per head."""
    import oracle_py as O
    R = rig(size)
    E, d = R.E, R.d
    rng = np.random.default_rng(E)
    wo_aos = random_q4(rng, E, E)
    wo = repack(wo_aos, E, E)
    a_ref = {pos: O.mul_mat(wo_aos, E, E, R.attn[pos]["out"], 1, nthreads=8) for pos in (0, DEEP_POS)}
    x = rng.standard_normal(E).astype(f32)
    ab, fb = (0.1 * rng.standard_normal(E)).astype(f32), (0.1 * rng.standard_normal(E)).astype(f32)
    w1, b1 = (1.0 + 0.1 * rng.standard_normal(E)).astype(f32), (0.1 * rng.standard_normal(E)).astype(f32)
    sp = [splits(d)] if E != BOTH_SPLITS else [1, 2]
    #        K      ab     two    pos       nsplit
    plan = [(32, None, False, 0, sp[0]), (512, ab, True, 0, sp[-1]), (544, None, True, DEEP_POS, sp[0]),
            (4 * E, ab, False, 0, sp[-1])]
    if len(sp) > 1:
        plan += [(512, ab, True, DEEP_POS, sp[0]), (32, None, False, 0, sp[-1])]
    il = 0
    for K, abv, two, pos, nsplit in plan:
        wf_aos = random_q4(rng, E, K)
        wf = repack(wf_aos, E, K)
        xf = (rng.standard_normal(K) * 1.5).astype(f32)
        f_ref = O.mul_mat(wf_aos, E, K, xf, 1, nthreads=8)
        v = join(x, a_ref[pos], abv, f_ref, fb)
        il += 1
        got = R.run(x=x, w1=w1, b1=b1, w2=R.w2 if two else None, b2=R.b2 if two else None, ab=abv, fb=fb, wo=wo, wf=wf,
                    xd=R.factors(xf), K=K, nsplit=nsplit, pos=pos, il=il, ws=R.ws)
        tag = (E, K, "ab" if abv is not None else "no ab", pos, nsplit)
        R.check(got, v, [(w1, b1)] + ([(R.w2, R.b2)] if two else []), tag)
        # the heads' own outputs are the oracle's as well
        assert np.array_equal(bits(host(R.aout)), bits(R.attn[pos]["out"])), tag + ("attention out",)
        aos = torch.empty_like(R.oq)
        hip.check(hip.lib().vsim_op_act_unpack(R.oq.data_ptr(), aos.data_ptr(), 1, E, None), "act_unpack")
        assert np.array_equal(host(aos), R.attn[pos]["aos"]), tag + ("attention Q4 row",)
        del wf


# ------------------------------------------------------------------ crafted rows
EXPECT = {"certified": (0, 0), "mean_uncertified": (1, 0), "scale_ambiguous": (0, 1)}


@pytest.mark.parametrize("size", SIZES, ids=size_id)
def test_crafted_rows(size):
    """Every family of tests/tail_ln_edges.py, steered in exactly (zero-scale wo and wf give a = f =
    +0, ab = fb = 0, so v = x + ((0 + 0) + (0 + 0)) = x): outputs equal the oracle's for both norms,
    and the launch adds exactly the family's counts to vsim_norm_fallbacks -- certified (0, 0),
    mean-uncertified (1, 0), scale-ambiguous (0, 1), moments-wrong and the mean-path rows what the
    restatement predicts."""
    R = rig(size)
    E = R.E
    fams = T.rows(E)
    il = 0
    seen = {}
    for name, rows in fams.items():
        if name in T.FAMILIES:
            assert len(rows) >= T.MIN_ROWS
        for i, r in enumerate(rows):
            il = (il + 1) % 255
            two = i % 2 == 0
            abv = np.zeros(E, f32) if i % 3 else None
            v = join(r.v, np.zeros(E, f32), abv, np.zeros(E, f32), np.zeros(E, f32))
            got = R.run(x=r.v, w1=r.w1, b1=r.b1, w2=R.w2 if two else None, b2=R.b2 if two else None, ab=abv,
                        epoch=2, il=il, ws=R.ws)
            R.check(got, v, [(r.w1, r.b1)] + ([(R.w2, R.b2)] if two else []), (E, name, i, r.note))
            assert got[2] == r.counters, (E, name, i, got[2], r.counters)
            if name in EXPECT:
                assert got[2] == EXPECT[name], (E, name, i)
            seen.setdefault(name, set()).add(got[2])
    assert seen["moments_wrong"] <= {(0, 0), (0, 1)}
    assert all(c[0] == 1 for c in seen["mean_paths"])


# ------------------------------------------------------------------ stale tags
@pytest.mark.parametrize("size", [SIZES[1], SIZES[3]], ids=size_id)
def test_stale_tags_never_match(size):
    """One shared workspace: row X at (epoch 1, layer 0), then row Y at (1, 1), (2, 0) and (1, 254).
    Every granule X's call left carries another tag, so each result is Y's; layers 255 and -1 have
    no tag and are refused."""
    R = rig(size)
    E = R.E
    R.ws.zero_()
    fam = T.rows(E)
    X, Y = fam["scale_ambiguous"][0], fam["mean_uncertified"][0]
    ones, zeros = np.ones(E, f32), np.zeros(E, f32)

    def call(r, epoch, il):
        got = R.run(x=r.v, w1=ones, b1=zeros, w2=R.w2, b2=R.b2, epoch=epoch, il=il, ws=R.ws)
        R.check(got, join(r.v, zeros, None, zeros, zeros), [(ones, zeros), (R.w2, R.b2)], (E, epoch, il))
        return got

    assert call(X, 1, 0)[2] == X.counters
    for epoch, il in ((1, 1), (2, 0), (1, 254)):
        got = call(Y, epoch, il)
        assert got[2] == Y.counters
        assert not np.array_equal(bits(got[0]), bits(X.v))
    for il in (255, -1):
        t, keep = R.args(x=Y.v, w1=ones, b1=zeros, epoch=1, il=il, ws=R.ws)
        assert hip.lib().vsim_op_tail_ln(t, None) == EINVAL


# ------------------------------------------------------------------ non-finite rows
@pytest.mark.parametrize("size", [SIZES[0], SIZES[2], SIZES[3]], ids=size_id)
def test_nonfinite_rows(size):
    """A joined row with one +inf, and one with a NaN: the call returns VSIM_OK with no spin timeout,
    the nibbles equal the oracle's, and the scales and factors are NaN exactly where the oracle's
    are.  The sign and payload of a NaN are not compared: x86 and the GPU propagate them differently."""
    import oracle_py as O
    R = rig(size)
    E = R.E
    ones, zeros = np.ones(E, f32), np.zeros(E, f32)
    for il, (name, x) in enumerate(T.nonfinite_rows(E)):
        jout, outs, delta = R.run(x=x, w1=ones, b1=zeros, w2=R.w2, b2=R.b2, epoch=3, il=il, ws=R.ws)
        v = join(x, zeros, None, zeros, zeros)
        assert np.array_equal(np.isnan(jout), np.isnan(v)) and np.array_equal(bits(jout[~np.isnan(v)]), bits(v[~np.isnan(v)]))
        assert delta == T.restate(v).counters == (1, 1), (E, name, delta)
        y = O.norm(v, E, 1)
        for i, (w, b) in enumerate(((ones, zeros), (R.w2, R.b2))):
            ref = O.quantize(T.affine(w, y, b)).reshape(-1, 20)
            soa, aos, xd = outs[i]
            aos = aos.reshape(-1, 20)
            assert np.array_equal(aos[:, 4:], ref[:, 4:]), (E, name, i, "nibbles")
            d_got, d_ref = aos[:, :4].copy().view(f32).reshape(-1), ref[:, :4].copy().view(f32).reshape(-1)
            assert np.array_equal(np.isnan(d_got), np.isnan(d_ref)), (E, name, i, "scales")
            assert np.array_equal(bits(d_got[~np.isnan(d_ref)]), bits(d_ref[~np.isnan(d_ref)]))
            # the factors d * (q - 8): NaN in every block whose scale is
            assert np.array_equal(np.isnan(xd).reshape(-1, 32), np.repeat(np.isnan(d_ref)[:, None], 32, axis=1))


# ------------------------------------------------------------------ argument errors
def test_tail_ln_argument_errors():
    R = rig(SIZES[1])  # E = 64, d = 64, H = 1
    E = R.E
    ones, zeros = np.ones(E, f32), np.zeros(E, f32)
    L = hip.lib()

    def rc(mut=None, **kw):
        base = dict(x=zeros, w1=ones, b1=zeros, ws=R.ws, epoch=5, il=7)
        base.update(kw)
        t, keep = R.args(**base)
        if mut:
            mut(t)
        return L.vsim_op_tail_ln(t, None)

    def setf(**f):
        def m(t):
            for k, v in f.items():
                obj, _, name = k.rpartition("__")
                setattr(getattr(t, obj) if obj else t, name, v)
        return m

    assert L.vsim_op_tail_ln(None, None) == EINVAL
    assert L.vsim_op_tail_ln(hip.TailLnArgs(), None) == EINVAL
    assert rc(setf(attn__B=2)) == EINVAL
    assert rc(nsplit=0) == EINVAL and rc(nsplit=3) == EINVAL
    own = dict(ws=None, ws_bytes=0)  # (another E: not the size's workspace)
    assert rc(setf(attn__d=48, **own)) == EINVAL  # d % 32 (E = 48 is no multiple of 32 either)
    assert rc(setf(attn__d=16, attn__H=4, **own)) == EINVAL  # E = 64, but d % 32
    assert rc(setf(attn__d=32, attn__H=2, **own), nsplit=2) == EINVAL  # 16-column parts are no whole blocks
    assert rc(setf(attn__d=512, **own)) == EINVAL
    assert rc(setf(attn__H=2)) == EINVAL  # the workspace is the smaller E's: short
    assert rc(setf(attn__H=8192 // 64, ws=None, ws_bytes=0)) == EINVAL  # E/32 = 256: never below the CU count
    assert rc(setf(attn__n_ctx=40000)) == EINVAL  # the scores alone exceed the LDS
    assert rc(K=48) == EINVAL and rc(K=0) == EINVAL
    assert rc(il=255) == EINVAL and rc(il=-1) == EINVAL
    for name in ("wo", "wf", "xd", "x", "fb", "w1", "b1", "jout", "q1", "xd1"):
        assert rc(setf(**{name: None})) == EINVAL, name
    # an incomplete second norm, from either end
    assert rc(w2=R.w2, b2=R.b2, mut=setf(q2=None)) == EINVAL and rc(w2=R.w2, b2=R.b2, mut=setf(xd2=None)) == EINVAL
    assert rc(w2=R.w2, b2=R.b2, mut=setf(b2=None)) == EINVAL and rc(setf(q2=R.q[1].data_ptr())) == EINVAL
    assert rc(setf(ws_bytes=hip.tail_ln_ws_bytes(E) - 8)) == EINVAL and rc(setf(ws=R.ws.data_ptr() + 16)) == EINVAL
    assert hip.tail_ln_ws_bytes(E) == 256 + 16 * E + 32 * (E // 32) + 8 * 128 and hip.tail_ln_ws_bytes(48) == 0
    assert rc() == OK and rc(setf(ws=None, ws_bytes=0)) == OK
    torch.cuda.synchronize()
