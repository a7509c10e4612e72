"""The fast decode step kernel by kernel (vsim_amd/csrc/fast_decode.hip through vsim_op_fast_gemv,
vsim_op_fast_tail, vsim_op_fast_oproj_join) against the fp64 restatement of tests/fast_ref.py.

Bounds (u = 2^-24; derived from the kernels' arithmetic, none fitted; every case prints its worst
error as a fraction of its bound):

GEMV row      |y - y64| <= (nb + 8) u A,  A = sum_b |d_w d_x s_b|, nb = K / 32 blocks.
              The device forms float(d_w d_x): one rounding per term, u A in all.  Each (wave,
              half-wave) partial chains its blocks by fma: n_p roundings of at most u A_p (its own
              magnitude sum), over all P partials at most ceil(nb / P) u A.  The P - 1 nonzero
              adds of the fixed-order partial sum round at most u A each.  1 + ceil(nb / P) + P - 1
              <= nb + 1 for 1 <= P <= nb; the slack of 7 covers a one-ulp d_x and second-order
              terms.  Split over sf, each partial row meets the bound with its own nb / sf and A_s,
              and so does their sum with nb and A.
+ bias        one rounding: + u |y64 + b|.
RoPE          c v - s v' with |c|, |s| <= 1: the partner's bound is added, and one rounding of the
              (double, rounded once) result.
GELU          fp16(s + b) is a second discontinuity: fast_ref.gelu_q4_check enumerates the fp16
              values admissible within the row bound and wants the block to be the exact
              quantization of one combination.
Attention     fast_ref.attn_tols: (d + 2) u sum |q_i k_i| scale on a score, (n + 8) u sum p |v| on an
              output, and for every e^x (the kernel's __expf, whose error this project does not
              derive) the relative allowance EPS_P = 4 x EXPF_REL, where EXPF_REL is the worst
              relative error of a probability measured against fp64 by
              test_expf_probability_error on exact arguments in [-87, 0]: 3.7e-6 on MI355X
              (3.685e-6 in the first run, recorded before any other test ran; the test keeps it pinned).
Join          the GEMV bound, the 4 roundings of x + ((a + b_o) + (f + b_proj)) at the magnitudes
              of their results, and the sf - 1 roundings of the partials' sum f.
Quantized outputs (fast_ref.q4_check): unambiguous values exact, ambiguous ones within a step; the
ambiguous share is a property of the inputs (it is computed from the reference and its bound
alone): at most 2 % asserted, 0 - 1.95 % for the chosen seeds (small rows: one element of 64 is 1.6 %).
GELU rows with two admissible fp16 inputs (enumerated, so not capped): 1.7 - 4.8 %.
Measured on MI355X: GEMV rows 0.001 - 0.18 of their bound (largest at K = 128), RoPE rows up to 0.18,
the join up to 0.51 (E = 128), attention partials up to 0.09.
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import fast_ref as R  # noqa: E402
from vsim_amd import hip  # noqa: E402
from vsim_amd import modelgen as mg  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = R.U
EXPF_REL = 3.7e-6        # measured (see above); never adjusted to a failing run
EPS_P = 4.0 * EXPF_REL
NAN32 = float("nan")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def dscalar(v):
    return torch.tensor([v], dtype=torch.int32, device=DEV)


def wpad(aos, rows, k):
    """W4T32 of the AoS weight in the front of a buffer with hip.FAST_PAD bytes of slack (0xFF:
    NaN scales, which the kernels must select away, not multiply by zero)."""
    n = hip.q4_bytes(rows, k)
    buf = torch.full((n + hip.FAST_PAD,), 0xFF, dtype=torch.uint8, device=DEV)
    src = dev(aos)
    hip.check(hip.lib().vsim_op_q4_repack(src.data_ptr(), buf.data_ptr(), rows, k, None), "repack")
    torch.cuda.synchronize()
    return buf


def soa(d, q):
    """A Q4 SoA activation row on the device from its blocks (d [nb], q [nb][32] signed)."""
    k = 32 * np.asarray(d).size
    src = dev(R.q4_pack(d, q))
    buf = torch.empty(k // 32 * 20, dtype=torch.uint8, device=DEV)
    hip.check(hip.lib().vsim_op_act_repack(src.data_ptr(), buf.data_ptr(), 1, k, None), "act_repack")
    torch.cuda.synchronize()
    return buf


def soa_parse(buf, k):
    aos = torch.empty(k // 32 * 20, dtype=torch.uint8, device=DEV)
    hip.check(hip.lib().vsim_op_act_unpack(buf.data_ptr(), aos.data_ptr(), 1, k, None), "act_unpack")
    d, q = R.q4_parse(host(aos), k)
    return d[0], q[0]


def rand_weight(rng, M, K, std=0.05):
    """Random Q4_0 weight: AoS bytes, and its (d, q).  Nibbles and scales are drawn directly."""
    nblk = M * K // 32
    d = (np.abs(rng.standard_normal(nblk)) * std / 7 + 1e-4).astype(np.float32)
    q = rng.integers(-8, 8, (nblk, 32)).astype(np.int8)
    aos = R.q4_pack(d, q)
    return aos, d.reshape(M, K // 32), q.reshape(M, K // 32, 32)


def rand_act(rng, K):
    d = (np.abs(rng.standard_normal(K // 32)) / 7 + 1e-3).astype(np.float32)
    q = rng.integers(-7, 8, (K // 32, 32)).astype(np.int8)
    return d, q


def padded(b):
    """A bias on the device, readable for every row of the last tile (include/vsim_hip.h)."""
    out = np.zeros((b.size + 31) // 32 * 32, np.float32)
    out[:b.size] = b
    return dev(out)


def ln_case(E, base):
    """A residual row and two affines whose normalized rows (the reference's) keep every y * id
    at least 1e-4 from a rounding boundary: the device's activation then equals the reference's.
    The first seed from `base` on that meets it; asserted."""
    for seed in range(base, base + 4000):
        rng = np.random.default_rng(seed)
        x = (rng.standard_normal(E) * 1.7 + 0.4).astype(np.float32)
        w = [(1.0 + 0.2 * rng.standard_normal(E)).astype(np.float32) for _ in range(2)]
        b = [(0.3 * rng.standard_normal(E)).astype(np.float32) for _ in range(2)]
        y = [R.layernorm_ref(x, w[i], b[i]) for i in range(2)]
        if min(R.q4_margin(v) for v in y) >= 1e-4:
            break
    assert min(R.q4_margin(v) for v in y) >= 1e-4
    return x, w, b, [R.q4_quantize_ref(v) for v in y]


# ------------------------------------------------------------------ vsim_op_fast_gemv
@pytest.mark.parametrize("M", [32, 50, 96])
@pytest.mark.parametrize("K", [128, 512, 2176, 4096, 8192])
def test_gemv_store_global_activation(K, M):
    """FE_STORE from a given Q4 activation (integer nibbles: nothing ambiguous).  K = 128: 4 blocks
    for 8 waves, some own none; M = 50: a partial last tile, rows past M stay unwritten; M = 96
    with a bias."""
    rng = np.random.default_rng(K * 100 + M)
    aos, wd, wq = rand_weight(rng, M, K)
    xd, xq = rand_act(rng, K)
    bias = rng.standard_normal(M).astype(np.float32) * np.float32(0.1) if M == 96 else None
    w, x = wpad(aos, M, K), soa(xd, xq)
    y = torch.full((M + 32,), 12345.0, dtype=torch.float32, device=DEV)
    bd = None if bias is None else padded(bias)
    hip.fast_gemv([(w, M, K, bd, y, hip.FE_STORE, 1)], xq=(None, x))
    got = host(y)
    y64, ab = R.q4_dot(wd, wq, xd, xq)
    tol = R.gemv_tol(K // 32, ab)
    if bias is not None:
        y64 = y64 + bias
        tol = tol + U * np.abs(y64)
    ratio = R.bound_ratio(got[:M], y64, tol)
    print(f"gemv store K={K} M={M}: worst error {ratio:.3f} x bound")
    assert ratio <= 1.0
    assert np.all(got[M:] == 12345.0)


@pytest.mark.parametrize("E", [128, 2176, 4096, 6144, 8192])
def test_gemv_layernorm_prologue(E):
    """The LayerNorm prologue with two different affines (job 0 reads affine 1, job 1 affine 0).
    E = 2176: two float4 per thread with a masked tail; 6144 and 8192: three and four."""
    x, w, b, act = ln_case(E, 1000 + E)
    rng = np.random.default_rng(E)
    M = 64
    ws = [rand_weight(rng, M, E) for _ in range(2)]
    wdev = [wpad(a[0], M, E) for a in ws]
    xs, wsd, bsd = dev(x), [dev(v) for v in w], [dev(v) for v in b]
    ys = [torch.full((M,), NAN32, dtype=torch.float32, device=DEV) for _ in range(2)]
    hip.fast_gemv([(wdev[0], M, E, None, ys[0], hip.FE_STORE, 1), (wdev[1], M, E, None, ys[1], hip.FE_STORE, 0)],
                  lnx=xs, lnw=wsd, lnb=bsd)
    for j, a in ((0, 1), (1, 0)):
        y64, ab = R.q4_dot(ws[j][1], ws[j][2], act[a][0], act[a][1])
        ratio = R.bound_ratio(host(ys[j]), y64, R.gemv_tol(E // 32, ab))
        print(f"gemv layernorm E={E} job {j} (affine {a}): worst error {ratio:.3f} x bound")
        assert ratio <= 1.0


@pytest.mark.parametrize("n_past", [0, 5, 8])
@pytest.mark.parametrize("biased", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("style,d,n_rot,E", [(1, 256, 64, 512), (0, 128, 32, 256)], ids=["gptj", "neox"])
def test_gemv_batch_of_four(style, d, n_rot, E, biased, n_past):
    """The batch the model issues per layer: FE_GELU_Q (32 tiles, activation 1), FE_ROPE_Q (E / 32
    tiles), FE_ROPE_K into a cache at row n_past, FE_V (8 tiles) into a cache; the biased cases
    take the LayerNorm prologue, the others two given Q4 rows.  n_ctx = 9: n_past = 8 is the last
    cache row and the last row of the cos/sin table.  Rows of the caches other than n_past keep
    their sentinel, and the `clear` words are zeroed (the word after them is not)."""
    n_ctx, F, Mv = 9, 1024, 256
    rng = np.random.default_rng(style * 1000 + n_past * 10 + biased)
    shapes = [F, E, E, Mv]
    ws = [rand_weight(rng, m, E) for m in shapes]
    wdev = [wpad(a[0], m, E) for a, m in zip(ws, shapes)]
    bias = [rng.standard_normal(m).astype(np.float32) * np.float32(0.2) for m in shapes]
    use_b = [True, biased, biased, biased]  # (the GELU epilogue always has its bias)
    bdev = [padded(v) if u else None for v, u in zip(bias, use_b)]
    if biased:
        x, lw, lb, act = ln_case(E, 5000 + E + n_past)
        src = dict(lnx=dev(x), lnw=[dev(v) for v in lw], lnb=[dev(v) for v in lb])
    else:
        act = [rand_act(rng, E) for _ in range(2)]
        src = dict(xq=[soa(*a) for a in act])
    cs = R.rope_table(n_ctx, n_rot)
    csd, npd = dev(cs), dscalar(n_past)
    oq = torch.full((F // 32 * 20,), 0xFF, dtype=torch.uint8, device=DEV)
    qb = torch.full((E,), NAN32, dtype=torch.float32, device=DEV)
    kc = torch.full((n_ctx, E), -777.0, dtype=torch.float32, device=DEV)
    vc = torch.full((n_ctx, Mv), -777.0, dtype=torch.float32, device=DEV)
    clear = torch.full((13,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    hip.fast_gemv([(wdev[0], F, E, bdev[0], None, hip.FE_GELU_Q, 1), (wdev[1], E, E, bdev[1], qb, hip.FE_ROPE_Q, 0),
                   (wdev[2], E, E, bdev[2], kc, hip.FE_ROPE_K, 0), (wdev[3], Mv, E, bdev[3], vc, hip.FE_V, 0)],
                  oq=oq, n_past=npd, cs=csd, d=d, n_rot=n_rot, style=style, clear=clear, nclear=12, **src)
    ref, tol = [], []
    for j, a in enumerate([1, 0, 0, 0]):
        y64, ab = R.q4_dot(ws[j][1], ws[j][2], act[a][0], act[a][1])
        t = R.gemv_tol(E // 32, ab)
        if use_b[j]:
            y64 = y64 + bias[j]
            t = t + U * np.abs(y64)
        ref.append(y64)
        tol.append(t)
    tab = _tables()[1]
    gd, gq = soa_parse(oq, F)
    share = R.gelu_q4_check(gq, gd, ref[0], tol[0], tab)
    rq = R.rope_ref(ref[1], n_past, cs, d, n_rot, style, tol=tol[1])
    rk = R.rope_ref(ref[2], n_past, cs, d, n_rot, style, tol=tol[2])
    kch, vch = host(kc), host(vc)
    ratios = (R.bound_ratio(host(qb), *rq), R.bound_ratio(kch[n_past], *rk), R.bound_ratio(vch[n_past], ref[3], tol[3]))
    print(f"gemv batch style={style} bias={biased} n_past={n_past}: Q {ratios[0]:.3f} K {ratios[1]:.3f} V {ratios[2]:.3f} "
          f"x bound; GELU rows with two admissible fp16 inputs {share:.4f}")
    assert max(ratios) <= 1.0
    others = np.arange(n_ctx) != n_past
    assert np.all(kch[others] == -777.0) and np.all(vch[others] == -777.0)
    cl = host(clear)
    assert np.all(cl[:12] == 0) and cl[12] == 0x5A5A5A5A


@functools.lru_cache(maxsize=None)
def _tables():
    e = np.zeros(65536, np.uint16)
    g = np.zeros(65536, np.uint16)
    hip.check(hip.lib().vsim_op_tables(hip.ptr(e), hip.ptr(g)), "tables")
    return e, g


# ------------------------------------------------------------------ vsim_op_fast_tail
class Tail:
    """Buffers of one vsim_op_fast_tail call; the half that is not under test is tiny."""

    def __init__(self, rng, d=32, H=1, n_ctx=64, M=32, K=64, sf=2):
        self.d, self.H, self.n_ctx, self.M, self.K, self.sf = d, H, n_ctx, M, K, sf
        self.E, self.nch = d * H, (n_ctx + 63) // 64
        self.w_aos, self.wd, self.wq = rand_weight(rng, M, K)
        self.xd, self.xq = rand_act(rng, K)
        self.w, self.x = wpad(self.w_aos, M, K), soa(self.xd, self.xq)
        self.ffp = torch.full((sf, M), NAN32, dtype=torch.float32, device=DEV)
        self.hcnt = torch.full((4 * H,), 7, dtype=torch.int32, device=DEV)  # (stale: the entry zeroes them)
        self.part = torch.empty((H, self.nch, d + 2), dtype=torch.float32, device=DEV)
        self.oq = torch.empty(self.E // 32 * 20, dtype=torch.uint8, device=DEV)
        self.np_dev = dscalar(0)

    def run(self, q, kc, vc, n_past, scale):
        self.part.fill_(NAN32)  # nothing stale may be read
        self.oq.fill_(0xFF)
        self.np_dev.fill_(n_past)
        hip.fast_tail(self.w, self.M, self.K, self.sf, self.x, self.ffp, q, kc, vc, self.np_dev, self.d, self.H,
                      self.nch, scale, self.part, self.hcnt, self.oq)
        return host(self.part), soa_parse(self.oq, self.E)


def attn_case(d, H, n_ctx, n_pasts, base, low_chunk=None):
    """q, K, V and the reference at every n_past.  Scores spread over about +-10: per head one
    large component of q (4 sqrt(d), so that score = 4 k) over a small dense part (0.05, which
    still moves a score by a hundred times its bound if a lane's products are dropped), so that
    sum |q_i k_i| -- and with it the derived score bound, and through it the share of outputs
    too close to a rounding boundary to be pinned -- stays near its minimum for that spread.
    low_chunk: that chunk's keys are turned to score about -80.  The first seed from `base`
    whose ambiguous share (the reference's alone) is at most 2 % at every n_past; asserted."""
    E, nch = d * H, (n_ctx + 63) // 64
    scale = float(np.float32(1.0 / np.sqrt(d)))
    for seed in range(base, base + 1000):
        rng = np.random.default_rng(seed)
        q = rng.standard_normal((H, d)) * 0.05
        for h in range(H):
            q[h, rng.integers(0, d)] = rng.choice([-1.0, 1.0]) * 4.0 * np.sqrt(d)
        q = q.reshape(E).astype(np.float32)
        kc = rng.standard_normal((n_ctx, E)).astype(np.float32)
        vc = rng.standard_normal((n_ctx, E)).astype(np.float32)
        if low_chunk is not None:
            qh = q.reshape(H, d).astype(np.float64)
            low = -80.0 / (scale * (qh * qh).sum(axis=1))  # k = low q: score -80
            sl = slice(64 * low_chunk, 64 * low_chunk + 64)
            kc[sl] = (0.02 * kc[sl].reshape(64, H, d) + (low[:, None] * qh)[None]).reshape(64, E).astype(np.float32)
        refs = []
        for n_past in n_pasts:
            r = R.attn_ref(q, kc, vc, n_past, d, H, nch, scale)
            refs.append((r, R.attn_tols(r, d, EPS_P)))
        if max(R.q4_ambiguous_share(r["out"], t["out"]) for r, t in refs) <= 0.02:
            break
    assert max(R.q4_ambiguous_share(r["out"], t["out"]) for r, t in refs) <= 0.02
    return q, kc, vc, scale, refs


def _check_attention(T, qd, kd, vd, n_past, scale, r, t, tag):
    part, (od, oq) = T.run(qd, kd, vd, n_past, scale)
    worst = R.attn_part_check(part, r, t)
    share = R.q4_check(oq, od, r["out"], t["out"])
    print(f"attention {tag} n_past={n_past}: partials worst {worst:.3f} x bound, ambiguous share {share:.4f}")
    assert share <= 0.02


@pytest.mark.parametrize("n_ctx", [200, 256])
@pytest.mark.parametrize("H", [2, 3])
@pytest.mark.parametrize("d", [32, 64, 96, 128, 256])
def test_tail_attention(d, H, n_ctx):
    """Chunk partials (m, l, o) and the merged, quantized output at every chunk edge; `part` is
    NaN before each launch.  d = 96 leaves lanes 24..63 idle, d = 32 lanes 8..63; n_ctx = 200 is no
    multiple of the chunk."""
    n_pasts = [0, 1, 7, 8, 62, 63, 64, 65, 127, 128, n_ctx - 1]
    q, kc, vc, scale, refs = attn_case(d, H, n_ctx, n_pasts, d * 10 + H + n_ctx)
    spread = (kc.reshape(n_ctx, H, d) * q.reshape(H, d)).sum(axis=2) * scale
    assert 8.0 < np.abs(spread).max() < 25.0
    T = Tail(np.random.default_rng(0), d, H, n_ctx)
    qd, kd, vd = dev(q), dev(kc), dev(vc)
    for n_past, (r, t) in zip(n_pasts, refs):
        _check_attention(T, qd, kd, vd, n_past, scale, r, t, f"d={d} H={H} n_ctx={n_ctx}")


def test_tail_attention_underflowing_chunk():
    """Chunk 1's maximum lies about 80 below the others': its merge weight underflows (n_past =
    255), or it is the last chunk and the others' do not (n_past = 100)."""
    d, H, n_ctx = 64, 2, 256
    q, kc, vc, scale, refs = attn_case(d, H, n_ctx, [255, 100], 77, low_chunk=1)
    r = refs[0][0]
    assert np.all(r["m"][:, 1] < r["m"].max(axis=1) - 70.0)
    T = Tail(np.random.default_rng(0), d, H, n_ctx)
    qd, kd, vd = dev(q), dev(kc), dev(vc)
    for n_past, (r, t) in zip([255, 100], refs):
        _check_attention(T, qd, kd, vd, n_past, scale, r, t, "underflow")


def test_expf_probability_error():
    """The measurement behind EPS_P.  One head of d = 64, 64 keys: q = e_0 and k_p = x_p e_0 with
    scale 1 make the scores the exact floats x_p (max 0), and v_p = e_p makes o_p the kernel's
    probability __expf(x_p) itself.  x: multiples of 1/64 over [-87, 0] (e^-87 is still a
    normal float).  Worst relative error against fp64 exp, printed; it must stay within the
    recorded EXPF_REL, of which the attention tests allow four times."""
    rng = np.random.default_rng(5)
    d, n = 64, 64
    T = Tail(rng, d, 1, n)
    q = np.zeros(d, np.float32)
    q[0] = 1.0
    vc = np.eye(n, d, dtype=np.float32)
    worst = 0.0
    for rep in range(16):
        x = -(rng.integers(0, 87 * 64, n) / 64.0)
        x[rng.integers(0, n)] = 0.0
        kc = np.zeros((n, d), np.float32)
        kc[:, 0] = x
        part, _ = T.run(dev(q), dev(kc), dev(vc), n - 1, 1.0)
        assert part[0, 0, 0] == 0.0
        p = part[0, 0, 2:].astype(np.float64)
        worst = max(worst, float(np.abs(p / np.exp(x) - 1.0).max()))
    print(f"__expf: worst relative error of a probability {worst:.3e} (recorded {EXPF_REL:.1e})")
    assert worst <= EXPF_REL


@pytest.mark.parametrize("M,K,sf", [(64, 1024, 2), (64, 20480, 4), (32, 32768, 4)])
def test_tail_fcout_partials(M, K, sf):
    """fc_out's K splits: every partial row against its own slice of the activation (a wrong
    offset of a split > 0 reads another slice) and their sum against the whole row.  K = 32768
    with sf = 4 is a split of exactly FD_MAXE values; K = 20480 is the 5120-wide model's."""
    rng = np.random.default_rng(K + sf)
    T = Tail(rng, M=M, K=K, sf=sf)
    q = rng.standard_normal(32).astype(np.float32)
    kv = rng.standard_normal((64, 32)).astype(np.float32)
    T.run(dev(q), dev(kv), dev(kv), 0, 1.0)
    ffp = host(T.ffp).astype(np.float64)
    nb = K // 32
    worst = 0.0
    for s in range(sf):
        y64, ab = R.q4_dot(T.wd, T.wq, T.xd, T.xq, s * nb // sf, (s + 1) * nb // sf)
        worst = max(worst, R.bound_ratio(ffp[s], y64, R.gemv_tol(nb // sf, ab)))
    y64, ab = R.q4_dot(T.wd, T.wq, T.xd, T.xq)
    total = R.bound_ratio(ffp.sum(axis=0), y64, R.gemv_tol(nb, ab))
    print(f"fc_out M={M} K={K} sf={sf}: partial rows worst {worst:.3f}, their sum {total:.3f} x bound")
    assert worst <= 1.0 and total <= 1.0
    assert np.all(host(T.hcnt)[0::4] == 1)  # one chunk workgroup counted per head, from zero


# ------------------------------------------------------------------ vsim_op_fast_oproj_join
@functools.lru_cache(maxsize=None)
def _oproj_case(E):
    """One weight, activation and fp64 product per width, shared by the bo / sf variants."""
    rng = np.random.default_rng(E)
    aos, wd, wq = rand_weight(rng, E, E)
    xd, xq = rand_act(rng, E)
    y64, ab = R.q4_dot(wd, wq, xd, xq)
    return wpad(aos, E, E), soa(xd, xq), y64, ab


@pytest.mark.parametrize("sf", [2, 4])
@pytest.mark.parametrize("with_bo", [False, True], ids=["nobo", "bo"])
@pytest.mark.parametrize("E", [128, 512, 2176, 8192])
def test_oproj_join(E, with_bo, sf):
    w, xq, s64, ab = _oproj_case(E)
    rng = np.random.default_rng(E + sf + with_bo)
    x, bproj, bo = (rng.standard_normal(E).astype(np.float32) for _ in range(3))
    ffp = rng.standard_normal((sf, E)).astype(np.float32)
    out = torch.full((E,), NAN32, dtype=torch.float32, device=DEV)
    ops = [dev(bo) if with_bo else None, dev(ffp), dev(bproj), dev(x)]
    hip.fast_oproj_join(w, E, xq, ops[0], ops[1], sf, ops[2], ops[3], out)
    f64 = ffp.astype(np.float64)
    a = s64 + (bo if with_bo else 0.0)
    f = f64.sum(axis=0) + bproj
    ref = R.join_ref(x, s64, bo if with_bo else None, ffp, bproj)
    tol = (R.gemv_tol(E // 32, ab) + U * (np.abs(a) + np.abs(f) + np.abs(a + f) + np.abs(ref)) +
           (sf - 1) * U * np.abs(f64).sum(axis=0))
    ratio = R.bound_ratio(host(out), ref, tol)
    print(f"oproj_join E={E} bo={with_bo} sf={sf}: worst error {ratio:.3f} x bound")
    assert ratio <= 1.0


# ------------------------------------------------------------------ wiring
def _f32(m, name, n):
    return dev(m.get_tensor(name, 4 * n).view(np.float32))


def _q4(m, name, rows, k):
    return wpad(m.get_tensor(name, rows * k // 32 * 20), rows, k)


@pytest.mark.parametrize("name", ["tiny-gptj", "small-gptj", "tiny-neox", "small-neox"])
def test_model_step_is_these_entries_composed(tmp_path, name):
    """One-layer models, n_ctx = 200, fast mode: the logits of every decode step from n_past = 0 to
    65 (0..3 and the chunk edge 63..65 among them) are bit-identical to vsim_op_get_rows, the three
    entries and the head (an FE_STORE job behind the final norm's prologue) composed on the model's
    own weights and a cache kept here.  Same kernels, same launch parameters, a deterministic
    step: a difference means model.cpp wires them otherwise than the tests above assume."""
    arch_s, hp0 = mg.CONFIGS[name]
    hp = mg.HParams(hp0.n_vocab, hp0.n_embd, hp0.n_head, 1, hp0.n_rot, hp0.use_parallel_residual)
    path = str(tmp_path / f"{name}-1.bin")
    mg.write_model(path, arch_s, hp, seed=21, std=0.05)
    gptj = arch_s == "gptj"
    n_ctx = 200
    m = hip.Model.load(path, hip.ARCH_GPTJ if gptj else hip.ARCH_GPTNEOX, n_ctx=n_ctx)
    m.set_mode(hip.MODE_FAST)
    E, V, H, F = hp.n_embd, hp.n_vocab, hp.n_head, 4 * hp.n_embd
    d, nch, sf = E // H, (n_ctx + 63) // 64, 2
    if gptj:
        p = "transformer.h.0."
        wte, lmh = _q4(m, "transformer.wte.weight", V, E), _q4(m, "lm_head.weight", V, E)
        lmh_b = padded(m.get_tensor("lm_head.bias", 4 * V).view(np.float32))
        lnf = (_f32(m, "transformer.ln_f.weight", E), _f32(m, "transformer.ln_f.bias", E))
        ln1 = ln2 = (_f32(m, p + "ln_1.weight", E), _f32(m, p + "ln_1.bias", E))
        wq, wk, wv, wo = (_q4(m, p + f"attn.{n}_proj.weight", E, E) for n in ("q", "k", "v", "out"))
        bq = bk = bv = bo = None
        wfc, bfc = _q4(m, p + "mlp.fc_in.weight", F, E), _f32(m, p + "mlp.fc_in.bias", F)
        wpr, bpr = _q4(m, p + "mlp.fc_out.weight", E, F), _f32(m, p + "mlp.fc_out.bias", E)
    else:
        p = "gpt_neox.layers.0."
        wte, lmh, lmh_b = _q4(m, "gpt_neox.embed_in.weight", V, E), _q4(m, "embed_out.weight", V, E), None
        lnf = (_f32(m, "gpt_neox.final_layer_norm.weight", E), _f32(m, "gpt_neox.final_layer_norm.bias", E))
        ln1 = (_f32(m, p + "input_layernorm.weight", E), _f32(m, p + "input_layernorm.bias", E))
        ln2 = (_f32(m, p + "post_attention_layernorm.weight", E), _f32(m, p + "post_attention_layernorm.bias", E))
        wq, wk, wv, wo = (_q4(m, p + f"attention.{n}.weight", E, E) for n in ("query", "key", "value", "dense"))
        bq, bk, bv, bo = (_f32(m, p + f"attention.{n}.bias", E) for n in ("query", "key", "value", "dense"))
        wfc, bfc = _q4(m, p + "mlp.dense_h_to_4h.weight", F, E), _f32(m, p + "mlp.dense_h_to_4h.bias", F)
        wpr, bpr = _q4(m, p + "mlp.dense_4h_to_h.weight", E, F), _f32(m, p + "mlp.dense_4h_to_h.bias", E)
    cs = dev(R.rope_table(n_ctx, hp.n_rot))
    scale = float(np.float32(1.0 / np.sqrt(float(np.float32(E) / np.float32(H)))))
    f32 = dict(dtype=torch.float32, device=DEV)
    x0, x1, qb, logits = (torch.zeros(n, **f32) for n in (E, E, E, V))
    kc, vc = torch.zeros((n_ctx, E), **f32), torch.zeros((n_ctx, E), **f32)
    ffp, part = torch.zeros(8 * E, **f32), torch.zeros(H * nch * (d + 2), **f32)
    oq3 = torch.zeros(F // 32 * 20, dtype=torch.uint8, device=DEV)
    oqa = torch.zeros(E // 32 * 20, dtype=torch.uint8, device=DEV)
    hcnt = torch.zeros(4 * H, dtype=torch.int32, device=DEV)
    tok_d, np_d = dscalar(0), dscalar(0)
    L = hip.lib()
    for n_past in range(66):
        tok = (7 * n_past + 3) % V
        want = m.eval(n_past, [tok])
        tok_d.fill_(tok)
        np_d.fill_(n_past)
        hip.check(L.vsim_op_get_rows(wte.data_ptr(), E, V, tok_d.data_ptr(), 1, x0.data_ptr(), None), "get_rows")
        hip.fast_gemv([(wfc, F, E, bfc, None, hip.FE_GELU_Q, 1), (wq, E, E, bq, qb, hip.FE_ROPE_Q, 0),
                       (wk, E, E, bk, kc, hip.FE_ROPE_K, 0), (wv, E, E, bv, vc, hip.FE_V, 0)],
                      lnx=x0, lnw=(ln1[0], ln2[0]), lnb=(ln1[1], ln2[1]), oq=oq3, n_past=np_d, cs=cs, d=d,
                      n_rot=hp.n_rot, style=1 if gptj else 0, clear=hcnt, nclear=4 * H)
        hip.fast_tail(wpr, E, F, sf, oq3, ffp, qb, kc, vc, np_d, d, H, nch, scale, part, hcnt, oqa)
        hip.fast_oproj_join(wo, E, oqa, bo, ffp, sf, bpr, x0, x1)
        hip.fast_gemv([(lmh, V, E, lmh_b, logits, hip.FE_STORE, 0)], lnx=x1, lnw=(lnf[0], lnf[0]), lnb=(lnf[1], lnf[1]))
        got = host(logits)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"{name}: step at n_past = {n_past} differs"
    m.close()


# ------------------------------------------------------------------ the context-length gap
def test_fast_mode_beyond_the_chunk_limit_runs_exact(tmp_path):
    """n_ctx = 4160 is 65 chunks, one more than the fast step's merge holds (launch_fast_tail
    refuses it).  Fast mode on such a model must not fail every decode step: it runs the exact
    step, so a short prompt and three decode steps equal exact mode bit for bit."""
    arch_s, hp = mg.CONFIGS["tiny-gptj"]
    path = str(tmp_path / "tiny-gptj.bin")
    mg.write_model(path, arch_s, hp, seed=5, std=0.05)
    m = hip.Model.load(path, hip.ARCH_GPTJ, n_ctx=4160)
    ids = [3, 1, 4, 1, 5]
    runs = {}
    for mode in (hip.MODE_EXACT, hip.MODE_FAST):
        m.set_mode(mode)
        out = [m.eval(0, ids).copy()]
        for i in range(3):
            out.append(m.eval(len(ids) + i, [int(np.argmax(out[-1]))]).copy())
        runs[mode] = out
    for a, b in zip(runs[hip.MODE_EXACT], runs[hip.MODE_FAST]):
        assert np.isfinite(b).all()
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    m.close()
