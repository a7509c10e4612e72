"""The exact decode step's GEMV batch (launch_gemv_chain_batch: k_gemv_solo or k_gemv_chain32) through
vsim_op_gemv_batch, bit for bit against the oracle: O.mul_mat plus the bias in float32, and for the
GELU-quantize epilogue O.gelu and O.quantize of that.  Every output buffer is poisoned before the
call and followed by a guard region that must stay as it was; the kernel the launch reports is
asserted in every case.

  * K at the seams of both kernels' chunk pipelines (tests/lnq_gemv_cases.py SOLO_NB, CHAIN32_NB);
  * the row counts at which the launch changes kernel, the half-empty last group, a partial tile;
  * four-job batches in both regimes, each job compared with the job run alone;
  * the epilogue's whole domain through zero-scale weights (acc = +0, so the epilogue sees the
    bias): every fp16 pattern, every fp16 rounding tie with its float32 neighbours, all-zero blocks,
    blocks with one value, blocks that mix the table's NaN and inf with finite values;
  * the model's exact step is vsim_op_get_rows, vsim_op_ln_quant, vsim_op_gemv_batch, vsim_op_tail_ln
    and vsim_op_q4_gemv composed.
tests/test_ln_quant_gemv_cpu.py shows on the CPU that these inputs bite.  No tolerance anywhere.
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import lnq_gemv_cases as C  # noqa: E402
from vsim_amd import hip  # noqa: E402
from vsim_amd import modelgen as mg  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
OK, EINVAL = 0, -1
GUARD = 256
SOLO, CHAIN32 = 1, 0
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
    torch.cuda.synchronize()
    return dst


def factors(x):
    """vsim_op_q4_quantize's factors of the float row x, on the device."""
    k = x.size
    xq = torch.empty(k // 32 * 20, dtype=torch.uint8, device=DEV)
    xd = torch.empty(k, dtype=torch.float32, device=DEV)
    hip.check(hip.lib().vsim_op_q4_quantize(dev(x).data_ptr(), k, 1, xq.data_ptr(), xd.data_ptr(), None), "quantize")
    return xd


class Guarded:
    """An output buffer of nbytes with GUARD bytes behind it, all poisoned."""

    def __init__(self, nbytes):
        self.nbytes = nbytes
        self.raw = torch.empty((nbytes + 15) // 16 * 16 + GUARD, dtype=torch.uint8, device=DEV)
        self.raw[:nbytes].fill_(0xFF)  # float32 NaNs
        self.raw[nbytes:].fill_(0x5C)

    def ptr(self):
        return self.raw.data_ptr()

    def read(self):
        """The payload bytes; asserts the guard."""
        h = host(self.raw)
        assert (h[self.nbytes:] == 0x5C).all(), "a store behind an output buffer"
        return h[:self.nbytes].copy()


class Job:
    """One job of a batch: operands on the device, fresh poisoned outputs, the oracle's expectation.
    acc: the product row (O.mul_mat, or zeros for a zero-scale weight)."""

    def __init__(self, w, M, K, xd, acc, bias=None, gelu_q=False, y=True):
        self.w, self.M, self.K, self.xd, self.gelu_q = w, M, K, xd, gelu_q
        self.bias_np = bias
        self.bias = None if bias is None else dev(bias)
        with np.errstate(all="ignore"):
            self.v = np.ascontiguousarray(acc, f32) if bias is None else (np.ascontiguousarray(acc, f32) + bias).astype(f32)
        self.want_y = y
        self.fresh()

    def fresh(self):
        self.y = Guarded(4 * self.M) if self.want_y else None
        self.oq = Guarded(self.M // 32 * 20) if self.gelu_q else None
        self.oxd = Guarded(4 * self.M) if self.gelu_q else None

    def tuple(self):
        g = lambda b: None if b is None else b.raw
        return (self.w, self.M, self.K, self.xd, self.bias, g(self.y), int(self.gelu_q), g(self.oq), g(self.oxd))

    def outputs(self):
        """(y bytes, oq bytes, oxd bytes), None where the job has none."""
        return tuple(None if b is None else b.read() for b in (self.y, self.oq, self.oxd))

    def check(self, tag):
        """The outputs equal the oracle's.  Returns the number of blocks compared NaN-class."""
        import oracle_py as O
        y, oq, oxd = self.outputs()
        if not self.gelu_q:
            assert np.array_equal(y.view(np.uint32), bits(self.v)), tag + ("y",)
            return 0
        g = O.gelu(self.v)
        ref = O.quantize(g)
        nanblk = ~np.isfinite(g.reshape(-1, 32)).all(axis=1)
        if y is not None:
            assert np.array_equal(y.view(np.uint32), bits(g)), tag + ("y",)
        n16 = self.M // 2
        assert np.array_equal(oq[:n16], C.q4_soa(ref)[:n16]), tag + ("nibbles",)
        d, d_ref = oq[n16:].copy().view(f32), C.q4_scales(ref)
        xd, xd_ref = oxd.view(f32), C.q4_factors(ref)
        fin = ~np.isnan(d_ref)
        assert not (np.isnan(d_ref) & ~nanblk).any()  # NaN-class only where the table gave a non-finite value
        assert np.array_equal(bits(d[fin]), bits(d_ref[fin])) and np.isnan(d[~fin]).all(), tag + ("scales",)
        fx = ~np.isnan(xd_ref)
        assert not (np.isnan(xd_ref).reshape(-1, 32).any(axis=1) & ~nanblk).any()
        assert np.array_equal(bits(xd[fx]), bits(xd_ref[fx])) and np.isnan(xd[~fx]).all(), tag + ("factors",)
        return int(nanblk.sum())


def run(jobs, kernel):
    got = hip.gemv_batch([j.tuple() for j in jobs])
    torch.cuda.synchronize()
    assert got == kernel == int(C.picks_solo([j.M for j in jobs])), (got, kernel)


def random_job(rng, M, K, bias=True, gelu_q=False, y=True, x_scale=1.0):
    import oracle_py as O
    aos = C.rand_q4_aos(rng, M, K)
    x = (rng.standard_normal(K) * x_scale).astype(f32)
    acc = O.mul_mat(aos, M, K, x, 1, nthreads=8)
    b = (0.5 * rng.standard_normal(M)).astype(f32) if bias or gelu_q else None
    return Job(repack(aos, M, K), M, K, factors(x), acc, b, gelu_q, y)


# ------------------------------------------------------------------ K seams
@pytest.mark.parametrize("nb", C.SOLO_NB)
def test_solo_k_seams(nb):
    """k_gemv_solo, M = 12288 (192 groups): K on both sides of one chunk (6 blocks), of the prefetch
    depth, of the pair-term ring and of the nit round-up; store epilogue with the bias."""
    j = random_job(np.random.default_rng(100 + nb), 12288, 32 * nb)
    run([j], SOLO)
    j.check((nb,))


@pytest.mark.parametrize("nb", C.CHAIN32_NB)
def test_chain32_k_seams(nb):
    """k_gemv_chain32, three tiles and a one-row second tile: K on both sides of 1..4 chunks of 8
    blocks (the LDS-DMA depth) and past them; with and without the bias."""
    for M, bias in ((96, True), (33, False)):
        j = random_job(np.random.default_rng(200 + nb + M), M, 32 * nb, bias=bias)
        run([j], CHAIN32)
        j.check((M, nb))


# ------------------------------------------------------------------ the choice of kernel
@pytest.mark.parametrize("M,kernel", [(12224, CHAIN32), (12256, SOLO), (12288, SOLO)])
def test_kernel_choice_gelu_q(M, kernel):
    """191 groups run as chain32, 192 as solo; 12256 rows leave the last group's second tile missing,
    so that consumer's upper half-wave runs quantize_half with ok = false.  nb = 7, GELU-quantize."""
    rng = np.random.default_rng(M)
    for y in (True, False):
        j = random_job(rng, M, 224, gelu_q=True, y=y, x_scale=30.0)
        run([j], kernel)
        assert j.check((M, y)) == 0


def test_kernel_choice_store_partial_tile():
    """M = 12230: 383 tiles, the last with 6 rows, 192 groups: solo, plain store."""
    j = random_job(np.random.default_rng(12230), 12230, 224, bias=False)
    run([j], SOLO)
    j.check((12230,))


# ------------------------------------------------------------------ batches
def _batch(rng, Ms, Ks, y_on_gelu):
    """[gelu_q job, odd tile count, M % 32 != 0, one tile]."""
    return [random_job(rng, Ms[0], Ks[0], gelu_q=True, y=y_on_gelu, x_scale=30.0), random_job(rng, Ms[1], Ks[1]),
            random_job(rng, Ms[2], Ks[2], bias=False), random_job(rng, Ms[3], Ks[3])]


@pytest.mark.parametrize("regime", ["chain32", "solo"])
def test_four_job_batches(regime):
    """Four jobs of different M -- a GELU-quantize job, an odd tile count (in solo: a group whose second
    tile is missing, with other jobs' groups behind it), a partial tile, one tile -- with y given and
    y NULL on the GELU job, with one K and with four; every job's outputs equal the oracle's and,
    byte for byte, those of the job run alone (whichever kernel that launch takes)."""
    solo = regime == "solo"
    Ms = (8192, 4128, 1000, 32) if solo else (128, 96, 50, 32)
    assert C.picks_solo(Ms) == solo and (Ms[1] // 32) % 2 == 1
    rng = np.random.default_rng(77 + solo)
    for Ks, y_on_gelu in (((224,) * 4, True), ((224,) * 4, False), ((416, 32, 608, 1376), True)):
        jobs = _batch(rng, Ms, Ks, y_on_gelu)
        run(jobs, SOLO if solo else CHAIN32)
        together = []
        for i, j in enumerate(jobs):
            j.check((regime, Ks, i))
            together.append(j.outputs())
        for i, j in enumerate(jobs):
            j.fresh()
            run([j], int(C.picks_solo([j.M])))
            for a, b in zip(together[i], j.outputs()):
                assert (a is None and b is None) or np.array_equal(a, b), (regime, Ks, i, "differs from the job alone")


# ------------------------------------------------------------------ the epilogue's whole domain
@functools.lru_cache(maxsize=None)
def zero_weight(M):
    """(W4T32 of M rows x 32 with every scale +0 under random nibbles, factors of a Gaussian row)."""
    rng = np.random.default_rng(M)
    return repack(C.rand_q4_aos(rng, M, 32, zero_scale=True), M, 32), factors((3 * rng.standard_normal(32)).astype(f32))


CHUNK = 8192  # rows per chain32 launch of the sweeps: 128 groups


def epilogue_rows(bias, y=True):
    """The rows `bias` (a multiple of 32) through the GELU-quantize epilogue: one solo launch when
    they make 192 groups, and chain32 launches of CHUNK rows.  Returns the NaN-class block count of
    each pass."""
    M = bias.size
    counts = []
    if C.picks_solo([M]):
        w, xd = zero_weight(M)
        j = Job(w, M, 32, xd, np.zeros(M, f32), bias, gelu_q=True, y=y)
        run([j], SOLO)
        counts.append(j.check(("solo",)))
    n = 0
    for r0 in range(0, M, CHUNK):
        m = min(CHUNK, M - r0)
        w, xd = zero_weight(m)
        j = Job(w, m, 32, xd, np.zeros(m, f32), bias[r0:r0 + m], gelu_q=True, y=y)
        run([j], CHAIN32)
        n += j.check(("chain32", r0))
    counts.append(n)
    return counts


def test_epilogue_every_half():
    """(a) every fp16 pattern widened to float32 as the bias: subnormals, both table ends, inf, NaN.
    NaN-class comparison touches only blocks with a non-finite table output: as many as the oracle has,
    at most 4 % of the sweep."""
    import oracle_py as O
    x = C.all_half_rows()
    want = int((~np.isfinite(O.gelu(x).reshape(-1, 32)).all(axis=1)).sum())
    counts = epilogue_rows(x)
    assert len(counts) == 2 and counts == [want, want] and 0 < want <= 0.04 * (x.size // 32)


def test_epilogue_rounding_ties():
    """(b) for every finite half h >= 0 the float32 midpoint of h and its successor and that
    midpoint's two float32 neighbours, both signs, 65520 past the largest half among them.  The last
    block (..., 65504, inf, inf, -0, NaN, NaN: the table's values for 65520 and -65520) is the row that
    showed the epilogues' amax tree taking another maximum than quantize_row_q4_0's MAX macro does
    when a block mixes NaNs with values (kern.hpp q4_half, SEQNAN)."""
    rows, _ = C.tie_rows()
    counts = epilogue_rows(np.ascontiguousarray(rows.transpose(2, 0, 1)).reshape(-1), y=True)
    # only the overflow rows around +-65520 give a non-finite table output
    assert len(counts) == 2 and counts[0] == counts[1] <= 2


def test_epilogue_zero_and_single_value_blocks():
    """(c) blocks that are all zero after GELU (a bias far below the table's last non-zero entry, +0,
    -0), and blocks with a single non-zero value at lane 0 and at lane 31, in both tiles of a solo
    group (the lower and the upper half-wave)."""
    import oracle_py as O
    assert not O.gelu(np.full(4, -40.0, f32)).any()
    for M, kernel in ((12288, SOLO), (512, CHAIN32)):
        b = np.full((M // 32, 32), -40.0, f32)
        b[1], b[2] = 0.0, -0.0
        for k, (blk, lane) in enumerate(((4, 0), (5, 0), (6, 31), (7, 31), (9, 0), (10, 31), (12, 17))):
            b[blk, lane] = (1.5, -0.75, 3e-5, 60000.0, -1e-3, 0.3, 7.0)[k]
        b[14, 0], b[14, 31] = 2.0, -2.0
        w, xd = zero_weight(M)
        for y in (True, False):
            j = Job(w, M, 32, xd, np.zeros(M, f32), b.reshape(-1), gelu_q=True, y=y)
            run([j], kernel)
            assert j.check((M, y)) == 0
        d = C.q4_scales(O.quantize(O.gelu(b.reshape(-1))))
        assert not d[[0, 1, 2, 3]].any() and d[[4, 5, 6, 7, 9, 10, 12, 14]].all()


def test_epilogue_blocks_mixing_nan_with_values():
    """The table gives NaN for -inf and inf for +inf; in a block that mixes them with finite values the
    order of quantize_row_q4_0's MAX macro shows: amax is the maximum behind the block's last NaN, or
    NaN when the last element is one (the tie sweep's last block is such a block).  NaN first, last,
    in the middle with the largest value before it, after an inf, before an inf, two NaNs, all NaN:
    each in a lower and in an upper half-wave block.  Scales and factors are finite wherever the
    oracle's are, and then compared bit for bit."""
    import oracle_py as O
    NEG, POS = f32(-70000.0), f32(70000.0)  # fp16(-70000) = -inf -> NaN, fp16(70000) = inf -> inf
    g = O.gelu(np.array([NEG, POS], f32))
    assert np.isnan(g[0]) and np.isposinf(g[1])
    rng = np.random.default_rng(9)

    def block(*puts):
        b = (4.0 * rng.standard_normal(32)).astype(f32)
        for lane, val in puts:
            b[lane] = val
        return b

    pats = [block((0, NEG)), block((31, NEG)), block((3, 50.0), (20, NEG)), block((13, NEG), (20, NEG), (3, 50.0)),
            block((5, POS), (9, NEG)), block((9, NEG), (25, POS)), block((30, NEG), (31, 9.0)), block((31, POS)),
            np.full(32, NEG, f32), block(*[(l, NEG) for l in range(0, 31)])]
    for M, kernel in ((12288, SOLO), (2048, CHAIN32)):
        b = (4.0 * rng.standard_normal((M // 32, 32))).astype(f32)
        for k, p in enumerate(pats):  # as it is and mirrored, each in a lower and an upper half-wave block
            b[2 + 2 * k] = b[3 + 2 * k] = p
            b[2 + 2 * (len(pats) + k)] = b[3 + 2 * (len(pats) + k)] = p[::-1]
        w, xd = zero_weight(M)
        j = Job(w, M, 32, xd, np.zeros(M, f32), b.reshape(-1), gelu_q=True)
        run([j], kernel)
        assert j.check((M,)) == 4 * len(pats)
        gl = O.gelu(b.reshape(-1)).reshape(-1, 32)
        d = C.q4_scales(O.quantize(gl.reshape(-1)))
        # the order rule itself: the scale is NaN exactly where the block's last element is
        assert np.array_equal(np.isnan(d), np.isnan(gl[:, 31])) and np.isfinite(d[2]) and np.isnan(d[4])


# ------------------------------------------------------------------ argument errors
def test_gemv_batch_argument_errors():
    L = hip.lib()
    rng = np.random.default_rng(1)
    j = random_job(rng, 64, 64, gelu_q=True)
    s = random_job(rng, 40, 64)
    import ctypes
    kern = ctypes.c_int32(-1)

    def rc(jobs, nj=None, at=0, **f):
        a = hip.gemv_batch_args([x.tuple() for x in jobs])
        if nj is not None:
            a.nj = nj
        for k, v in f.items():
            setattr(a.j[at], k, v)
        return L.vsim_op_gemv_batch(a, ctypes.byref(kern), None)

    assert L.vsim_op_gemv_batch(None, None, None) == EINVAL
    assert rc([j], nj=0) == EINVAL and rc([j], nj=5) == EINVAL and rc([j], nj=-1) == EINVAL
    for K in (0, -32, 48, 16):
        assert rc([s], K=K) == EINVAL, K
    assert rc([s], M=0) == EINVAL and rc([s], M=-5) == EINVAL
    for name in ("w", "xd", "y"):
        assert rc([s], **{name: None}) == EINVAL, name
    for name in ("w", "xd", "bias", "oq", "oxd"):
        assert rc([j], **{name: None}) == EINVAL, name
    assert rc([j], M=40) == EINVAL  # GELU-quantize needs whole tiles
    assert rc([s, j], M=40, gelu_q=1, oq=j.oq.ptr(), oxd=j.oxd.ptr()) == EINVAL
    for name, off in (("w", 4), ("w", 8), ("xd", 4), ("xd", 8), ("bias", 2), ("y", 2)):
        assert rc([s], **{name: getattr(hip.gemv_batch_args([s.tuple()]).j[0], name) + off}) == EINVAL, (name, off)
    for name in ("oq", "oxd"):
        assert rc([j], **{name: getattr(hip.gemv_batch_args([j.tuple()]).j[0], name) + 2}) == EINVAL, name
    assert rc([s, j, s], at=2, w=None) == EINVAL and rc([s, j, s, s], at=3, K=48) == EINVAL  # any job of the batch
    assert rc([j], y=None) == OK and rc([s], bias=None) == OK and rc([s, j, s, j]) == OK and kern.value == CHAIN32
    assert L.vsim_op_gemv_batch(hip.gemv_batch_args([s.tuple()]), None, None) == OK  # the out parameter is optional
    torch.cuda.synchronize()


# ------------------------------------------------------------------ wiring
def _f32(m, name, n):
    return dev(m.get_tensor(name, 4 * n).view(np.float32))


def _q4(m, name, rows, k):
    return repack(m.get_tensor(name, rows * k // 32 * 20), rows, k)


def _layer(m, gptj, il, E, F):
    """The layer's tensors: dict of device buffers, None for what the architecture has not."""
    if gptj:
        p = f"transformer.h.{il}."
        t = dict(ln1=(_f32(m, p + "ln_1.weight", E), _f32(m, p + "ln_1.bias", E)), ln2=None,
                 bq=None, bk=None, bv=None, bo=None)
        for k, n in (("wq", "q"), ("wk", "k"), ("wv", "v"), ("wo", "out")):
            t[k] = _q4(m, p + f"attn.{n}_proj.weight", E, E)
        t.update(wfc=_q4(m, p + "mlp.fc_in.weight", F, E), bfc=_f32(m, p + "mlp.fc_in.bias", F),
                 wpr=_q4(m, p + "mlp.fc_out.weight", E, F), bpr=_f32(m, p + "mlp.fc_out.bias", E))
        return t
    p = f"gpt_neox.layers.{il}."
    t = dict(ln1=(_f32(m, p + "input_layernorm.weight", E), _f32(m, p + "input_layernorm.bias", E)),
             ln2=(_f32(m, p + "post_attention_layernorm.weight", E), _f32(m, p + "post_attention_layernorm.bias", E)))
    for k, n in (("q", "query"), ("k", "key"), ("v", "value"), ("o", "dense")):
        t["w" + k] = _q4(m, p + f"attention.{n}.weight", E, E)
        t["b" + k] = _f32(m, p + f"attention.{n}.bias", E)
    t.update(wfc=_q4(m, p + "mlp.dense_h_to_4h.weight", F, E), bfc=_f32(m, p + "mlp.dense_h_to_4h.bias", F),
             wpr=_q4(m, p + "mlp.dense_4h_to_h.weight", E, F), bpr=_f32(m, p + "mlp.dense_4h_to_h.bias", E))
    return t


@pytest.mark.parametrize("name,n_layer", [("tiny-neox", 1), ("tiny-neox", 2), ("tiny-gptj", 1), ("tiny-gptj", 2)])
def test_model_step_is_these_entries_composed(tmp_path, name, n_layer):
    """Tiny models (n_embd = 128), exact mode: the logits of every decode step from n_past = 0 to 5 are
    bit-identical to vsim_op_get_rows, vsim_op_ln_quant (layer 0's norms), then per layer
    vsim_op_gemv_batch {fc_in GELU-quantize, Q, K, V} and vsim_op_tail_ln (with the next layer's
    norms, or the final norm), and vsim_op_q4_gemv for the lm_head, composed on the model's own
    tensors and a KV cache kept here.  A difference means model.cpp wires the launches otherwise
    than the op tests assume."""
    arch_s, hp0 = mg.CONFIGS[name]
    hp = mg.HParams(hp0.n_vocab, hp0.n_embd, hp0.n_head, n_layer, hp0.n_rot, hp0.use_parallel_residual)
    path = str(tmp_path / f"{name}-{n_layer}.bin")
    mg.write_model(path, arch_s, hp, seed=31 + n_layer, std=0.05)
    gptj = arch_s == "gptj"
    n_ctx = 64
    m = hip.Model.load(path, hip.ARCH_GPTJ if gptj else hip.ARCH_GPTNEOX, n_ctx=n_ctx)
    m.set_mode(hip.MODE_EXACT)
    E, V, H, F = hp.n_embd, hp.n_vocab, hp.n_head, 4 * hp.n_embd
    d = E // H
    if gptj:
        wte, lmh = _q4(m, "transformer.wte.weight", V, E), _q4(m, "lm_head.weight", V, E)
        lmh_b = _f32(m, "lm_head.bias", V)
        lnf = (_f32(m, "transformer.ln_f.weight", E), _f32(m, "transformer.ln_f.bias", E))
    else:
        wte, lmh, lmh_b = _q4(m, "gpt_neox.embed_in.weight", V, E), _q4(m, "embed_out.weight", V, E), None
        lnf = (_f32(m, "gpt_neox.final_layer_norm.weight", E), _f32(m, "gpt_neox.final_layer_norm.bias", E))
    layers = [_layer(m, gptj, il, E, F) for il in range(n_layer)]
    scale = float(np.float32(1.0 / np.sqrt(float(np.float32(E) / np.float32(H)))))
    fz = dict(dtype=torch.float32, device=DEV)
    R = [torch.zeros(E, **fz), torch.zeros(E, **fz)]
    Qb, Kb, Vb, xd1, xd2, xda, logits = (torch.zeros(n, **fz) for n in (E, E, E, E, E, E, V))
    xd3 = torch.zeros(F, **fz)
    q1, q2, qa = (torch.zeros(E // 32 * 20, dtype=torch.uint8, device=DEV) for _ in range(3))
    q3 = torch.zeros(F // 32 * 20, dtype=torch.uint8, device=DEV)
    kc = [torch.zeros((n_ctx, E), **fz) for _ in range(n_layer)]
    vc = [torch.zeros((n_ctx, E), **fz) for _ in range(n_layer)]
    kp = [torch.tensor([t.data_ptr()], dtype=torch.int64, device=DEV) for t in kc]
    vp = [torch.tensor([t.data_ptr()], dtype=torch.int64, device=DEV) for t in vc]
    tok_d = torch.zeros(1, dtype=torch.int32, device=DEV)
    np_d = torch.zeros(1, dtype=torch.int32, device=DEV)
    L = hip.lib()
    for n_past in range(6):
        tok = (7 * n_past + 3) % V
        want = m.eval(n_past, [tok])
        tok_d.fill_(tok)
        np_d.fill_(n_past)
        cur = 0
        hip.check(L.vsim_op_get_rows(wte.data_ptr(), E, V, tok_d.data_ptr(), 1, R[cur].data_ptr(), None), "get_rows")
        l0 = layers[0]
        two = l0["ln2"] is not None
        hip.ln_quant(hip.ln_quant_args(R[cur], E, l0["ln1"][0], l0["ln1"][1], q1, xd1,
                                       *((l0["ln2"][0], l0["ln2"][1], q2, xd2) if two else ())))
        for il, t in enumerate(layers):
            kern = hip.gemv_batch([(t["wfc"], F, E, xd2 if two else xd1, t["bfc"], None, 1, q3, xd3),
                                   (t["wq"], E, E, xd1, t["bq"], Qb, 0, None, None),
                                   (t["wk"], E, E, xd1, t["bk"], Kb, 0, None, None),
                                   (t["wv"], E, E, xd1, t["bv"], Vb, 0, None, None)])
            assert kern == CHAIN32
            nxt = layers[il + 1] if il + 1 < n_layer else None
            n1 = nxt["ln1"] if nxt else lnf
            n2 = nxt["ln2"] if nxt and two else None
            a = hip.AttnBatchArgs(hip.ptr(Qb), hip.ptr(Kb), hip.ptr(Vb), hip.ptr(kp[il]), hip.ptr(vp[il]), hip.ptr(np_d),
                                  None, None, 1, d, H, hp.n_rot, 1 if gptj else 0, n_ctx, 1, scale, None, hip.ptr(qa),
                                  hip.ptr(xda))
            hip.tail_ln(hip.tail_ln_args(a, 1, t["wo"], t["wpr"], xd3, F, R[cur], t["bo"], t["bpr"], n1[0], n1[1],
                                         n2[0] if n2 else None, n2[1] if n2 else None, R[cur ^ 1], q1, xd1,
                                         q2 if n2 else None, xd2 if n2 else None, n_past + 1, il))
            cur ^= 1
        hip.check(L.vsim_op_q4_gemv(lmh.data_ptr(), V, E, q1.data_ptr(), xd1.data_ptr(), 1, hip.ptr(lmh_b),
                                    logits.data_ptr(), hip.MODE_EXACT, None), "lm_head")
        got = host(logits)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"{name} x{n_layer}: step at n_past = {n_past} differs"
    m.close()
