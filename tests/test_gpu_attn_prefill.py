"""The fast prompt attention path as the model's prompt layer runs it (run_layer, kv16_epi): the
K and V GEMMs' fp16 side copies (gemm_f16.hip: G2Epi::h16 row-major, h16_t transposed in vt_pos
order), k_kv_f16's conversion of the cached keys around a fresh range, and the attention kernels
on the caller's scratch -- each through its op entry, against tests/attn_ref.py.

* the copies are bit-equal to fp16 of the GEMM's own f32 output, nothing else of the buffer is
  touched (ragged N, unaligned p0, both dequant kernels, the pair launch, the stream-K finisher);
* k_kv_f16 gives exactly attn_ref.kv_images of the cache, zero padding included, and with a fresh
  range leaves exactly that range alone;
* GEMM copies + fresh attention are bit-identical to the attention converting the whole cache;
* the attention is held per element to the derived bound of attn_ref (and to the older
  2e-2 max|V| against unrounded fp64), at a flat and a peaked score scale, both fresh settings;
* a structural case whose answer is known exactly (the diagonal key's value);
* a long GPT-J prompt batch on top of an existing cache against the oracle.
"""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import attn_ref as R  # noqa: E402
from test_gpu_ops import DEV, dev, host, repack  # noqa: E402
from vsim_amd import hip  # noqa: E402
from vsim_amd import modelgen as mg  # noqa: E402

pytestmark = pytest.mark.gpu

SENT = 0x3555   # fp16 0.333: "written by the GEMM epilogue" / "never written"
JUNK = 0x7BFF   # fp16 65504: what a reused scratch may hold


def layout(E, nk):
    b, o, l = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_int()
    hip.check(hip.lib().vsim_op_attn_prefill_layout(E, nk, ctypes.byref(b), ctypes.byref(o), ctypes.byref(l)), "layout")
    assert l.value == R.ldt_of(nk) and b.value == 2 * (o.value + E * l.value) and o.value >= nk * E
    return b.value, o.value, l.value


def rope_cs(n_pos, n_rot):
    half = n_rot // 2
    theta = np.arange(n_pos, dtype=np.float64)[:, None] * 10000.0 ** (-2.0 * np.arange(half) / n_rot)[None, :]
    return dev(np.ascontiguousarray(np.stack([np.cos(theta), np.sin(theta)], axis=-1)))


def q4_weight(rng, M, K):
    return repack(mg.quantize_q4_0(rng.standard_normal(M * K).astype(np.float32) * np.float32(0.05)), M, K)


def halves(n, fill):
    return torch.full((n,), fill, dtype=torch.int16, device=DEV)


def vt_index(p0, n):
    return torch.from_numpy(R.vt_pos(p0 + np.arange(n)).astype(np.int64)).to(DEV)


def k_copy_ok(buf, y, M, N, p0):
    """buf [rows][M] int16: rows p0 .. p0 + N are fp16(y), every other half still SENT."""
    want = torch.full_like(buf, SENT).view(-1, M)
    want[p0:p0 + N] = y.view(N, M).to(torch.float16).view(torch.int16)
    return torch.equal(buf.view(-1, M), want)


def vt_copy_ok(buf, y, M, N, p0, ld):
    want = torch.full_like(buf, SENT).view(M, ld)
    want[:, vt_index(p0, N)] = y.view(N, M).to(torch.float16).view(torch.int16).t()
    return torch.equal(buf.view(M, ld), want)


def gemm_k(L, w, M, K, x, N, bias, cs, d, n_rot, p0, y=None, h16=None):
    """The K projection: RoPE epilogue, row-major copy.  Returns y, the copy buffer."""
    y = torch.empty(N * M, device=DEV) if y is None else y
    buf = halves((p0 + N + 3) * M, SENT) if h16 is None else h16
    hip.check(L.vsim_op_gemm_q4_256_h16(w.data_ptr(), M, K, x.data_ptr(), N, bias, y.data_ptr() if torch.is_tensor(y) else y,
                                        cs.data_ptr(), d, n_rot, p0, buf.data_ptr() if torch.is_tensor(buf) else buf, 0, 0,
                                        None), "gemm K copy")
    return y, buf


def gemm_v(L, w, M, K, x, N, bias, p0, ld, y=None, h16=None):
    """The V projection: plain epilogue, transposed copy."""
    y = torch.empty(N * M, device=DEV) if y is None else y
    buf = halves(M * ld, SENT) if h16 is None else h16
    hip.check(L.vsim_op_gemm_q4_256_h16(w.data_ptr(), M, K, x.data_ptr(), N, bias, y.data_ptr() if torch.is_tensor(y) else y,
                                        None, 0, 0, p0, buf.data_ptr() if torch.is_tensor(buf) else buf, ld, 1, None),
              "gemm V^T copy")
    return y, buf


@pytest.mark.parametrize("N,p0", [(N, p0) for N in (257, 300) for p0 in (0, 4, 37, 64)])
@pytest.mark.parametrize("d,K", [(128, 128), (128, 192), (256, 128), (256, 192)])
def test_gemm_fp16_copies(d, K, N, p0):
    """M = 512: two row tiles; N: two column tiles, the second ragged (257: one column; 300: a
    run of 8 cut at 4); p0 = 4, 37: every V^T run of 8 on the scalar path, 0 / 64: the aligned
    quads; K = 128 the register-dequant kernel (and the pair launch), 192 the in-LDS one."""
    M, n_rot = 512, 64
    rng = np.random.default_rng(d + K + N + p0)
    L = hip.lib()
    w0, w1 = q4_weight(rng, M, K), q4_weight(rng, M, K)
    x = dev((rng.standard_normal((N, K)) * 0.5).astype(np.float16))
    b = dev((rng.standard_normal(M) * 0.1).astype(np.float32))
    cs = rope_cs(p0 + N, n_rot)
    ld = R.ldt_of(p0 + N)
    for bias in (None, b.data_ptr()):
        yk, bk = gemm_k(L, w1, M, K, x, N, bias, cs, d, n_rot, p0)
        yv, bv = gemm_v(L, w1, M, K, x, N, bias, p0, ld)
        y0k, y0v = torch.empty(N * M, device=DEV), torch.empty(N * M, device=DEV)
        hip.check(L.vsim_op_gemm_q4_256(w1.data_ptr(), M, K, x.data_ptr(), N, bias, y0k.data_ptr(), None, cs.data_ptr(),
                                        d, n_rot, p0, 0, None, None), "gemm rope")
        hip.check(L.vsim_op_gemm_q4_256(w1.data_ptr(), M, K, x.data_ptr(), N, bias, y0v.data_ptr(), None, None, 0, 0, 0,
                                        0, None, None), "gemm")
        torch.cuda.synchronize()
        assert k_copy_ok(bk, yk, M, N, p0), f"K copy, bias {bias is not None}"
        assert vt_copy_ok(bv, yv, M, N, p0, ld), f"V^T copy, bias {bias is not None}"
        assert torch.equal(yk.view(torch.int32), y0k.view(torch.int32)), "y with the K copy"
        assert torch.equal(yv.view(torch.int32), y0v.view(torch.int32)), "y with the V^T copy"
    if K % 128 == 0:  # the paired Q / K launch: the copy rides on the second weight only
        yq, yk2 = torch.empty(N * M, device=DEV), torch.empty(N * M, device=DEV)
        bk2 = halves((p0 + N + 3) * M, SENT)
        hip.check(L.vsim_op_gemm_q4_256_pair_h16(w0.data_ptr(), w1.data_ptr(), M, K, x.data_ptr(), N, yq.data_ptr(),
                                                 yk2.data_ptr(), cs.data_ptr(), d, n_rot, p0, bk2.data_ptr(), None), "pair")
        yk, _ = gemm_k(L, w1, M, K, x, N, None, cs, d, n_rot, p0)
        yq1, _ = gemm_k(L, w0, M, K, x, N, None, cs, d, n_rot, p0)
        torch.cuda.synchronize()
        assert k_copy_ok(bk2, yk2, M, N, p0), "pair: K copy"
        assert torch.equal(yk2.view(torch.int32), yk.view(torch.int32)), "pair: y1"
        assert torch.equal(yq.view(torch.int32), yq1.view(torch.int32)), "pair: y0"


def test_gemm_fp16_copies_streamk():
    """A grid of at least half and fewer than 3/4 of the CUs with K >= 256 (two K units): both
    epilogues split every tile between two workgroups and the finisher writes the copy.  Split
    or not, each copy is fp16 of the y of its own run."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    N, K, d, n_rot, p0 = 2048, 256, 256, 64, 40
    M = 256 * -(-cus // 16)  # 8 column tiles: M / 256 * 8 >= cus / 2
    tiles = M // 256 * 8
    assert cus <= 2 * tiles and 4 * tiles < 3 * cus, (cus, tiles)
    rng = np.random.default_rng(cus)
    L = hip.lib()
    w = q4_weight(rng, M, K)
    x = dev((rng.standard_normal((N, K)) * 0.5).astype(np.float16))
    b = dev((rng.standard_normal(M) * 0.1).astype(np.float32))
    cs = rope_cs(p0 + N, n_rot)
    ld = R.ldt_of(p0 + N)
    ys = {}
    was = L.vsim_gemm_set_streamk(1)
    try:
        for sk in (0, 1):
            L.vsim_gemm_set_streamk(sk)
            yk, bk = gemm_k(L, w, M, K, x, N, None, cs, d, n_rot, p0)
            yv, bv = gemm_v(L, w, M, K, x, N, b.data_ptr(), p0, ld)
            torch.cuda.synchronize()
            assert k_copy_ok(bk, yk, M, N, p0), f"K copy, stream-K {sk}"
            assert vt_copy_ok(bv, yv, M, N, p0, ld), f"V^T copy, stream-K {sk}"
            ys[sk] = (yk, yv)
    finally:
        L.vsim_gemm_set_streamk(was)
    for a, c in zip(ys[0], ys[1]):  # (the split really ran: another summation order)
        assert int((a != c).sum()) > 0
        assert bool(((a - c).abs() <= 1e-3).all())


KV_CASES = [(0, 64), (0, 9), (1, 8), (37, 200), (62, 9), (64, 257), (130, 64)]


@pytest.mark.parametrize("n_past,N", KV_CASES)
@pytest.mark.parametrize("d,H", [(64, 2), (256, 1)])
def test_kv_f16_images(d, H, n_past, N):
    """k_kv_f16 through the attention on a caller's scratch.  fresh off: K16 rows [0, nk) and the
    whole V^T area are attn_ref.kv_images of the cache (zero padding included); K16 rows
    [nk, ldt) are never written.  fresh on: the range [n_past, nk) keeps what was there, every
    other key is converted, the padding is zero -- whole fresh 64-key blocks (skipped), 4-key
    groups that straddle n_past or nk (element by element), the launch skipped altogether for
    (0, 64)."""
    E, nk = d * H, n_past + N
    rng = np.random.default_rng(d + 3 * n_past + N)
    Q = rng.standard_normal((N, E)).astype(np.float32)
    K = rng.standard_normal((nk, E)).astype(np.float32)
    V = rng.standard_normal((nk, E)).astype(np.float32)
    q_, k_, v_ = dev(Q), dev(K), dev(V)
    nbytes, vt_off, ldt = layout(E, nk)
    scale = float(np.float32(1.0 / np.sqrt(d)))
    out = torch.empty(N * E, device=DEV)
    L = hip.lib()
    wk, wv = R.kv_images(K, V, d)

    def run(scr, fresh):
        hip.check(L.vsim_op_attn_prefill_scratch(q_.data_ptr(), k_.data_ptr(), v_.data_ptr(), d, H, N, n_past, scale,
                                                 out.data_ptr(), None, scr.data_ptr(), nbytes, fresh, None), "attn")
        s = host(scr).view(np.uint16)
        return s[:ldt * E].reshape(ldt, E), s[vt_off:vt_off + E * ldt].reshape(H, d, ldt)

    k16, vt = run(halves(nbytes // 2, JUNK), 0)
    assert R.images_mismatch(k16.view(np.float16), vt.view(np.float16), K, V, d) is None
    assert (k16[nk:] == JUNK).all()
    # fresh: the epilogues' halves (SENT) among a reused scratch's junk
    want_k = np.full((ldt, E), JUNK, np.uint16)
    want_k[:n_past] = wk[:n_past].view(np.uint16)
    want_k[n_past:nk] = SENT
    want_v = wv.view(np.uint16).copy()
    want_v[:, :, R.vt_pos(np.arange(n_past, nk))] = SENT
    init_k = np.full((ldt, E), JUNK, np.uint16)
    init_k[n_past:nk] = SENT
    init_v = np.full((H, d, ldt), JUNK, np.uint16)
    init_v[:, :, R.vt_pos(np.arange(n_past, nk))] = SENT
    scr = np.full(nbytes // 2, JUNK, np.uint16)
    scr[:ldt * E] = init_k.reshape(-1)
    scr[vt_off:vt_off + E * ldt] = init_v.reshape(-1)
    k16, vt = run(dev(scr.view(np.int16)), 1)
    assert np.array_equal(k16, want_k), "K16 with a fresh range"
    bad = np.argwhere(vt != want_v)
    assert bad.size == 0, f"V^T with a fresh range: {len(bad)} halves, first (head, dim, position) {bad[0].tolist()}"


@pytest.mark.parametrize("n_past", [0, 37, 200])
@pytest.mark.parametrize("d", [64, 128, 256])
def test_fresh_composition_bit_identical(d, n_past):
    """run_layer's composition on the op entries: K (RoPE; through the pair launch for n_past =
    37) and V from the GEMMs into cache rows [n_past, nk) and into the scratch, then the
    attention with fresh = true.  The scratch then holds exactly the images of the whole cache,
    and the result has the bits of vsim_op_attn_prefill / _q16 on the same caches."""
    E, N, n_rot = 512, 300, 64
    H, nk = E // d, n_past + N
    rng = np.random.default_rng(d + n_past)
    L = hip.lib()
    wq, wk, wv = (q4_weight(rng, E, E) for _ in range(3))
    x = dev((rng.standard_normal((N, E)) * 0.5).astype(np.float16))
    cs = rope_cs(nk, n_rot)
    kc = dev((rng.standard_normal((nk, E)) * 0.6).astype(np.float32))
    vc = dev((rng.standard_normal((nk, E)) * 0.6).astype(np.float32))
    nbytes, vt_off, ldt = layout(E, nk)
    scr = halves(nbytes // 2, JUNK)
    row = n_past * E * 4
    qb = torch.empty(N * E, device=DEV)
    if n_past == 37:
        hip.check(L.vsim_op_gemm_q4_256_pair_h16(wq.data_ptr(), wk.data_ptr(), E, E, x.data_ptr(), N, qb.data_ptr(),
                                                 kc.data_ptr() + row, cs.data_ptr(), d, n_rot, n_past, scr.data_ptr(),
                                                 None), "pair")
    else:
        hip.check(L.vsim_op_gemm_q4_256(wq.data_ptr(), E, E, x.data_ptr(), N, None, qb.data_ptr(), None, cs.data_ptr(), d,
                                        n_rot, n_past, 0, None, None), "gemm Q")
        gemm_k(L, wk, E, E, x, N, None, cs, d, n_rot, n_past, y=kc.data_ptr() + row, h16=scr)
    gemm_v(L, wv, E, E, x, N, None, n_past, ldt, y=vc.data_ptr() + row, h16=scr.data_ptr() + 2 * vt_off)
    scale = float(np.float32(1.0 / np.sqrt(d)))
    a, b = torch.empty(N * E, device=DEV), torch.empty(N * E, device=DEV)
    hip.check(L.vsim_op_attn_prefill_scratch(qb.data_ptr(), kc.data_ptr(), vc.data_ptr(), d, H, N, n_past, scale,
                                             a.data_ptr(), None, scr.data_ptr(), nbytes, 1, None), "attn fresh")
    hip.check(L.vsim_op_attn_prefill(qb.data_ptr(), kc.data_ptr(), vc.data_ptr(), d, H, N, n_past, scale, b.data_ptr(),
                                     None), "attn")
    torch.cuda.synchronize()
    s = host(scr).view(np.float16)
    msg = R.images_mismatch(s[:ldt * E].reshape(ldt, E), s[vt_off:vt_off + E * ldt].reshape(H, d, ldt), host(kc), host(vc), d)
    assert msg is None, msg
    assert not bool(torch.isnan(b).any())
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    if d == 256:
        a16, b16 = halves(N * E, SENT), halves(N * E, JUNK)
        hip.check(L.vsim_op_attn_prefill_scratch(qb.data_ptr(), kc.data_ptr(), vc.data_ptr(), d, H, N, n_past, scale,
                                                 None, a16.data_ptr(), scr.data_ptr(), nbytes, 1, None), "q16 fresh")
        hip.check(L.vsim_op_attn_prefill_q16(qb.data_ptr(), kc.data_ptr(), vc.data_ptr(), d, H, N, n_past, scale,
                                             b16.data_ptr(), None), "q16")
        torch.cuda.synchronize()
        assert torch.equal(a16, b16)


@pytest.mark.parametrize("qmul", [1.0, 8.0], ids=["flat", "peaked"])
@pytest.mark.parametrize("d,H,N,n_past", [(256, 2, 200, 0), (256, 3, 300, 37), (256, 1, 64, 130), (256, 2, 1100, 40),
                                           (128, 3, 130, 17), (96, 2, 64, 5), (64, 4, 9, 40), (128, 1, 257, 100),
                                           (64, 1, 300, 130)])
def test_attn_prefill_bound(d, H, N, n_past, qmul):
    """Per element |y - ref16| <= c 2^-11 A + T (attn_ref's derivation; ref16 the float64
    attention of the operands as the kernel rounds them), and the 2e-2 max|V| tier against the
    unrounded float64 attention.  fresh off converts the whole cache; fresh on finds the new
    keys' images in a scratch of junk, as the GEMM epilogues leave them."""
    E, nk = d * H, n_past + N
    rng = np.random.default_rng(d + N + n_past)
    Q = (rng.standard_normal((N, E)) * qmul).astype(np.float32)
    K = rng.standard_normal((nk, E)).astype(np.float32)
    V = rng.standard_normal((nk, E)).astype(np.float32)
    scale = float(np.float32(1.0 / np.sqrt(d)))
    ref = R.Ref(Q, K, V, d, n_past, scale)
    q_, k_, v_ = dev(Q), dev(K), dev(V)
    nbytes, vt_off, ldt = layout(E, nk)
    wk, wv = R.kv_images(K, V, d)
    scr = np.full(nbytes // 2, JUNK, np.uint16)
    k_img = scr[:ldt * E].reshape(ldt, E)
    v_img = scr[vt_off:vt_off + E * ldt].reshape(H, d, ldt)
    k_img[n_past:nk] = wk[n_past:].view(np.uint16)
    pos = R.vt_pos(np.arange(n_past, nk))
    v_img[:, :, pos] = wv.view(np.uint16)[:, :, pos]
    ratios = []
    for fresh, s in ((0, halves(nbytes // 2, JUNK)), (1, dev(scr.view(np.int16)))):
        out = torch.full((N * E,), float("nan"), device=DEV)
        hip.check(hip.lib().vsim_op_attn_prefill_scratch(q_.data_ptr(), k_.data_ptr(), v_.data_ptr(), d, H, N, n_past,
                                                         scale, out.data_ptr(), None, s.data_ptr(), nbytes, fresh, None),
                  "attn")
        y = host(out).reshape(N, E)
        r = ref.ratio(y)
        ratios.append(r)
        print(f"d {d} H {H} N {N} n_past {n_past} Q x {qmul:g} fresh {fresh}: max |y - ref16| / (c 2^-11 A + T) = {r:.3f}"
              f" (c {ref.c.min():.2f} .. {ref.c.max():.2f})")
        ref.check(y, f"fresh {fresh}")
    assert ratios[0] == ratios[1], "the two fresh settings read the same images"


@pytest.mark.parametrize("d", [64, 128, 256])
def test_attn_prefill_selects_the_diagonal(d):
    """A case with a known answer.  Dim 0 of each head holds the key's index j and 40 / qs for
    every query, so a score is 40 j bits plus noise of a few bits from the other dims: each
    query's own key (j = n_past + q) outweighs the one before by more than 2^-30, and key
    n_past + q + 1, 40 bits more attractive still, is masked.  V[j][dim] = j + dim (exact in
    fp16).  The output is the diagonal key's value, bit for bit: the others' total weight is
    below 2^-29, less than half an ulp of any output.  N = 300 at n_past = 63: the diagonal
    crosses every 64-key and 128-query boundary at every offset."""
    H, N, n_past = 2, 300, 63
    E, nk = d * H, n_past + N
    rng = np.random.default_rng(d)
    scale = float(np.float32(1.0 / np.sqrt(d)))
    qs = float(np.float32(scale) * R.LOG2E_F32)
    Q = (rng.standard_normal((N, E)) * 0.05 / qs).astype(np.float32)
    K = rng.standard_normal((nk, E)).astype(np.float32)
    Q[:, ::d] = 40.0 / qs
    K[:, ::d] = np.arange(nk)[:, None]
    V = (np.arange(nk)[:, None] + (np.arange(E) % d)[None, :]).astype(np.float32)
    q16 = R.q16_of(Q, scale)
    assert (q16[:, ::d] == 40).all()
    want = V[n_past:]
    # (the construction holds: in float64 the others move no output by 2^-27 of itself)
    assert float(np.max(np.abs(R.attention(Q, K, V, d, n_past, scale)[0] - want) / want)) < 2.0 ** -27
    out = torch.full((N * E,), float("nan"), device=DEV)
    q_, k_, v_ = dev(Q), dev(K), dev(V)
    hip.check(hip.lib().vsim_op_attn_prefill(q_.data_ptr(), k_.data_ptr(), v_.data_ptr(), d, H, N, n_past, scale,
                                             out.data_ptr(), None), "attn")
    y = host(out).reshape(N, E)
    bad = np.argwhere(y != want)
    assert bad.size == 0, f"{len(bad)} outputs are not the diagonal key's, first (query, column) {bad[0].tolist()}: " \
                          f"{y[tuple(bad[0])]} for {want[tuple(bad[0])]}"


@pytest.mark.parametrize("H", [4, 2])
def test_long_prompt_on_a_cache_vs_oracle(H, tmp_path):
    """GPT-J, E = 512, fast mode: 37 tokens, then a 300-token batch on top of them (the GEMM
    epilogues' copies at p0 = 37, k_kv_f16 around them), against the oracle doing the same two
    evals; the bounds of tests/test_gpu_prefill.py, unedited.  H = 2: head dim 256."""
    import oracle_py as O
    from test_gpu_prefill import FAST_COS_MIN, NTH, stats
    hp = mg.HParams(512, 512, H, 2, 64)
    path = str(tmp_path / f"gptj-h{H}.bin")
    mg.write_model(path, "gptj", hp, seed=5, std=0.05)
    res = []
    for seed in range(4):
        ids = [int(v) for v in np.random.default_rng(100 + seed).integers(0, hp.n_vocab, 337)]
        om = O.Model(path, hip.ARCH_GPTJ)
        dm = hip.Model.load(path, hip.ARCH_GPTJ)
        dm.set_mode(hip.MODE_FAST)
        om.eval(0, ids[:37], nthreads=NTH)
        dm.eval(0, ids[:37])
        lo, lf = om.eval(37, ids[37:], nthreads=NTH), dm.eval(37, ids[37:])
        dm.close()
        res.append(stats(lf, lo))
    msg = f"GPT-J E 512 H {H}, 300 tokens at n_past 37: cos {['%.5f' % r[0] for r in res]}, " \
          f"top-1 {sum(r[2] for r in res)}/4, in the oracle's top 5 {sum(r[3] for r in res)}/4"
    print(msg)
    assert min(r[0] for r in res) >= FAST_COS_MIN, msg
    assert all(r[3] for r in res), msg
