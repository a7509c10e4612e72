"""The batched decode step's two kernels through their op entries, bit for bit.

k_gemm_exact_rows (vsim_op_q4_gemm_rows): the exact Q4_0 product for 1..32 activation rows against
the oracle's mul_mat (ggml.c:4891-5165 with its INIT quantization) and against the decode GEMV on
the same device operands.  k_attn_decode_batch (vsim_op_attn_decode_batch): B single-query
attentions, each on a cache and at a position of its own, against the oracle's ops composed per
sequence (rope -> kq -> scale (-> alibi) -> soft_max -> kqv -> quantize_row_q4_0).
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import attn_edges as A  # noqa: E402
from vsim_amd import hip  # noqa: E402
from vsim_amd import modelgen as mg  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
EINVAL = -1


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


def quantize(x, k, n):
    """x: device float32 [n][k] -> (xq Q4 SoA rows, xd factors), vsim_op_q4_quantize."""
    xq = torch.empty(n * k // 32 * 20, dtype=torch.uint8, device=DEV)
    xd = torch.empty(n * k, dtype=torch.float32, device=DEV)
    hip.check(hip.lib().vsim_op_q4_quantize(x.data_ptr(), k, n, xq.data_ptr(), xd.data_ptr(), None), "quantize")
    return xq, xd


# ------------------------------------------------------------------ k_gemm_exact_rows
# one-block K and n = 2; ragged M round the 32-row weight tile and the kernel's 16-row tile; n on
# both sides of 16 (one or two chains per lane), below 4 (one wave computes), not a multiple of 4
# (a wave's last DPP rows idle), 32 (every slot); K = 4096 / 16384: chunked staging and a long
# chain; K = 96 and 64: a last chunk of fewer than four blocks; M = 4096: 256 workgroups
@pytest.mark.parametrize("M,K,n", [(1, 32, 2), (33, 64, 3), (100, 96, 5), (130, 256, 8), (257, 4096, 17),
                                   (96, 16384, 32), (4096, 64, 31), (50, 128, 1)])
def test_gemm_rows_vs_oracle_and_gemv(M, K, n):
    import oracle_py as O
    rng = np.random.default_rng(M * 7 + K * 3 + n)
    w_aos = mg.quantize_q4_0(rng.standard_normal(M * K).astype(np.float32) * np.float32(0.02))
    x = (rng.standard_normal(n * K) * 1.5).astype(np.float32)
    w = repack(w_aos, M, K)
    xq, xd = quantize(dev(x), K, n)
    y = torch.full((n * M,), float("nan"), dtype=torch.float32, device=DEV)
    hip.q4_gemm_rows(w, M, K, xd, n, None, y)
    y_or = O.mul_mat(w_aos, M, K, x, n, nthreads=8).reshape(n, M)
    assert np.array_equal(bits(host(y).reshape(n, M)), bits(y_or))
    b = rng.standard_normal(M).astype(np.float32)
    bd = dev(b)
    yb = torch.full((n * M,), float("nan"), dtype=torch.float32, device=DEV)
    hip.q4_gemm_rows(w, M, K, xd, n, bd, yb)
    assert np.array_equal(bits(host(yb).reshape(n, M)), bits(y_or + b[None, :]))
    # the decode GEMV (n <= 32: chain-GEMV jobs) on the same device operands
    for bias, got in ((None, y), (bd, yb)):
        yg = torch.empty(n * M, dtype=torch.float32, device=DEV)
        hip.check(hip.lib().vsim_op_q4_gemv(w.data_ptr(), M, K, xq.data_ptr(), xd.data_ptr(), n,
                                            None if bias is None else bias.data_ptr(), yg.data_ptr(),
                                            hip.MODE_EXACT, None), "gemv")
        assert np.array_equal(bits(host(yg)), bits(host(got)))


def test_gemm_rows_argument_errors():
    M, K = 32, 64
    w = torch.zeros(hip.q4_bytes(M, K), dtype=torch.uint8, device=DEV)
    xd = torch.zeros(33 * K, dtype=torch.float32, device=DEV)
    y = torch.zeros(33 * M, dtype=torch.float32, device=DEV)
    L = hip.lib()
    assert L.vsim_op_q4_gemm_rows(w.data_ptr(), M, K, xd.data_ptr(), 0, None, y.data_ptr(), None) == EINVAL
    assert L.vsim_op_q4_gemm_rows(w.data_ptr(), M, K, xd.data_ptr(), 33, None, y.data_ptr(), None) == EINVAL
    assert L.vsim_op_q4_gemm_rows(w.data_ptr(), M, 48, xd.data_ptr(), 2, None, y.data_ptr(), None) == EINVAL
    assert L.vsim_op_q4_gemm_rows(w.data_ptr(), M, K, None, 2, None, y.data_ptr(), None) == EINVAL
    assert L.vsim_op_q4_gemm_rows(w.data_ptr(), M, K, xd.data_ptr(), 32, None, y.data_ptr(), None) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------ k_attn_decode_batch
N_CTX = 512


def _reference_row(style, q, k, v, kc, vc, pos, d, H, n_rot, alibi, nth):
    """One sequence's step from the oracle's ops (tests/attn_edges.py reference_row): (out [E], its
    Q4_0 AoS blocks, the K and V cache rows it writes)."""
    return A.reference_row((style, d, H, n_rot, alibi, nth), (q, k, v, kc, vc, pos))


def _launch(style, q, k, v, kcs, vcs, pos, d, H, n_rot, scale, slopes, nth, cs):
    """vsim_op_attn_decode_batch over the rows given (device tensors; kcs / vcs lists of per-row
    caches): (out [B][E], oq AoS bytes [B][E/32*20], oq SoA bytes, oxd [B][E])."""
    B, E = len(pos), d * H
    kp = torch.tensor([t.data_ptr() for t in kcs], dtype=torch.int64, device=DEV)
    vp = torch.tensor([t.data_ptr() for t in vcs], dtype=torch.int64, device=DEV)
    npd = dev(np.asarray(pos, np.int32))
    out = torch.full((B * E,), float("nan"), dtype=torch.float32, device=DEV)
    oq = torch.zeros(B * E // 32 * 20, dtype=torch.uint8, device=DEV)
    oxd = torch.full((B * E,), float("nan"), dtype=torch.float32, device=DEV)
    hip.attn_decode_batch(q, k, v, kp, vp, npd, cs, slopes, B, d, H, n_rot, style, N_CTX, nth, scale, out, oq, oxd)
    aos = torch.empty_like(oq)
    hip.check(hip.lib().vsim_op_act_unpack(oq.data_ptr(), aos.data_ptr(), B, E, None), "act_unpack")
    return host(out).reshape(B, E), host(aos).reshape(B, -1), oq, oxd


# (style, d, H, n_rot, alibi, kqv_nth): both RoPE styles and ALiBi, each head dim with 2 and 3
# heads, the key grouping of --threads 1 and 3
CASES = [(0, 64, 2, 32, False, 1), (0, 96, 3, 24, False, 3), (0, 256, 3, 64, False, 1),
         (1, 256, 2, 64, False, 3), (1, 64, 3, 64, False, 1), (1, 96, 2, 32, False, 1),
         (0, 64, 3, 0, True, 3), (0, 96, 2, 0, True, 1), (0, 256, 2, 0, True, 1)]


@pytest.mark.parametrize("style,d,H,n_rot,alibi,nth", CASES)
def test_attn_decode_batch_vs_oracle(style, d, H, n_rot, alibi, nth):
    E, kt = d * H, 8192 // d  # kt: keys per V tile (ATT_VTF / d)
    rng = np.random.default_rng(1000 * d + 10 * H + n_rot + nth)
    scale = float(A.head_scale(d))
    slopes_h = A.slopes(H) if alibi else None
    slopes = dev(slopes_h) if alibi else None
    cs = None  # the RoPE table is the library's own (vsim_op_rope's, checked against the reference)
    # positions at the kernel's seams: first key, the four-keys-per-wave step, the V tile, deep
    for pos in ([0, 15, 16, 300], [kt - 1, kt, kt + 1, 301]):
        B = len(pos)
        q, k, v = (rng.standard_normal((B, E)).astype(np.float32) for _ in range(3))
        kc_h = [rng.standard_normal((N_CTX, E)).astype(np.float32) for _ in range(B)]
        vc_h = [rng.standard_normal((N_CTX, E)).astype(np.float32) for _ in range(B)]
        for b in range(B):  # nothing at or past a row's position may be read before it is written
            kc_h[b][pos[b]:] = np.nan
            vc_h[b][pos[b]:] = np.nan
        qd, kd, vd = dev(q), dev(k), dev(v)
        kcs, vcs = [dev(a) for a in kc_h], [dev(a) for a in vc_h]
        out, aos, oq, oxd = _launch(style, qd, kd, vd, kcs, vcs, pos, d, H, n_rot, scale, slopes, nth, cs)
        for b in range(B):
            r_out, r_aos, r_k, r_v = _reference_row(style, q[b], k[b], v[b], kc_h[b], vc_h[b], pos[b], d, H, n_rot,
                                                    alibi, nth)
            assert np.array_equal(bits(out[b]), bits(r_out)), (pos[b], "out")
            assert np.array_equal(aos[b], r_aos), (pos[b], "Q4 row")
            assert np.array_equal(bits(host(kcs[b])[pos[b]]), bits(r_k)), (pos[b], "K cache row")
            assert np.array_equal(bits(host(vcs[b])[pos[b]]), bits(r_v)), (pos[b], "V cache row")
            assert np.isnan(host(kcs[b])[pos[b] + 1:]).all() and np.isnan(host(vcs[b])[pos[b] + 1:]).all()
        # the Q4 rows and their factors are vsim_op_q4_quantize's of the float rows
        xq2, xd2 = quantize(dev(out), E, B)
        assert np.array_equal(host(oq), host(xq2))
        assert np.array_equal(bits(host(oxd)), bits(host(xd2)))
        # each row alone (B = 1) on a fresh cache: the same bits as inside the batch
        for b in range(B):
            kc1, vc1 = dev(kc_h[b]), dev(vc_h[b])
            o1, a1, _, x1 = _launch(style, qd[b:b + 1].contiguous(), kd[b:b + 1].contiguous(),
                                    vd[b:b + 1].contiguous(), [kc1], [vc1], [pos[b]], d, H, n_rot, scale, slopes,
                                    nth, cs)
            assert np.array_equal(bits(o1[0]), bits(out[b])) and np.array_equal(a1[0], aos[b])
            assert np.array_equal(bits(host(x1)), bits(host(oxd).reshape(B, E)[b]))
            assert np.array_equal(bits(host(kc1)[pos[b]]), bits(host(kcs[b])[pos[b]]))


def test_attn_decode_batch_argument_errors():
    a = hip.AttnBatchArgs()
    assert hip.lib().vsim_op_attn_decode_batch(a, None) == EINVAL
    z = torch.zeros(64 * 2 * 33, dtype=torch.float32, device=DEV)
    p = torch.zeros(33, dtype=torch.int64, device=DEV)
    n = torch.zeros(33, dtype=torch.int32, device=DEV)
    for B, d in ((0, 64), (33, 64), (1, 48), (1, 512)):
        a = hip.AttnBatchArgs(z.data_ptr(), z.data_ptr(), z.data_ptr(), p.data_ptr(), p.data_ptr(), n.data_ptr(), None,
                              None, B, d, 2, 0, 0, N_CTX, 1, 1.0, None, z.data_ptr(), z.data_ptr())
        assert hip.lib().vsim_op_attn_decode_batch(a, None) == EINVAL, (B, d)
