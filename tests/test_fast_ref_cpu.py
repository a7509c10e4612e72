"""The checkers of tests/fast_ref.py bite (CPU only): the fp64 restatement's own output, rounded
to float as a kernel would leave it, passes every checker, and each of the errors the per-kernel
GPU tests (tests/test_gpu_fast_ops.py) exist to catch fails one.
"""
import numpy as np
import pytest

import fast_ref as R
from vsim_amd import hip
from vsim_amd import modelgen as mg

U = R.U


def _weights(rng, M, K):
    return R.q4_parse(mg.quantize_q4_0(rng.standard_normal(M * K).astype(np.float32) * np.float32(0.05)), K)


def _act(rng, K):
    d, q = R.q4_parse(mg.quantize_q4_0(rng.standard_normal(K).astype(np.float32)), K)
    return d[0], q[0]


def test_q4_pack_parse_roundtrip():
    rng = np.random.default_rng(0)
    aos = mg.quantize_q4_0(rng.standard_normal(3 * 96).astype(np.float32))
    d, q = R.q4_parse(aos, 96)
    assert d.shape == (3, 3) and q.shape == (3, 3, 32) and q.min() >= -8 and q.max() <= 7
    assert np.array_equal(R.q4_pack(d, q), aos)
    d2, q2 = R.q4_quantize_ref(mg.dequantize_q4_0(aos, 96))
    assert np.array_equal(q2.reshape(q.shape), q)  # (quantizing the dequantized row gives its nibbles back)


def test_q4_dot_matches_dequantized_product():
    rng = np.random.default_rng(1)
    M, K = 40, 256
    wd, wq = _weights(rng, M, K)
    xd, xq = _act(rng, K)
    y, a = R.q4_dot(wd, wq, xd, xq)
    W = (wd[:, :, None].astype(np.float64) * wq).reshape(M, K)
    x = (xd[:, None].astype(np.float64) * xq).reshape(K)
    assert np.allclose(y, W @ x, rtol=1e-12, atol=1e-12)
    assert np.all(a >= np.abs(y) - 1e-12)
    # the K splits of fc_out add up
    y0, a0 = R.q4_dot(wd, wq, xd, xq, 0, 4)
    y1, a1 = R.q4_dot(wd, wq, xd, xq, 4, 8)
    assert np.allclose(y0 + y1, y, rtol=1e-12, atol=1e-12) and np.allclose(a0 + a1, a)


def test_gemv_bound_catches_a_dropped_last_block():
    rng = np.random.default_rng(2)
    M, K = 32, 4096
    nb = K // 32
    wd, wq = _weights(rng, M, K)
    xd, xq = _act(rng, K)
    y64, ab = R.q4_dot(wd, wq, xd, xq)
    tol = R.gemv_tol(nb, ab)
    y = y64.astype(np.float32)
    assert R.bound_ratio(y, y64, tol) <= 1.0
    short, _ = R.q4_dot(wd, wq, xd, xq, 0, nb - 1)
    row = int(np.argmax(np.abs(y64 - short)))
    bad = y.copy()
    bad[row] = np.float32(short[row])
    assert R.bound_ratio(bad, y64, tol) > 1.0


def _quantized(rng, n=256):
    y64 = rng.standard_normal(n) * 0.7
    tol = 1e-6 * np.abs(y64) + 1e-7
    d, q = R.q4_quantize_ref(y64.astype(np.float32))
    return y64, tol, d, q


def test_q4_check_passes_the_reference_and_small_perturbations():
    rng = np.random.default_rng(3)
    y64, tol, d, q = _quantized(rng)
    assert R.q4_check(q, d, y64, tol) <= 0.02
    # any y within the tolerance quantizes to something the checker accepts
    for _ in range(20):
        yp = y64 + tol * rng.uniform(-1, 1, y64.size)
        dp, qp = R.q4_quantize_ref(yp.astype(np.float32))
        R.q4_check(qp, dp, y64, tol)


def test_q4_check_catches_one_nibble():
    rng = np.random.default_rng(4)
    y64, tol, d, q = _quantized(rng)
    t = np.abs(y64.reshape(-1, 32)) / (np.abs(y64.reshape(-1, 32)).max(axis=1) / 7.0)[:, None]
    blk, i = np.argwhere(np.abs(t - np.floor(t) - 0.5) > 0.2)[0]  # far from a boundary: unambiguous
    for step in (1, -1):
        bad = q.copy()
        bad[blk, i] += step
        if -8 <= bad[blk, i] <= 7:
            with pytest.raises(AssertionError):
                R.q4_check(bad, d, y64, tol)


def test_q4_check_catches_a_scaled_d():
    rng = np.random.default_rng(5)
    y64, tol, d, q = _quantized(rng)
    bad = d.copy()
    bad[3] = np.float32(bad[3] * np.float32(1.0 + 2.0 ** -10))
    with pytest.raises(AssertionError):
        R.q4_check(q, bad, y64, tol)


def test_gelu_check_passes_the_reference_and_catches_a_nibble():
    e = np.zeros(65536, np.uint16)
    tab = np.zeros(65536, np.uint16)
    hip.check(hip.lib().vsim_op_tables(hip.ptr(e), hip.ptr(tab)), "tables")  # host-built: no GPU
    rng = np.random.default_rng(6)
    s64 = rng.standard_normal(128) * 1.5
    tol = 2e-6 * np.abs(s64) + 1e-7
    g = tab[R.f2h_bits(s64.astype(np.float32))].view(np.float16).astype(np.float32)
    d, q = R.q4_quantize_ref(g)
    share = R.gelu_q4_check(q, d, s64, tol, tab)
    assert share <= 0.05
    bad = q.copy()
    bad[1, 5] += 1 if bad[1, 5] < 7 else -1
    with pytest.raises(AssertionError):
        R.gelu_q4_check(bad, d, s64, tol, tab)


def test_layernorm_ref_normalizes():
    rng = np.random.default_rng(7)
    x = (rng.standard_normal(2176) * 3 + 0.5).astype(np.float32)
    y = R.layernorm_ref(x, np.ones(2176, np.float32), np.zeros(2176, np.float32))
    assert abs(float(y.mean())) < 1e-6 and abs(float(y.astype(np.float64).var()) - 1.0) < 1e-4
    w = rng.standard_normal(2176).astype(np.float32)
    b = rng.standard_normal(2176).astype(np.float32)
    assert np.allclose(R.layernorm_ref(x, w, b), w * y + b, rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("style,d,n_rot", [(1, 256, 64), (0, 128, 32)])
def test_rope_check_catches_a_shifted_partner(style, d, n_rot):
    rng = np.random.default_rng(8)
    v64 = rng.standard_normal(2 * d)
    tol = 1e-6 * np.abs(v64) + 1e-7
    cs = R.rope_table(8, n_rot)
    y64, ty = R.rope_ref(v64, 5, cs, d, n_rot, style, tol=tol)
    assert np.array_equal(y64[n_rot:d], v64[n_rot:d])  # dims past n_rot pass through
    # the kernel's float result of a float input within tol passes
    v = (v64 + 0.5 * tol).astype(np.float32)
    y = R.rope_ref(v, 5, cs, d, n_rot, style).astype(np.float32)
    assert R.bound_ratio(y, y64, ty) <= 1.0
    bad = R.rope_ref(v, 5, cs, d, n_rot, style, shift=1).astype(np.float32)
    assert R.bound_ratio(bad, y64, ty) > 1.0
    # position 0 is the identity
    assert np.array_equal(R.rope_ref(v64, 0, cs, d, n_rot, style), v64)


def _attn_case(rng, d=64, H=2, n_ctx=200, n_past=150):
    E = d * H
    q = rng.standard_normal(E).astype(np.float32) * 2
    kc = rng.standard_normal((n_ctx, E)).astype(np.float32) * 2
    vc = rng.standard_normal((n_ctx, E)).astype(np.float32)
    kc[64:128] *= np.float32(0.05)  # a chunk whose maximum differs from the others'
    return q, kc, vc, n_past, d, H, (n_ctx + 63) // 64, np.float32(1.0 / np.sqrt(d))


def _as_device(r, d, H):
    part = np.concatenate([r["m"][:, :, None], r["l"][:, :, None], r["o"]], axis=2).astype(np.float32)
    od, oq = R.q4_quantize_ref(r["out"].astype(np.float32))
    return part, od, oq


def test_attention_checks_pass_the_reference_and_match_plain_softmax():
    rng = np.random.default_rng(9)
    case = _attn_case(rng)
    q, kc, vc, n_past, d, H, nch, scale = case
    r = R.attn_ref(*case)
    for h in range(H):
        sl = slice(h * d, (h + 1) * d)
        s = kc[:n_past + 1, sl].astype(np.float64) @ q[sl].astype(np.float64) * float(scale)
        p = np.exp(s - s.max())
        assert np.allclose(r["out"][sl], (p / p.sum()) @ vc[:n_past + 1, sl].astype(np.float64), rtol=1e-12, atol=1e-14)
    t = R.attn_tols(r, d, eps_p=4e-6)
    part, od, oq = _as_device(r, d, H)
    assert R.attn_part_check(part, r, t) <= 1.0
    assert R.q4_check(oq, od, r["out"], t["out"]) <= 0.02


@pytest.mark.parametrize("mutation", [dict(own_max_chunk=1), dict(drop_last_key=True)])
def test_attention_checks_catch(mutation):
    rng = np.random.default_rng(10)
    case = _attn_case(rng, n_past=130)
    d, H = case[4], case[5]
    r = R.attn_ref(*case)
    t = R.attn_tols(r, d, eps_p=4e-6)
    bad = R.attn_ref(*case, **mutation)
    part, od, oq = _as_device(bad, d, H)
    with pytest.raises(AssertionError):
        R.q4_check(oq, od, r["out"], t["out"])
    if "drop_last_key" in mutation:  # (a wrong merge weight leaves the partials themselves right)
        with pytest.raises(AssertionError):
            R.attn_part_check(part, r, t)


def test_join_ref_order():
    rng = np.random.default_rng(11)
    x, a, bo, bp = (rng.standard_normal(64) for _ in range(4))
    ffp = rng.standard_normal((4, 64))
    assert np.allclose(R.join_ref(x, a, bo, ffp, bp), x + a + bo + ffp.sum(0) + bp)
    assert np.allclose(R.join_ref(x, a, None, ffp, bp), x + a + ffp.sum(0) + bp)
