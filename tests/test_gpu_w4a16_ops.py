"""The weight-only mode's two kernels through their op entries (vsim_op_w4a16_rows,
vsim_op_q4_gemm_w4a16_rows), against tests/w4a16_ref.py:

* the row operand (fp16 bits and exponent) is the restatement's, bit for bit, for every row family;
* the product lies within the derived bound of the fp64 evaluation of the same formula on the same
  operand, at every shape where the kernel takes another path;
* a row's outputs are the same bits whatever n is, wherever the row stands and whatever stands
  beside it -- NaN and Inf rows included;
* nothing behind the weight or behind row n - 1 is read; the argument errors.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import fast_ref as R  # noqa: E402
import w4a16_ref as W  # noqa: E402
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


def repack(aos_np, rows, k, slack=0):
    """W4T32 image of the AoS blocks at the front of a buffer of q4_bytes + slack bytes; the slack
    is NaN-patterned."""
    src = dev(aos_np)
    dst = torch.full((hip.q4_bytes(rows, k) + slack,), 0xFF, dtype=torch.uint8, device=DEV)
    hip.check(hip.lib().vsim_op_q4_repack(src.data_ptr(), dst.data_ptr(), rows, k, None), "repack")
    return dst


def operand(x, n, K):
    """vsim_op_w4a16_rows of the first n rows of the device tensor x, into buffers of exactly n rows
    followed by one guard row; returns (x16 device, e device, h numpy [n][K], e numpy [n])."""
    x16 = torch.full(((n + 1) * K,), 7.0, dtype=torch.float16, device=DEV)
    e = torch.full((n + 1,), 12345, dtype=torch.int32, device=DEV)
    hip.w4a16_rows(x, K, n, x16, e)
    hh, eh = host(x16).reshape(n + 1, K), host(e)
    assert (hh[n] == 7.0).all() and eh[n] == 12345, "operand rows >= n written"
    return x16, e, hh[:n], eh[:n]


def product(w, M, K, x16, e, n, bias, rows=33):
    """The entry on a NaN-prefilled y of `rows` rows."""
    y = torch.full((rows * M,), float("nan"), dtype=torch.float32, device=DEV)
    hip.q4_gemm_w4a16_rows(w, M, K, x16, e, n, bias, y)
    out = host(y).reshape(rows, M)
    assert np.isnan(out[n:]).all(), "rows >= n written"
    return out[:n]


def weights(M, K, seed):
    rng = np.random.default_rng(seed)
    aos = mg.quantize_q4_0(rng.standard_normal(M * K).astype(np.float32) * np.float32(0.02))
    b = rng.standard_normal(M).astype(np.float32)
    return aos, b


def families(K, seed):
    """32 rows: random rows of several scales, one 1e30 outlier among O(1) values, f32 subnormals, an
    all-zero row, a row of -0.0, a NaN row and an Inf row between finite rows."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((32, K)) * 1.5).astype(np.float32)
    x[1] *= np.float32(1e-6)
    x[2] *= np.float32(3e4)
    x[3, K // 2] = 1e30
    x[4] = np.float32(1e-40) * rng.standard_normal(K).astype(np.float32)
    x[5] = 0.0
    x[6] = -0.0
    x[8, 3] = np.nan
    x[10, K - 1] = np.inf
    x[11] = x[7]                       # (a duplicate of a finite row: same bits expected)
    x[12, 0] = -np.inf
    x[12, 1] = np.nan
    x[13, :K - 1] = 0.0                # one non-zero element, the last
    x[14] = np.float32(-65504.0)
    x[15] = np.float32(1.0e36) * np.sign(x[15])   # large, the products still finite
    return x


BAD_ROWS = (8, 10, 12)


@pytest.mark.parametrize("K", [32, 64, 544, 1056])
def test_operand_bits(K):
    x = families(K, K)
    _, _, h, e = operand(dev(x), 32, K)
    hr, er = W.row_operand(x)
    assert np.array_equal(e, er), (e, er)
    assert np.array_equal(h.view(np.uint16), hr.view(np.uint16)), np.argwhere(h.view(np.uint16) != hr.view(np.uint16))[:5]
    assert all(er[j] == W.NONFINITE for j in BAD_ROWS) and (er != W.NONFINITE).sum() == 32 - len(BAD_ROWS)
    assert ((np.abs(hr[3]) < 2.0 ** -14).sum() == K - 1) and er[4] > 127   # the families do what they say
    # a row alone, and rows at other indices: the same bits
    for j in (0, 3, 4, 8, 31):
        _, _, h1, e1 = operand(dev(x[j:j + 1]), 1, K)
        assert e1[0] == er[j] and np.array_equal(h1[0].view(np.uint16), hr[j].view(np.uint16)), j
    perm = np.random.default_rng(K).permutation(32)[:17]
    _, _, hp, ep = operand(dev(x[perm]), 17, K)
    assert np.array_equal(ep, er[perm]) and np.array_equal(hp.view(np.uint16), hr[perm].view(np.uint16))
    # rows at a 4-byte aligned address take the scalar form of the kernel (the aligned ones above the
    # float4 form): the same bits
    buf = torch.zeros(32 * K + 1, dtype=torch.float32, device=DEV)
    buf[1:] = dev(x).reshape(-1)
    assert buf[1:].data_ptr() % 16 == 4
    _, _, hm, em = operand(buf[1:], 32, K)
    assert np.array_equal(em, er) and np.array_equal(hm.view(np.uint16), hr.view(np.uint16))


# M: half a tile, a ragged last tile, several tiles.  K: one block (fifteen empty partials), fewer
# blocks than partials, 17 and 33 blocks (ragged partial counts on both sides of P = 16, and a
# second trip of the two-block loop).  n round the MFMA's 16 columns.
@pytest.mark.parametrize("K", [32, 64, 544, 1056])
@pytest.mark.parametrize("M", [16, 40, 96])
def test_product_bound_and_row_independence(M, K):
    aos, b = weights(M, K, M * 7 + K)
    w, bd = repack(aos, M, K), dev(b)
    wd, wq = R.q4_parse(aos, K)
    x = families(K, M + K)
    xd_ = dev(x)
    x16, e, h, eh = operand(xd_, 32, K)
    hr, er = W.row_operand(x)
    assert np.array_equal(eh, er) and np.array_equal(h.view(np.uint16), hr.view(np.uint16))
    y64, tol = W.product64(wd, wq, hr, er)           # computed once, shared by every n below
    y64b, tolb = W.product64(wd, wq, hr, er, b)
    good = np.array([j for j in range(32) if j not in BAD_ROWS])
    full, fullb = product(w, M, K, x16, e, 32, None), product(w, M, K, x16, e, 32, bd)
    per_row = np.maximum(np.abs(full[good] - y64[good]) / tol[good], np.abs(fullb[good] - y64b[good]) / tolb[good]).max(axis=1)
    worst = float(per_row.max())
    print(f"gemm_w4a16_rows M={M} K={K}: worst error {worst:.4f} x bound (row {good[per_row.argmax()]}; "
          f"random rows {per_row[[0, 7, 9]].max():.4f})")
    assert worst <= 1.0
    for j in BAD_ROWS:  # the non-finite rule, and nothing else touched
        assert (bits(full[j]) == W.QNAN_BITS).all() and (bits(fullb[j]) == W.QNAN_BITS).all(), j
    assert np.isfinite(full[good]).all()
    assert not full[5].any() and not full[6].any()    # zero rows: +0 or -0 sums, no NaN
    assert np.array_equal(bits(full[11]), bits(full[7]))
    # every n: the first n rows' bits are those of the n = 32 launch
    for n in (1, 15, 16, 17):
        assert np.array_equal(bits(product(w, M, K, x16, e, n, None)), bits(full[:n])), n
        assert np.array_equal(bits(product(w, M, K, x16, e, n, bd)), bits(fullb[:n])), n
    # every row alone (its own operand launch too), and rows at other indices beside other rows
    for j in range(32):
        x1, e1, _, _ = operand(xd_[j:j + 1].contiguous(), 1, K)
        assert np.array_equal(bits(product(w, M, K, x1, e1, 1, bd, rows=2)[0]), bits(fullb[j])), j
    perm = np.random.default_rng(M + K).permutation(32)
    for n in (32, 17):
        xp, ep, _, _ = operand(dev(x[perm[:n]]), n, K)
        assert np.array_equal(bits(product(w, M, K, xp, ep, n, None)), bits(full[perm[:n]])), n


def test_nothing_read_behind_the_operands():
    M, K, n = 40, 544, 5
    aos, b = weights(M, K, 1)
    x = families(K, 2)[:n]
    bd = dev(b)
    x16, e, _, _ = operand(dev(x), n, K)
    want = product(repack(aos, M, K), M, K, x16, e, n, bd)
    # a NaN-patterned region behind the weight; x with NaN rows behind row n - 1; the operand's own
    # guard row (7.0) replaced by NaN
    xg = np.concatenate([x, np.full((3, K), np.nan, np.float32)])
    x16g, eg, _, _ = operand(dev(xg), n, K)
    x16g[n * K:] = float("nan")
    got = product(repack(aos, M, K, slack=4096), M, K, x16g, eg, n, bd)
    assert np.array_equal(bits(got), bits(want))


def test_subnormal_operands_count():
    """Does the matrix core take fp16 subnormal inputs at their value?  The case's product is made of
    subnormal h alone; a core that flushed them would give zeros (w4a16_ref's flag says which rule
    the restatement follows, and test_w4a16_ref_cpu.py shows the two rules are far apart)."""
    wd, wq, x, _ = W.subnormal_case()
    M, K = wd.shape[0], wd.shape[1] * 32
    w = repack(R.q4_pack(wd, wq), M, K)
    x16, e, h, eh = operand(dev(x), 1, K)
    hr, er = W.row_operand(x)
    assert np.array_equal(h.view(np.uint16), hr.view(np.uint16)) and eh[0] == er[0]
    y = product(w, M, K, x16, e, 1, None, rows=2)
    y64, tol = W.product64(wd, wq, hr, er)
    kept = W.bound_ratio(y, y64, tol)
    print(f"subnormal operands: {kept:.4f} x bound with subnormals kept; outputs {y[0][:4]} against {y64[0][:4]}")
    assert W.MFMA_KEEPS_F16_SUBNORMALS and np.abs(y64).min() > 0 and kept <= 1.0


def test_argument_errors():
    M, K = 32, 64
    w = torch.zeros(hip.q4_bytes(M, K), dtype=torch.uint8, device=DEV)
    x = torch.zeros(33 * K, dtype=torch.float32, device=DEV)
    x16 = torch.zeros(33 * K, dtype=torch.float16, device=DEV)
    e = torch.zeros(33, dtype=torch.int32, device=DEV)
    y = torch.zeros(33 * M, dtype=torch.float32, device=DEV)
    f, g = hip.lib().vsim_op_w4a16_rows, hip.lib().vsim_op_q4_gemm_w4a16_rows
    X, H, Ex, Wp, Y = x.data_ptr(), x16.data_ptr(), e.data_ptr(), w.data_ptr(), y.data_ptr()
    assert f(X, K, 0, H, Ex, None) == EINVAL
    assert f(X, K, 33, H, Ex, None) == EINVAL
    assert f(X, 48, 2, H, Ex, None) == EINVAL
    assert f(X, 0, 2, H, Ex, None) == EINVAL
    assert f(None, K, 2, H, Ex, None) == EINVAL
    assert f(X, K, 2, None, Ex, None) == EINVAL
    assert f(X, K, 2, H, None, None) == EINVAL
    assert f(X, K, 32, H, Ex, None) == 0
    assert g(Wp, M, K, H, Ex, 0, None, Y, None) == EINVAL
    assert g(Wp, M, K, H, Ex, 33, None, Y, None) == EINVAL
    assert g(Wp, M, 48, H, Ex, 2, None, Y, None) == EINVAL
    assert g(Wp, 0, K, H, Ex, 2, None, Y, None) == EINVAL
    assert g(Wp, -5, K, H, Ex, 2, None, Y, None) == EINVAL
    assert g(None, M, K, H, Ex, 2, None, Y, None) == EINVAL
    assert g(Wp, M, K, None, Ex, 2, None, Y, None) == EINVAL
    assert g(Wp, M, K, H, None, 2, None, Y, None) == EINVAL
    assert g(Wp, M, K, H, Ex, 2, None, None, None) == EINVAL
    assert g(Wp, M, K, H, Ex, 32, None, Y, None) == 0
    torch.cuda.synchronize()
