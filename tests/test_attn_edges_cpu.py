"""The generators of tests/attn_edges.py bite: on the oracle's own CPU ops every certificate row
defeats an exactly summed score, every softmax family shows the table edge it is named after, and
the quantizer rows hand quantize_row_q4_0 the golden edge blocks."""
import numpy as np
import pytest

import attn_edges as A
import oracle_py as O

CASES, ids = A.CASES, A.case_id
N_CTX = 512


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_gross_certificate_rows_defeat_the_exact_sum(case):
    d, H = case[1], case[2]
    scale = A.head_scale(d)
    for row, keys in A.cert_gross(case, N_CTX):
        ref = A.reference_row(case, row, want_p=True)
        s, p = ref[4], ref[5]
        ex = A.exact_scores(case, row)
        # the crafted keys, and only they, have another score when summed exactly
        differ = bits(s) != bits(ex)
        assert differ[:, keys].all() and differ.sum() == H * len(keys)
        # each is the oracle's sequential sum, lies within 2 of its head's maximum and has probability
        sc = (s * scale).astype(np.float32)
        assert ((sc.max(axis=1, keepdims=True) - sc)[:, keys] < 2.0).all()
        assert (p[:, keys] > 1e-4).all()
        K, qr = ref[7], ref[6]
        for h in range(H):
            for key in keys:
                assert bits(A.seq_dot(K[key, h * d:(h + 1) * d], qr[h * d:(h + 1) * d])) == bits(s[h, key])
        alt = A.reference_row(case, row, scores=ex)
        assert not np.array_equal(bits(ref[0]), bits(alt[0]))
        assert not np.array_equal(ref[1], alt[1])  # the Q4 row moves too


def test_gross_rows_cover_the_kernel_key_map():
    """Every 16-lane row, every one of the ATT_KB steps, the first, a middle and the last wave of
    the 16-wave kernel and of the tail's 11-wave one; same-lane pairs from d = 96 up."""
    keys = A.CERT_KEYS
    assert {k % 4 for k in keys} == {0, 1, 2, 3} and {k % 16 // 4 for k in keys} == {0, 1, 2, 3}
    assert {0, 5, 15} <= {k // 16 % 16 for k in keys} and {0, 5, 10} <= {k // 16 % 11 for k in keys}
    lane = lambda i: i % 64 // 4  # noqa: E731
    for d, n_rot in ((64, 32), (64, 0), (96, 24), (96, 32), (96, 0), (256, 64), (256, 0)):
        a, b = A.cert_ab(d, n_rot, False)
        assert n_rot <= a < b < d and lane(a) != lane(b)
        same = A.cert_ab(d, n_rot, True)
        assert (same is None) == (d == 64 or (d, n_rot) == (96, 32))
        if same:
            assert n_rot <= same[0] < same[1] < d and lane(same[0]) == lane(same[1])


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_one_ulp_rows_survive_and_bite(case):
    d = case[1]
    rows = A.cert_one_ulp(case, N_CTX)
    assert len(rows) == A.ONE_ULP_ROWS >= 8
    scale = A.head_scale(d)
    for row in rows:
        ref = A.reference_row(case, row, want_p=True)
        s, p = ref[4], ref[5]
        e = A.exact_dot(ref[7][20, :d], ref[6][:d])
        assert abs(int(s[0, 20].view(np.uint32)) - int(e.view(np.uint32))) == 1
        # the two leaders sit near 4096 and share the probability
        sc = (s[0] * scale).astype(np.float32)
        assert 2048 < sc[20] < 8192 and abs(sc[20] - sc[9]) < 2 and p[0, 20] > 0.1 and p[0, 9] > 0.1
        alt_s = s.copy()
        alt_s[0, 20] = e
        alt = A.reference_row(case, row, scores=alt_s)
        assert not np.array_equal(bits(ref[0]), bits(alt[0]))


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_softmax_families_show_their_property(case):
    _, d, H, _, alibi, _ = case
    scale = A.head_scale(d)
    fam = A.softmax_rows(case, N_CTX)
    sl = A.slopes(H) if alibi else None

    def look(row):
        ref = A.reference_row(case, row, want_p=True)
        sc = (ref[4] * scale).astype(np.float32)  # the oracle's scale (and alibi) in float32
        if alibi:
            sc = (sl[:, None] + sc).astype(np.float32)
        diff = (sc - sc.max(axis=1, keepdims=True)).astype(np.float32)
        assert np.isfinite(ref[4]).all() and np.isfinite(ref[5]).all()
        return diff, ref[5]

    with np.errstate(over="ignore"):
        diff, p = look(fam["overflow"][0])
        assert (p[diff < -65504] == 0).all() and (diff < -65504).sum() >= 30 * H and (p > 0).sum() >= 2 * H
        diff, p = look(fam["denormal"][0])
        ratio = p / p.max(axis=1, keepdims=True)
        assert ((ratio > 0) & (ratio < 6.2e-5)).sum() >= 30 * H and (p > 0).all()
        diff, p = look(fam["tiny"][0])
        h16 = diff.astype(np.float16)
        assert ((h16 != 0) & (np.abs(h16) < 6.1e-5)).sum() >= 10 * H and ((h16 == 0) & (diff != 0)).sum() >= 5 * H
        assert (bits(p) == bits(p[:, :1])).all()  # exp of every such argument is 1.0
    for row in fam["tie"]:
        diff, p = look(row)
        top = diff == 0
        assert (top.sum(axis=1) == (3 if row is fam["tie"][1] else 2)).all()
        for h in range(H):
            assert len(set(bits(p[h][top[h]]).tolist())) == 1 and (p[h][~top[h]] < p[h][top[h]][0]).all()
    for row, nk in zip(fam["equal"], (1, 17, 300)):
        diff, p = look(row)
        assert p.shape[1] == nk and (diff == 0).all() and (bits(p) == bits(p[:, :1])).all()
    diff, p = look(fam["onehot"][0])
    assert ((p == 1.0).sum(axis=1) == 1).all() and ((p == 0.0).sum(axis=1) == p.shape[1] - 1).all()


@pytest.mark.parametrize("case", A.QUANT_CASES, ids=ids)
def test_quantizer_rows_are_the_golden_edge_blocks(case):
    x, y = A.qrow_edges()
    assert np.array_equal(O.quantize(x), y)
    rows = A.quant_rows(case, N_CTX)
    for row in rows[:2]:
        out, aos = A.reference_row(case, row)[:2]
        assert np.array_equal(bits(out), bits(x)) and np.array_equal(aos, y)
    out, aos = A.reference_row(case, rows[2])[:2]
    # (the golden all-zero block: d = 0, every nibble 8)
    assert not out.any() and not np.signbit(out).any() and np.array_equal(aos, np.tile(y[:20], 6))
