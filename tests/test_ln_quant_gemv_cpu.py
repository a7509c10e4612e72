"""The inputs of tests/test_gpu_ln_quant.py and tests/test_gpu_gemv_batch.py bite (no GPU): each
property a kernel could get wrong changes the expected bits on the rows those tests feed it.
"""
import os
import re

import numpy as np
import pytest

import lnq_gemv_cases as C
import oracle_py as O
import tail_ln_edges as T

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _const(src, name):
    m = re.search(r"\b" + name + r"\s*=\s*(\d+)", src)
    assert m, name
    return int(m.group(1))


def test_constants_and_lists_follow_the_sources():
    """The shapes the lists were derived from are the kernels' own, and the lists are what those
    shapes give."""
    chain = open(os.path.join(ROOT, "vsim_amd", "csrc", "gemv_chain.hip")).read()
    layer = open(os.path.join(ROOT, "vsim_amd", "csrc", "layer.hip")).read()
    kern = open(os.path.join(ROOT, "vsim_amd", "csrc", "kern.hpp")).read()
    assert (_const(chain, "SOLO_CB"), _const(chain, "SOLO_PF"), _const(chain, "C5_RING"),
            _const(chain, "SOLO_MIN_GROUPS")) == (C.SOLO_CB, C.SOLO_PF, C.C5_RING, C.SOLO_MIN_GROUPS)
    assert re.search(r"using C2Gemv = C2Shape<%d, %d, false>" % (C.C2_CB, C.C2_DEPTH), chain)
    assert (_const(layer, "LNQ_THREADS"), _const(layer, "LNQ_SPLIT")) == (C.LNQ_NT, C.LNQ_SPLIT)
    assert re.search(r"template <int NT, bool CERT = true, int UP = %d>" % C.LNQ_UP, kern)
    assert C.solo_seam_blocks() == C.SOLO_NB and C.chain32_seam_blocks() == C.CHAIN32_NB
    # nit = (nch + 2 + PF) rounded up to PF + 1: the lists hold both sides of each step
    nit = lambda nb: (-(-nb // C.SOLO_CB) + 2 + C.SOLO_PF) // (C.SOLO_PF + 1) * (C.SOLO_PF + 1)
    assert {nit(nb) for nb in C.SOLO_NB} == {4, 8, 12} and nit(12) != nit(13) and nit(36) != nit(37)
    assert C.LNQ_ONE_PASS == 8192 and C.LNQ_SIZES[-2:] == [8192, 8224] and max(C.LNQ_SIZES) <= C.LNQ_MAX_N
    assert [n // 32 for n in C.LNQ_SIZES[:8]] == [1, 4, 7, 8, 9, 33, 64, 192]
    lens = {n: [b1 - b0 for b0, b1 in C.slices(n)] for n in C.LNQ_SIZES}
    assert all(sum(l) == n // 32 for n, l in lens.items())
    assert 0 in lens[32] and 0 in lens[224] and 0 not in lens[256]          # empty slices below 8 blocks
    assert len(set(lens[288])) > 1 and len(set(lens[1056])) > 1             # uneven slices
    assert any(l % 2 for l in lens[1056]) and any(l > 1 and l % 2 for l in lens[8224])  # odd: the ok = false half
    assert all(l % 2 == 0 for l in lens[2048] + lens[6144] + lens[8192])    # even
    # the kernel choice at the seam sizes of the GEMV tests
    assert not C.picks_solo([12224]) and C.picks_solo([12256]) and C.picks_solo([12288]) and C.picks_solo([12230])
    assert ((12256 + 31) // 32) % 2 == 1  # its last group has one tile


def test_join_forms_differ_on_the_chosen_rows():
    """Per size: every pair of the four forms differs in bits somewhere, and so does every form from
    the same sum added in another order."""
    for n in C.LNQ_SIZES:
        ops = C.join_operands(n, n)
        rows = {form: C.join(form, *ops) for form in C.JOIN_FORMS}
        forms = list(rows)
        for i, p in enumerate(forms):
            assert not np.array_equal(bits(rows[p]), bits(ops[0])), (n, p)
            for q in forms[i + 1:]:
                assert not np.array_equal(bits(rows[p]), bits(rows[q])), (n, p, q)
            for k, other in enumerate(C.join_other_orders(p, *ops)):
                assert not np.array_equal(bits(rows[p]), bits(other)), (n, p, k)
                assert np.allclose(rows[p], other, rtol=1e-5, atol=1e-6)  # (the same sum)


def test_tie_rows_separate_the_roundings():
    """The tie rows' halves under round-to-nearest-even are the oracle's GELU lookups; truncation and
    round-half-up each give another half on at least one row of every binade, for both signs."""
    rows, h = C.tie_rows()
    assert rows.shape == (2, 3, 31744) and rows.size % 32 == 0
    _, gtab = O.tables()
    rne = C.f2h_rne(rows)
    assert np.array_equal(O.gelu(rows.reshape(-1)).view(np.uint32) >> 0,
                          gtab[rne.reshape(-1)].view(np.float16).astype(f32).view(np.uint32))
    # what the three rows around a midpoint must round to
    up = np.where(h == C.LAST_HALF, 0x7C00, h + 1).astype(np.uint16)
    even = np.where(h % 2 == 0, h, up)
    for s, sign in enumerate((0, 0x8000)):
        assert np.array_equal(rne[s, 0], h | sign) and np.array_equal(rne[s, 2], up | sign)
        assert np.array_equal(rne[s, 1], even | sign)
    tr, hu = C.f2h_trunc(rows), C.f2h_half_up(rows)
    assert np.array_equal(tr[0], np.stack([h, h, h])) and np.array_equal(hu[0], np.stack([h, up, up]))
    bin_ = C.half_binade(h)
    for s in range(2):
        for b in range(31):
            sel = bin_ == b
            assert sel.any()
            assert (tr[s][:, sel] != rne[s][:, sel]).any(), ("truncation", s, b)
            assert (hu[s][:, sel] != rne[s][:, sel]).any(), ("half-up", s, b)
    # past the largest half: 65520 itself and above overflow, the float below it does not
    assert rne[0, :, -1].tolist() == [0x7BFF, 0x7C00, 0x7C00] and rows[0, 1, -1] == 65520.0


def test_nonfinite_blocks_of_the_half_sweep_are_few():
    """Sweep (a) in blocks of 32: the oracle alone has a non-finite GELU output in at most 4 % of the
    blocks, and exactly those blocks have a NaN scale."""
    x = C.all_half_rows()
    g = O.gelu(x).reshape(-1, 32)
    bad = ~np.isfinite(g).all(axis=1)
    assert 0 < bad.sum() <= 0.04 * g.shape[0]
    d = C.q4_scales(O.quantize(g.reshape(-1)))
    assert not np.isnan(d[~bad]).any()
    assert (~np.isfinite(d[bad])).all()


@pytest.mark.parametrize("nb", sorted(set(C.SOLO_NB) | set(C.CHAIN32_NB)))
def test_seam_k_rows_feel_their_last_block_and_the_block_order(nb):
    """64 rows at every K of the seam lists: without the last block (the oracle at K - 32) some of the
    outputs change, and so they do with two adjacent blocks of x exchanged (nb = 1 has no pair)."""
    K = 32 * nb
    rng = np.random.default_rng(900 + nb)
    aos = C.rand_q4_aos(rng, 64, K).reshape(64, nb, 20)
    x = rng.standard_normal(K).astype(f32)
    ref = O.mul_mat(aos.reshape(-1), 64, K, x, 1)
    short = O.mul_mat(np.ascontiguousarray(aos[:, :nb - 1]).reshape(-1), 64, K - 32, x[:K - 32], 1) if nb > 1 \
        else np.zeros(64, f32)
    assert (bits(short) != bits(ref)).any()
    for b in {0, nb - 2} if nb > 1 else ():
        xs = x.reshape(nb, 32).copy()
        xs[[b, b + 1]] = xs[[b + 1, b]]
        assert (bits(O.mul_mat(aos.reshape(-1), 64, K, xs.reshape(-1), 1)) != bits(ref)).any(), b


def test_steering_is_exact():
    """A zero-scale weight gives +0 from the oracle's product whatever the nibbles and the row, so the
    epilogue sees the bias itself; w = 0 leaves b unchanged in the affine, so the quantizer sees the
    golden row."""
    rng = np.random.default_rng(5)
    for K in (32, 224):
        aos = C.rand_q4_aos(rng, 96, K, zero_scale=True)
        y = O.mul_mat(aos, 96, K, (rng.standard_normal(K) * 3).astype(f32), 1)
        assert not bits(y).any()
    # +0 + bias is the bias, bit for bit, except that -0 becomes +0 (the GPU test's reference adds too)
    bias = np.concatenate([C.all_half_rows()[:0x7C01], C.all_half_rows()[0x8000:0xFC01], C.tie_rows()[0].reshape(-1)])
    same = bits(np.zeros_like(bias) + bias) == bits(bias)
    assert same.sum() == bias.size - 1 and bits(bias[~same])[0] == 0x80000000
    gold = np.load(os.path.join(ROOT, "tests", "golden", "ops_qrow.npz"))
    b = gold["x"]
    y = O.norm(rng.standard_normal(b.size).astype(f32), b.size, 1)
    z = T.affine(np.zeros(b.size, f32), y, b)
    assert np.array_equal(z, b) and np.array_equal(O.quantize(z), gold["y"]) and np.isfinite(b).all()
    assert b.size == 4288 and b.size // 32 == 134


def test_restatement_of_k_ln_quant_on_the_certificate_rows():
    """lnq_restate (k_ln_quant's own orders) on the rows of tail_ln_edges: what each family must add
    to vsim_norm_fallbacks per job.  The mean certificate is the tail's, so the mean families carry
    over; k_ln_quant has no moments shortcut, so a moments-wrong row is an ordinary certified row."""
    seen = {}
    for E, _, _ in T.SIZES:
        for name, rows in T.rows(E).items():
            for r in rows:
                c, scale = C.lnq_restate(r.v)
                seen.setdefault(name, set()).add(c)
                # the scale the restatement hands on is the sequential norm's
                assert bits(scale) == bits(T.seq_norm(r.v)[1]), (E, name)
    print("k_ln_quant fallback deltas per job:", {k: sorted(v) for k, v in seen.items()})
    assert seen["certified"] == {(0, 0)} and seen["moments_wrong"] == {(0, 0)}
    assert seen["mean_uncertified"] == {(1, 0)} and seen["scale_ambiguous"] == {(0, 1)}
    assert all(c[0] == 1 for c in seen["mean_paths"])
