"""The rows of tests/tail_ln_edges.py bite, shown without a GPU: with its certificates on, the numpy
restatement of the layer tail's LayerNorm (lnt_owner) gives the oracle's bits on every generated
row; with one certificate switched off, every family built against that certificate has rows whose
output bits are no longer the oracle's.  The oracle's composition is what the kernel's outputs are
compared with on the GPU: O.norm, the float32 affine w * y + b in two roundings, O.quantize."""
import time

import numpy as np
import pytest

import oracle_py as O
import tail_ln_edges as T

SIZES = [s[0] for s in T.SIZES]
# the certificate each family is built against: the switch that disables it
SWITCH = {"mean_uncertified": "any_order_mean", "moments_wrong": "accept_moments", "scale_ambiguous": "always_sc_lo"}


def oracle_out(row):
    y = O.norm(row.v, row.v.size, 1)
    return y, O.quantize(T.affine(row.w1, y, row.b1))


def test_generation_is_quick_and_complete():
    """Every family has at least MIN_ROWS rows at every size, the scale-ambiguous one of both kinds,
    from fixed seeds, and all six sizes together take well under a minute."""
    T.rows.cache_clear()
    t0 = time.time()
    for E in SIZES:
        fam = T.rows(E)
        for name in T.FAMILIES:
            assert len(fam[name]) >= T.MIN_ROWS, (E, name, len(fam[name]))
        kinds = [r.seq_is for r in fam["scale_ambiguous"]]
        assert kinds.count("lo") >= 2 and kinds.count("hi") >= 2, (E, kinds)
        assert len(fam["mean_paths"]) >= 5, E  # most candidate kinds leave the mean uncertified
    assert time.time() - t0 < 30.0
    a = T.rows(SIZES[0])["scale_ambiguous"][0].v.copy()
    T.rows.cache_clear()
    assert np.array_equal(T.bits(a), T.bits(T.rows(SIZES[0])["scale_ambiguous"][0].v))  # seeded


@pytest.mark.parametrize("E", SIZES)
def test_restatement_is_the_oracle(E):
    """Certificates on: y and the Q4 bytes of norm 1 equal the oracle's on every row, and every row
    takes the path its family is named after."""
    for name, rows in T.rows(E).items():
        for i, r in enumerate(rows):
            st = T.restate(r.v)
            y, q = oracle_out(r)
            assert np.array_equal(T.bits(st.y), T.bits(y)), (name, i)
            assert np.array_equal(r.out(), q), (name, i)
            assert np.array_equal(T.bits(T.seq_norm(r.v)[0]), T.bits(y)), (name, i)  # the generator's own reference
            assert st.counters == r.counters
            if name == "certified":
                assert st.mean_ok and st.moments_ok and st.counters == (0, 0)
            elif name == "mean_uncertified":
                assert not st.mean_ok and st.counters == (1, 0)
            elif name == "mean_paths":
                assert not st.mean_ok and st.counters[0] == 1
            elif name == "moments_wrong":
                assert st.mean_ok and not st.moments_ok
                assert T.bits(st.sc_moments) != T.bits(st.scale)
            else:
                assert st.mean_ok and not st.moments_ok and st.counters == (0, 1)
                assert T.bits(st.sc_lo) != T.bits(st.sc_hi)
                assert T.bits(st.scale) == T.bits(st.sc_lo if r.seq_is == "lo" else st.sc_hi)


@pytest.mark.parametrize("family", sorted(SWITCH))
@pytest.mark.parametrize("E", SIZES)
def test_disabled_certificate_fails_on_its_family(E, family):
    """One certificate off: rows of the family built against it leave the oracle's bits (every row
    for the mean and the moments, the rows whose sequential scale is sc_hi for always-sc_lo), and
    the certified rows do not care."""
    sw = {SWITCH[family]: True}
    rows = T.rows(E)[family]
    differ = [not np.array_equal(r.out(**sw), oracle_out(r)[1]) for r in rows]
    if family == "scale_ambiguous":
        assert differ == [r.seq_is == "hi" for r in rows]
        assert sum(differ) >= 2
    else:
        assert all(differ) and len(differ) >= T.MIN_ROWS
    for r in T.rows(E)["certified"]:
        assert np.array_equal(r.out(**sw), oracle_out(r)[1])


def test_nonfinite_rows_take_both_fallbacks():
    """A row with an inf or a NaN fails the mean certificate and has a NaN interval: both counters
    move, every output of the norm is NaN, as the oracle's."""
    for E in SIZES[:3]:
        for name, v in T.nonfinite_rows(E):
            st = T.restate(v)
            assert st.counters == (1, 1), (E, name)
            assert np.isnan(st.y).all() and np.isnan(O.norm(v, E, 1)).all()
