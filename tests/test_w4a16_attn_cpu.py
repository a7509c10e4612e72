"""Weight-only mode's fp16 attention on the CPU: the numpy restatement of its per-row contract
(tests/w4a16_attn_cases.py) on the inputs of tests/test_gpu_w4a16_attn_ops.py.

The restatement gives every row the same bits in a prompt, in a prompt fed in two pieces, in the
single-query form alone or inside a ragged batch, and whatever the cache's stale tail holds, and it
passes tests/attn_ref.py's checker.  Six shortcuts a kernel of this kind may take are rejected on the
same inputs:
  shared_max      the running maximum shared across the 32-query group
  npast_blocks    key blocks aligned to n_past instead of key 0
  v_tail          V of keys past the last key not zeroed
  visit_no_rule   invisible blocks visited, and no rule for the sign of zero
      -> the row-independence comparator: a row's bits change with its neighbours, its batch or its tail;
  p_rtz           P cut off to fp16 without rounding (what a packing convert toward zero does; P
                  left in fp32 altogether would only be more accurate, which no error bound can
                  reject: the device's two forms share their code for this step instead)
  mask_value      masking by a large negative score (-1e4) instead of exclusion
      -> attn_ref.Ref.check, imported unchanged.
"""
import numpy as np
import pytest

import attn_ref as R
import w4a16_attn_cases as C

F32 = np.float32


def roped(d, style, n_rot, seed=0, qmul=1.0):
    q, k, v = C.random_world(d, seed, qmul)
    pos = np.arange(C.N_CTX)
    return C.rope_np(q, pos, d, n_rot, style), C.rope_np(k, pos, d, n_rot, style), v


def with_tail(K, V, nk, kind):
    """The cache of a sequence of nk keys in a slot whose rows past them are stale."""
    Kc, Vc = K.copy(), V.copy()
    Kc[nk:] = C.stale_rows(C.N_CTX - nk, K.shape[1], kind, row0=nk)
    Vc[nk:] = C.stale_rows(C.N_CTX - nk, K.shape[1], kind, seed=1, row0=nk)
    return Kc, Vc


def prompt(Q, K, V, d, N, n_past, variant=None, tail="nan"):
    Kc, Vc = with_tail(K, V, n_past + N, tail)
    return C.emulate_prompt(Q[n_past:n_past + N], Kc, Vc, d, n_past, C.head_scale(d), variant)


def rows(Q, K, V, d, pos, variant=None, tail="nan"):
    caches = [with_tail(K, V, p + 1, tail) for p in pos]
    return C.emulate_rows(Q[list(pos)], caches, pos, d, C.head_scale(d), variant)


@pytest.fixture(scope="module", params=C.DS)
def world(request):
    d = request.param
    style, n_rot = C.ROPE[d]
    return (d,) + roped(d, style, n_rot)


def test_restatement_is_row_independent_and_within_the_bound(world):
    d, Q, K, V = world
    worst = 0.0
    for N, n_past in C.PROMPTS:
        yp = prompt(Q, K, V, d, N, n_past)
        pos = list(range(n_past, n_past + N))
        assert C.rows_differ(yp, rows(Q, K, V, d, pos)) == [], (N, n_past)
        assert C.rows_differ(yp, prompt(Q, K, V, d, N, n_past, tail="mixed")) == [], (N, n_past)
        ref = R.Ref(Q[n_past:n_past + N], K[:n_past + N], V[:n_past + N], d, n_past, C.head_scale(d))
        worst = max(worst, ref.check(yp, f"d={d} N={N} n_past={n_past}"))
    # two pieces; the single-query form under every tail
    yp = prompt(Q, K, V, d, 130, 61)
    two = np.concatenate([prompt(Q, K, V, d, 70, 61), prompt(Q, K, V, d, 60, 131)])
    assert C.rows_differ(yp, two) == []
    pos = C.ragged_positions()
    yr = rows(Q, K, V, d, pos)
    for tail in ("mixed", "finite"):
        assert C.rows_differ(yr, rows(Q, K, V, d, pos, tail=tail)) == []
    print(f"d={d}: restatement's worst ratio to the bound {worst:.3f}")


def test_seams(world):
    d, Q, K, V = world
    pos = list(C.SEAMS)
    yr = rows(Q, K, V, d, pos, tail="mixed")
    full = prompt(Q, K, V, d, C.N_CTX, 0)
    assert C.rows_differ(yr, full[pos]) == []
    R.Ref(Q, K, V, d, 0, C.head_scale(d)).check(full, f"seams d={d}")


@pytest.mark.parametrize("variant", ["shared_max", "npast_blocks"])
def test_neighbours_and_alignment(world, variant):
    """The shortcut's prompt rows differ from its single-query rows (and from its own rows in a
    prompt fed in two pieces): a row's bits change with its neighbours or its batch."""
    d, Q, K, V = world
    N, n_past = 130, 61
    yp = prompt(Q, K, V, d, N, n_past, variant)
    yr = rows(Q, K, V, d, list(range(n_past, n_past + N)), variant)
    bad = C.rows_differ(yp, yr)
    two = np.concatenate([prompt(Q, K, V, d, 70, n_past, variant), prompt(Q, K, V, d, 60, n_past + 70, variant)])
    bad2 = C.rows_differ(yp, two)
    print(f"d={d} {variant}: {len(bad)} of {N} rows differ between the forms, {len(bad2)} between one piece and two")
    assert len(bad) > N // 2
    assert bad2


def test_v_tail(world):
    """V of keys past the last key not zeroed: a row's bits change with the slot's stale tail."""
    d, Q, K, V = world
    for N, n_past in ((33, 0), (5, 62)):
        clean = prompt(Q, K, V, d, N, n_past, "v_tail", tail="finite")
        stale = prompt(Q, K, V, d, N, n_past, "v_tail", tail="mixed")
        # (every row whose last block holds a key past the prompt's last)
        want = [i for i in range(N) if (n_past + i) // 64 == (n_past + N - 1) // 64 and (n_past + N) % 64]
        assert C.rows_differ(clean, stale) == want and np.isnan(stale).any()
    pos = [p for p in C.SEAMS if p % 64 != 63]  # (a row at a block's last key reads no key past its own)
    assert len(C.rows_differ(rows(Q, K, V, d, pos, "v_tail", tail="finite"),
                             rows(Q, K, V, d, pos, "v_tail", tail="mixed"))) == len(pos)


@pytest.mark.parametrize("d", C.DS)
def test_sign_of_zero(d):
    """The search finds a zero-family case on which visiting invisible blocks without a rule flips
    the sign of a zero between the two forms; the restatement (canonical zero) gives one set of bits
    there, -0 nowhere, and passes the checker."""
    found = C.zero_search(d)
    assert found is not None, "no seed of the zero family flips a bit under visit_no_rule"
    seed, q, k, v = found
    N, n_past = C.ZERO_PROMPT
    scale = C.head_scale(d)
    i = C.ZERO_POS - n_past
    # the flipped element: -0 in the single-query form, +0 in the prompt form (dimension 0 of a head)
    Kc, Vc = with_tail(k, v, n_past + N, "nan")
    yp = C.emulate_prompt(q[n_past:n_past + N], Kc, Vc, d, n_past, scale, "visit_no_rule")
    yr = C.emulate_rows(q[C.ZERO_POS:C.ZERO_POS + 1], [with_tail(k, v, C.ZERO_POS + 1, "nan")], [C.ZERO_POS], d, scale,
                        "visit_no_rule")
    assert C.bits(yr)[0, 0] == 0x80000000 and C.bits(yp)[i, 0] == 0
    good_p = prompt(q, k, v, d, N, n_past)
    good_r = rows(q, k, v, d, list(range(n_past, n_past + N)))
    assert C.rows_differ(good_p, good_r) == []
    assert not (C.bits(good_p) == 0x80000000).any()
    R.Ref(q[n_past:n_past + N], k[:n_past + N], v[:n_past + N], d, n_past, scale).check(good_p, f"zero family d={d}")
    print(f"d={d}: zero family seed {seed}")


@pytest.mark.parametrize("d", C.DS)
def test_p_rtz_rejected(d):
    """P cut off toward zero: every weight errs downwards by up to 2^-10 while l does not.  Over many
    keys that averages to the 2^-11 A the bound grants a rounded P; the two-key family shows it
    undiluted.  The search finds a seed on which the checker rejects the shortcut; the restatement
    passes on the same inputs."""
    found = C.pair_search(d)
    assert found is not None, "no seed of the two-key family shows p_rtz"
    seed, q, k, v, ref = found
    N, n_past = C.PAIR_PROMPT
    bad = prompt(q, k, v, d, N, n_past, "p_rtz")
    print(f"d={d}: two-key family seed {seed}, p_rtz ratio {ref.ratio(bad):.3f}, c up to {ref.c.max():.2f}")
    with pytest.raises(AssertionError):
        ref.check(bad, "p_rtz")
    good = prompt(q, k, v, d, N, n_past)
    ref.check(good, "two-key family")
    assert C.rows_differ(good, rows(q, k, v, d, list(range(N)))) == []


@pytest.mark.parametrize("d", C.DS)
def test_mask_value_rejected(d):
    """-1e4 for a masked score: the zero family's early rows see only scores below it, so the
    masked keys take the maximum and the weights."""
    _, q, k, v = C.zero_search(d)
    N, n_past = C.ZERO_PROMPT
    ref = R.Ref(q[n_past:n_past + N], k[:n_past + N], v[:n_past + N], d, n_past, C.head_scale(d))
    y = prompt(q, k, v, d, N, n_past, "mask_value")
    assert ref.ratio(y) > 100.0
    with pytest.raises(AssertionError):
        ref.check(y, "mask_value")
    # ... and on ordinary scores it is the restatement, bit for bit: only such rows show it
    style, n_rot = C.ROPE[d]
    Q, K, V = roped(d, style, n_rot)
    assert C.rows_differ(prompt(Q, K, V, d, 33, 0, "mask_value"), prompt(Q, K, V, d, 33, 0)) == []
