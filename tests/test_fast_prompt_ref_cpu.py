"""The checker of tests/fast_prompt_ref.py has teeth (no GPU needed).

For every configuration and batch pair of tests/test_gpu_fast_prompt_layer.py:
  * a device that computes every stage's fp64 value from its own inputs and rounds it as the kernel
    does (fp32, the quantized fp16 operand, Q4 rows) passes every stage;
  * the share of ambiguous elements of every quantizing stage, a property of the reference and its
    bound alone, stays within the 2 % cap;
  * each wrong variant of a stage (fast_prompt_ref.VARIANTS) is rejected by that stage's check, on
    every configuration that has it, with std = 0.05 weights and biases.
One more wrong variant, the ALiBi slope of the neighbouring head, cannot be rejected by any fp64 check:
ggml_alibi, as the reference's BLOOM graph uses it, adds (j + 1) m_h to every key of query row j, a
constant along the softmax's axis.  The neighbouring head's slope therefore gives the same attention
in exact arithmetic (asserted below to 1e-12); only the bit-for-bit comparison of the model against
the composition sees it, and the slopes themselves are pinned against their definition here.
"""
import functools

import numpy as np
import pytest

import fast_prompt_ref as P
import fast_ref as R
from vsim_amd import hip
from vsim_amd import modelgen as mg

CASES = [(c, pr) for c in P.CONFIGS for pr in P.PAIRS]
IDS = [f"{c.name}-{a}+{b}" for c, (a, b) in CASES]


@functools.lru_cache(maxsize=None)
def rope_cs(n_pos, n_rot):
    return R.rope_table(n_pos, n_rot) if n_rot else None


@functools.lru_cache(maxsize=None)
def layer_of(cfg, root):
    path = str(root / f"{cfg.name}.bin")
    mg.write_model(path, cfg.arch, cfg.hparams(3), seed=cfg.seed, std=P.STD)
    return P.read_weights(path, cfg.arch, [1])[2][1]


@functools.lru_cache(maxsize=None)
def clean(cfg, pair, root):
    """Both evals of a batch pair on the rounding device: [(n_past, st)], the cache rows carried over."""
    L = layer_of(cfg, root)
    n1, n2 = pair
    cs = rope_cs(n1 + n2 + 1, cfg.n_rot)
    sl = P.alibi_slopes(cfg.H) if cfg.alibi else None
    st1 = P.simulate(cfg, L, P.resid_rows(cfg, n1, 0), 0, cs, sl)
    st2 = P.simulate(cfg, L, P.resid_rows(cfg, n2, n1), n1, cs, sl, st1["Knew"], st1["Vnew"])
    return L, cs, sl, [(0, st1), (n1, st2)]


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    return tmp_path_factory.mktemp("fast_prompt_ref")


def test_gelu_is_lip_lipschitz_and_the_table_is_within_its_term():
    """max |g'| < LIP on a fine grid over the fp16 range that matters, and every entry of the library's
    table is fp16(float(g(h))) within the table term of gelu_tol."""
    s = np.linspace(-12.0, 12.0, 2_400_001)
    g = P.gelu(s)
    slope = np.abs(np.diff(g) / np.diff(s)).max()
    assert 1.12 < slope < P.LIP
    e, tab = np.zeros(65536, np.uint16), np.zeros(65536, np.uint16)
    hip.check(hip.lib().vsim_op_tables(hip.ptr(e), hip.ptr(tab)), "tables")
    h = np.arange(65536, dtype=np.uint16).view(np.float16).astype(np.float64)
    ok = np.isfinite(h)
    g64 = P.gelu(h[ok])
    err = np.abs(tab.view(np.float16).astype(np.float64)[ok] - g64)
    assert np.all(err <= P.H16 * (1 + 2.0 ** -12) * np.abs(g64) + 2.0 ** -25)


@pytest.mark.parametrize("H", [1, 2, 3, 8, 12, 16])
def test_alibi_slopes_are_the_library_s(H):
    got = np.zeros(H, np.float32)
    hip.check(hip.lib().vsim_op_alibi_slopes(hip.ptr(got), H), "alibi_slopes")
    assert np.array_equal(got.view(np.uint32), P.alibi_slopes(H).view(np.uint32))
    if H == 8:  # 2^-1 .. 2^-8
        assert np.array_equal(got, 2.0 ** -np.arange(1.0, 9.0))


def test_plan_follows_the_documented_thresholds():
    c = {c.name: c for c in P.CONFIGS}
    p = P.plan(c["gptj-d128"], 300)
    assert p.pf and p.g2 and p.rope_epi and p.attn16 and p.kv16 and p.pair and p.join_epi and not p.attn_q16
    assert P.plan(c["gptj-d256"], 300).attn_q16 and P.plan(c["gptj-d256"], 9).attn_q16
    assert not P.plan(c["gptj-e384"], 300).pair and P.plan(c["gptj-e384"], 300).rope_epi
    p = P.plan(c["neox-par"], 300)
    assert p.g2 and not p.rope_epi and p.attn16 and not p.kv16 and p.join_epi
    p = P.plan(c["bloom"], 300)
    assert p.g2 and not p.attn16 and not p.join_epi
    for name in c:
        assert not P.plan(c[name], 255).g2 and P.plan(c[name], 256).g2
        assert not P.plan(c[name], 7).pf and P.plan(c[name], 8).pf
        assert not P.plan(c[name], 7).attn16


def test_crafted_rows():
    for N in (3, 9, 72, 300):
        x = P.resid_rows(P.CONFIGS[0], N, 0)
        assert sum(not r.any() for r in x) == 1
        assert sum(np.count_nonzero(r) == 1 for r in x) == 1
        assert sum(np.abs(r).max() > 1e3 for r in x) == 1


@pytest.mark.parametrize("cfg,pair", CASES, ids=IDS)
def test_the_reference_s_own_outputs_pass(cfg, pair, root):
    L, cs, sl, evals = clean(cfg, pair, root)
    for n_past, st in evals:
        ratios, shares = P.check(cfg, L, st, n_past, cs, sl)
        assert max(ratios.values()) <= 1.0
        for stage, s in shares.items():
            print(f"{cfg.name} N {st['inpL'].shape[0]} at {n_past}: ambiguous share of {stage} {s:.4f}")
            assert s <= P.AMB_CAP, f"{stage}: ambiguous share {s:.4f}"


@pytest.mark.parametrize("cfg,pair", CASES, ids=IDS)
def test_every_wrong_variant_is_rejected(cfg, pair, root):
    L, cs, sl, evals = clean(cfg, pair, root)
    n_past, st = evals[1]
    stages = {s.name: s for s in P.walk(cfg, L, st, n_past, cs, sl)}
    tried = 0
    for variant, (names, has) in P.VARIANTS.items():
        if not has(cfg):
            continue
        for alt in names:
            name = next(n for n in alt.split("|") if n in stages)
            stg = stages[name]
            bad = stg.device(frozenset([variant]))
            with pytest.raises(AssertionError):
                stg.check(bad)
            stg.check(stg.device())  # (and the same stage takes the right value)
            tried += 1
    assert tried >= 4


def test_alibi_slope_cannot_be_seen_by_an_fp64_check(root):
    """The per-row ALiBi term cancels in the softmax: the neighbouring head's slope moves the fp64
    attention by rounding noise only, far inside any bound."""
    cfg = next(c for c in P.CONFIGS if c.alibi)
    L, cs, sl, evals = clean(cfg, (72, 72), root)
    n_past, st = evals[1]
    kc = np.concatenate([st["kc_old"], st["Knew"]])
    vc = np.concatenate([st["vc_old"], st["Vnew"]])
    sc = float(np.float32(1.0 / np.sqrt(cfg.d)))
    a, tol = P.attn_exact(st["Q"], kc, vc, cfg.d, n_past, sc, sl)
    b, _ = P.attn_exact(st["Q"], kc, vc, cfg.d, n_past, sc, sl, slope_shift=1)
    assert np.abs(a - b).max() <= 1e-12 * np.abs(a).max()
    assert np.abs(a - b).max() < 1e-3 * tol[tol > 0].min()
