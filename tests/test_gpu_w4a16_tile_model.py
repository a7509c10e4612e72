"""Weight-only prompts on k_gemm_w4a16_tile through the model executor: with the switch at 2 (the tile
kernel at every N of a prompt batch) every logit and every cache row is bit for bit what the switch at
0 (k_gemm_w4a16_rows on chunks of 32 rows) gives, and both are the mode's one contract: the
single-token evals.  The four graphs (GPT-NeoX parallel and serial, GPT-J, BLOOM) at E = 128, 4 heads,
vocabulary 128, n_ctx = 320, scratch and caches poisoned first.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from vsim_amd import hip  # noqa: E402
from vsim_amd import modelgen as mg  # noqa: E402

pytestmark = pytest.mark.gpu

ARCH = {"gptj": hip.ARCH_GPTJ, "gptneox": hip.ARCH_GPTNEOX, "bloom": hip.ARCH_BLOOM}
CONFIGS = dict(mg.CONFIGS)
CONFIGS["tiny-neox-serial"] = ("gptneox", mg.HParams(128, 128, 4, 2, 8, 0))
CFGS = ["tiny-neox", "tiny-neox-serial", "tiny-gptj", "tiny-bloom"]
N_CTX = 320
TILE, ROWS = "k_gemm_w4a16_tile", "k_gemm_w4a16_rows"


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b, what):
    if not np.array_equal(bits(a), bits(b)):
        bad = np.argwhere(bits(a) != bits(b))
        pytest.fail(f"{what}: {len(bad)} values differ, first {bad[:4].tolist()}")


def load(cfg, tmp_path, mode=hip.MODE_W4A16):
    arch_s, hp = CONFIGS[cfg]
    path = str(tmp_path / f"{cfg}.bin")
    mg.write_model(path, arch_s, hp, seed=11, std=0.05)
    dm = hip.Model.load(path, ARCH[arch_s], n_ctx=N_CTX)
    dm.set_mode(mode)
    return dm, hp


def tokens_of(hp, n, seed):
    return [int(t) for t in np.random.default_rng(seed).integers(0, hp.n_vocab, n)]


@pytest.fixture
def switch():
    old = hip.w4a16_set_tile_gemm(1)
    yield
    hip.w4a16_set_tile_gemm(old)


def names(dm):
    return [k["name"] for k in dm.profile_kernels()]


@pytest.mark.parametrize("cfg", CFGS)
def test_tile_prompts_equal_chunked_prompts_and_single_token_evals(cfg, tmp_path, switch):
    dm, hp = load(cfg, tmp_path)
    dm.seq_reserve(2)
    toks = tokens_of(hp, 300, 3)
    tail = toks[290:293]

    def runs(sw):
        """Everything a prompt batch can be, with the switch at sw: {what: logits}; after each, three
        further single-token evals from the cache it left."""
        assert hip.w4a16_set_tile_gemm(sw) in (0, 1, 2)
        out = {}

        def further(what, n_past, seq=None):
            for i, t in enumerate(tail):
                out[f"{what} +{i + 1}"] = dm.eval(n_past + i, [t]) if seq is None else dm.eval_seq(seq, n_past + i, [t])

        for n in (33, 129, 257):
            dm.debug_poison(N_CTX)
            out[f"eval {n}"] = dm.eval(0, toks[:n])
            further(f"eval {n}", n)
        dm.debug_poison(N_CTX)
        dm.eval(0, toks[:40], want_logits=False)
        out["eval 40 + 90"] = dm.eval(40, toks[40:130])
        further("eval 40 + 90", 130)
        dm.debug_poison(N_CTX)
        out["eval_seq 70"] = dm.eval_seq(1, 0, toks[:70])
        further("eval_seq 70", 70, seq=1)
        dm.debug_poison(N_CTX)
        out["score 131"] = dm.score(0, toks[:131], want_logits=True)[2]
        further("score 131", 131)
        return out

    tile = runs(2)
    chunked = runs(0)
    assert set(tile) == set(chunked)
    for what in tile:
        assert np.isfinite(tile[what]).all(), what
        same(tile[what], chunked[what], f"{cfg}: {what}, switch 2 against switch 0")
    # ... and both are the existing contract: the single-token evals, at a few positions
    hip.w4a16_set_tile_gemm(2)
    dm.debug_poison(N_CTX)
    single = {}
    for i in range(131):
        lg = dm.eval(i, [toks[i]])
        if i in (0, 32, 33, 63, 64, 128, 129, 130):
            single[i] = lg
    same(tile["eval 33"], single[32], f"{cfg}: prompt of 33")
    same(tile["eval 129"], single[128], f"{cfg}: prompt of 129")
    same(tile["eval 40 + 90"], single[129], f"{cfg}: 40 + 90")
    for i, lg in single.items():
        same(tile["score 131"][i], lg, f"{cfg}: score row {i}")
    dm.close()


def test_default_setting_takes_the_tile_kernel_from_its_threshold(tmp_path, switch):
    dm, hp = load("tiny-neox", tmp_path)
    T = hip.W4A16_TILE_MIN_N
    assert 32 < T < N_CTX
    toks = tokens_of(hp, T, 9)
    assert hip.w4a16_set_tile_gemm(1) == 1            # the default; the setter returns the old value
    for sw, n, want in ((1, T, True), (1, T - 1, False), (2, 33, True), (0, T, False), (1, T, True)):
        hip.w4a16_set_tile_gemm(sw)
        dm.set_profile(True)
        dm.eval(0, toks[:n])
        got = names(dm)
        dm.set_profile(False)
        # (the head takes the last row alone: a one-row product, on the rows kernel unless the switch is 2)
        assert (TILE in got) == want and (ROWS in got) == (sw != 2), (sw, n, got)
    # the setter: old values back, other values select 1
    assert hip.w4a16_set_tile_gemm(0) == 1
    assert hip.w4a16_set_tile_gemm(2) == 0
    assert hip.w4a16_set_tile_gemm(5) == 2
    assert hip.w4a16_set_tile_gemm(-1) == 1
    assert hip.w4a16_set_tile_gemm(1) == 1
    dm.close()


def test_exact_mode_and_the_batched_step_do_not_see_the_switch(tmp_path, switch):
    dm, hp = load("tiny-gptj", tmp_path, mode=hip.MODE_EXACT)
    dm.seq_reserve(4)
    toks = tokens_of(hp, 70, 4)
    got = []
    for sw in (0, 2):
        hip.w4a16_set_tile_gemm(sw)
        dm.set_mode(hip.MODE_EXACT)
        dm.set_profile(True)
        row = [dm.eval(0, toks), dm.eval(70, [toks[0]])]
        assert TILE not in names(dm)
        dm.set_profile(False)
        dm.set_mode(hip.MODE_W4A16)
        for s in range(3):
            dm.eval_seq(s, 0, toks[:5 + s], want_logits=False)
        dm.set_profile(True)
        row.append(dm.decode_batch_w4a16([0, 1, 2], [5, 6, 7], toks[10:13])[0])
        assert TILE not in names(dm)
        dm.set_profile(False)
        got.append(row)
    for a, b, what in zip(got[0], got[1], ("exact prompt", "exact step", "batched step")):
        same(a, b, what)
    dm.close()
