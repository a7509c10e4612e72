"""Weight-only mode's fp16 attention through the model executor (vsim_w4a16_set_attn).

With the switch at 1 the mode's one promise holds on every path: a 70-token prompt's logits, and the
cache rows it leaves (read through two further evals), are bit for bit those of 70 single-token evals
on the captured step, of the same on the general path, of eval_seq into a slot, of the batched step's
rows at ragged positions over four slots (one reused), of Model.score's rows, of the prompt fed as
40 + 30 tokens, and at every vsim_w4a16_set_tile_gemm.  Two-layer models, vocabulary 128, n_ctx 192:
GPT-NeoX parallel (E 128, d 64) and serial (E 384, d 96), GPT-J (E 256, d 256 and d 128), BLOOM
(E 128, d 64: ALiBi, keeps the exact path's attention at either setting, as a d = 32 model does).
The switch changes the bits of the models that take it and of nothing else (exact mode, fast mode);
toggling it between steps drops the captured graphs; the profile names the new kernels where
expected and never k_kq.  Quality: at least W.QUALITY_FLOOR = 8 times nearer to the ideal forward than
the oracle's exact mode is (a d = 64 quality model; profiles/w4a16_attn_parity.txt holds a run's distances).
"""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import w4a16_ref as W  # noqa: E402
from vsim_amd import hip  # noqa: E402
from vsim_amd import modelgen as mg  # noqa: E402

pytestmark = pytest.mark.gpu

ARCH = {"gptj": hip.ARCH_GPTJ, "gptneox": hip.ARCH_GPTNEOX, "bloom": hip.ARCH_BLOOM}
CONFIGS = {
    "neox-par-d64": ("gptneox", mg.HParams(128, 128, 2, 2, 16, 1)),
    "neox-ser-d96": ("gptneox", mg.HParams(128, 384, 4, 2, 24, 0)),
    "gptj-d256": ("gptj", mg.HParams(128, 256, 1, 2, 64)),
    "gptj-d128": ("gptj", mg.HParams(128, 256, 2, 2, 32)),
    "bloom-d64": ("bloom", mg.HParams(128, 128, 2, 2, 0, 0)),
    "neox-d32": ("gptneox", mg.HParams(128, 128, 4, 2, 8, 1)),
}
TAKES = ["neox-par-d64", "neox-ser-d96", "gptj-d256", "gptj-d128"]
KEEPS = ["bloom-d64", "neox-d32"]
N_CTX = 192
NP = 70
TILE, ROWS, EXACT_ROWS = "k_attn_w4a16_tile", "k_attn_w4a16_rows", "k_attn_decode_batch"


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
    """Restores the process-wide switches."""
    old = hip.w4a16_set_attn(0)
    yield
    hip.w4a16_set_attn(old)
    hip.w4a16_set_step(1)
    hip.w4a16_set_tile_gemm(1)


def names(dm):
    return [k["name"] for k in dm.profile_kernels()]


def paths(dm, hp, toks, tail):
    """Every path a row can take, at the current switches: {what: logits}.  `single i` are the 70
    single-token evals' rows; every prompt form is followed by two further single-token evals from the
    cache it left."""
    out = {}

    def further(what, n_past, seq=None):
        for i, t in enumerate(tail):
            out[f"{what} +{i + 1}"] = dm.eval(n_past + i, [t]) if seq is None else dm.eval_seq(seq, n_past + i, [t])

    for step in (1, 0):
        hip.w4a16_set_step(step)
        dm.debug_poison(N_CTX)
        for i in range(NP):
            out[f"step{step} {i}"] = dm.eval(i, [toks[i]])
        further(f"step{step}", NP)
    hip.w4a16_set_step(1)
    for tg in (0, 1, 2):
        hip.w4a16_set_tile_gemm(tg)
        dm.debug_poison(N_CTX)
        out[f"eval tile_gemm={tg}"] = dm.eval(0, toks[:NP])
        further(f"eval tile_gemm={tg}", NP)
    hip.w4a16_set_tile_gemm(1)
    dm.debug_poison(N_CTX)
    dm.eval(0, toks[:40], want_logits=False)
    out["eval 40 + 30"] = dm.eval(40, toks[40:NP])
    further("eval 40 + 30", NP)
    dm.debug_poison(N_CTX)
    out["eval_seq"] = dm.eval_seq(1, 0, toks[:NP])
    further("eval_seq", NP, seq=1)
    dm.debug_poison(N_CTX)
    out["score"] = dm.score(0, toks[:NP], want_logits=True)[2]
    further("score", NP)
    # the batched step: four slots at ragged positions; slot 2 held a longer sequence before
    dm.debug_poison(N_CTX)
    pos = [5, 33, 64, NP - 1]
    other = tokens_of(hp, NP, 99)
    dm.eval_seq(2, 0, other, want_logits=False)
    for s, p in enumerate(pos):
        if p:
            dm.eval_seq(s, 0, toks[:p], want_logits=False)
    out["batch"] = dm.decode_batch_w4a16([0, 1, 2, 3], pos, [toks[p] for p in pos])[0]
    out["batch pos"] = pos
    return out


def check_paths(cfg, out):
    for k, v in out.items():
        if k != "batch pos":
            assert np.isfinite(v).all(), k
    for i in range(NP):
        same(out[f"step0 {i}"], out[f"step1 {i}"], f"{cfg}: single-token eval {i}, general path against the step")
        same(out["score"][i], out[f"step1 {i}"], f"{cfg}: score row {i}")
    for b, p in enumerate(out["batch pos"]):
        same(out["batch"][b], out[f"step1 {p}"], f"{cfg}: batched step row {b} at {p}")
    last = out[f"step1 {NP - 1}"]
    for what in ("eval tile_gemm=0", "eval tile_gemm=1", "eval tile_gemm=2", "eval 40 + 30", "eval_seq"):
        same(out[what], last, f"{cfg}: {what}")
    for what in ("step0", "eval tile_gemm=0", "eval tile_gemm=1", "eval tile_gemm=2", "eval 40 + 30", "eval_seq", "score"):
        for j in (1, 2):
            same(out[f"{what} +{j}"], out[f"step1 +{j}"], f"{cfg}: {what}, further eval {j} (the cache rows)")


@pytest.mark.parametrize("cfg", TAKES + KEEPS)
def test_one_row_one_set_of_bits_on_every_path(cfg, tmp_path, switch):
    dm, hp = load(cfg, tmp_path)
    dm.seq_reserve(4)
    toks, tail = tokens_of(hp, NP, 3), tokens_of(hp, 2, 4)
    hip.w4a16_set_attn(1)
    on = paths(dm, hp, toks, tail)
    check_paths(cfg, on)
    hip.w4a16_set_attn(0)
    off = paths(dm, hp, toks, tail)
    check_paths(cfg, off)
    keys = [k for k in on if k != "batch pos"]
    differs = any(not np.array_equal(bits(on[k]), bits(off[k])) for k in keys)
    if cfg in TAKES:
        assert not np.array_equal(bits(on["eval_seq"]), bits(off["eval_seq"])), "switch 1 changed no logit"
    else:
        assert not differs, f"{cfg} must keep the exact path's attention at either setting"
    dm.close()


@pytest.mark.parametrize("mode", [hip.MODE_EXACT, hip.MODE_FAST], ids=["exact", "fast"])
def test_other_modes_do_not_see_the_switch(mode, tmp_path, switch):
    dm, hp = load("gptj-d128", tmp_path, mode=mode)
    toks = tokens_of(hp, NP, 5)
    got = []
    for sw in (0, 1):
        hip.w4a16_set_attn(sw)
        dm.set_profile(True)
        row = [dm.eval(0, toks), dm.eval(NP, [toks[0]]), dm.eval(NP + 1, [toks[1]])]
        got.append(row)
        assert TILE not in names(dm) and ROWS not in names(dm)
        dm.set_profile(False)
    for a, b in zip(*got):
        same(a, b, "another mode's logits across the switch")
    dm.close()


def test_toggle_between_steps_drops_the_graphs(tmp_path, switch):
    dm, hp = load("neox-par-d64", tmp_path)
    toks = tokens_of(hp, 12, 6)
    dm.set_graph(True)
    assert hip.w4a16_set_attn(0) == 0
    dm.eval(0, toks[:10], want_logits=False)
    a0 = [dm.eval(10, [toks[10]]), dm.eval(11, [toks[11]])]    # (captured at switch 0)
    assert hip.w4a16_set_attn(1) == 0
    a1 = [dm.eval(10, [toks[10]]), dm.eval(11, [toks[11]])]
    assert not np.array_equal(bits(a0[1]), bits(a1[1])), "the captured step did not see the switch"
    assert hip.w4a16_set_attn(0) == 1
    b0 = [dm.eval(10, [toks[10]]), dm.eval(11, [toks[11]])]
    same(b0[0], a0[0], "switch 0 again, position 10")
    same(b0[1], a0[1], "switch 0 again, position 11")
    # switch 1's step rows are its prompt's rows (from a cache made at switch 1: the deeper layers'
    # keys depend on the attention before them, so a1 above stood on switch 0's)
    hip.w4a16_set_attn(1)
    dm.debug_poison(N_CTX)
    dm.eval(0, toks[:10], want_logits=False)
    c1 = [dm.eval(10, [toks[10]]), dm.eval(11, [toks[11]])]
    dm.debug_poison(N_CTX)
    same(dm.eval(0, toks[:12]), c1[1], "switch 1: step row against the prompt")
    # the setter: other values select 0, the old value comes back
    assert hip.w4a16_set_attn(7) == 1
    assert hip.w4a16_set_attn(-1) == 0
    assert hip.w4a16_set_attn(1) == 0
    assert hip.w4a16_set_attn(0) == 1
    dm.close()


@pytest.mark.parametrize("cfg", ["gptj-d256", "bloom-d64"])
def test_profile_names(cfg, tmp_path, switch):
    dm, hp = load(cfg, tmp_path)
    dm.seq_reserve(2)
    toks = tokens_of(hp, 40, 7)

    def run(sw):
        hip.w4a16_set_attn(sw)
        got = {}
        dm.set_profile(True)
        dm.eval(0, toks[:33])
        dm.eval(33, toks[33:36])   # (a short piece: no N threshold applies)
        got["prompt"] = names(dm)
        dm.set_profile(False)
        dm.set_profile(True)
        dm.eval(36, [toks[36]])
        got["step"] = names(dm)
        dm.set_profile(False)
        dm.eval_seq(1, 0, toks[:9], want_logits=False)
        dm.set_profile(True)
        dm.decode_batch_w4a16([0, 1], [37, 9], [toks[37], toks[9]])
        got["batch"] = names(dm)
        dm.set_profile(False)
        return got

    on, off = run(1), run(0)
    takes = cfg != "bloom-d64"
    for what in ("prompt", "step", "batch"):
        assert "k_kq" not in on[what] or not takes, (what, on[what])
        assert TILE not in off[what] and ROWS not in off[what], (what, off[what])
    if takes:
        assert TILE in on["prompt"] and ROWS not in on["prompt"] and EXACT_ROWS not in on["prompt"], on["prompt"]
        assert ROWS in on["step"] and EXACT_ROWS not in on["step"], on["step"]
        assert ROWS in on["batch"] and EXACT_ROWS not in on["batch"], on["batch"]
        assert EXACT_ROWS in off["step"] and EXACT_ROWS in off["batch"]
    else:
        assert on == off and EXACT_ROWS in on["step"] and EXACT_ROWS in on["batch"]
    dm.close()


def test_quality(tmp_path, switch):
    """A d = 64 quality model (W's recipe at two heads): the RMS distance of the device's logits to
    the ideal forward (W.neox_forward with W.mm_ideal) at switch 1 against the oracle's exact-mode
    distance: at least W.QUALITY_FLOOR = 8 times nearer.  Both settings' distances are printed."""
    hp = mg.HParams(128, 128, 2, 2, 16)
    path = os.path.join(str(tmp_path), "w4a16_attn_quality.bin")
    mg.write_model(path, "gptneox", hp, seed=W.QUALITY_SEED, std=W.QUALITY_STD)
    tokens = tokens_of(hp, W.QUALITY_N, W.QUALITY_TOKENS_SEED)
    ideal = W.neox_forward(path, tokens, W.mm_ideal)
    d_exact = W.rms(W.oracle_exact_rows(path, tokens), ideal)
    dm = hip.Model.load(path, hip.ARCH_GPTNEOX, n_ctx=W.N_CTX)
    dm.set_mode(hip.MODE_W4A16)
    dist = {}
    for sw in (0, 1):
        hip.w4a16_set_attn(sw)
        dist[sw] = W.rms(dm.score(0, tokens, want_logits=True)[2], ideal)
    dm.close()
    print(f"PARITY d=64 quality model (seed {W.QUALITY_SEED}, {W.QUALITY_N} rows x {hp.n_vocab} logits, RMS to the ideal "
          f"forward): oracle exact mode {d_exact:.5f}; weight-only switch 0 {dist[0]:.4e} ({d_exact / dist[0]:.1f} x nearer); "
          f"switch 1 {dist[1]:.4e} ({d_exact / dist[1]:.1f} x nearer); floor {W.QUALITY_FLOOR}")
    assert d_exact / dist[1] >= W.QUALITY_FLOOR
