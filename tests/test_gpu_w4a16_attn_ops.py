"""Weight-only mode's fp16 attention through its op entries: k_attn_w4a16_tile
(vsim_op_attn_w4a16_prompt) and k_attn_w4a16_rows (vsim_op_attn_w4a16_rows), H = 2, n_ctx = 256, head
dims 64, 96, 128 and 256, GPT-J and rotate-half RoPE and none.

Row independence, bit for bit (uint32, so -0 != +0): row i of a prompt of N queries at n_past is the
single-query entry's row at position n_past + i on a cache holding the same keys and a stale tail --
alone (B = 1), inside a ragged, permuted batch of 32, and when the prompt is fed in two pieces; the
stale-tail family (NaN, +-Inf and 6e4 past the last key) and the sign-of-zero family (the case the
CPU search finds, tests/w4a16_attn_cases.py) give the same bits in both forms.
Accuracy: every case passes tests/attn_ref.py's Ref.check (c 2^-11 A + T, and 2e-2 max|V| against
fp64); the worst ratio per head dim is printed (RATIO lines; profiles/w4a16_attn_ratios.txt holds a run's).
Cache rows: what the single-query entry writes equals vsim_op_attn_decode_batch's, and nothing else is
written.  Argument errors: VSIM_EINVAL.
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import attn_ref as R  # noqa: E402
import w4a16_attn_cases as C  # noqa: E402
from vsim_amd import hip  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
EINVAL = -1
H, N_CTX = C.H, C.N_CTX
CONFIGS = [(d,) + C.ROPE[d] for d in C.DS] + [C.ROPE_NONE]
IDS = [f"d{d}-{'gptj' if s else 'neox'}-rot{r}" for d, s, r in CONFIGS]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


class World:
    """One sequence of N_CTX tokens on the device: q, k, v before RoPE, and what the exact path's
    vsim_op_rope_kv_write makes of them -- the queries after RoPE and the full K / V cache."""

    def __init__(self, d, style, n_rot, qkv):
        self.d, self.style, self.n_rot, self.E = d, style, n_rot, H * d
        self.scale = C.head_scale(d)
        self.q, self.k, self.v = (dev(a) for a in qkv)
        self.Qr = self.q.clone()
        self.Kc = torch.empty_like(self.k)
        self.Vc = torch.empty_like(self.v)
        hip.check(hip.lib().vsim_op_rope_kv_write(style, self.Qr.data_ptr(), self.k.data_ptr(), self.v.data_ptr(),
                                                  self.Kc.data_ptr(), self.Vc.data_ptr(), d, H, N_CTX, 0, n_rot, None),
                  "rope_kv_write")
        torch.cuda.synchronize()
        self.Qr_h, self.Kc_h, self.Vc_h = host(self.Qr), host(self.Kc), host(self.Vc)
        self.refs = {}

    def cache(self, nk, tail="nan"):
        """(K, V) device caches holding keys [0, nk) and a stale tail."""
        kc, vc = self.Kc.clone(), self.Vc.clone()
        if nk < N_CTX:
            kc[nk:] = dev(C.stale_rows(N_CTX - nk, self.E, tail, row0=nk))
            vc[nk:] = dev(C.stale_rows(N_CTX - nk, self.E, tail, seed=1, row0=nk))
        return kc, vc

    def prompt(self, N, n_past, tail="nan"):
        """vsim_op_attn_w4a16_prompt: out [N][E]; the scratch starts as NaN halves."""
        kc, vc = self.cache(n_past + N, tail)
        nbytes = hip.attn_prefill_layout(self.E, n_past + N)[0]
        scratch = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
        out = torch.full((N, self.E), float("nan"), dtype=torch.float32, device=DEV)
        hip.attn_w4a16_prompt(self.Qr[n_past:n_past + N].contiguous(), kc, vc, self.d, H, N, n_past, self.scale, out,
                              scratch)
        return host(out)

    def rows(self, pos, caches):
        """vsim_op_attn_w4a16_rows: rows at positions pos, row b on caches[b] = (K, V); out [B][E]."""
        B = len(pos)
        idx = torch.tensor(list(pos), dtype=torch.int64, device=DEV)
        q, k, v = (t[idx].contiguous() for t in (self.q, self.k, self.v))
        kp = torch.tensor([c[0].data_ptr() for c in caches], dtype=torch.int64, device=DEV)
        vp = torch.tensor([c[1].data_ptr() for c in caches], dtype=torch.int64, device=DEV)
        npd = dev(np.asarray(pos, np.int32))
        out = torch.full((B, self.E), float("nan"), dtype=torch.float32, device=DEV)
        hip.attn_w4a16_rows(q, k, v, kp, vp, npd, None, B, self.d, H, self.n_rot, self.style, N_CTX, self.scale, out)
        return host(out)

    def decode(self, N, n_past, tail="nan"):
        """N single-query calls (B = 1) at n_past, n_past + 1, ... on one cache that starts with the
        keys before n_past and a stale tail: (out [N][E], the cache afterwards)."""
        cache = self.cache(n_past, tail)
        out = np.concatenate([self.rows([n_past + i], [cache]) for i in range(N)])
        return out, cache

    def ref(self, N, n_past):
        if (N, n_past) not in self.refs:
            nk = n_past + N
            self.refs[N, n_past] = R.Ref(self.Qr_h[n_past:nk], self.Kc_h[:nk], self.Vc_h[:nk], self.d, n_past, self.scale)
        return self.refs[N, n_past]


@functools.lru_cache(maxsize=None)
def random_world(cfg):
    d, style, n_rot = cfg
    return World(d, style, n_rot, C.random_world(d))


@functools.lru_cache(maxsize=None)
def full_prompt(cfg):
    """The whole sequence as one prompt: every position's row, computed once."""
    return random_world(cfg).prompt(N_CTX, 0)


def ratio_line(what, d, r):
    print(f"RATIO {what} d={d} {r:.4f}")


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_prompt_rows_are_single_query_rows(cfg):
    W = random_world(cfg)
    worst = 0.0
    for N, n_past in C.PROMPTS:
        yp = W.prompt(N, n_past)
        yr, (kc, vc) = W.decode(N, n_past)
        assert C.rows_differ(yp, yr) == [], (N, n_past)
        assert C.rows_differ(yp, full_prompt(cfg)[n_past:n_past + N]) == [], (N, n_past)
        worst = max(worst, W.ref(N, n_past).check(yp, f"{cfg} N={N} n_past={n_past}"))
        # the decode's cache: the keys the exact path's prompt write gives, and the tail untouched
        nk = n_past + N
        want_k, want_v = W.cache(nk)
        assert np.array_equal(C.bits(host(kc)), C.bits(host(want_k))), (N, n_past, "K cache")
        assert np.array_equal(C.bits(host(vc)), C.bits(host(want_v))), (N, n_past, "V cache")
    ratio_line("prompts", W.d, worst)


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_whole_context_within_bound(cfg):
    W = random_world(cfg)
    ratio_line("context", W.d, W.ref(N_CTX, 0).check(full_prompt(cfg), f"{cfg} whole context"))


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_ragged_permuted_batch(cfg):
    """B = 32 at ragged positions (the seams among them) in a permuted order, every row on a cache of
    its own with a mixed stale tail: each row is the prompt's row at its position."""
    W = random_world(cfg)
    for seed in (0, 1):
        pos = C.ragged_positions(seed)
        caches = [W.cache(p, "mixed") for p in pos]
        y = W.rows(pos, caches)
        assert C.rows_differ(y, full_prompt(cfg)[pos]) == [], seed
        for b in (0, 13, 31):  # no row past p is written, row p is the prompt write's
            kc, vc = (host(t) for t in caches[b])
            want_k, want_v = (host(t) for t in W.cache(pos[b] + 1, "mixed"))
            assert np.array_equal(C.bits(kc), C.bits(want_k)) and np.array_equal(C.bits(vc), C.bits(want_v)), pos[b]


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_prompt_in_two_pieces(cfg):
    W = random_world(cfg)
    N, n_past = 130, 61
    two = np.concatenate([W.prompt(70, n_past), W.prompt(60, n_past + 70)])
    assert C.rows_differ(W.prompt(N, n_past), two) == []


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_stale_tail(cfg):
    """NaN, +-Inf and 6e4 in the cache rows past the last key change no bit, in either form."""
    W = random_world(cfg)
    for N, n_past in ((33, 0), (5, 62), (130, 61)):
        yp = W.prompt(N, n_past, "mixed")
        assert np.isfinite(yp).all()
        assert C.rows_differ(yp, full_prompt(cfg)[n_past:n_past + N]) == [], (N, n_past)
    yr, _ = W.decode(5, 62, "mixed")
    assert C.rows_differ(yr, full_prompt(cfg)[62:67]) == []


@pytest.mark.parametrize("d", C.DS)
def test_sign_of_zero(d):
    """The zero family's case on which an unruled kernel flips the sign of a zero (found by the CPU
    search): both forms give the same bits, -0 nowhere, within the bound."""
    found = C.zero_search(d)
    assert found is not None
    seed, q, k, v = found
    W = World(d, 0, 0, (q, k, v))
    N, n_past = C.ZERO_PROMPT
    yp = W.prompt(N, n_past)
    yr, _ = W.decode(N, n_past)
    assert C.rows_differ(yp, yr) == []
    i = C.ZERO_POS - n_past
    assert C.bits(yp)[i, 0] == 0 and C.bits(yr)[i, 0] == 0 and C.bits(yp)[i, d] == 0
    assert not (C.bits(yp) == 0x80000000).any()
    ratio_line("zero-family", d, W.ref(N, n_past).check(yp, f"zero family d={d} seed={seed}"))
    # ... and the row alone in a batch of its own size, after rows that do not see block 1
    pos = [C.ZERO_POS, 3, 63, 64]
    y4 = W.rows(pos, [W.cache(p) for p in pos])
    assert C.rows_differ(y4[:1], yp[i:i + 1]) == []


@pytest.mark.parametrize("d", C.DS)
def test_two_key_family(d):
    """The case on which a P cut off toward zero misses the bound (found by the CPU search)."""
    found = C.pair_search(d)
    assert found is not None
    seed, q, k, v, ref = found
    W = World(d, 0, 0, (q, k, v))
    N, n_past = C.PAIR_PROMPT
    yp = W.prompt(N, n_past)
    ratio_line("two-key-family", d, W.ref(N, n_past).check(yp, f"two-key family d={d} seed={seed}"))
    assert C.rows_differ(yp, W.decode(N, n_past)[0]) == []


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_cache_rows_equal_decode_batch(cfg):
    """The K / V rows the single-query entry writes are vsim_op_attn_decode_batch's, bit for bit, and
    no other cache row changes."""
    W = random_world(cfg)
    pos = [0, 63, 64, 200]
    B, E = len(pos), W.E
    idx = torch.tensor(pos, dtype=torch.int64, device=DEV)
    q, k, v = (t[idx].contiguous() for t in (W.q, W.k, W.v))
    got = []
    for new in (False, True):
        caches = [W.cache(p, "mixed") for p in pos]
        kp = torch.tensor([c[0].data_ptr() for c in caches], dtype=torch.int64, device=DEV)
        vp = torch.tensor([c[1].data_ptr() for c in caches], dtype=torch.int64, device=DEV)
        npd = dev(np.asarray(pos, np.int32))
        out = torch.empty((B, E), dtype=torch.float32, device=DEV)
        if new:
            hip.attn_w4a16_rows(q, k, v, kp, vp, npd, None, B, W.d, H, W.n_rot, W.style, N_CTX, W.scale, out)
        else:
            # (the exact kernel reads only keys <= p too; its Q4 row goes to scratch tensors)
            oq = torch.zeros(B * E // 32 * 20, dtype=torch.uint8, device=DEV)
            oxd = torch.empty((B, E), dtype=torch.float32, device=DEV)
            hip.attn_decode_batch(q, k, v, kp, vp, npd, None, None, B, W.d, H, W.n_rot, W.style, N_CTX, 1, W.scale, out,
                                  oq, oxd)
        got.append([(host(c[0]), host(c[1])) for c in caches])
    for b in range(B):
        for j in (0, 1):
            assert np.array_equal(C.bits(got[0][b][j]), C.bits(got[1][b][j])), (pos[b], "KV"[j])
        before = host(W.cache(pos[b], "mixed")[0])
        changed = np.nonzero((C.bits(before) != C.bits(got[1][b][0])).any(axis=1))[0]
        assert changed.tolist() == [pos[b]]


def test_argument_errors():
    L = hip.lib()
    d, E = 64, 128
    z = torch.zeros(33 * 512, dtype=torch.float32, device=DEV)
    p = torch.zeros(33, dtype=torch.int64, device=DEV)
    n = torch.zeros(33, dtype=torch.int32, device=DEV)
    Z, P, NP = z.data_ptr(), p.data_ptr(), n.data_ptr()

    def rows_args(**kw):
        f = dict(q=Z, k=Z, v=Z, kc=P, vc=P, n_past=NP, cs=None, alibi=None, B=1, d=d, H=2, n_rot=0, style=0,
                 n_ctx=N_CTX, kqv_nth=0, scale=1.0, out=Z, oq=None, oxd=None)
        f.update(kw)
        return hip.AttnBatchArgs(f["q"], f["k"], f["v"], f["kc"], f["vc"], f["n_past"], f["cs"], f["alibi"], f["B"], f["d"],
                                 f["H"], f["n_rot"], f["style"], f["n_ctx"], f["kqv_nth"], f["scale"], f["out"], f["oq"],
                                 f["oxd"])

    assert L.vsim_op_attn_w4a16_rows(None, None) == EINVAL
    bad = [dict(d=32), dict(d=80), dict(d=512), dict(d=96, H=1), dict(B=0), dict(B=33), dict(out=None), dict(oq=Z),
           dict(oxd=Z), dict(alibi=Z), dict(q=None), dict(k=None), dict(v=None), dict(kc=None), dict(vc=None),
           dict(n_past=None), dict(n_rot=3), dict(n_rot=66)]
    for kw in bad:
        assert L.vsim_op_attn_w4a16_rows(rows_args(**kw), None) == EINVAL, kw
        assert b"attn_w4a16_rows" in L.vsim_last_error()
    nbytes = hip.attn_prefill_layout(E, 70)[0]
    s = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    S = s.data_ptr()

    def prompt(Q=Z, kc=Z, vc=Z, d=d, H=2, N=6, n_past=64, out=Z, scratch=S, nb=nbytes):
        return L.vsim_op_attn_w4a16_prompt(Q, kc, vc, d, H, N, n_past, 1.0, out, scratch, nb, None)

    for kw in (dict(d=32), dict(d=80), dict(d=96, H=1), dict(N=0), dict(n_past=-1), dict(Q=None), dict(kc=None),
               dict(vc=None), dict(out=None), dict(scratch=None), dict(nb=nbytes - 1)):
        assert prompt(**kw) == EINVAL, kw
        assert b"attn_w4a16_prompt" in L.vsim_last_error()
    assert prompt() == 0
    torch.cuda.synchronize()
