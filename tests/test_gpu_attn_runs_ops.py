"""Runs of rows through the attention op entries: vsim_op_attn_decode_runs (k_kv_rows +
k_attn_decode_runs) and vsim_op_attn_w4a16_runs (k_kv_rows + k_attn_w4a16_runs).

A run is len consecutive tokens of one sequence as len consecutive rows on one cache at positions
p, p + 1, ..  The reference is the one-launch entry (vsim_op_attn_decode_batch /
vsim_op_attn_w4a16_rows) called row by row with B = 1 on a copy of the caches; the comparison is
bitwise (uint32) on out, the Q4 row (nibbles and scales), oxd and every K / V cache row.  H = 2,
n_ctx = 288.  Every cache row at or past a run's start is NaN before the call, and the rows past the
run's end are NaN afterwards.  Run positions: from 0 on an empty cache, across key 16 (another wave
reads the new key), across key 64 (the fp16 form's block seam), across key 256 (the KQ sweep of 16
waves x 16 keys wraps), ending on the last cache row.
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from vsim_amd import hip  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
EINVAL = -1
H, N_CTX = 2, 288
# (run lengths, run starts), one cache per run
BATCHES = [
    ([1, 3, 1, 8], [0, 14, 287, 60]),
    ([1, 3, 1, 8], [63, 254, 15, 280]),
    ([32], [0]),
    ([32], [250]),
    ([32], [256]),
]
# (d, style, n_rot, alibi, kqv_nth)
EXACT = [
    (32, 0, 32, False, 1), (32, 1, 16, False, 4), (64, 1, 64, False, 1), (64, 0, 0, True, 4),
    (128, 0, 64, False, 4), (128, 1, 128, True, 1), (256, 0, 256, False, 1), (256, 1, 64, False, 4),
    (256, 0, 0, False, 1),
]
# (d, style, n_rot)
FP16 = [(64, 0, 32), (64, 1, 64), (96, 0, 48), (96, 1, 96), (128, 1, 64), (128, 0, 0), (256, 0, 256), (256, 1, 128)]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    torch.cuda.synchronize()
    a = t.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.float32 else a


def ptrs(ts):
    return torch.tensor([t.data_ptr() for t in ts], dtype=torch.int64, device=DEV)


@functools.lru_cache(maxsize=None)
def world(d):
    """Rows before RoPE for 32 batch rows and a finite history for the caches."""
    rng = np.random.default_rng(1000 + d)
    E = H * d
    q, k, v = (dev(rng.standard_normal((32, E)).astype(np.float32)) for _ in range(3))
    hk, hv = (dev(rng.standard_normal((N_CTX, E)).astype(np.float32)) for _ in range(2))
    slopes = dev(np.asarray([0.25, 0.0625], np.float32))
    return q, k, v, hk, hv, slopes


@functools.lru_cache(maxsize=None)
def rope_table(n_rot):
    """[N_CTX][n_rot / 2] {cos, sin} doubles on the device (both sides of every comparison read the
    same table, so how its last bit was rounded does not matter here); None without RoPE."""
    if n_rot == 0:
        return None
    theta = 10000.0 ** (-2.0 * np.arange(n_rot // 2) / n_rot)
    ang = np.arange(N_CTX)[:, None] * theta[None, :]
    return dev(np.stack([np.cos(ang), np.sin(ang)], axis=-1).astype(np.float64))


def fresh_caches(d, starts):
    """One (K, V) pair per run: the history below the run's start, NaN from there on."""
    hk, hv = world(d)[3:5]
    out = []
    for p in starts:
        kc, vc = hk.clone(), hv.clone()
        kc[p:] = float("nan")
        vc[p:] = float("nan")
        out.append((kc, vc))
    return out


class Exact:
    def __init__(self, cfg):
        self.d, self.style, self.n_rot, self.alibi, self.nth = cfg
        self.E = H * self.d
        self.scale = 1.0 / np.sqrt(self.d)

    def call(self, fn, rows, caches, pos):
        q, k, v, _, _, slopes = world(self.d)
        B, E = len(rows), self.E
        idx = torch.tensor(rows, dtype=torch.int64, device=DEV)
        out = torch.full((B, E), float("nan"), dtype=torch.float32, device=DEV)
        oq = torch.zeros(B * (E // 32) * 20, dtype=torch.uint8, device=DEV)
        oxd = torch.full((B, E), float("nan"), dtype=torch.float32, device=DEV)
        fn(q[idx].contiguous(), k[idx].contiguous(), v[idx].contiguous(), ptrs([c[0] for c in caches]),
           ptrs([c[1] for c in caches]), dev(np.asarray(pos, np.int32)), rope_table(self.n_rot), slopes if self.alibi else None, B, self.d, H,
           self.n_rot, self.style, N_CTX, self.nth, self.scale, out, oq, oxd)
        nb = B * (E // 32) * 16
        oqb = bits(oq)
        return {"out": bits(out), "oq nibbles": oqb[:nb].reshape(B, -1), "oq scales": oqb[nb:].reshape(B, -1),
                "oxd": bits(oxd)}

    def runs(self, rows, caches, pos):
        return self.call(hip.attn_decode_runs, rows, caches, pos)

    def one(self, row, cache, p):
        return self.call(hip.attn_decode_batch, [row], [cache], [p])


class Fp16:
    def __init__(self, cfg):
        self.d, self.style, self.n_rot = cfg
        self.E = H * self.d
        self.scale = 1.0 / np.sqrt(self.d)

    def call(self, fn, rows, caches, pos):
        q, k, v = world(self.d)[:3]
        B = len(rows)
        idx = torch.tensor(rows, dtype=torch.int64, device=DEV)
        out = torch.full((B, self.E), float("nan"), dtype=torch.float32, device=DEV)
        fn(q[idx].contiguous(), k[idx].contiguous(), v[idx].contiguous(), ptrs([c[0] for c in caches]),
           ptrs([c[1] for c in caches]), dev(np.asarray(pos, np.int32)), rope_table(self.n_rot), B, self.d, H, self.n_rot,
           self.style, N_CTX,
           self.scale, out)
        return {"out": bits(out)}

    def runs(self, rows, caches, pos):
        return self.call(hip.attn_w4a16_runs, rows, caches, pos)

    def one(self, row, cache, p):
        return self.call(hip.attn_w4a16_rows, [row], [cache], [p])


def check_batches(F, what):
    for lens, starts in BATCHES:
        # the reference: every run row by row, B = 1, on its own copy of the caches
        ref_caches = fresh_caches(F.d, starts)
        want, row = [], 0
        for r, (n, p) in enumerate(zip(lens, starts)):
            for j in range(n):
                want.append(F.one(row, ref_caches[r], p + j))
                row += 1
        N = row
        caches = fresh_caches(F.d, starts)
        per_row_cache = [caches[r] for r, n in enumerate(lens) for _ in range(n)]
        pos = [p + j for n, p in zip(lens, starts) for j in range(n)]
        got = F.runs(list(range(N)), per_row_cache, pos)
        for key, g in got.items():
            w = np.concatenate([x[key] for x in want])
            bad = np.nonzero((g != w).reshape(N, -1).any(axis=1))[0]
            assert bad.size == 0, f"{what} {lens} at {starts}: {key} differs in rows {bad.tolist()}"
        if "out" in got:
            assert not np.isnan(got["out"].view(np.float32)).any(), (what, lens, starts)
        for r, (n, p) in enumerate(zip(lens, starts)):
            for j, name in enumerate("KV"):
                g, w = bits(caches[r][j]), bits(ref_caches[r][j])
                bad = np.nonzero((g != w).any(axis=1))[0]
                assert bad.size == 0, f"{what} {lens} at {starts}: {name} cache of run {r} differs in rows {bad.tolist()}"
                f = g.view(np.float32)
                assert not np.isnan(f[:p + n]).any() and np.isnan(f[p + n:]).all(), (what, lens, starts, r, name)


@pytest.mark.parametrize("cfg", EXACT, ids=[f"d{c[0]}-s{c[1]}-rot{c[2]}-alibi{int(c[3])}-nth{c[4]}" for c in EXACT])
def test_decode_runs_rows_are_one_row_calls(cfg):
    check_batches(Exact(cfg), f"attn_decode_runs {cfg}")


@pytest.mark.parametrize("cfg", FP16, ids=[f"d{c[0]}-s{c[1]}-rot{c[2]}" for c in FP16])
def test_w4a16_runs_rows_are_one_row_calls(cfg):
    check_batches(Fp16(cfg), f"attn_w4a16_runs {cfg}")


def test_runs_beside_other_caches_order_free():
    """A run's rows need not be neighbours of one another in the batch: rows of two runs interleaved
    give the rows of the runs one after the other (positions, not row order, tie a row to its keys)."""
    F = Exact((64, 1, 64, False, 1))
    starts = [14, 60]
    caches = fresh_caches(64, starts)
    a = F.runs([0, 1, 2, 3, 4, 5], [caches[0]] * 3 + [caches[1]] * 3, [14, 15, 16, 60, 61, 62])
    caches2 = fresh_caches(64, starts)
    order = [0, 3, 1, 4, 2, 5]
    b = F.runs(order, [(caches2[0], caches2[1])[i // 3] for i in order], [[14, 15, 16, 60, 61, 62][i] for i in order])
    for key in a:
        assert np.array_equal(a[key][order], b[key]), key
    for r in (0, 1):
        for j in (0, 1):
            assert np.array_equal(bits(caches[r][j]), bits(caches2[r][j]))


def test_argument_errors():
    L = hip.lib()
    z = torch.zeros(33 * 512, dtype=torch.float32, device=DEV)
    p = torch.zeros(33, dtype=torch.int64, device=DEV)
    n = torch.zeros(33, dtype=torch.int32, device=DEV)
    Z, P, NP = z.data_ptr(), p.data_ptr(), n.data_ptr()

    def args(**kw):
        f = dict(q=Z, k=Z, v=Z, kc=P, vc=P, n_past=NP, cs=None, alibi=None, B=1, d=64, H=2, n_rot=0, style=0,
                 n_ctx=N_CTX, kqv_nth=0, scale=1.0, out=Z, oq=None, oxd=None)
        f.update(kw)
        return hip.AttnBatchArgs(f["q"], f["k"], f["v"], f["kc"], f["vc"], f["n_past"], f["cs"], f["alibi"], f["B"], f["d"],
                                 f["H"], f["n_rot"], f["style"], f["n_ctx"], f["kqv_nth"], f["scale"], f["out"], f["oq"],
                                 f["oxd"])

    assert L.vsim_op_attn_w4a16_runs(None, None) == EINVAL
    for kw in [dict(d=32), dict(d=80), dict(d=512), dict(d=96, H=1), dict(B=0), dict(B=33), dict(out=None), dict(oq=Z),
               dict(oxd=Z), dict(alibi=Z), dict(q=None), dict(k=None), dict(v=None), dict(kc=None), dict(vc=None),
               dict(n_past=None), dict(n_rot=3), dict(n_rot=66)]:
        assert L.vsim_op_attn_w4a16_runs(args(**kw), None) == EINVAL, kw
        assert b"attn_w4a16_runs" in L.vsim_last_error()
    # the exact form's: whatever vsim_op_attn_decode_batch refuses
    assert L.vsim_op_attn_decode_runs(None, None) == EINVAL
    ok = dict(oq=Z, oxd=Z)  # (never launched here: the cache pointer arrays hold nulls)
    for kw in [dict(B=0), dict(B=33), dict(d=48), dict(d=288), dict(d=0), dict(q=None), dict(k=None), dict(v=None),
               dict(kc=None), dict(vc=None), dict(n_past=None), dict(oq=None), dict(oxd=None), dict(n_rot=3),
               dict(n_rot=66), dict(H=0), dict(n_ctx=0)]:
        a = args(**{**ok, **kw})
        assert L.vsim_op_attn_decode_batch(a, None) == EINVAL, kw
        assert L.vsim_op_attn_decode_runs(a, None) == EINVAL, kw
    assert L.vsim_op_attn_decode_runs(args(**{**ok, "q": None}), None) == EINVAL
    assert b"attn_decode_runs" in L.vsim_last_error()
