"""vsim_op_topk_rows (k_sample_topk_rows): the candidate lists of B logits rows from one launch,
every row with its own window, k, temperature and penalty.  Every comparison is bitwise on the
values and exact on the ids, against vsim_op_topk run on each row alone and against the numpy
restatement (tests/sample_ref.py)."""
import functools

import numpy as np
import pytest
import torch

import sample_ref as R
from vsim_amd import hip

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EINVAL = -1
KS, NWS = (1, 20, 40, 64), (0, 1, 64, 1024)
OUT_BYTES = hip.TOPK_OUT_DTYPE.itemsize
FILL = 0xEE  # what the output blocks hold before a launch: entries past k must keep it


@functools.lru_cache(maxsize=None)
def rows_of(n, B):
    """B rows of n distinct float32 values of both signs, each row its own permutation and scale."""
    out = np.empty((B, n), np.float32)
    for b in range(B):
        g = np.random.default_rng(1000 * n + b)
        v = ((np.arange(n, dtype=np.float64) - n / 2 + 0.25) * (1e-3 + 1e-4 * b)).astype(np.float32)
        assert np.unique(v).size == n
        out[b] = g.permutation(v)
    out.setflags(write=False)
    return out


def row_params(x, b, seed=0):
    """Row b's parameters: k and the window length cycle through KS x NWS (all 16 pairs within 32
    rows); the window holds the row's best ids (so the penalty reorders the head), duplicates and
    ids outside [0, n); temperature and penalty are the row's own."""
    n = x.size
    g = np.random.default_rng(seed + 31 * b + n)
    k, nw = min(KS[b % 4], n), NWS[(b // 4) % 4]
    top = [int(t) for t in np.argsort(-x.astype(np.float64))[:5]]
    pool = top + top[:2] + [n, n + 7, -1, -2 ** 31, 2 ** 31 - 1] + [int(t) for t in g.integers(0, n, 64)]
    win = [pool[int(i)] for i in g.integers(0, len(pool), nw)]
    if nw >= 64:
        win[:7] = top + top[:2]
    return dict(win=win, temp=0.5 + 0.05 * b, penalty=1.0 + 0.03 * b, k=k)


def pack(params):
    """The rows' TopkParams blocks as a device byte tensor."""
    a = np.zeros(len(params), hip.TOPK_PARAMS_DTYPE)
    a["win"] = 0x55555555  # ids past nw must not matter
    for b, p in enumerate(params):
        a[b]["scale"], a[b]["penalty"] = 1.0 / R.widen(p["temp"]), R.widen(p["penalty"])
        a[b]["k"], a[b]["nw"] = p["k"], len(p["win"])
        a[b]["win"][:len(p["win"])] = np.asarray(p["win"], np.int64).astype(np.int32)
    return torch.tensor(a.view(np.uint8).reshape(-1), device=DEV)


def strided(rows, ldx, lead=0):
    """The rows at stride ldx in one device buffer, `lead` floats in; the gaps hold +inf, which
    would head every list if a row read past its n."""
    B, n = rows.shape
    buf = np.full(lead + B * ldx, np.inf, np.float32)
    for b in range(B):
        buf[lead + b * ldx: lead + b * ldx + n] = rows[b]
    t = torch.tensor(buf, device=DEV)
    return t, t.data_ptr() + 4 * lead


def launch_rows(xptr, ldx, n, params, stream=None):
    pd = pack(params)
    out = torch.full((len(params) * OUT_BYTES,), FILL, dtype=torch.uint8, device=DEV)
    hip.topk_rows(xptr, ldx, n, len(params), pd, out, stream)
    return out, pd


def unpack(out):
    return out.cpu().numpy().view(hip.TOPK_OUT_DTYPE)


def single(xptr, n, p):
    """vsim_op_topk on one row alone."""
    k = p["k"]
    wd = torch.tensor(np.asarray(p["win"], np.int64).astype(np.int32), device=DEV) if len(p["win"]) else None
    val = torch.zeros(k, dtype=torch.float64, device=DEV)
    ids = torch.full((k,), -1, dtype=torch.int32, device=DEV)
    hip.topk(xptr, n, wd, 1.0 / R.widen(p["temp"]), R.widen(p["penalty"]), k, val, ids)
    torch.cuda.synchronize()
    return val.cpu().numpy(), ids.cpu().numpy()


def check(rows, xptr, ldx, params, o, what, against_single=True):
    B, n = rows.shape
    R.check_rows(list(rows), params, o["val"], o["id"])
    raw = o.view(np.uint8).reshape(B, OUT_BYTES)
    for b, p in enumerate(params):
        k = p["k"]
        assert (raw[b, 8 * k:8 * hip.TOPK_MAX] == FILL).all() and (raw[b, 8 * hip.TOPK_MAX + 4 * k:] == FILL).all(), \
            (what, b, "entries past k were written")
        if against_single:
            sv, si = single(xptr + 4 * b * ldx, n, p)
            assert np.array_equal(o["id"][b][:k], si), (what, b)
            assert np.array_equal(o["val"][b][:k].view(np.uint64), sv.view(np.uint64)), (what, b)


def odd_ldx(n):
    return n + 3 if (n + 3) % 2 else n + 4


@pytest.mark.parametrize("B", [1, 3, 32])
@pytest.mark.parametrize("n", [1, 20, 257, 1025, 4099, 50400, 250880])
def test_rows_match_single_launches_and_numpy(n, B):
    """ldx > n and odd, the buffer one float in: every row is 4-byte aligned only.  n = 1025 puts one
    id past the first 1024; n = 250,880 takes the most workgroups a row gets."""
    rows = rows_of(n, B)
    ldx = odd_ldx(n)
    buf, xptr = strided(rows, ldx, lead=1)
    assert any((xptr + 4 * b * ldx) % 16 for b in range(B))
    params = [row_params(rows[b], b) for b in range(B)]
    for p, x in zip(params, rows):  # tie-free through k + 1: the reference's own order is what is checked
        c = np.sort(R.candidates(x, p["win"], p["temp"], p["penalty"]))[::-1][:p["k"] + 1]
        assert np.unique(c).size == c.size
    out, _ = launch_rows(xptr, ldx, n, params)
    torch.cuda.synchronize()
    check(rows, xptr, ldx, params, unpack(out), (n, B))


@pytest.mark.parametrize("n", [1025, 50400])
def test_dense_rows_and_every_workgroup_count_give_the_same_bytes(n):
    """ldx == n, and vsim_topk_rows_set_wg from one workgroup per row to 64: the split of a row does
    not show in its 768 bytes."""
    B = 5
    rows = rows_of(n, B)
    buf, xptr = strided(rows, n)
    params = [row_params(rows[b], b + 3) for b in range(B)]
    old = hip.topk_rows_set_wg(0)
    try:
        want = None
        for wg in (0, 1, 2, 7, 16, 64):
            hip.topk_rows_set_wg(wg)
            out, _ = launch_rows(xptr, n, n, params)
            torch.cuda.synchronize()
            o = unpack(out)
            if want is None:
                check(rows, xptr, n, params, o, (n, wg))
                want = o.tobytes()
            assert o.tobytes() == want, wg
    finally:
        hip.topk_rows_set_wg(old)


@pytest.mark.parametrize("n", [257, 50400])
def test_a_row_does_not_depend_on_its_place_or_its_batch(n):
    B = 32
    rows = rows_of(n, B)
    ldx = odd_ldx(n)
    p0 = row_params(rows[0], 9)
    # the row first in a batch of 32, last in another whose other rows and parameters differ, and alone
    a = np.array(rows)
    b = np.array(rows[::-1])
    b[:-1] *= np.float32(1.5)
    pa = [p0] + [row_params(a[i], i) for i in range(1, B)]
    pb = [row_params(b[i], i + 5) for i in range(B - 1)] + [p0]
    got = []
    for data, params, idx in ((a, pa, 0), (b, pb, B - 1), (a[:1], [p0], 0)):
        buf, xptr = strided(data, ldx)
        out, _ = launch_rows(xptr, ldx, n, params)
        torch.cuda.synchronize()
        o = unpack(out)
        R.check_rows(list(data), params, o["val"], o["id"])
        got.append(o[idx].tobytes())
    assert len(got[0]) == 768 and got[0] == got[1] == got[2]


def test_ties_signed_zeros_and_minus_infinity():
    n, B = 4099, 6
    g = np.random.default_rng(5)
    levels = np.array([-3.5, -1.0, -0.0, 0.0, 0.25, 1.0, 2.0, 2.0000002], np.float32)
    rows = np.empty((B, n), np.float32)
    rows[0] = 1.25                                                              # all equal
    rows[1] = np.where(g.integers(0, 2, n) == 1, np.float32(-0.0), np.float32(0.0))  # +-0.0
    rows[2] = levels[g.integers(0, 8, n)]                                       # massive ties
    rows[3] = g.standard_normal(n)
    rows[3][g.permutation(n)[:n - 29]] = -np.inf                                # -inf entries reach the list
    rows[4] = -np.inf
    rows[5] = rows[1]
    params = [dict(win=[], temp=0.85, penalty=1.3, k=64),
              dict(win=[], temp=1.0, penalty=1.0, k=20),
              dict(win=[int(t) for t in np.flatnonzero(rows[2] == levels[-1])[:40]], temp=0.85, penalty=1.3, k=40),
              dict(win=[int(t) for t in g.integers(0, n, 64)], temp=0.85, penalty=1.3, k=64),
              dict(win=[0, 5], temp=0.7, penalty=1.2, k=20),
              dict(win=[1, 2, 3, 250], temp=0.85, penalty=1.3, k=20)]
    buf, xptr = strided(rows, n + 1)
    out, _ = launch_rows(xptr, n + 1, n, params)
    torch.cuda.synchronize()
    o = unpack(out)
    check(rows, xptr, n + 1, params, o, "specials")
    assert list(o["id"][0]) == list(range(64))
    assert list(o["id"][4][:20]) == list(range(20)) and np.isneginf(o["val"][4][:20]).all()
    for b in (1, 5):  # the values keep the logits' sign bits
        k = params[b]["k"]
        assert np.array_equal(np.signbit(o["val"][b][:k]), np.signbit(rows[b][o["id"][b][:k]]))
    assert np.signbit(o["val"][1][:20]).any() and not np.signbit(o["val"][1][:20]).all()


def test_back_to_back_launches_share_the_workspace():
    """B = 32, B = 5 and a vsim_op_topk on one stream with no synchronize in between, twice over."""
    n = 50400
    rows = rows_of(n, 32)
    buf, xptr = strided(rows, n)
    p32 = [row_params(rows[b], b) for b in range(32)]
    p5 = [row_params(rows[b + 8], b + 1, seed=3) for b in range(5)]
    p1 = row_params(rows[20], 6, seed=4)
    w1 = torch.tensor(np.asarray(p1["win"], np.int64).astype(np.int32), device=DEV)
    torch.cuda.synchronize()
    outs = []
    for _ in range(2):
        o32, k32 = launch_rows(xptr, n, n, p32)
        o5, k5 = launch_rows(xptr + 4 * 8 * n, n, n, p5)
        val = torch.zeros(p1["k"], dtype=torch.float64, device=DEV)
        ids = torch.zeros(p1["k"], dtype=torch.int32, device=DEV)
        hip.topk(xptr + 4 * 20 * n, n, w1, 1.0 / R.widen(p1["temp"]), R.widen(p1["penalty"]), p1["k"], val, ids)
        outs.append((o32, o5, val, ids, k32, k5))
    torch.cuda.synchronize()
    for o32, o5, val, ids, _, _ in outs:
        a, b = unpack(o32), unpack(o5)
        R.check_rows(list(rows), p32, a["val"], a["id"])
        R.check_rows(list(rows[8:13]), p5, b["val"], b["id"])
        R.check_rows([rows[20]], [p1], [val.cpu().numpy()], [ids.cpu().numpy()])


def test_any_block_contents_stay_in_bounds():
    """k and nw outside their limits are clamped by the kernel; k > n repeats id n - 1."""
    n, B = 20, 4
    rows = rows_of(n, B)
    buf, xptr = strided(rows, n)
    a = np.zeros(B, hip.TOPK_PARAMS_DTYPE)
    a["scale"], a["penalty"] = 1.0, 1.0
    a["k"] = [0, -5, 1000, 40]
    a["nw"] = [-3, 2 ** 31 - 1, 0, 5000]
    a["win"] = 3
    out = torch.full((B * OUT_BYTES,), FILL, dtype=torch.uint8, device=DEV)
    hip.topk_rows(xptr, n, n, B, torch.tensor(a.view(np.uint8).reshape(-1), device=DEV), out)
    torch.cuda.synchronize()
    o = unpack(out)
    for b, k in enumerate((1, 1, 64, 40)):
        ids = o["id"][b][:k]
        assert ((ids >= 0) & (ids < n)).all()
        pen = [] if b in (0, 2) else [3]
        wv, wi = R.topk(rows[b], pen, 1.0, 1.0, min(k, n))
        assert np.array_equal(ids[:n], wi) and (ids[n:] == n - 1).all()


def test_argument_errors():
    L = hip.lib()
    x = torch.zeros(4 * 128, dtype=torch.float32, device=DEV)
    pb = torch.zeros(33 * hip.TOPK_PARAMS_DTYPE.itemsize, dtype=torch.uint8, device=DEV)
    out = torch.zeros(33 * OUT_BYTES, dtype=torch.uint8, device=DEV)
    X, P, O_ = x.data_ptr(), pb.data_ptr(), out.data_ptr()
    for args in ((X, 128, 128, 0, P, O_), (X, 128, 128, 33, P, O_), (X, 128, 128, -1, P, O_),
                 (X, 128, 0, 1, P, O_), (X, 128, -4, 1, P, O_), (X, 127, 128, 2, P, O_),
                 (None, 128, 128, 1, P, O_), (X, 128, 128, 1, None, O_), (X, 128, 128, 1, P, None)):
        assert L.vsim_op_topk_rows(*args, None) == EINVAL, args
    assert b"topk_rows" in L.vsim_last_error()
    assert L.vsim_op_topk_rows(X, 128, 128, 4, P, O_, None) == 0  # (k = 0 in the blocks: clamped)
    torch.cuda.synchronize()
    assert hip.TOPK_PARAMS_DTYPE.itemsize == 4120 and OUT_BYTES == 768
