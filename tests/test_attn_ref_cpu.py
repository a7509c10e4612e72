"""The teeth of tests/attn_ref.py, shown without a GPU: a float32 / float16 numpy emulation of
attn_prefill.hip's block loop (64-key blocks, the running maximum, alpha, fp32 l, fp16 P, V^T read
in vt_pos order from the scratch image) passes the checker, with fp16-denormal probabilities kept
and flushed; each mutation of it -- the mistakes a kernel of this kind makes -- is rejected, at a
flat and at a peaked score scale (Q x 1 and Q x 8)."""
import numpy as np
import pytest

import attn_ref as R

F32 = np.float32


def emulate(Q, K16, Vt16, d, n_past, scale, ftz=False, mut=None, mut_key=5):
    """k_attn_prefill_f16's arithmetic per query on the scratch images K16 [nk][E], Vt16 [H][d][ldt].
    mut: mask+1 (a query sees the key after its own), mask-1 (it misses its own), drop (key
    mut_key contributes nothing), noalpha (O is not rescaled when the maximum moves)."""
    N, E = Q.shape
    nk = n_past + N
    q16 = R.q16_of(Q, scale).astype(F32)
    qpos = n_past + np.arange(N)
    out = np.empty((N, E), F32)
    with np.errstate(invalid="ignore"):
        for h in range(E // d):
            sl = slice(h * d, (h + 1) * d)
            m = np.full(N, -np.inf, F32)
            l = np.zeros(N, F32)
            O = np.zeros((N, d), F32)
            for k0 in range(0, R.ldt_of(nk), R.AP_BK):
                keys = k0 + np.arange(R.AP_BK)
                s = q16[:, sl] @ K16[np.minimum(keys, nk - 1), sl].astype(F32).T
                lim = qpos + {"mask+1": 1, "mask-1": -1}.get(mut, 0)
                s[keys[None, :] > lim[:, None]] = -np.inf
                mnew = np.maximum(m, s.max(axis=1))
                alpha = np.where(mnew == -np.inf, F32(1), np.exp2(m - mnew)).astype(F32)
                p = np.where(s == -np.inf, F32(0), np.exp2(s - mnew[:, None])).astype(F32)
                if mut == "drop":
                    p[:, keys == mut_key] = 0
                l = l * alpha + p.sum(axis=1, dtype=F32)
                P = p.astype(np.float16)
                if ftz:
                    P[P < R.DENORM] = 0
                if mut != "noalpha":
                    O *= alpha[:, None]
                O += P.astype(F32) @ Vt16[h][:, k0 + R.vt_pos(np.arange(R.AP_BK))].astype(F32).T
                m = mnew
            out[:, sl] = O / l[:, None]
    return out


D, H, N, NPAST = 64, 2, 150, 37  # three key blocks, 5 padding columns, two 128-query blocks
SCALE = float(F32(1.0 / np.sqrt(D)))


@pytest.fixture(scope="module", params=[1.0, 8.0], ids=["flat", "peaked"])
def case(request):
    rng = np.random.default_rng(11)
    E, nk = D * H, NPAST + N
    Q = (rng.standard_normal((N, E)) * request.param).astype(F32)
    K = rng.standard_normal((nk, E)).astype(F32)
    V = rng.standard_normal((nk, E)).astype(F32)
    return Q, K, V, R.Ref(Q, K, V, D, NPAST, SCALE)


def test_vt_pos():
    p = R.vt_pos(np.arange(64))
    assert p[:16].tolist() == [0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7, 12, 13, 14, 15]
    assert np.array_equal(p[16:32], 16 + p[:16]) and np.array_equal(R.vt_pos(p), np.arange(64))
    assert int(R.vt_pos(1000)) == 1000 - 8 + 4  # 1000 % 16 == 8


def test_images():
    rng = np.random.default_rng(2)
    K, V = (rng.standard_normal((70, 128)).astype(F32) for _ in range(2))
    K16, Vt = R.kv_images(K, V, 64)
    assert Vt.shape == (2, 64, 128) and not Vt[:, :, 80:].any()
    assert Vt[1, 3, 8] == np.float16(V[4, 67]) and Vt[1, 3, 72] == np.float16(V[68, 67]) and Vt[0, 0, 68] == 0
    assert R.images_mismatch(K16, Vt, K, V, 64) is None
    stale = Vt.copy()
    stale[1, 7, 75] = 1.0  # (key 71 of 70: a padding column)
    assert "padding" in R.images_mismatch(K16, stale, K, V, 64)
    assert R.images_mismatch(K16, R.kv_images(K, V, 64, swap=False)[1], K, V, 64) is not None


@pytest.mark.parametrize("ftz", [False, True], ids=["denormals", "flushed"])
def test_emulation_within_bound(case, ftz):
    Q, K, V, ref = case
    K16, Vt = R.kv_images(K, V, D)
    r = ref.check(emulate(Q, K16, Vt, D, NPAST, SCALE, ftz=ftz), "emulation")
    print(f"emulation (ftz={ftz}): max ratio {r:.3f}, c up to {ref.c.max():.2f}")


@pytest.mark.parametrize("mut", ["mask+1", "mask-1", "drop", "noalpha"])
def test_mutation_rejected(case, mut):
    Q, K, V, ref = case
    K16, Vt = R.kv_images(K, V, D)
    r = ref.ratio(emulate(Q, K16, Vt, D, NPAST, SCALE, mut=mut))
    print(f"{mut}: ratio {r:.3g}")
    assert r > 4.0
    with pytest.raises(AssertionError):
        ref.check(emulate(Q, K16, Vt, D, NPAST, SCALE, mut=mut), mut)


def test_unswapped_quads_rejected(case):
    Q, K, V, ref = case
    K16, Vt = R.kv_images(K, V, D, swap=False)  # (the kernel still reads in vt_pos order)
    assert ref.ratio(emulate(Q, K16, Vt, D, NPAST, SCALE)) > 4.0


def test_pad_column_rejected(case):
    """A stale padding column: the image check sees any non-zero half; the attention multiplies
    it by a zero probability, so only a NaN or an infinity there reaches the output -- as NaN."""
    Q, K, V, ref = case
    K16, Vt = R.kv_images(K, V, D)
    Vt[1, 9, R.vt_pos(NPAST + N + 1)] = 3.0
    assert R.images_mismatch(K16, Vt, K, V, D) is not None
    Vt[1, 9, R.vt_pos(NPAST + N + 1)] = np.inf
    y = emulate(Q, K16, Vt, D, NPAST, SCALE)
    assert ref.ratio(y) == np.inf
    with pytest.raises(AssertionError):
        ref.check(y, "pad")
