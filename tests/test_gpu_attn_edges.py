"""The exact decode heads (attn.hpp attn_body) on adversarial rows and at deep positions, bit for
bit against the oracle's ops, through both of its instantiations: k_attn_decode_batch
(vsim_op_attn_decode_batch: 1024 threads, one workgroup per head) and the fused layer tail's head
role (vsim_op_tail_attn: 704 threads, write-through stores, one or two workgroups per head).

The rows come from tests/attn_edges.py; tests/test_attn_edges_cpu.py shows on the CPU that each
family does what it is named after (the certificate rows defeat an exactly summed score, so only
the kernel's sequential redo of the key gives the oracle's bits).  No tolerances anywhere.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import attn_edges as A  # noqa: E402
from vsim_amd import hip  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
EINVAL = -1
N_CTX = 512
CASES, QUANT_CASES, ids = A.CASES, A.QUANT_CASES, A.case_id
DEEP_CASES = [(0, 64, 2, 32, False, 1), (0, 64, 3, 0, True, 3), (0, 256, 3, 64, False, 1), (1, 256, 2, 64, False, 3)]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def tail_splits(d):
    """The fused tail's head splits for head dim d: column parts are whole 32-blocks."""
    return (1, 2) if (d // 2) % 32 == 0 else (1,)


class Result:
    """One row's device results: out, the Q4 row (SoA as stored, and AoS), its factors, the cache
    rows at pos and whether everything past pos is still NaN."""

    def __init__(self, out, oq, oxd, kc, vc, pos, E):
        aos = torch.empty_like(oq)
        hip.check(hip.lib().vsim_op_act_unpack(oq.data_ptr(), aos.data_ptr(), 1, E, None), "act_unpack")
        xq2 = torch.empty_like(oq)
        xd2 = torch.empty_like(oxd)
        hip.check(hip.lib().vsim_op_q4_quantize(out.data_ptr(), E, 1, xq2.data_ptr(), xd2.data_ptr(), None), "quantize")
        self.out, self.soa, self.aos, self.oxd = host(out), host(oq), host(aos), host(oxd)
        self.requant = (host(xq2), host(xd2))
        kh, vh = host(kc), host(vc)
        self.k, self.v = kh[pos], vh[pos]
        self.rest_nan = bool(np.isnan(kh[pos + 1:]).all() and np.isnan(vh[pos + 1:]).all())

    def same_as(self, o):
        return (np.array_equal(bits(self.out), bits(o.out)) and np.array_equal(self.soa, o.soa) and
                np.array_equal(bits(self.oxd), bits(o.oxd)) and np.array_equal(bits(self.k), bits(o.k)) and
                np.array_equal(bits(self.v), bits(o.v)))


def run_batch(case, rows, n_ctx, sl):
    """vsim_op_attn_decode_batch over up to four rows at once: [Result]."""
    style, d, H, n_rot, _, nth = case
    B, E = len(rows), d * H
    assert B <= 4
    q, k, v = (dev(np.stack([r[i] for r in rows])) for i in range(3))
    kcs, vcs = [dev(r[3]) for r in rows], [dev(r[4]) for r in rows]
    kp = torch.tensor([t.data_ptr() for t in kcs], dtype=torch.int64, device=DEV)
    vp = torch.tensor([t.data_ptr() for t in vcs], dtype=torch.int64, device=DEV)
    npd = dev(np.asarray([r[5] for r in rows], np.int32))
    out = torch.full((B, E), float("nan"), dtype=torch.float32, device=DEV)
    oq = torch.zeros(B * E // 32 * 20, dtype=torch.uint8, device=DEV)
    oxd = torch.full((B, E), float("nan"), dtype=torch.float32, device=DEV)
    hip.attn_decode_batch(q, k, v, kp, vp, npd, None, sl, B, d, H, n_rot, style, n_ctx, nth, float(A.head_scale(d)),
                          out, oq, oxd)
    nb = E // 32
    res = []
    for b, r in enumerate(rows):  # row b's Q4 SoA row: its nibbles, then its scales
        oq_b = torch.cat([oq[b * nb * 16:(b + 1) * nb * 16], oq[B * nb * 16 + b * nb * 4:B * nb * 16 + (b + 1) * nb * 4]])
        res.append(Result(out[b].contiguous(), oq_b.contiguous(), oxd[b].contiguous(), kcs[b], vcs[b], r[5], E))
    return res


def run_tail(case, row, n_ctx, sl, nsplit):
    """vsim_op_tail_attn for one row on fresh caches: Result."""
    style, d, H, n_rot, _, nth = case
    E = d * H
    q, k, v, kc, vc = (dev(row[i]) for i in range(5))
    kp = torch.tensor([kc.data_ptr()], dtype=torch.int64, device=DEV)
    vp = torch.tensor([vc.data_ptr()], dtype=torch.int64, device=DEV)
    npd = dev(np.asarray([row[5]], np.int32))
    out = torch.full((E,), float("nan"), dtype=torch.float32, device=DEV)
    oq = torch.zeros(E // 32 * 20, dtype=torch.uint8, device=DEV)
    oxd = torch.full((E,), float("nan"), dtype=torch.float32, device=DEV)
    hip.tail_attn(q, k, v, kp, vp, npd, None, sl, d, H, n_rot, style, n_ctx, nth, float(A.head_scale(d)), out, oq,
                  oxd, nsplit)
    return Result(out, oq, oxd, kc, vc, row[5], E)


def check_rows(case, rows, n_ctx, what):
    """Every row through the batch entry (four at a time) and through the tail entry at each
    split: out, the Q4 AoS row, the factors and both cache
    rows equal the oracle's, and the tail's row equals the batch entry's."""
    d, H, alibi = case[1], case[2], case[4]
    sl = dev(A.slopes(H)) if alibi else None
    refs = [A.reference_row(case, r) for r in rows]
    got = []
    for i in range(0, len(rows), 4):
        got += run_batch(case, rows[i:i + 4], n_ctx, sl)
    entries = [("batch", got)]
    for sp in tail_splits(d):
        entries.append((f"tail/{sp}", [run_tail(case, r, n_ctx, sl, sp) for r in rows]))
    for name, res in entries:
        for i, (r, ref, g) in enumerate(zip(rows, refs, res)):
            tag = (what, name, i, r[5])
            assert np.array_equal(bits(g.out), bits(ref[0])), tag + ("out",)
            assert np.array_equal(g.aos, ref[1]), tag + ("Q4 row",)
            assert np.array_equal(bits(g.k), bits(ref[2])), tag + ("K cache row",)
            assert np.array_equal(bits(g.v), bits(ref[3])), tag + ("V cache row",)
            assert g.rest_nan, tag + ("cache past pos",)
            # the Q4 row and its factors are vsim_op_q4_quantize's of the float row
            assert np.array_equal(g.soa, g.requant[0]) and np.array_equal(bits(g.oxd), bits(g.requant[1])), tag
            if name != "batch":
                assert g.same_as(got[i]), tag + ("tail vs batch",)
    return len(entries)


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_gross_certificate_rows(case):
    n = check_rows(case, [r for r, _ in A.cert_gross(case, N_CTX)], N_CTX, "cert_gross")
    assert n == 1 + len(tail_splits(case[1]))


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_one_ulp_certificate_rows(case):
    rows = list(A.cert_one_ulp(case, N_CTX))
    assert len(rows) == A.ONE_ULP_ROWS >= 8
    check_rows(case, rows, N_CTX, "cert_one_ulp")


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_softmax_extremes(case):
    for name, rows in A.softmax_rows(case, N_CTX).items():
        check_rows(case, rows, N_CTX, name)


@pytest.mark.parametrize("case", QUANT_CASES, ids=ids)
def test_quantizer_edge_rows(case):
    x, y = A.qrow_edges()
    rows = A.quant_rows(case, N_CTX)
    check_rows(case, rows, N_CTX, "quant")
    # (and the bytes are the golden ones, not only the oracle's of today)
    assert np.array_equal(A.reference_row(case, rows[0])[1], y) and np.array_equal(A.reference_row(case, rows[1])[1], y)


def deep_positions(d, n_ctx):
    """The V ring's steady state from its first tile on (t + 3 < nt: n_past >= 3 KT) for the
    unsplit head (KT = 8192 / d keys per tile) and the split one (twice that), the 1024 boundary,
    and the last cache row (the last score slot before the V tiles in LDS)."""
    kt = 8192 // d
    return sorted({3 * kt - 1, 3 * kt, 4 * kt + 1, 6 * kt - 1, 6 * kt, 8 * kt + 1, 1023, 1024, n_ctx - 1})


@pytest.mark.parametrize("case", DEEP_CASES, ids=ids)
def test_deep_positions(case):
    d = case[1]
    n_ctx = 2048
    rows = [A.gaussian_row(case, n_ctx, pos, 100 + pos) for pos in deep_positions(d, n_ctx)]
    # (n_ctx = 2048 at d = 256 is past the context up to which the executor fuses the heads, but
    # within the kernel's LDS: the tail entry takes it)
    assert check_rows(case, rows, n_ctx, "deep") == 3


def test_tail_attn_argument_errors():
    d, H = 64, 2
    z = torch.zeros(4096 * 4, dtype=torch.float32, device=DEV)
    o = torch.zeros(4096 * 4, dtype=torch.float32, device=DEV)
    oq = torch.zeros(4096 * 4, dtype=torch.uint8, device=DEV)
    c = torch.full((2, 2048 * 256), float("nan"), dtype=torch.float32, device=DEV)
    p = torch.tensor([c[0].data_ptr()], dtype=torch.int64, device=DEV)
    pv = torch.tensor([c[1].data_ptr()], dtype=torch.int64, device=DEV)
    n = torch.zeros(1, dtype=torch.int32, device=DEV)
    L = hip.lib()

    def args(B=1, d=d, H=H, n_ctx=N_CTX):
        return hip.AttnBatchArgs(z.data_ptr(), z.data_ptr(), z.data_ptr(), p.data_ptr(), pv.data_ptr(), n.data_ptr(),
                                 None, None, B, d, H, 0, 0, n_ctx, 1, 1.0, None, oq.data_ptr(), o.data_ptr())

    assert L.vsim_op_tail_attn(hip.AttnBatchArgs(), 1, None) == EINVAL
    assert L.vsim_op_tail_attn(args(B=2), 1, None) == EINVAL
    assert L.vsim_op_tail_attn(args(), 0, None) == EINVAL and L.vsim_op_tail_attn(args(), 3, None) == EINVAL
    assert L.vsim_op_tail_attn(args(d=48), 1, None) == EINVAL and L.vsim_op_tail_attn(args(d=512), 1, None) == EINVAL
    assert L.vsim_op_tail_attn(args(d=96), 2, None) == EINVAL  # 48-column parts are no whole blocks
    assert L.vsim_op_tail_attn(args(d=32, H=65), 2, None) == EINVAL  # H * nsplit > 128
    assert L.vsim_op_tail_attn(args(d=256, n_ctx=40000), 1, None) == EINVAL  # the scores alone exceed the LDS
    assert L.vsim_op_tail_attn(args(), 2, None) == 0
    torch.cuda.synchronize()
