"""The fast-mode prompt layer as a whole (run_layer / PromptBatch::mm / run_head in VSIM_MODE_FAST,
vsim_amd/csrc/model.cpp), pinned in two steps that leave no slack between them:

(a) Wiring.  A middle pipeline stage (layer 1 of a three-layer file, resid_in -> resid_out) equals, bit
    for bit on all N x E values, the same launches made here through the op entries: same order, same
    shapes, the file's weights repacked with vsim_op_q4_repack, one KV cache and one attention scratch
    of the composition's own kept across a batch pair.  Which launch a shape takes is read from the
    thresholds documented in include/vsim_hip.h (fast_prompt_ref.plan restates them); the process-wide
    switches stay at their defaults.  The second eval of a pair runs on the first one's cache rows, so
    its equality also shows that the cache rows and the fp16 K / V^T copies are the same.
(b) Meaning.  Every intermediate of that composition is checked against tests/fast_prompt_ref.py: the
    fp64 value of the step, computed from the composition's actual input to it, under the step's bound
    (derived there; none fitted).  The worst error / bound per stage is printed (RATIO lines;
    profiles/fast_prompt_layer_ratios.txt holds a run's).
(c) Whole model.  Tokens in, the last row's logits out, for two-layer models: embedding rows, both
    layers and the head, bit for bit; and every row of vsim_model_eval_score's logits_all.

Measured on MI355X (profiles/fast_prompt_layer_ratios.txt): all 28 layer cases, the whole models and the
scoring rows equal bit for bit; GEMM stages 0.0002 - 0.005 of their bound, the residual join in fc_out's
epilogue up to 0.18, the attention 0.23 - 0.63, the f32 LayerNorm below 8 rows up to 0.75 (the bias add's
one rounding), the f32 GELU below 8 rows up to 0.87 (two fp16 roundings, argument and table entry, in equal
parts); ambiguous elements of a quantizing stage at most 1.03 % (the GELU operand).
"""
import ctypes
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import fast_prompt_ref as P  # noqa: E402
import fast_ref as R  # noqa: E402
from vsim_amd import hip  # noqa: E402
from vsim_amd import modelgen as mg  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
N_CTX = 512
ARCH = {"gptj": hip.ARCH_GPTJ, "gptneox": hip.ARCH_GPTNEOX, "bloom": hip.ARCH_BLOOM}


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)  # (a copy: the file's tensors are read-only views)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def f32(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def f16(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float16, device=DEV)


def ck(rc, what):
    hip.check(rc, what)


def p(t):
    return None if t is None else t.data_ptr()


@functools.lru_cache(maxsize=None)
def rope_table(n_rot):
    return R.rope_table(N_CTX, n_rot) if n_rot else None


class DevWeights:
    """A fast_prompt_ref.Weights on the device: matrices as W4T32 (vsim_op_q4_repack), vectors f32."""

    def __init__(self, W):
        self.shape = W.shape
        self.w, self.f = {}, {k: dev(v) for k, v in W.f.items()}
        for role, aos in W.aos.items():
            M, K = W.shape[role]
            src = dev(aos)
            buf = torch.zeros(hip.q4_bytes(M, K) + hip.FAST_PAD, dtype=torch.uint8, device=DEV)
            ck(hip.lib().vsim_op_q4_repack(src.data_ptr(), buf.data_ptr(), M, K, None), "repack")
            self.w[role] = buf
        torch.cuda.synchronize()


class Q4Rows:
    """vsim_op_q4_quantize's output for n rows of k values."""

    def __init__(self, n, k):
        self.n, self.k = n, k
        self.xq = torch.zeros(hip.q4_bytes(n, k), dtype=torch.uint8, device=DEV)
        self.xd = torch.zeros(n * k, dtype=torch.float32, device=DEV)

    def make(self, x):
        ck(hip.lib().vsim_op_q4_quantize(x.data_ptr(), self.k, self.n, self.xq.data_ptr(), self.xd.data_ptr(), None), "quantize")
        return self

    def parse(self):
        aos = torch.empty(self.n * self.k // 32 * 20, dtype=torch.uint8, device=DEV)
        ck(hip.lib().vsim_op_act_unpack(self.xq.data_ptr(), aos.data_ptr(), self.n, self.k, None), "act_unpack")
        return R.q4_parse(host(aos), self.k)


class Comp:
    """The model's prompt launches through the op entries, on buffers of its own."""

    def __init__(self, cfg, layers, glob=None):
        self.cfg, E = cfg, cfg.E
        self.L = [DevWeights(W) for W in layers]
        self.G = DevWeights(glob) if glob is not None else None
        self.kc = [torch.zeros((N_CTX, E), dtype=torch.float32, device=DEV) for _ in layers]
        self.vc = [torch.zeros((N_CTX, E), dtype=torch.float32, device=DEV) for _ in layers]
        b = ctypes.c_size_t()
        ck(hip.lib().vsim_op_attn_prefill_layout(E, N_CTX, ctypes.byref(b), None, None), "layout")
        self.scr_bytes = b.value
        self.scr = torch.zeros(b.value // 2, dtype=torch.int16, device=DEV)
        self.cs = dev(rope_table(cfg.n_rot)) if cfg.n_rot else None
        self.slopes = dev(P.alibi_slopes(cfg.H)) if cfg.alibi else None
        self.scale = float(np.float32(1.0 / np.sqrt(float(np.float32(E) / np.float32(cfg.H)))))

    # ---- products (PromptBatch::mm): the fp16 operand on the wide or the small-tile GEMM, else Q4 rows
    def mm(self, w, shape, N, bias, y, x16=None, q4=None):
        lib, (M, K) = hip.lib(), shape
        if x16 is not None and N >= 256 and K % 64 == 0:
            ck(lib.vsim_op_gemm_q4_256(p(w), M, K, p(x16), N, p(bias), p(y), None, None, 0, 0, 0, 0, None, None), "gemm_q4_256")
        elif x16 is not None:
            ck(lib.vsim_op_gemm_q4_f16x(p(w), M, K, p(x16), N, p(bias), p(y), None), "gemm_q4_f16x")
        else:
            ck(lib.vsim_op_q4_gemv(p(w), M, K, p(q4.xq), p(q4.xd), N, p(bias), p(y), hip.MODE_FAST, None), "q4_gemv")

    def norm(self, x, N, w, b, x16, y):
        """LayerNorm + affine: straight to the fp16 operand, or f32 rows."""
        lib, E = hip.lib(), self.cfg.E
        if x16 is not None:
            ck(lib.vsim_op_norm_f16q(p(x), E, N, p(w), p(b), p(x16), None), "norm_f16q")
        else:
            ck(lib.vsim_op_norm(p(x), p(y), E, N, p(w), p(b), None), "norm")

    def layer(self, i, inpL, n_past, rec=None):
        """One layer on the residual rows inpL [N][E] (updated in place); rec collects every intermediate."""
        cfg, lib, W = self.cfg, hip.lib(), self.L[i]
        N, E, H, d, F = inpL.shape[0], cfg.E, cfg.H, cfg.d, cfg.F
        pl = P.plan(cfg, N)
        w, f, shp = W.w, W.f, W.shape
        kc, vc = self.kc[i], self.vc[i]
        row = n_past * E * 4
        nk = n_past + N
        rec = {} if rec is None else rec

        def keep(key, t):
            rec[key] = t.clone() if torch.is_tensor(t) else t

        keep("inpL", inpL)
        xa = f16(N, E) if pl.pf else None
        xb = f16(N, F) if pl.pf else None
        cur1, q1 = (None, None) if pl.pf else (f32(N, E), Q4Rows(N, E))
        self.norm(inpL, N, f["ln1_w"], f["ln1_b"], xa, cur1)
        if pl.pf:
            keep("xa", xa)
        else:
            q1.make(cur1)
            keep("cur1", cur1)
            rec["xq1"] = q1.parse()
        bq, bk, bv, bo = (f.get(k) if cfg.bias else None for k in ("bq", "bk", "bv", "bo"))
        Qb, Kb, Vb = f32(N, E), f32(N, E), f32(N, E)
        if pl.rope_epi:
            vt_off, ldt = ctypes.c_size_t(), ctypes.c_int()
            ck(lib.vsim_op_attn_prefill_layout(E, nk, None, ctypes.byref(vt_off), ctypes.byref(ldt)), "layout")
            k16, vt16 = self.scr.data_ptr(), self.scr.data_ptr() + 2 * vt_off.value
            rope = (p(self.cs), d, cfg.n_rot, n_past)
            if pl.pair and pl.kv16:
                ck(lib.vsim_op_gemm_q4_256_pair_h16(p(w["wq"]), p(w["wk"]), E, E, p(xa), N, p(Qb), kc.data_ptr() + row, *rope,
                                                    k16, None), "pair_h16")
            elif pl.pair:
                ck(lib.vsim_op_gemm_q4_256_pair(p(w["wq"]), p(w["wk"]), E, E, p(xa), N, p(Qb), kc.data_ptr() + row, *rope,
                                                None), "pair")
            else:
                ck(lib.vsim_op_gemm_q4_256(p(w["wq"]), E, E, p(xa), N, None, p(Qb), None, *rope, 0, None, None), "gemm Q")
                if pl.kv16:
                    ck(lib.vsim_op_gemm_q4_256_h16(p(w["wk"]), E, E, p(xa), N, None, kc.data_ptr() + row, *rope, k16, 0, 0,
                                                   None), "gemm K h16")
                else:
                    ck(lib.vsim_op_gemm_q4_256(p(w["wk"]), E, E, p(xa), N, None, kc.data_ptr() + row, None, *rope, 0, None,
                                               None), "gemm K")
            if pl.kv16:
                ck(lib.vsim_op_gemm_q4_256_h16(p(w["wv"]), E, E, p(xa), N, None, vc.data_ptr() + row, None, 0, 0, n_past,
                                               vt16, ldt.value, 1, None), "gemm V h16")
            else:
                ck(lib.vsim_op_gemm_q4_256(p(w["wv"]), E, E, p(xa), N, None, vc.data_ptr() + row, None, None, 0, 0, 0, 0,
                                           None, None), "gemm V")
        else:
            for role, b, y in (("wq", bq, Qb), ("wk", bk, Kb), ("wv", bv, Vb)):
                self.mm(w[role], shp[role], N, b, y, xa, q1)
            keep("Qb", Qb)
            keep("Kb", Kb)
            keep("Vb", Vb)
            ck(lib.vsim_op_rope_kv_write(cfg.style, p(Qb), p(Kb), p(Vb), p(kc), p(vc), d, H, N, n_past, cfg.n_rot, None),
               "rope_kv_write")
        keep("Q", Qb)
        keep("Knew", kc[n_past:nk])
        keep("Vnew", vc[n_past:nk])
        if n_past:
            keep("kc_old", kc[:n_past])
            keep("vc_old", vc[:n_past])
        attn_in = f32(N, E)
        if pl.attn16:
            ck(lib.vsim_op_attn_prefill_scratch(p(Qb), p(kc), p(vc), d, H, N, n_past, self.scale,
                                                None if pl.attn_q16 else p(attn_in), p(xb) if pl.attn_q16 else None,
                                                p(self.scr), self.scr_bytes, 1 if pl.kv16 else 0, None), "attn_prefill")
        else:
            kq = f32(H, N, nk)
            ck(lib.vsim_op_kq_causal(p(kc), E, p(Qb), E, d, H, nk, N, n_past, p(kq), None), "kq")
            if cfg.alibi:
                ck(lib.vsim_op_attn_softmax_alibi(p(kq), nk, N, H, n_past, self.scale, p(self.slopes), None), "softmax")
            else:
                ck(lib.vsim_op_attn_softmax(p(kq), nk, N, H, n_past, self.scale, None), "softmax")
            ck(lib.vsim_op_kqv_causal_merged(p(vc), E, p(kq), d, H, nk, N, n_past, p(attn_in), None), "kqv")
        q2 = None
        if pl.attn_q16:
            # the checker's side launches: the same attention writing f32, and its quantization
            side = f32(N, E)
            ck(lib.vsim_op_attn_prefill(p(Qb), p(kc), p(vc), d, H, N, n_past, self.scale, p(side), None), "attn side")
            side16 = f16(N, E)
            ck(lib.vsim_op_act_quant_f16(p(side), E, N, None, 0, p(side16), None), "act_quant side")
            keep("attn_in", side)
            keep("xb_a_side", side16)
        else:
            keep("attn_in", attn_in)
            if pl.pf:
                ck(lib.vsim_op_act_quant_f16(p(attn_in), E, N, None, 0, p(xb), None), "act_quant")
            else:
                q2 = Q4Rows(N, E).make(attn_in)
                rec["xq2"] = q2.parse()
        if pl.pf:
            keep("xb_a", xb.reshape(-1)[:N * E].reshape(N, E))  # (the [N][F] buffer's first N E halves)
        attn = f32(N, E)
        self.mm(w["wo"], shp["wo"], N, bo, attn, None if xb is None else xb, q2)
        keep("attn", attn)
        # the MLP's input
        serial, keep_joined = cfg.residual != "parallel", cfg.residual == "serial_joined"
        fq, cur2 = q1, None
        if cfg.two_norms:
            if serial:
                cur2 = attn.clone()  # (the model's device-to-device copy)
                ck(lib.vsim_op_add_rows(p(cur2), p(inpL), N * E, None), "add_rows")
                keep("joined", cur2)
            src = cur2 if serial else inpL
            ny = None if pl.pf else (f32(N, E) if keep_joined or not serial else cur2)
            self.norm(src, N, f["ln2_w"], f["ln2_b"], xa, ny)
            if pl.pf:
                keep("xa2", xa)
            else:
                keep("cur2", ny)
                fq = Q4Rows(N, E).make(ny)
                rec["xqn"] = fq.parse()
        fch = f32(N, F)
        q3 = None
        if pl.g2:
            ck(lib.vsim_op_gemm_q4_256(p(w["wfc"]), F, E, p(xa), N, p(f["bfc"]), None, p(xb), None, 0, 0, 0, 0, None, None),
               "fc_in gelu-quantize")
            # the checker's side launches: the plain GEMM and its bias + GELU + quantize
            self.mm(w["wfc"], shp["wfc"], N, None, fch, xa, None)
            side16 = f16(N, F)
            ck(lib.vsim_op_act_quant_f16(p(fch), F, N, p(f["bfc"]), 1, p(side16), None), "act_quant side")
            keep("fch", fch)
            keep("xb_g_side", side16)
            keep("xb_g", xb)
        else:
            self.mm(w["wfc"], shp["wfc"], N, None, fch, xa, fq)
            keep("fch", fch)
            if pl.pf:
                ck(lib.vsim_op_act_quant_f16(p(fch), F, N, p(f["bfc"]), 1, p(xb), None), "act_quant gelu")
                keep("xb_g", xb)
            else:
                ck(lib.vsim_op_gelu_bias(p(fch), p(fch), N * F, p(f["bfc"]), F, None), "gelu_bias")
                keep("g", fch)
                q3 = Q4Rows(N, F).make(fch)
                rec["xq3"] = q3.parse()
        # fc_out and the residual
        if pl.join_epi:
            ck(lib.vsim_op_gemm_q4_256(p(w["wproj"]), E, F, p(xb), N, p(f["bproj"]), p(inpL), None, None, 0, 0, 0, 1,
                                       None if serial else p(attn), None), "fc_out join")
        else:
            ff = f32(N, E)
            self.mm(w["wproj"], shp["wproj"], N, f["bproj"], ff, xb, q3)
            keep("ff", ff)
            if keep_joined:
                inpL.copy_(cur2)
                ck(lib.vsim_op_add_rows(p(inpL), p(ff), N * E, None), "add_rows")
            else:
                ck(lib.vsim_op_add_residual(p(inpL), p(attn), p(ff), N * E, 1 if serial else 0, None), "add_residual")
        keep("out", inpL)
        torch.cuda.synchronize()
        return rec

    # ---- the embedding and the head (enqueue_prompt, run_head)
    def embed(self, tokens):
        cfg, lib, G = self.cfg, hip.lib(), self.G
        N, E, V = len(tokens), cfg.E, G.shape["wte"][0]
        tok = dev(np.asarray(tokens, np.int32))
        x = f32(N, E)
        ck(lib.vsim_op_get_rows(p(G.w["wte"]), E, V, p(tok), N, p(x), None), "get_rows")
        if "emb_w" in G.f:
            y = f32(N, E)
            ck(lib.vsim_op_norm(p(x), p(y), E, N, p(G.f["emb_w"]), p(G.f["emb_b"]), None), "emb norm")
            x = y
        torch.cuda.synchronize()
        return x

    def head(self, x):
        """The final norm and the lm_head product of the rows x [n][E]: the n-row rule of a prompt batch."""
        cfg, G = self.cfg, self.G
        n, E, V = x.shape[0], cfg.E, G.shape["lmh"][0]
        out = f32(n, V)
        if n >= 8:
            xa = f16(n, E)
            self.norm(x, n, G.f["lnf_w"], G.f["lnf_b"], xa, None)
            self.mm(G.w["lmh"], G.shape["lmh"], n, G.f.get("lmh_b"), out, xa, None)
        else:
            cur = f32(n, E)
            self.norm(x, n, G.f["lnf_w"], G.f["lnf_b"], None, cur)
            self.mm(G.w["lmh"], G.shape["lmh"], n, G.f.get("lmh_b"), out, None, Q4Rows(n, E).make(cur))
        return host(out)


def to_host(rec):
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in rec.items()}


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """Model files by (configuration, layers), written once."""
    root, made = tmp_path_factory.mktemp("fast_prompt_layer"), {}

    def get(cfg, n_layer):
        if (cfg, n_layer) not in made:
            path = str(root / f"{cfg.name}-{n_layer}.bin")
            mg.write_model(path, cfg.arch, cfg.hparams(n_layer), seed=cfg.seed, std=P.STD)
            made[(cfg, n_layer)] = path
        return made[(cfg, n_layer)]
    return get


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


@pytest.mark.parametrize("pair", P.PAIRS, ids=lambda pr: f"{pr[0]}+{pr[1]}")
@pytest.mark.parametrize("cfg", P.CONFIGS, ids=lambda c: c.name)
def test_layer_stage_is_the_op_entries_composed_and_means_the_reference(cfg, pair, files):
    path = files(cfg, 3)
    W = P.read_weights(path, cfg.arch, [1])[2][1]
    m = hip.Model.load(path, ARCH[cfg.arch], n_ctx=N_CTX, layer_begin=1, layer_end=2)
    m.set_mode(hip.MODE_FAST)
    comp = Comp(cfg, [W])
    cs = rope_table(cfg.n_rot)
    slopes = P.alibi_slopes(cfg.H) if cfg.alibi else None
    prev = None
    try:
        for n_past, N in ((0, pair[0]), (pair[0], pair[1])):
            x = dev(P.resid_rows(cfg, N, n_past))
            want = f32(N, cfg.E)
            m.eval(n_past, resid_in=x, resid_out=want, want_logits=False)
            st = to_host(comp.layer(0, x.clone(), n_past))
            # (a) wiring: all N x E values, bit for bit
            got, ref = st["out"], host(want)
            assert not np.isnan(ref).any()
            diff = got.view(np.uint32) != ref.view(np.uint32)
            assert not diff.any(), (f"{cfg.name} N {N} at {n_past}: {int(diff.sum())} of {diff.size} values differ from the "
                                    f"composition, first (row, column) {np.argwhere(diff)[0].tolist()}")
            # (b) meaning: every intermediate against fp64 on its actual input
            if prev is not None:
                st["kc_prev"], st["vc_prev"] = prev
            ratios, shares = P.check(cfg, W, st, n_past, cs, slopes)
            for stage, r in ratios.items():
                print(f"RATIO {cfg.name} {pair[0]}+{pair[1]} N={N}@{n_past} {stage} {r:.4f}")
            for stage, s in shares.items():
                print(f"SHARE {cfg.name} {pair[0]}+{pair[1]} N={N}@{n_past} {stage} {s:.5f}")
                assert s <= P.AMB_CAP, f"{stage}: ambiguous share {s:.4f}"
            prev = (st["Knew"], st["Vnew"])
    finally:
        m.close()


WHOLE = [c for c in P.CONFIGS if c.name in ("gptj-d128", "neox-par", "bloom")]


def _tokens(cfg, n, seed):
    return [int(v) for v in np.random.default_rng([cfg.seed, n, seed]).integers(0, 512, n)]


@pytest.mark.parametrize("cfg", WHOLE, ids=lambda c: c.name)
def test_whole_model_is_the_op_entries_composed(cfg, files):
    """Two layers with the embedding and the head: the last row's logits of a 300-token prompt, and of
    37 then 300 tokens, bit for bit."""
    path = files(cfg, 2)
    _, G, Ls = P.read_weights(path, cfg.arch, [0, 1])
    m = hip.Model.load(path, ARCH[cfg.arch], n_ctx=N_CTX)
    m.set_mode(hip.MODE_FAST)
    try:
        for batches in ((300,), (37, 300)):
            comp = Comp(cfg, [Ls[0], Ls[1]], G)
            n_past = 0
            for n in batches:
                ids = _tokens(cfg, n, n_past)
                want = m.eval(n_past, ids)
                x = comp.embed(ids)
                for i in range(2):
                    comp.layer(i, x, n_past)
                got = comp.head(x[n - 1:n])[0]
                assert not np.isnan(want).any()
                assert same_bits(got, want), f"{cfg.name}: logits of {n} tokens at {n_past} differ from the composition"
                n_past += n
    finally:
        m.close()


def test_score_rows_are_the_op_entries_composed(files):
    """Every row of vsim_model_eval_score's logits_all at the default chunk size (256 rows, then 44): the
    head's n-row rule per chunk."""
    cfg = WHOLE[0]
    path = files(cfg, 2)
    _, G, Ls = P.read_weights(path, cfg.arch, [0, 1])
    m = hip.Model.load(path, ARCH[cfg.arch], n_ctx=N_CTX)
    m.set_mode(hip.MODE_FAST)
    try:
        ids = _tokens(cfg, 300, 5)
        _, _, want = m.score(0, ids, want_logits=True)
        comp = Comp(cfg, [Ls[0], Ls[1]], G)
        x = comp.embed(ids)
        for i in range(2):
            comp.layer(i, x, 0)
        got = np.concatenate([comp.head(x[0:256]), comp.head(x[256:300])])
        assert not np.isnan(want).any()
        diff = got.view(np.uint32) != want.view(np.uint32)
        assert not diff.any(), f"{int(diff.any(axis=1).sum())} of 300 logits rows differ, first row {int(np.argwhere(diff)[0][0])}"
    finally:
        m.close()
