"""The model quantizer on the GPU: k_quantize_w through vsim_op_q4_quantize_w (W4T32, AoS and
histogram outputs, row chunks, every refusal), the quantizing loader (vsim_model_load_file_ex,
many staging chunks and the default) and the vsim-quantize tool, all compared bit for bit with
the numpy restatement that tests/test_quantize_cpu.py pins to the reference's own output."""
import ctypes
import dataclasses
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from vsim_amd import hip  # noqa: E402
from vsim_amd import modelgen as mg  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDEN = os.path.join(ROOT, "tests", "golden")
BUILD = os.path.join(ROOT, "vsim_amd", "_build")
DEV = "cuda"
VSIM_EINVAL = -1
ARCH = {"gptneox": hip.ARCH_GPTNEOX, "gptj": hip.ARCH_GPTJ, "bloom": hip.ARCH_BLOOM}
# (rows, K): one block; a partial tile; one row into the second tile with K no multiple of 64;
# the fixture with every crafted row; K no multiple of the 256-column tile; many tiles of full width
SHAPES = [(1, 32), (31, 64), (33, 96), (70, 128), (130, 160), (257, 4096)]
SRC = [(hip.SRC_F16, np.float16), (hip.SRC_F32, np.float32)]
RECORDED = json.load(open(os.path.join(GOLDEN, "quantize_files.json")))
_inputs = {}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def source(rows, k, dtype):
    """The case's input in its source type and what the quantizer must make of it (computed once)."""
    key = (rows, k, np.dtype(dtype).name)
    if key not in _inputs:
        if (rows, k) == (70, 128):
            x = np.load(os.path.join(GOLDEN, "quantize_w.npz"))["x"]
        else:
            rng = np.random.Generator(np.random.PCG64(rows * 10007 + k))
            x = (rng.standard_normal((rows, k), dtype=np.float32) * np.float32(0.02)).astype(np.float16).astype(np.float32)
            x[rows - 1, k - 1] = np.nan       # the last element of the last block
            x[0, 0:32] = 0.0
            x[rows // 2, k // 2] = -np.inf
        src = np.ascontiguousarray(x.astype(dtype))
        aos, hist = mg.quantize_q4_0_w(src.astype(np.float32))
        _inputs[key] = (src, aos, hist)
    return _inputs[key]


def repacked(aos, rows, k):
    dst = torch.full((hip.q4_bytes(rows, k),), 0x5A, dtype=torch.uint8, device=DEV)
    hip.check(hip.lib().vsim_op_q4_repack(dev(aos).data_ptr(), dst.data_ptr(), rows, k, None), "repack")
    return host(dst)


# ------------------------------------------------------------------ op
@pytest.mark.parametrize("rows,k", SHAPES)
@pytest.mark.parametrize("src_type,dtype", SRC)
def test_op_outputs(rows, k, src_type, dtype):
    src, aos, hist = source(rows, k, dtype)
    x = dev(src)
    want_w = repacked(aos, rows, k)
    # each output alone (poisoned buffers: every byte, padding rows included, must be written)
    w = torch.full((hip.q4_bytes(rows, k),), 0x5A, dtype=torch.uint8, device=DEV)
    hip.quantize_w(x, src_type, rows, k, w=w, w_rows=rows)
    assert np.array_equal(host(w), want_w)
    a = torch.full((aos.size,), 0x5A, dtype=torch.uint8, device=DEV)
    hip.quantize_w(x, src_type, rows, k, aos=a)
    assert np.array_equal(host(a), aos)
    # both in one call, with the histogram; a second call accumulates; padding rows are not counted
    w2, a2 = torch.full_like(w, 0xA5), torch.full_like(a, 0xA5)
    h = torch.zeros(16, dtype=torch.int64, device=DEV)
    hip.quantize_w(x, src_type, rows, k, w=w2, w_rows=rows, aos=a2, hist=h)
    assert np.array_equal(host(w2), want_w) and np.array_equal(host(a2), aos)
    assert np.array_equal(host(h).astype(np.uint64), hist) and int(hist.sum()) == rows * k
    hip.quantize_w(x, src_type, rows, k, aos=a2, hist=h)
    assert np.array_equal(host(h).astype(np.uint64), 2 * hist)


@pytest.mark.parametrize("src_type,dtype", SRC)
def test_op_row_chunks(src_type, dtype):
    """A 130-row weight filled as rows [0, 64) then [64, 130) equals one call; the first chunk
    leaves the rest of the weight alone."""
    rows, k = 130, 160
    src, aos, _ = source(rows, k, dtype)
    x = dev(src)
    w = torch.full((hip.q4_bytes(rows, k),), 0x5A, dtype=torch.uint8, device=DEV)
    hip.quantize_w(x[:64], src_type, 64, k, w=w, w_rows=rows, row0=0)
    first = host(w).copy()
    hip.quantize_w(x[64:], src_type, rows - 64, k, w=w, w_rows=rows, row0=64)
    want = repacked(aos, rows, k)
    assert np.array_equal(host(w), want)
    # W4T32: tile t's nibbles at [t*nb*512, (t+1)*nb*512), scales after all nibbles
    nb, tiles = k // 32, (rows + 31) // 32
    touched = np.zeros(first.size, bool)
    touched[:2 * nb * 512] = True
    touched[tiles * nb * 512:tiles * nb * 512 + 2 * nb * 128] = True
    assert np.array_equal(first[touched], want[touched]) and (first[~touched] == 0x5A).all()


def test_op_refusals():
    src, _, _ = source(33, 96, np.float32)
    x = dev(src)
    w = torch.zeros(hip.q4_bytes(64, 96), dtype=torch.uint8, device=DEV)
    a = torch.zeros(33 * 3 * 20, dtype=torch.uint8, device=DEV)
    L = hip.lib()

    def rc(xp, st, rows, k, wp, w_rows, row0, ap):
        return L.vsim_op_q4_quantize_w(xp, st, rows, k, wp, w_rows, row0, ap, None, None)

    xp, wp, ap = x.data_ptr(), w.data_ptr(), a.data_ptr()
    assert rc(xp, hip.SRC_F32, 33, 96, wp, 64, 0, ap) == 0
    assert rc(xp, hip.SRC_F32, 33, 48, wp, 64, 0, ap) == VSIM_EINVAL    # k % 32
    assert rc(xp, hip.SRC_F32, 16, 96, wp, 64, 16, None) == VSIM_EINVAL  # row0 % 32
    assert rc(xp, hip.SRC_F32, 33, 96, wp, 64, 32, None) == VSIM_EINVAL  # row0 + rows > w_rows
    assert rc(xp, hip.SRC_F32, 33, 96, None, 0, 0, None) == VSIM_EINVAL  # no target
    assert rc(xp, 2, 33, 96, wp, 64, 0, ap) == VSIM_EINVAL               # src_type
    assert rc(xp, -1, 33, 96, wp, 64, 0, ap) == VSIM_EINVAL
    torch.cuda.synchronize()


# ------------------------------------------------------------------ model
def write_pair(tmp_path, cfg, ft):
    """The F16 / F32 source file and the Q4_0 file the quantizer must make of it."""
    arch_s, hp = mg.CONFIGS[cfg]
    hp = dataclasses.replace(hp, ftype=ft)
    src, q4 = str(tmp_path / "src.bin"), str(tmp_path / "q4_0.bin")
    mg.write_model(src, arch_s, hp, seed=RECORDED["seed"], std=RECORDED["std"])
    open(q4, "wb").write(mg.expected_q4_0_image(arch_s, hp, RECORDED["seed"], RECORDED["std"]))
    return src, q4, arch_s, hp


def decode_logits(model, n_steps=8):
    ids, n_past, out = [1, 2, 3, 4, 5], 0, []
    for _ in range(n_steps + 1):
        lg = model.eval(n_past, ids)
        out.append(lg.view(np.uint32).copy())
        n_past += len(ids)
        ids = [int(np.argmax(lg))]
    return out


@pytest.mark.parametrize("cfg", ["tiny-neox", "tiny-gptj", "tiny-bloom"])
@pytest.mark.parametrize("ft", [1, 0])
@pytest.mark.parametrize("chunk_rows", [32, 96, 0])  # many chunks; a partial last one (128 = 96 + 32); the default
def test_quantizing_loader(cfg, ft, chunk_rows, tmp_path):
    src, q4, arch_s, hp = write_pair(tmp_path, cfg, ft)
    prev = hip.quantize_set_chunk_rows(chunk_rows)
    try:
        m = hip.Model.load(src, ARCH[arch_s], n_ctx=64, quantize=True)
    finally:
        hip.quantize_set_chunk_rows(prev)
    ref = hip.Model.load(q4, ARCH[arch_s], n_ctx=64)
    _, tensors = mg.read_model(q4, arch_s)
    n_mat = 0
    for name, (ne, tft, raw) in tensors.items():
        got = m.get_tensor(name, len(raw))
        assert np.array_equal(got, np.frombuffer(raw, np.uint8)), name
        n_mat += tft == 2
    assert n_mat == sum(1 for _, _, kind in mg.tensor_specs(arch_s, hp) if kind == "q")
    for i, (a, b) in enumerate(zip(decode_logits(m), decode_logits(ref))):
        assert np.array_equal(a, b), i
    m.close()
    ref.close()


def test_quantizing_loader_without_flag_refuses(tmp_path):
    """flags = 0 is the plain loader: an F16 file is refused with its message."""
    src, _, arch_s, _ = write_pair(tmp_path, "tiny-neox", 1)
    for load in (lambda h: hip.lib().vsim_model_load_file_ex(src.encode(), 0, 64, 0, 0, -1, 0, ctypes.byref(h)),
                 lambda h: hip.lib().vsim_model_load_file(src.encode(), 0, 64, 0, 0, -1, ctypes.byref(h))):
        h = ctypes.c_void_p()
        assert load(h) == -4
        assert "quantize the file to Q4_0 (f16 == 2) first" in hip.lib().vsim_last_error().decode()


def test_quantizing_loader_checks(tmp_path):
    """The plain loader's truncation and shape messages, on an F16 file."""
    src, _, arch_s, hp = write_pair(tmp_path, "tiny-neox", 1)
    buf = open(src, "rb").read()
    cut = str(tmp_path / "cut.bin")
    open(cut, "wb").write(buf[:len(buf) - 7])
    h = ctypes.c_void_p()
    assert hip.lib().vsim_model_load_file_ex(cut.encode(), 0, 64, 0, 0, -1, 1, ctypes.byref(h)) == -4
    assert "truncated" in hip.lib().vsim_last_error().decode()
    open(cut, "wb").write(buf[:len(buf) // 2])
    assert hip.lib().vsim_model_load_file_ex(cut.encode(), 0, 64, 0, 0, -1, 1, ctypes.byref(h)) == -4
    err = hip.lib().vsim_last_error().decode()
    assert "truncated" in err or "missing" in err, err


def test_set_tensor_src(tmp_path):
    """vsim_model_set_tensor_src: one matrix from float16 and from float32 values, BLOOM's fused
    query_key_value over its three slots, in many chunks; a 1-D tensor through the F32 path."""
    src, q4, arch_s, hp = write_pair(tmp_path, "tiny-bloom", 1)
    m = hip.Model.load(q4, ARCH[arch_s], n_ctx=64)
    E = hp.n_embd
    rng = np.random.Generator(np.random.PCG64(9))
    prev = hip.quantize_set_chunk_rows(32)
    try:
        for name, rows in (("layers.1.attention.query_key_value.weight", 3 * E), ("layers.0.feed_forward.w1.weight", 4 * E)):
            for dt in (np.float16, np.float32):
                v = (rng.standard_normal((rows, E), dtype=np.float32) * np.float32(0.05)).astype(np.float16).astype(dt)
                m.set_tensor_src(name, v)
                want = mg.quantize_q4_0_w(v.astype(np.float32))[0]
                assert np.array_equal(m.get_tensor(name, want.size), want), (name, dt)
    finally:
        hip.quantize_set_chunk_rows(prev)
    b = rng.standard_normal(E, dtype=np.float32)
    m.set_tensor_src("norm.bias", b)
    assert np.array_equal(m.get_tensor("norm.bias", 4 * E).view(np.float32), b)
    with pytest.raises(hip.VsimError):
        m.set_tensor_src("norm.bias", b.astype(np.float16))
    with pytest.raises(hip.VsimError):
        m.set_tensor_src("layers.0.feed_forward.w1.weight", np.zeros((E, E), np.float16))
    m.close()


@pytest.mark.parametrize("chunk_rows", [32, 96, 0])
def test_set_tensor_src_rows_not_a_multiple_of_32(chunk_rows):
    """A 130-row matrix (n_vocab = 130): the last chunk is partial and ends inside a tile, whose
    padding rows it writes; the tensor reads back as the expected blocks."""
    m = hip.Model.create(hip.ARCH_GPTJ, dict(n_vocab=130, n_embd=128, n_head=4, n_layer=1, n_rot=16,
                                             use_parallel_residual=1), n_ctx=64)
    src, aos, _ = source(130, 160, np.float16)
    v = np.ascontiguousarray(src[:, :128])
    prev = hip.quantize_set_chunk_rows(chunk_rows)
    try:
        m.set_tensor_src("transformer.wte.weight", v)
    finally:
        hip.quantize_set_chunk_rows(prev)
    want = mg.quantize_q4_0_w(v.astype(np.float32))[0]
    assert np.array_equal(m.get_tensor("transformer.wte.weight", want.size), want)
    m.close()


def test_quantizing_loader_pipeline_halves(tmp_path):
    """tiny-neox as two stages [0,1) and [1,2), both loaded with quantize=True (each skips the
    other's F16 records by their size), against one stage."""
    src, q4, arch_s, hp = write_pair(tmp_path, "tiny-neox", 1)
    full = hip.Model.load(q4, hip.ARCH_GPTNEOX, n_ctx=64)
    s0 = hip.Model.load(src, hip.ARCH_GPTNEOX, n_ctx=64, layer_begin=0, layer_end=1, quantize=True)
    s1 = hip.Model.load(src, hip.ARCH_GPTNEOX, n_ctx=64, layer_begin=1, layer_end=2, quantize=True)
    ids, n_past = [1, 2, 3, 4, 5], 0
    for step in range(4):
        r = torch.empty((len(ids), hp.n_embd), dtype=torch.float32, device=DEV)
        s0.eval(n_past, ids, resid_out=r)
        lp = s1.eval(n_past, None, resid_in=r)
        lf = full.eval(n_past, ids)
        assert np.array_equal(lp.view(np.uint32), lf.view(np.uint32)), step
        n_past += len(ids)
        ids = [int(np.argmax(lf))]
    for m in (full, s0, s1):
        m.close()


def test_cli_quantize_flag(tmp_path):
    """vsim-hip --quantize on the F16 file prints the token stream of the plain run on the Q4_0
    file; without the flag the F16 file is refused as before."""
    src, q4, arch_s, hp = write_pair(tmp_path, "tiny-gptj", 1)
    exe = os.path.join(BUILD, "vsim-hip")
    common = ["-p", "1 2 3 4 5", "-n", "8", "-s", "7", "--n_ctx", "64"]

    def stream(args):
        r = subprocess.run([exe, "gptj", *args, *common], capture_output=True, text=True, timeout=120)
        return r.returncode, r.stdout[r.stdout.find("<|BEGIN>"):r.stdout.find("<END|>")], r.stderr

    rc_q, out_q, err_q = stream(["--quantize", "-m", src])
    rc_p, out_p, _ = stream(["-m", q4])
    assert rc_q == 0 and rc_p == 0, err_q
    assert out_q == out_p and out_q.startswith("<|BEGIN>") and len(out_q.split()) > 1 + 5  # the prompt's ids and at least one sampled id
    rc, _, err = stream(["-m", src])
    assert rc != 0 and "quantize the file to Q4_0" in err


# ------------------------------------------------------------------ tool
@pytest.mark.parametrize("cfg,ft", [("tiny-neox", 1), ("tiny-gptj", 0), ("tiny-bloom", 1)])
def test_tool_on_the_device(cfg, ft, tmp_path):
    src, q4, arch_s, hp = write_pair(tmp_path, cfg, ft)
    want = RECORDED["files"][f"{cfg}/f{ft}"]["output_sha256"]
    exe = os.path.join(BUILD, "vsim-quantize")
    out_d, out_h = str(tmp_path / "dev.bin"), str(tmp_path / "host.bin")
    r = subprocess.run([exe, arch_s, src, out_d, "2", "--device", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-2000:]
    assert hashlib.sha256(open(out_d, "rb").read()).hexdigest() == want
    r = subprocess.run([exe, arch_s, src, out_h, "2", "--host"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(out_h, "rb").read() == open(out_d, "rb").read()
    # the library call gives the same file and the histogram of the host path
    out_l = str(tmp_path / "lib.bin")
    st_d = hip.quantize_file(src, out_l, ARCH[arch_s], device=0)
    st_h = hip.quantize_file(src, out_h, ARCH[arch_s], device=-1)
    assert open(out_l, "rb").read() == open(out_d, "rb").read() and st_d == st_h
    m = hip.Model.load(out_d, ARCH[arch_s], n_ctx=64)  # the plain loader takes it
    m.eval(0, [1, 2, 3])
    m.close()
