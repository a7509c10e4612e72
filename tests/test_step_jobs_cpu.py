"""decode_jobs.hpp (vsim_amd/csrc): the fast and the weight-only step's kernel arguments, from values alone.

The sibling of test_decode_jobs_cpu.py for the header's other two sections, in the same way: a
stand-alone program includes the header, builds every aggregate from operands at made-up addresses
and prints the fields; the expected lines below are written out from the layouts the kernels read.
A W4T32 weight of M rows and K values keeps ceil(M/32) * 32 * (K/32) * 16 bytes of nibbles ahead of
its scales; the scales of a Q4 SoA row of k values start (k/32) * 16 bytes behind its nibbles; a
weight-only row operand has its halves where the row's factors are and its exponent where the
nibbles are.  Compiled as HIP for the host alone; no HIP call, no GPU, nothing loaded into Python.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HEADER = os.path.join(ROOT, "vsim_amd", "csrc", "decode_jobs.hpp")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

PROGRAM = r"""
#include "%s"
#include <cstdio>
using namespace vsim;
// operands at made-up addresses: never dereferenced, only compared
template <class T = float> static T *at(unsigned long a) { return (T *)a; }
static unsigned long u(const void *p) { return (unsigned long)p; }
static void show_w(const W4 &w) { printf(" w.qs=%%lx w.d=%%lx rows=%%d k=%%d tiles=%%d", u(w.qs), u(w.d), w.rows, w.k, w.tiles); }
static void show(const char *name, const FastGemv &P) {
  printf("%%s xq=%%lx,%%lx xd=%%lx,%%lx nj=%%d tab=%%lx oq_qs=%%lx oq_d=%%lx npast=%%lx cs=%%lx d=%%d n_rot=%%d style=%%d "
         "lnx=%%lx lnw=%%lx,%%lx lnb=%%lx,%%lx clear=%%lx nclear=%%d\n", name, u(P.xq[0]), u(P.xq[1]), u(P.xd[0]), u(P.xd[1]),
         P.nj, u(P.gelu_tab), u(P.oq_qs), u(P.oq_d), u(P.npast), u(P.cs), P.d, P.n_rot, P.style, u(P.lnx), u(P.lnw[0]),
         u(P.lnw[1]), u(P.lnb[0]), u(P.lnb[1]), u(P.clear), P.nclear);
  for (int i = 0; i < 4; ++i) {  // (the slots past nj stay zero)
    printf("%%s.j%%d", name, i);
    show_w(P.j[i].w);
    printf(" bias=%%lx y=%%lx epi=%%d act=%%d\n", u(P.j[i].bias), u(P.j[i].y), P.j[i].epi, P.j[i].act);
  }
}
static void show(const char *name, const W4a16Ln &A) {
  printf("%%s x=%%lx n=%%d w1=%%lx b1=%%lx h1=%%lx e1=%%lx w2=%%lx b2=%%lx h2=%%lx e2=%%lx\n", name, u(A.x), A.n, u(A.w1),
         u(A.b1), u(A.h1), u(A.e1), u(A.w2), u(A.b2), u(A.h2), u(A.e2));
}
static void show(const char *name, const W4a16Gemv &B) {
  printf("%%s nj=%%d\n", name, B.nj);
  for (int i = 0; i < 4; ++i) {
    const W4a16GemvJob &j = B.j[i];
    printf("%%s.j%%d", name, i);
    show_w(j.w);
    printf(" x16=%%lx e=%%lx bias=%%lx res=%%lx res_a=%%lx y=%%lx\n", u(j.x16), u(j.e), u(j.bias), u(j.res), u(j.res_a), u(j.y));
  }
}
int main() {
  for (int E : {128, 4096, 8192, 16384, 32768}) printf("sf E=%%d %%d\n", E, fast_sf(E));
  for (int n : {1, 64, 65, 200, 4160}) printf("nchunk n_ctx=%%d %%d\n", n, fast_nchunk(n));

  // K1 of a layer: four jobs under the LayerNorm prologue, every field a value of its own.  The
  // Q4 rows are given too: under a prologue they must not reach the kernel.
  const Q4Rows r0 = q4_rows(at<void>(0x4000), 64), r1 = q4_rows(at<void>(0x5000), 64);
  const FastJob four[4] = {fast_job(at<void>(0x10000), 96, 64, at(0x210), nullptr, FE_GELU_Q, 1),
                           fast_job(at<void>(0x20000), 64, 64, at(0x220), at(0x320), FE_ROPE_Q, 0),
                           fast_job(at<void>(0x30000), 64, 64, at(0x230), at(0x330), FE_ROPE_K, 0),
                           fast_job(at<void>(0x40000), 64, 64, nullptr, at(0x340), FE_V, 0)};
  const FastPos pos{at<int>(0x1a00), at<double2>(0x1500), 32, 8, 1};
  const Q4Rows g = q4_rows(at<void>(0x8000), 96);
  show("ln4", fast_gemv(FastAct{.lnx = at(0x70), .n = {NormRow{at(0x10), at(0x20)}, NormRow{at(0x40), at(0x50)}},
                                .x = {r0, r1}},
                        four, 4, at<uint16_t>(0x190), g, pos, at<unsigned>(0xb0), 28));
  // the head's form from global rows: one FE_STORE job; what goes with a GELU job, a RoPE job or
  // counters is given and must be left out
  const FastJob one = fast_job(at<void>(0x50000), 33, 64, at(0x250), at(0x350), FE_STORE, 1);
  show("rows1", fast_gemv(FastAct{.x = {r0, r1}}, &one, 1, at<uint16_t>(0x190), g, pos, nullptr, 28));

  const Q4Rows o = q4_rows(at<void>(0x2000), 96 * 7);
  const FastTail T = fast_tail_job(w4_view(at<void>(0x60000), 64, 256), q4_rows(at<void>(0x7000), 256), at(0x400), 4,
                                   FastAttn{.q = at(0x1200), .kc = at(0x1800), .vc = at(0x1900), .npast = at<int>(0x1a00),
                                            .d = 96, .H = 7, .nchunk = 5, .scale = 0.375f, .part = at(0x1b00),
                                            .hcnt = at<unsigned>(0x1c00), .o = o});
  printf("tail");
  show_w(T.wf);
  printf(" xf_qs=%%lx xf_d=%%lx ffp=%%lx sf=%%d q=%%lx kc=%%lx vc=%%lx npast=%%lx d=%%d H=%%d nchunk=%%d scale=%%g part=%%lx "
         "hcnt=%%lx oq_qs=%%lx oq_d=%%lx\n", u(T.xf_qs), u(T.xf_d), u(T.ffp), T.sf, u(T.q), u(T.kc), u(T.vc), u(T.npast), T.d,
         T.H, T.nchunk, (double)T.scale, u(T.part), u(T.hcnt), u(T.oq_qs), u(T.oq_d));
  const FastOproj P = fast_oproj_job(w4_view(at<void>(0x70000), 672, 672), o, at(0x260), at(0x400), 4, at(0x270), at(0x70),
                                     at(0x80));
  printf("oproj");
  show_w(P.w);
  printf(" xq=%%lx xd=%%lx bo=%%lx ffp=%%lx sf=%%d bproj=%%lx x=%%lx out=%%lx\n", u(P.xq), u(P.xd), u(P.bo), u(P.ffp), P.sf,
         u(P.bproj), u(P.x), u(P.out));

  const W4a16Operand x1 = w4a16_operand(ActRow{o, at(0x3000)});
  printf("operand h=%%lx e=%%lx\n", u(x1.h), u(x1.e));
  const W4a16Operand x2{at<_Float16>(0x3100), at<int32_t>(0x2100)};
  const NormRow n1{at(0x10), at(0x20)}, n2{at(0x40), at(0x50)}, part{nullptr, at(0x50)};
  show("ln-two", w4a16_ln_job(at(0x70), 1056, n1, x1, &n2, x2));
  show("ln-one", w4a16_ln_job(at(0x70), 1056, n1, x1, nullptr, x2));
  show("ln-default", w4a16_ln_job(at(0x70), 1056, n1, x1));
  // a second norm given in part (an op entry's caller): passed on as it is, for the launcher to refuse
  show("ln-part", w4a16_ln_job(at(0x70), 1056, n1, x1, &part, W4a16Operand{at<_Float16>(0x3100), nullptr}));

  const W4a16GemvJob plain = w4a16_gemv_job(at<void>(0x60000), 96, 64, x1, at(0x170), at(0x180));
  show("gemv1", w4a16_gemv({plain}));
  show("gemv4", w4a16_gemv({plain, w4a16_gemv_job(at<void>(0x20000), 64, 64, x2, nullptr, at(0x380), at(0x390)),
                            w4a16_gemv_job(at<void>(0x30000), 64, 64, x1, at(0x230), at(0x3a0), at(0x3a0), at(0x3b0)),
                            w4a16_gemv_job(at<void>(0x50000), 33, 64, x2, at(0x250), at(0x350))}));
  return 0;
}
"""

NOJOB = " w.qs=0 w.d=0 rows=0 k=0 tiles=0"
# K = 64: 2 blocks per row; a weight tile of 32 rows holds 32 * 2 * 16 = 0x400 bytes of nibbles
W96 = " w.qs=60000 w.d=60c00 rows=96 k=64 tiles=3"

EXPECTED = [
    # FD_SF = 2 doubles while 4E / sf > FD_MAXE = 8192: 4 * 8192 / 2 = 16384 does not fit, / 4 does.
    # E = 16384: 8, whose slice of 8192 fits; E = 32768: 8 still, the cap, though the slice of 16384 does
    # not fit.  This is the current behaviour: the launchers refuse both widths (n_embd beyond FD_MAXE).
    "sf E=128 2",
    "sf E=4096 2",
    "sf E=8192 4",
    "sf E=16384 8",
    "sf E=32768 8",
    # ceil(n_ctx / 64); 4160 gives 65, one past FD_MAXCH
    "nchunk n_ctx=1 1",
    "nchunk n_ctx=64 1",
    "nchunk n_ctx=65 2",
    "nchunk n_ctx=200 4",
    "nchunk n_ctx=4160 65",
    # a prologue: no global rows.  The GELU row of M = 96 values: scales (96 / 32) * 16 = 0x30 behind the nibbles
    "ln4 xq=0,0 xd=0,0 nj=4 tab=190 oq_qs=8000 oq_d=8030 npast=1a00 cs=1500 d=32 n_rot=8 style=1 "
    "lnx=70 lnw=10,40 lnb=20,50 clear=b0 nclear=28",
    "ln4.j0 w.qs=10000 w.d=10c00 rows=96 k=64 tiles=3 bias=210 y=0 epi=1 act=1",
    "ln4.j1 w.qs=20000 w.d=20800 rows=64 k=64 tiles=2 bias=220 y=320 epi=2 act=0",
    "ln4.j2 w.qs=30000 w.d=30800 rows=64 k=64 tiles=2 bias=230 y=330 epi=3 act=0",
    "ln4.j3 w.qs=40000 w.d=40800 rows=64 k=64 tiles=2 bias=0 y=340 epi=4 act=0",
    # global rows of 64 values: scales 2 * 16 = 0x20 behind the nibbles; no GELU job: no table, no row;
    # no RoPE job: d = 1; no counters: nclear = 0; 33 rows: 2 tiles
    "rows1 xq=4000,5000 xd=4020,5020 nj=1 tab=0 oq_qs=0 oq_d=0 npast=1a00 cs=1500 d=1 n_rot=8 style=1 "
    "lnx=0 lnw=0,0 lnb=0,0 clear=0 nclear=0",
    "rows1.j0 w.qs=50000 w.d=50800 rows=33 k=64 tiles=2 bias=250 y=350 epi=0 act=1",
    "rows1.j1" + NOJOB + " bias=0 y=0 epi=0 act=0",
    "rows1.j2" + NOJOB + " bias=0 y=0 epi=0 act=0",
    "rows1.j3" + NOJOB + " bias=0 y=0 epi=0 act=0",
    # fc_out 64 x 256: 2 tiles * 32 rows * 8 blocks * 16 = 0x2000; its row of 256 values: 8 * 16 = 0x80;
    # the attention row of 96 * 7 = 672 values: 21 blocks, scales 21 * 16 = 0x150 behind the nibbles
    "tail w.qs=60000 w.d=62000 rows=64 k=256 tiles=2 xf_qs=7000 xf_d=7080 ffp=400 sf=4 q=1200 kc=1800 vc=1900 "
    "npast=1a00 d=96 H=7 nchunk=5 scale=0.375 part=1b00 hcnt=1c00 oq_qs=2000 oq_d=2150",
    # the out-projection 672 x 672: 21 tiles * 32 rows * 21 blocks * 16 = 0x37200
    "oproj w.qs=70000 w.d=a7200 rows=672 k=672 tiles=21 xq=2000 xd=2150 bo=260 ffp=400 sf=4 bproj=270 x=70 out=80",
    # the halves where the row's factors are, the exponent where its nibbles are
    "operand h=3000 e=2000",
    "ln-two x=70 n=1056 w1=10 b1=20 h1=3000 e1=2000 w2=40 b2=50 h2=3100 e2=2100",
    "ln-one x=70 n=1056 w1=10 b1=20 h1=3000 e1=2000 w2=0 b2=0 h2=0 e2=0",
    "ln-default x=70 n=1056 w1=10 b1=20 h1=3000 e1=2000 w2=0 b2=0 h2=0 e2=0",
    "ln-part x=70 n=1056 w1=10 b1=20 h1=3000 e1=2000 w2=0 b2=50 h2=3100 e2=0",
    "gemv1 nj=1",
    "gemv1.j0" + W96 + " x16=3000 e=2000 bias=170 res=0 res_a=0 y=180",
    "gemv1.j1" + NOJOB + " x16=0 e=0 bias=0 res=0 res_a=0 y=0",
    "gemv1.j2" + NOJOB + " x16=0 e=0 bias=0 res=0 res_a=0 y=0",
    "gemv1.j3" + NOJOB + " x16=0 e=0 bias=0 res=0 res_a=0 y=0",
    # the three join forms: none, res, res + res_a (y may be res)
    "gemv4 nj=4",
    "gemv4.j0" + W96 + " x16=3000 e=2000 bias=170 res=0 res_a=0 y=180",
    "gemv4.j1 w.qs=20000 w.d=20800 rows=64 k=64 tiles=2 x16=3100 e=2100 bias=0 res=390 res_a=0 y=380",
    "gemv4.j2 w.qs=30000 w.d=30800 rows=64 k=64 tiles=2 x16=3000 e=2000 bias=230 res=3a0 res_a=3b0 y=3a0",
    "gemv4.j3 w.qs=50000 w.d=50800 rows=33 k=64 tiles=2 x16=3100 e=2100 bias=250 res=0 res_a=0 y=350",
]


def test_step_jobs_fields(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.fail("hipcc not found (the header includes common.hpp, which only a HIP compiler takes)")
    src, exe = tmp_path / "jobs.cpp", tmp_path / "jobs"
    src.write_text(PROGRAM % HEADER)
    subprocess.run([HIPCC, "--offload-host-only", "-x", "hip", "-std=c++17", "-O1", "-Wall", "-Wno-unused-function",
                    "-o", str(exe), str(src)], check=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    assert got == EXPECTED
