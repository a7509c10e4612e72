"""decode_jobs.hpp (vsim_amd/csrc): the exact decode step's kernel arguments, from values alone.

A stand-alone program includes the header, builds every job from operands at made-up addresses and
prints the fields; the expected values below are written out from the layouts the kernels read:
the scales of `rows` Q4 SoA rows of k values start rows*(k/32)*16 bytes behind their nibbles; the
tail workspace is the epoch on a 256-byte line, og [E] and jg [E] (8 bytes each), rec [2 E/32]
(16 bytes each) and 128 flags (8 bytes each).  The header pulls in common.hpp (device intrinsics,
_Float16), so the program is compiled as HIP for the host alone; it makes no HIP call and runs
without a GPU.  Nothing is loaded into Python.
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
static void show(const char *name, const LnQuantJob &j) {
  printf("%%s x=%%lx w=%%lx b=%%lx qs=%%lx d=%%lx xd=%%lx ja=%%lx jab=%%lx jf=%%lx jfb=%%lx jout=%%lx ep=%%lx\n", name, u(j.x),
         u(j.w), u(j.b), u(j.qs), u(j.d), u(j.xd), u(j.ja), u(j.jab), u(j.jf), u(j.jfb), u(j.jout), u(j.ep));
}
static void show(const char *name, const TailLn &n) {
  printf("%%s x=%%lx ab=%%lx fb=%%lx jout=%%lx w1=%%lx b1=%%lx q1=%%lx d1=%%lx xd1=%%lx w2=%%lx b2=%%lx q2=%%lx d2=%%lx xd2=%%lx "
         "og=%%lx jg=%%lx rec=%%lx ep=%%lx stats=%%lx il=%%d\n", name, u(n.x), u(n.ab), u(n.fb), u(n.jout), u(n.w1), u(n.b1),
         u(n.q1), u(n.d1), u(n.xd1), u(n.w2), u(n.b2), u(n.q2), u(n.d2), u(n.xd2), u(n.og), u(n.jg), u(n.rec), u(n.ep),
         u(n.stats), n.il);
}
static void show(const char *name, const AttnJob &a) {
  printf("%%s q=%%lx k=%%lx v=%%lx kc=%%lx vc=%%lx npast=%%lx cs=%%lx etab=%%lx d=%%d H=%%d n_rot=%%d style=%%d n_ctx=%%d "
         "nsplit=%%d kqv_nth=%%d scale=%%g alibi=%%lx oq_qs=%%lx oq_d=%%lx oxd=%%lx out=%%lx\n", name, u(a.q), u(a.k), u(a.v),
         u(a.kc), u(a.vc), u(a.npast), u(a.cs), u(a.etab), a.d, a.H, a.n_rot, a.style, a.n_ctx, a.nsplit, a.kqv_nth,
         (double)a.scale, u(a.alibi), u(a.oq_qs), u(a.oq_d), u(a.oxd), u(a.out));
}
int main() {
  const unsigned long base = 0x100000;
  for (int kr : {32 << 8 | 1, 4096 << 8 | 1, 16384 << 8 | 1, 64 << 8 | 5}) {
    const Q4Rows q = q4_rows(at<void>(base), kr >> 8, kr & 255);
    printf("q4 k=%%d rows=%%d qs=%%lu d=%%lu\n", kr >> 8, kr & 255, u(q.qs) - base, u(q.d) - base);
  }
  const Q4Rows q1 = q4_rows(at<void>(base), 4096);  // (rows defaults to 1)
  printf("q4 default rows d=%%lu\n", u(q1.d) - base);
  for (int E : {32, 1056, 8192}) {
    const TailWs w = tail_ws_carve(at<void>(base), E);
    printf("ws E=%%d ep=%%lu og=%%lu jg=%%lu rec=%%lu hflag=%%lu bytes=%%zu\n", E, u(w.ep) - base, u(w.og) - base,
           u(w.jg) - base, u(w.rec) - base, u(w.hflag) - base, tail_ws_bytes(E));
  }
  const TailWs w0 = tail_ws_carve(nullptr, 1056);
  printf("ws null %%lu %%lu %%lu %%lu %%lu\n", u(w0.ep), u(w0.og), u(w0.jg), u(w0.rec), u(w0.hflag));
  printf("scale %%a %%a\n", (double)default_attn_scale(4096, 16), (double)default_attn_scale(2560, 32));

  // an attention whose every field holds a value of its own
  AttnDesc D;
  D.d = 96, D.H = 7, D.n_rot = 24, D.style = 1, D.n_ctx = 333, D.nsplit = 2, D.kqv_nth = 5, D.scale = 0.375f;
  D.alibi = at(0x1100), D.q = at(0x1200), D.k = at(0x1300), D.v = at(0x1400), D.cs = at<double2>(0x1500);
  D.etab = at<uint16_t>(0x1600), D.o = ActRow{q4_rows(at<void>(0x2000), 96 * 7), at(0x3000)}, D.out = at(0x1700);
  show("attn", attn_job(D, at(0x1800), at(0x1900), at<int>(0x1a00)));
  D.nsplit = 1, D.n_rot = 0, D.cs = nullptr, D.alibi = nullptr;
  show("attn-plain", attn_job(D, nullptr, nullptr, nullptr));

  const TailWs W = tail_ws_carve(at<void>(base), 1056);
  const NormRow n1{at(0x10), at(0x20), {q4_rows(at<void>(0x4000), 1056), at(0x30)}};
  const NormRow n2{at(0x40), at(0x50), {q4_rows(at<void>(0x5000), 1056), at(0x60)}};
  show("tail1", tail_ln_job(at(0x70), at(0x80), at(0x90), at(0xa0), n1, nullptr, W, at<unsigned>(0xb0), 3));
  show("tail2", tail_ln_job(at(0x70), at(0x80), nullptr, at(0xa0), n1, &n2, W, at<unsigned>(0xb0), 254));

  const LnJoin join{at(0x100), at(0x110), at(0x120), at(0x130), at(0x140)};
  const LnQuantPair a = ln_quant_jobs(at(0x70), n1, &n2, &join, at<unsigned>(0x150));
  printf("pair-join two=%%d second=%%d\n", a.two, a.second() == &a.j2);
  show("pair-join.1", a.j1);
  show("pair-join.2", a.j2);
  const LnQuantPair b = ln_quant_jobs(at(0x70), n1, &n2, nullptr, nullptr);
  show("pair-plain.1", b.j1);
  show("pair-plain.2", b.j2);
  const LnQuantPair c = ln_quant_jobs(at(0x70), n1, nullptr, &join, nullptr);
  printf("one-join two=%%d second=%%lx\n", c.two, u(c.second()));
  show("one-join.1", c.j1);

  GemvJob J = gemv_job(at<void>(0x6000), 96, 64, ActRow{q4_rows(at<void>(0x7000), 64), at(0x160)}, at(0x170), at(0x180));
  printf("gemv w.qs=%%lx w.d=%%lx rows=%%d k=%%d tiles=%%d xd=%%lx xqs=%%lx xdd=%%lx bias=%%lx y=%%lx epi=%%d tab=%%lx oq_qs=%%lx\n",
         u(J.w.qs), u(J.w.d), J.w.rows, J.w.k, J.w.tiles, u(J.xd), u(J.xqs), u(J.xdd), u(J.bias), u(J.y), J.epi,
         u(J.gelu_tab), u(J.oq_qs));
  gelu_quant_into(J, at<uint16_t>(0x190), ActRow{q4_rows(at<void>(0x8000), 96), at(0x1a0)});
  printf("gelu epi=%%d tab=%%lx oq_qs=%%lx oq_d=%%lx oxd=%%lx y=%%lx\n", J.epi, u(J.gelu_tab), u(J.oq_qs), u(J.oq_d), u(J.oxd),
         u(J.y));
  const GemvJob X = gemv_job(at<void>(0x6000), 33, 32, at(0x160), Q4Rows{}, nullptr, at(0x180));
  printf("gemv-exact tiles=%%d w.d=%%lx xd=%%lx xqs=%%lx xdd=%%lx epi=%%d\n", X.w.tiles, u(X.w.d), u(X.xd), u(X.xqs), u(X.xdd),
         X.epi);
  const GemvBatch B = gemv_batch({J, X});
  printf("batch nj=%%d %%d %%d %%lx\n", B.nj, B.j[0].epi, B.j[1].w.rows, u(B.j[2].w.qs));
  return 0;
}
"""

# 1056 values: 33 blocks, scales 33 * 16 = 0x210 behind the nibbles
WS1056 = "og=100100 jg=102200 rec=104300 ep=100000"
NORM1 = "qs=4000 d=4210 xd=30"
JOIN = "ja=100 jab=110 jf=120 jfb=130"
NOJOIN = "ja=0 jab=0 jf=0 jfb=0"

EXPECTED = [
    # the scale plane: rows * (k / 32) * 16 bytes behind the base
    "q4 k=32 rows=1 qs=0 d=16",
    "q4 k=4096 rows=1 qs=0 d=2048",
    "q4 k=16384 rows=1 qs=0 d=8192",
    "q4 k=64 rows=5 qs=0 d=160",
    "q4 default rows d=2048",
    # 0, 256, 256 + 8 E, 256 + 16 E, 256 + 17 E; 17 E + 1280 bytes
    "ws E=32 ep=0 og=256 jg=512 rec=768 hflag=800 bytes=1824",
    "ws E=1056 ep=0 og=256 jg=8704 rec=17152 hflag=18208 bytes=19232",
    "ws E=8192 ep=0 og=256 jg=65792 rec=131328 hflag=139520 bytes=140544",
    "ws null 0 0 0 0 0",
    # 1/sqrt(256) = 2^-4; 1/sqrt(80) rounded to float
    "scale 0x1p-4 0x1.c9f25cp-4",
    # 96 * 7 = 672 values: 21 blocks, scales 21 * 16 = 0x150 behind the nibbles
    "attn q=1200 k=1300 v=1400 kc=1800 vc=1900 npast=1a00 cs=1500 etab=1600 d=96 H=7 n_rot=24 style=1 n_ctx=333 "
    "nsplit=2 kqv_nth=5 scale=0.375 alibi=1100 oq_qs=2000 oq_d=2150 oxd=3000 out=1700",
    "attn-plain q=1200 k=1300 v=1400 kc=0 vc=0 npast=0 cs=0 etab=1600 d=96 H=7 n_rot=0 style=1 n_ctx=333 "
    "nsplit=1 kqv_nth=5 scale=0.375 alibi=0 oq_qs=2000 oq_d=2150 oxd=3000 out=1700",
    "tail1 x=70 ab=90 fb=a0 jout=80 w1=10 b1=20 q1=4000 d1=4210 xd1=30 w2=0 b2=0 q2=0 d2=0 xd2=0 "
    + WS1056 + " stats=b0 il=3",
    "tail2 x=70 ab=0 fb=a0 jout=80 w1=10 b1=20 q1=4000 d1=4210 xd1=30 w2=40 b2=50 q2=5000 d2=5210 xd2=60 "
    + WS1056 + " stats=b0 il=254",
    # the second job: the same row and join operands, no jout, no epoch
    "pair-join two=1 second=1",
    "pair-join.1 x=70 w=10 b=20 " + NORM1 + " " + JOIN + " jout=140 ep=150",
    "pair-join.2 x=70 w=40 b=50 qs=5000 d=5210 xd=60 " + JOIN + " jout=0 ep=0",
    "pair-plain.1 x=70 w=10 b=20 " + NORM1 + " " + NOJOIN + " jout=0 ep=0",
    "pair-plain.2 x=70 w=40 b=50 qs=5000 d=5210 xd=60 " + NOJOIN + " jout=0 ep=0",
    "one-join two=0 second=0",
    "one-join.1 x=70 w=10 b=20 " + NORM1 + " " + JOIN + " jout=140 ep=0",
    # a 96 x 64 weight: 3 tiles * 32 rows * 2 blocks * 16 bytes = 0xc00 of nibbles; the row's 2 blocks: 0x20
    "gemv w.qs=6000 w.d=6c00 rows=96 k=64 tiles=3 xd=160 xqs=7000 xdd=7020 bias=170 y=180 epi=0 tab=0 oq_qs=0",
    # the epilogue's row of M = 96 values: scales (96 / 32) * 16 = 0x30 behind the nibbles
    "gelu epi=1 tab=190 oq_qs=8000 oq_d=8030 oxd=1a0 y=180",
    "gemv-exact tiles=2 w.d=6400 xd=160 xqs=0 xdd=0 epi=0",
    "batch nj=2 1 33 0",
]


def test_decode_jobs_fields(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.fail("hipcc not found (the header includes common.hpp, which only a HIP compiler takes)")
    src, exe = tmp_path / "jobs.cpp", tmp_path / "jobs"
    src.write_text(PROGRAM % HEADER)
    subprocess.run([HIPCC, "--offload-host-only", "-x", "hip", "-std=c++17", "-O1", "-Wall", "-Wno-unused-function",
                    "-o", str(exe), str(src)], check=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    assert got == EXPECTED
