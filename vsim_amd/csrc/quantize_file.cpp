// vsim_amd/csrc/quantize_file.cpp — vsim_quantize_file: the reference's quantize_gptneox /
// quantize_gptj / quantize_bloom (quantize_gptneox.cpp:143-311, type 2) as a streaming pass over
// the file, with the block quantizer on the GPU (k_quantize_w's AoS output) or in a plain host
// loop of the same semantics (device == -1).
//
// The host half of this file (the host quantizer, the record walker, the pass itself) uses no
// HIP type: built with -DVSIM_QUANT_HOST_ONLY it stands alone, which is how the sanitizer check
// (host/quantize_host_check.cpp) compiles it.
#include "quantize_file.hpp"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <memory>

#include "../../include/vsim_hip.h"

#ifndef VSIM_QUANT_HOST_ONLY
#include "common.hpp"
#else
namespace vsim {
static thread_local std::string t_qerr;
void set_error(const std::string &msg) { t_qerr = msg; }
}  // namespace vsim
extern "C" const char *vsim_last_error(void) { return vsim::t_qerr.c_str(); }
#endif

namespace vsim {

namespace {

constexpr int QKW = 32, QBW = 20;
constexpr size_t CHUNK_BYTES = 64u << 20;  // source bytes per streamed chunk
std::atomic<int> g_verbose{0};

float half_to_float(uint16_t h) {  // exact, subnormals included
  const uint32_t sign = (uint32_t)(h & 0x8000u) << 16;
  const uint32_t e = (h >> 10) & 0x1Fu, m = h & 0x3FFu;
  uint32_t w;
  if (e == 0x1F) {
    w = sign | 0x7F800000u | (m << 13);
  } else if (e != 0) {
    w = sign | ((e + 112u) << 23) | (m << 13);
  } else if (m == 0) {
    w = sign;
  } else {  // subnormal half: m * 2^-24
    int sh = 0;
    uint32_t mm = m;
    while (!(mm & 0x400u)) { mm <<= 1; ++sh; }
    w = sign | ((113u - sh) << 23) | ((mm & 0x3FFu) << 13);
  }
  float f;
  memcpy(&f, &w, 4);
  return f;
}

// (int8_t)round(v) as the reference's x86 build evaluates it: out of range and NaN give INT_MIN
// from the conversion, whose low byte is 0 (x86_round_i8 in common.hpp is the device's copy)
int round_i8(float v) {
  const float r = roundf(v);
  const int32_t i = fabsf(r) < 2147483648.0f ? (int32_t)r : INT32_MIN;
  return (int)(int8_t)(uint8_t)((uint32_t)i & 0xFFu);
}

int bad(const std::string &why) {
  set_error("quantize: " + why);
  return VSIM_EFILE;
}

bool rd(FILE *f, void *p, size_t n) { return fread(p, 1, n, f) == n; }

}  // namespace

void quantize_w_host(const void *src, int src_type, size_t nblocks, uint8_t *aos, uint64_t *hist) {
  for (size_t b = 0; b < nblocks; ++b) {
    float v[QKW];
    if (src_type == VSIM_SRC_F16) {
      uint16_t h[QKW];
      memcpy(h, (const uint8_t *)src + b * QKW * 2, sizeof h);
      for (int l = 0; l < QKW; ++l) v[l] = half_to_float(h[l]);
    } else {
      memcpy(v, (const uint8_t *)src + b * QKW * 4, sizeof v);
    }
    float amax = 0.0f;
    for (int l = 0; l < QKW; ++l) {
      const float f = fabsf(v[l]);
      amax = amax < f ? f : amax;  // std::max(amax, f): a NaN is ignored
    }
    const float d = amax / 7.0f;
    const float id = d != 0.0f ? 1.0f / d : 0.0f;
    uint8_t *o = aos + b * QBW;
    memcpy(o, &d, 4);
    for (int l = 0; l < QKW; l += 2) {
      const int q0 = (round_i8(v[l] * id) + 8) & 0xF, q1 = (round_i8(v[l + 1] * id) + 8) & 0xF;
      o[4 + l / 2] = (uint8_t)(q0 | (q1 << 4));
      if (hist) {
        hist[q0]++;
        hist[q1]++;
      }
    }
  }
}

int quant_read_prologue(FILE *f, int arch, std::vector<uint8_t> &raw, size_t &f16_off) {
  raw.clear();
  auto take = [&](size_t n) {
    const size_t at = raw.size();
    raw.resize(at + n);
    if (rd(f, raw.data() + at, n)) return true;
    raw.resize(at);
    return false;
  };
  auto i32_at = [&](size_t off) {
    int32_t v;
    memcpy(&v, raw.data() + off, 4);
    return v;
  };
  if (!take(4) || (uint32_t)i32_at(0) != 0x67676d6cu) return bad("bad magic");
  // gptneox: n_vocab n_embd n_head n_layer n_rot use_parallel_residual f16 (vsim.cpp:119-150)
  // gptj:    n_vocab n_embd n_head n_layer n_rot f16, then a second vocab count
  // bloom:   n_vocab n_embd n_mult n_head n_layer f16 (convert_bloom_to_ggml.py:79-85)
  const int nfields = arch == VSIM_ARCH_GPTNEOX ? 7 : 6;
  if (arch != VSIM_ARCH_GPTNEOX && arch != VSIM_ARCH_GPTJ && arch != VSIM_ARCH_BLOOM) {
    set_error("quantize: unknown architecture");
    return VSIM_EINVAL;
  }
  if (!take(4 * (size_t)nfields)) return bad("truncated header");
  f16_off = 4 + 4 * (size_t)(nfields - 1);
  int32_t nv = i32_at(4);
  if (arch == VSIM_ARCH_GPTJ) {
    if (!take(4)) return bad("truncated vocab count");
    nv = i32_at(raw.size() - 4);
  }
  if (nv < 0 || nv > (1 << 24)) return bad("vocab count out of range");
  for (int i = 0; i < nv; ++i) {
    if (!take(4)) return bad("truncated vocab");
    const uint32_t len = (uint32_t)i32_at(raw.size() - 4);
    if (len > (1u << 20)) return bad("corrupt vocab");
    if (!take(len)) return bad("truncated vocab");
  }
  return VSIM_OK;
}

int quant_read_record(FILE *f, QuantRecord &r) {
  int32_t head[3];
  const size_t got = fread(head, 1, sizeof head, f);
  if (got == 0) return 1;  // end of file between records
  if (got != sizeof head) return bad("truncated tensor record");
  r = QuantRecord();
  r.n_dims = head[0];
  r.ftype = head[2];
  const int32_t ln = head[1];
  if (r.n_dims < 1 || r.n_dims > 2 || ln < 1 || ln > 512) return bad("corrupt tensor record (n_dims / name length)");
  r.nelements = 1;
  for (int i = 0; i < r.n_dims; ++i) {
    if (!rd(f, &r.ne[i], 4)) return bad("truncated tensor record");
    if (r.ne[i] <= 0) return bad("corrupt tensor dimensions");
    r.nelements *= (size_t)r.ne[i];
  }
  r.name.assign((size_t)ln, 0);
  if (!rd(f, &r.name[0], (size_t)ln)) return bad("truncated tensor record");
  // quantize_gptneox.cpp:171-185: the name matches ".*weight" and the tensor is 2-D
  const bool weight = r.name.size() >= 6 && r.name.compare(r.name.size() - 6, 6, "weight") == 0;
  r.quantize = weight && r.n_dims == 2;
  if (r.quantize) {
    if (r.ftype == 2 || r.ftype == 3)
      return bad("unsupported ftype for integer quantization: " + r.name + " is already quantized (ftype " +
                 std::to_string(r.ftype) + ")");
    if (r.ftype != 0 && r.ftype != 1)
      return bad("unsupported ftype for integer quantization: unknown ftype " + std::to_string(r.ftype) + " in " +
                 r.name);
    if (r.ne[0] % QKW) return bad("tensor " + r.name + " has ne[0] not a multiple of 32");
  } else if (r.ftype != 0 && r.ftype != 1) {
    return bad("unknown ftype " + std::to_string(r.ftype) + " in " + r.name);
  }
  r.src_bytes = r.nelements * (r.ftype == 0 ? 4u : 2u);
  return VSIM_OK;
}

namespace {

// The block quantizer behind the pass: chunks of whole rows in, AoS blocks out.
struct Backend {
  virtual ~Backend() {}
  virtual int reserve(size_t in_bytes, size_t out_bytes) = 0;
  virtual void *in() = 0;  // where the next chunk is read to
  // quantize the chunk in in(): rows x k of src_type -> *out (valid until the next call)
  virtual int run(int src_type, int rows, int k, const uint8_t **out) = 0;
  virtual int begin_tensor() { return VSIM_OK; }
  virtual int end_tensor(uint64_t hist[16]) = 0;
};

struct HostBackend : Backend {
  std::vector<uint8_t> src, dst;
  uint64_t h[16] = {0};
  int reserve(size_t in_bytes, size_t out_bytes) override {
    if (src.size() < in_bytes) src.resize(in_bytes);
    if (dst.size() < out_bytes) dst.resize(out_bytes);
    return VSIM_OK;
  }
  void *in() override { return src.data(); }
  int run(int src_type, int rows, int k, const uint8_t **out) override {
    quantize_w_host(src.data(), src_type, (size_t)rows * (size_t)(k / QKW), dst.data(), h);
    *out = dst.data();
    return VSIM_OK;
  }
  int begin_tensor() override {
    memset(h, 0, sizeof h);
    return VSIM_OK;
  }
  int end_tensor(uint64_t hist[16]) override {
    memcpy(hist, h, sizeof h);
    return VSIM_OK;
  }
};

#ifndef VSIM_QUANT_HOST_ONLY
struct DeviceBackend : Backend {
  void *h_in = nullptr, *h_out = nullptr, *d_in = nullptr, *d_out = nullptr;
  uint64_t *d_hist = nullptr;
  size_t cap_in = 0, cap_out = 0;
  hipStream_t s = nullptr;
  int init(int device) {
    VSIM_HIP(hipSetDevice(device));
    VSIM_HIP(hipStreamCreate(&s));
    VSIM_HIP(hipMalloc((void **)&d_hist, 16 * sizeof(uint64_t)));
    return VSIM_OK;
  }
  ~DeviceBackend() override {
    if (s) (void)hipStreamSynchronize(s);
    release();
    if (d_hist) (void)hipFree(d_hist);
    if (s) (void)hipStreamDestroy(s);
  }
  void release() {
    if (h_in) (void)hipHostFree(h_in);
    if (h_out) (void)hipHostFree(h_out);
    if (d_in) (void)hipFree(d_in);
    if (d_out) (void)hipFree(d_out);
    h_in = h_out = d_in = d_out = nullptr;
    cap_in = cap_out = 0;
  }
  int reserve(size_t in_bytes, size_t out_bytes) override {
    if (in_bytes <= cap_in && out_bytes <= cap_out) return VSIM_OK;
    in_bytes = in_bytes > cap_in ? in_bytes : cap_in;
    out_bytes = out_bytes > cap_out ? out_bytes : cap_out;
    release();
    VSIM_HIP(hipHostMalloc(&h_in, in_bytes, hipHostMallocDefault));
    VSIM_HIP(hipHostMalloc(&h_out, out_bytes, hipHostMallocDefault));
    VSIM_HIP(hipMalloc(&d_in, in_bytes));
    VSIM_HIP(hipMalloc(&d_out, out_bytes));
    cap_in = in_bytes;
    cap_out = out_bytes;
    return VSIM_OK;
  }
  void *in() override { return h_in; }
  int run(int src_type, int rows, int k, const uint8_t **out) override {
    const size_t nin = (size_t)rows * k * (src_type == VSIM_SRC_F16 ? 2 : 4);
    const size_t nout = (size_t)rows * (k / QKW) * QBW;
    VSIM_HIP(hipMemcpyAsync(d_in, h_in, nin, hipMemcpyHostToDevice, s));
    if (int rc = launch_quantize_w(d_in, src_type, rows, k, nullptr, 0, 0, d_out, d_hist, s)) return rc;
    VSIM_HIP(hipMemcpyAsync(h_out, d_out, nout, hipMemcpyDeviceToHost, s));
    VSIM_HIP(hipStreamSynchronize(s));
    *out = (const uint8_t *)h_out;
    return VSIM_OK;
  }
  int begin_tensor() override {
    VSIM_HIP(hipMemsetAsync(d_hist, 0, 16 * sizeof(uint64_t), s));
    return VSIM_OK;
  }
  int end_tensor(uint64_t hist[16]) override {
    VSIM_HIP(hipMemcpyAsync(hist, d_hist, 16 * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    VSIM_HIP(hipStreamSynchronize(s));
    return VSIM_OK;
  }
};
#endif

struct File {
  FILE *f = nullptr;
  ~File() {
    if (f) fclose(f);
  }
};

int quantize_pass(FILE *fin, FILE *fout, int arch, Backend &be, vsim_quantize_stats &st) {
  const bool verbose = g_verbose.load() != 0;
  auto wr = [&](const void *p, size_t n) {
    st.bytes_out += n;
    return fwrite(p, 1, n, fout) == n;
  };
  auto werr = []() { return bad("cannot write the output file"); };
  std::vector<uint8_t> raw;
  size_t f16_off = 0;
  if (int rc = quant_read_prologue(fin, arch, raw, f16_off)) return rc;
  const int32_t two = 2;
  memcpy(raw.data() + f16_off, &two, 4);
  st.bytes_in += raw.size();
  if (!wr(raw.data(), raw.size())) return werr();
  std::vector<uint8_t> copy_buf;
  while (true) {
    QuantRecord r;
    const int rc = quant_read_record(fin, r);
    if (rc == 1) break;
    if (rc) return rc;
    const size_t head_bytes = 12 + 4 * (size_t)r.n_dims + r.name.size();
    st.bytes_in += head_bytes;
    const int32_t head[3] = {r.n_dims, (int32_t)r.name.size(), r.quantize ? 2 : r.ftype};
    if (!wr(head, sizeof head) || !wr(r.ne, 4 * (size_t)r.n_dims) || !wr(r.name.data(), r.name.size())) return werr();
    uint64_t hist[16] = {0};
    size_t out_bytes = 0;
    if (r.quantize) {
      const int k = r.ne[0], rows = r.ne[1];
      const size_t esz = r.ftype == 0 ? 4 : 2, row_in = (size_t)k * esz, row_out = (size_t)(k / QKW) * QBW;
      size_t chunk = CHUNK_BYTES / row_in;
      if (chunk < 1) chunk = 1;
      if (chunk > (size_t)rows) chunk = (size_t)rows;
      if (int e = be.reserve(chunk * row_in, chunk * row_out)) return e;
      if (int e = be.begin_tensor()) return e;
      for (size_t r0 = 0; r0 < (size_t)rows; r0 += chunk) {
        const size_t n = std::min(chunk, (size_t)rows - r0);
        if (!rd(fin, be.in(), n * row_in)) return bad("truncated tensor " + r.name);
        const uint8_t *q = nullptr;
        if (int e = be.run(r.ftype == 0 ? VSIM_SRC_F32 : VSIM_SRC_F16, (int)n, k, &q)) return e;
        if (!wr(q, n * row_out)) return werr();
      }
      if (int e = be.end_tensor(hist)) return e;
      out_bytes = (size_t)rows * row_out;
      for (int i = 0; i < 16; ++i) st.hist[i] += hist[i];
      st.n_quantized++;
    } else {
      copy_buf.resize(std::min(r.src_bytes, (size_t)1 << 20));
      for (size_t left = r.src_bytes; left;) {
        const size_t n = std::min(left, copy_buf.size());
        if (!rd(fin, copy_buf.data(), n)) return bad("truncated tensor " + r.name);
        if (!wr(copy_buf.data(), n)) return werr();
        left -= n;
      }
      out_bytes = r.src_bytes;
      st.n_copied++;
    }
    st.bytes_in += r.src_bytes;
    if (verbose) {
      static const char *const tn[2] = {"f32", "f16"};
      printf("%48s - [%6d, %6d], type = %4s ", r.name.c_str(), r.ne[0], r.ne[1], tn[r.ftype]);
      if (r.quantize) {
        printf("-> q4_0, size = %9.3f MB -> %9.3f MB | hist: ", r.src_bytes / 1048576.0, out_bytes / 1048576.0);
        for (int i = 0; i < 16; ++i) printf("%5.3f ", (double)hist[i] / (double)r.nelements);
        printf("\n");
      } else {
        printf("copied,  size = %9.3f MB\n", out_bytes / 1048576.0);
      }
    }
  }
  if (fflush(fout) != 0) return werr();
  if (verbose) {
    uint64_t sum = 0;
    for (int i = 0; i < 16; ++i) sum += st.hist[i];
    printf("quantize: %d tensors quantized, %d copied, %.2f MB -> %.2f MB\nquantize: hist: ", st.n_quantized,
           st.n_copied, st.bytes_in / 1048576.0, st.bytes_out / 1048576.0);
    for (int i = 0; i < 16; ++i) printf("%5.3f ", sum ? (double)st.hist[i] / (double)sum : 0.0);
    printf("\n");
  }
  return VSIM_OK;
}

}  // namespace
}  // namespace vsim

using namespace vsim;

extern "C" {

int vsim_quantize_set_verbose(int on) { return g_verbose.exchange(on ? 1 : 0); }

int vsim_quantize_file(const char *in, const char *out, int arch, int device, vsim_quantize_stats *st) {
  if (!in || !out) { set_error("quantize: null argument"); return VSIM_EINVAL; }
  if (strcmp(in, out) == 0) {  // opening the output would empty the input
    set_error("quantize: input and output are the same file");
    return VSIM_EINVAL;
  }
  vsim_quantize_stats local;
  memset(&local, 0, sizeof local);
  if (st) *st = local;
  int rc;
  {
    File fi, fo;
    fi.f = fopen(in, "rb");
    if (!fi.f) return bad(std::string("cannot open ") + in);
    std::unique_ptr<Backend> be;
    if (device < 0) {
      be.reset(new HostBackend());
    } else {
#ifndef VSIM_QUANT_HOST_ONLY
      DeviceBackend *d = new DeviceBackend();
      be.reset(d);
      if (int e = d->init(device)) return e;
#else
      set_error("quantize: this build has no device path");
      return VSIM_ENODEV;
#endif
    }
    fo.f = fopen(out, "wb");
    if (!fo.f) return bad(std::string("cannot open ") + out + " for writing");
    rc = quantize_pass(fi.f, fo.f, arch, *be, local);
    if (rc == VSIM_OK) {
      const int c = fclose(fo.f);
      fo.f = nullptr;
      if (c != 0) rc = bad("cannot write the output file");
    }
  }
  if (rc != VSIM_OK) {
    remove(out);  // never leave a partly written model behind
    return rc;
  }
  if (st) *st = local;
  return VSIM_OK;
}

}  // extern "C"
