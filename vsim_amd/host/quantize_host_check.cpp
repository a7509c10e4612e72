// vsim_amd/host/quantize_host_check.cpp — the file quantizer's host half run on its own, for the
// sanitizer build (Makefile `asan-quantize`: -fsanitize=address,undefined, no GPU, no library):
//   quantize_host_check <arch 0|1|2> <model-f16-or-f32.bin> <work directory>
// It walks the good file's records, quantizes the file with device == -1, then cuts the file at
// every kind of place (magic, header, vocab, a record's header, a record's data, the last
// record) and expects each cut to be refused with VSIM_EFILE and no output left behind; and it
// runs the host block quantizer over the non-finite inputs.  Prints "quantize_host_check: ok".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../include/vsim_hip.h"
#include "../csrc/quantize_file.hpp"

namespace {

int fail(const std::string &why) {
  fprintf(stderr, "quantize_host_check: FAILED: %s (last error: %s)\n", why.c_str(), vsim_last_error());
  return 1;
}

bool exists(const std::string &p) {
  FILE *f = fopen(p.c_str(), "rb");
  if (f) fclose(f);
  return f != nullptr;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 4) { fprintf(stderr, "usage: %s arch model.bin workdir\n", argv[0]); return 2; }
  const int arch = atoi(argv[1]);
  const std::string good = argv[2], dir = argv[3];

  // the walker over the good file: offsets of the places to cut at
  std::vector<size_t> cuts = {2};
  size_t n_records = 0, size = 0;
  {
    FILE *f = fopen(good.c_str(), "rb");
    if (!f) return fail("cannot open " + good);
    std::vector<uint8_t> raw;
    size_t f16_off = 0;
    if (vsim::quant_read_prologue(f, arch, raw, f16_off)) { fclose(f); return fail("prologue"); }
    cuts.push_back(f16_off + 1);     // inside the header
    cuts.push_back(raw.size() - 1);  // inside the vocab
    while (true) {
      vsim::QuantRecord r;
      const long at = ftell(f);
      const int rc = vsim::quant_read_record(f, r);
      if (rc == 1) break;
      if (rc) { fclose(f); return fail("record walk"); }
      const long data = ftell(f);
      if (n_records < 3 || r.quantize) {
        cuts.push_back((size_t)at + 5);                    // inside the record's header
        cuts.push_back((size_t)data - 1);                  // inside its name
        cuts.push_back((size_t)data + r.src_bytes / 2);    // inside its data
      }
      if (fseek(f, (long)r.src_bytes, SEEK_CUR)) { fclose(f); return fail("seek"); }
      ++n_records;
    }
    size = (size_t)ftell(f);
    fclose(f);
    cuts.push_back(size - 7);
  }
  printf("quantize_host_check: %zu records, %zu bytes, %zu cuts\n", n_records, size, cuts.size());

  const std::string out = dir + "/out-q4_0.bin";
  vsim_quantize_stats st;
  if (vsim_quantize_file(good.c_str(), out.c_str(), arch, -1, &st) != VSIM_OK) return fail("quantize the good file");
  uint64_t sum = 0;
  for (int i = 0; i < 16; ++i) sum += st.hist[i];
  if (st.n_quantized <= 0 || sum == 0 || st.bytes_in != size || !exists(out)) return fail("statistics of the good file");
  // the result is a Q4_0 file: quantizing it again is refused
  const std::string out2 = dir + "/out2.bin";
  if (vsim_quantize_file(out.c_str(), out2.c_str(), arch, -1, nullptr) != VSIM_EFILE || exists(out2))
    return fail("a Q4_0 input was not refused");

  std::vector<uint8_t> whole(size);
  {
    FILE *f = fopen(good.c_str(), "rb");
    if (!f || fread(whole.data(), 1, size, f) != size) return fail("read " + good);
    fclose(f);
  }
  const std::string cut = dir + "/cut.bin", cut_out = dir + "/cut-out.bin";
  for (size_t c : cuts) {
    FILE *f = fopen(cut.c_str(), "wb");
    if (!f || fwrite(whole.data(), 1, c, f) != c) return fail("write " + cut);
    fclose(f);
    const int rc = vsim_quantize_file(cut.c_str(), cut_out.c_str(), arch, -1, nullptr);
    if (rc != VSIM_EFILE) return fail("a file cut at " + std::to_string(c) + " was not refused");
    if (exists(cut_out)) return fail("a file cut at " + std::to_string(c) + " left an output file");
  }

  // the block quantizer on non-finite and degenerate blocks (F32 and F16 sources)
  {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    std::vector<float> x(5 * 32, 0.25f);
    x[0] = nan; x[1] = -7.0f;                      // a NaN is ignored: d = 1
    for (int i = 0; i < 32; ++i) x[32 + i] = nan;  // all NaN: d = 0
    x[64 + 3] = inf; x[96 + 4] = -inf;
    for (int i = 0; i < 32; ++i) x[128 + i] = i == 5 ? 1e-44f : 0.0f;  // id overflows
    uint8_t aos[5 * 20];
    uint64_t hist[16] = {0};
    vsim::quantize_w_host(x.data(), VSIM_SRC_F32, 5, aos, hist);
    float d0;
    memcpy(&d0, aos, 4);
    if (d0 != 1.0f || (aos[4] & 0xF) != 8 || (aos[4] >> 4) != 1) return fail("NaN rule");
    uint64_t n = 0;
    for (int i = 0; i < 16; ++i) n += hist[i];
    if (n != 5 * 32) return fail("histogram count");
    const uint16_t h[32] = {0x0001, 0x7C00, 0xFC00, 0x7E00, 0x7BFF, 0x8000, 0x03FF, 0x0400};
    vsim::quantize_w_host(h, VSIM_SRC_F16, 1, aos, nullptr);
  }
  printf("quantize_host_check: ok\n");
  return 0;
}
