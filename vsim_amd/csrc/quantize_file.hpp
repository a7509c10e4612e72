// vsim_amd/csrc/quantize_file.hpp — the file quantizer's host pieces (no HIP types): the host
// restatement of the weight quantizer and the walker over a ggml model file's records.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <cstdio>
#include <string>
#include <vector>

namespace vsim {

// ggml_quantize_q4_0 (utils.cpp:425-482) of nblocks consecutive 32-blocks of F32 (src_type 0) or
// F16 (1) values: 20-byte AoS blocks into aos, hist[code]++ (hist may be null).  The semantics of
// k_quantize_w (quantize_w.hip), NaN rule included.
void quantize_w_host(const void *src, int src_type, size_t nblocks, uint8_t *aos, uint64_t *hist);

// magic, header and vocab of an `arch` file, as raw bytes; f16_off = offset of the header's last
// field.  0 or VSIM_EFILE (reason in vsim_last_error()).
int quant_read_prologue(FILE *f, int arch, std::vector<uint8_t> &raw, size_t &f16_off);

struct QuantRecord {
  int32_t n_dims = 0, ftype = 0;
  int32_t ne[2] = {1, 1};
  std::string name;
  size_t nelements = 0;
  bool quantize = false;  // 2-D and named *weight: rewritten as Q4_0
  size_t src_bytes = 0;   // bytes of data that follow in the input file
};
// the next record's header: 0, 1 at the end of the file, or VSIM_EFILE
int quant_read_record(FILE *f, QuantRecord &r);

}  // namespace vsim
