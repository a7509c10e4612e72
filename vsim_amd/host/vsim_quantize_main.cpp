// vsim_amd/host/vsim_quantize_main.cpp — `vsim-quantize`, the file quantizer's CLI.
//
// The reference has one tool per architecture with the argv `model-f16.bin model-q4_0.bin type`
// (quantize_gptneox.cpp:333-372, quantize_gptj.cpp, quantize_bloom.cpp); this one takes the model
// type first, as vsim-hip does, then the same three arguments:
//   vsim-quantize <gptneox|gptj|codegen|bloom> model-f16.bin model-q4_0.bin 2 [--device N|--host]
// Type 2 is Q4_0; type 3 (Q4_1) is not a format this library runs and is refused.  The work is
// the library's (vsim_quantize_file): on GPU N (default 0) or, with --host, in a host loop.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../../include/vsim_hip.h"

namespace {
void usage(const char *argv0) {
  fprintf(stderr, "usage: %s <gptneox|gptj|codegen|bloom> model-f16.bin model-q4_0.bin type [--device N|--host]\n", argv0);
  fprintf(stderr, "  type = 2 - q4_0\n");
  fprintf(stderr, "  type = 3 - q4_1 (not supported: this library runs Q4_0 only)\n");
}
}  // namespace

int main(int argc, char **argv) {
  if (argc < 5) { usage(argv[0]); return 1; }
  const std::string model_type = argv[1];
  int arch;
  if (model_type == "gptneox") arch = VSIM_ARCH_GPTNEOX;
  else if (model_type == "gptj" || model_type == "codegen") arch = VSIM_ARCH_GPTJ;
  else if (model_type == "bloom") arch = VSIM_ARCH_BLOOM;
  else { fprintf(stderr, "%s: unknown model type: %s\n", argv[0], model_type.c_str()); return 1; }
  const int type = atoi(argv[4]);
  if (type == 3) {
    fprintf(stderr, "%s: type 3 (q4_1) is not supported: this library runs Q4_0 (type 2) only\n", argv[0]);
    return 1;
  }
  if (type != 2) { fprintf(stderr, "%s: invalid quantization type %s\n", argv[0], argv[4]); return 1; }
  int device = 0;
  for (int i = 5; i < argc; ++i) {
    const std::string a = argv[i];
    if (a == "--host") device = -1;
    else if (a == "--device" && i + 1 < argc) device = atoi(argv[++i]);
    else { fprintf(stderr, "%s: unknown argument: %s\n", argv[0], a.c_str()); usage(argv[0]); return 1; }
  }
  printf("vsim-quantize: '%s' -> '%s' (q4_0) on %s\n", argv[2], argv[3],
         device < 0 ? "the host" : ("GPU " + std::to_string(device)).c_str());
  const auto t0 = std::chrono::steady_clock::now();
  vsim_quantize_stats st;
  vsim_quantize_set_verbose(1);
  if (vsim_quantize_file(argv[2], argv[3], arch, device, &st) != VSIM_OK) {
    fprintf(stderr, "%s: failed to quantize '%s': %s\n", argv[0], argv[2], vsim_last_error());
    return 1;
  }
  const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  printf("vsim-quantize: quantize time = %8.2f ms\n", s * 1e3);
  return 0;
}
