// vsim_amd/csrc/sampler.hpp — the sampler object (vsim_sampler_* in vsim_hip.h), shared by
// sampler.cpp (the host stages) and model.cpp (the sampled decode step).
#pragma once

#include <stdint.h>

#include <random>
#include <vector>

#include "../../include/vsim_hip.h"

struct vsim_sampler {
  vsim_sample_params p{};
  // the reference's widened arguments (vsim.cpp:866-873 passes the float parameters to double
  // arguments and top_k through a float)
  int top_k = 0;
  double top_p = 0.0, temp = 0.0, repeat_penalty = 0.0;
  std::mt19937 rng;
  std::vector<int32_t> win;  // last repeat_last_n tokens, oldest first (vsim.cpp:875-876)
  uint64_t picks = 0, host_picks = 0;
};
