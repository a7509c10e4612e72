// vsim_amd/csrc/sampler.cpp — the sampler object: the host stages of the reference's
// sample_top_p_top_k_repeat_penalty (utils.cpp:339-422) and the last-n window of its main loop
// (vsim.cpp:875-876).  Host code only: nothing here touches the GPU.
//
// The candidate stage (penalty, temperature, ordered top-k) has two makers: k_sample_topk on
// the device (sample.hip; vsim_op_topk, the model's sampled step) and sample_host's loop over
// the logits.  Both end in finish(), the only copy of the k-element stage: softmax in double
// with glibc's exp, the top-p cut, std::discrete_distribution over std::mt19937.
#include <algorithm>
#include <cmath>
#include <string>

#include "common.hpp"
#include "sampler.hpp"

using namespace vsim;

namespace {

// utils.cpp:373-421 on the ordered candidates; pushes the chosen id into the window
int32_t finish(vsim_sampler *s, std::vector<std::pair<double, int32_t>> &cand) {
  double maxl = -INFINITY;
  for (auto &kv : cand) maxl = std::max(maxl, kv.first);
  std::vector<double> probs;
  probs.reserve(cand.size());
  double sum = 0.0;
  for (auto &kv : cand) {
    const double pr = std::exp(kv.first - maxl);
    probs.push_back(pr);
    sum += pr;
  }
  for (auto &pr : probs) pr /= sum;
  if (s->top_p < 1.0f) {
    double cum = 0.0f;
    for (int i = 0; i < (int)probs.size(); i++) {
      cum += probs[i];
      if (cum >= s->top_p) {
        probs.resize(i + 1);
        cand.resize(i + 1);
        break;
      }
    }
    cum = 1.0 / cum;
    for (auto &pr : probs) pr *= cum;
  }
  // (fewer than two weights: libstdc++ returns 0 without drawing from the generator)
  std::discrete_distribution<> dist(probs.begin(), probs.end());
  const int32_t id = cand[dist(s->rng)].second;
  vsim_sampler_accept(s, id);
  return id;
}

}  // namespace

extern "C" {

int vsim_sampler_create(const vsim_sample_params *p, vsim_sampler **out) {
  if (!p || !out) { set_error("sampler_create: null argument"); return VSIM_EINVAL; }
  if (p->repeat_last_n < 0) { set_error("sampler_create: repeat_last_n < 0"); return VSIM_EINVAL; }
  auto *s = new vsim_sampler();
  s->p = *p;
  s->top_k = (int)(float)p->top_k;
  s->top_p = p->top_p;
  s->temp = p->temp;
  s->repeat_penalty = p->repeat_penalty;
  s->rng.seed(p->seed);
  s->win.assign((size_t)p->repeat_last_n, 0);
  *out = s;
  return VSIM_OK;
}

int vsim_sampler_accept(vsim_sampler *s, int32_t token) {
  if (!s) { set_error("sampler_accept: null sampler"); return VSIM_EINVAL; }
  if (s->win.empty()) return VSIM_OK;  // repeat_last_n = 0: no window
  s->win.erase(s->win.begin());
  s->win.push_back(token);
  return VSIM_OK;
}

int vsim_sampler_pick(vsim_sampler *s, const double *val, const int32_t *id, int k, int32_t *token) {
  if (!s || !val || !id || !token) { set_error("sampler_pick: null argument"); return VSIM_EINVAL; }
  if (k < 1 || k > VSIM_TOPK_MAX) {
    set_error("sampler_pick: k must be in 1.." + std::to_string(VSIM_TOPK_MAX));
    return VSIM_EINVAL;
  }
  std::vector<std::pair<double, int32_t>> cand((size_t)k);
  for (int i = 0; i < k; ++i) cand[i] = {val[i], id[i]};
  *token = finish(s, cand);
  ++s->picks;
  return VSIM_OK;
}

int vsim_sampler_sample_host(vsim_sampler *s, const float *logits, int n, int32_t *token) {
  if (!s || !logits || !token) { set_error("sampler_sample_host: null argument"); return VSIM_EINVAL; }
  // (the reference's partial_sort past the end of the candidates is undefined)
  if (s->top_k < 1 || s->top_k > n) { set_error("sampler_sample_host: top_k must be in 1..n"); return VSIM_EINVAL; }
  std::vector<std::pair<double, int32_t>> cand;
  cand.reserve(n);
  const double scale = 1.0 / s->temp, repeat_penalty = s->repeat_penalty;
  for (int i = 0; i < n; ++i) {
    if (std::find(s->win.begin(), s->win.end(), i) != s->win.end())
      cand.push_back({logits[i] < 0.0 ? logits[i] * scale * repeat_penalty : logits[i] * scale / repeat_penalty, i});
    else
      cand.push_back({logits[i] * scale, i});
  }
  std::partial_sort(cand.begin(), cand.begin() + s->top_k, cand.end(),
                    [](const std::pair<double, int32_t> &a, const std::pair<double, int32_t> &b) {
                      return a.first > b.first;
                    });
  cand.resize(s->top_k);
  *token = finish(s, cand);
  ++s->host_picks;
  return VSIM_OK;
}

int vsim_sampler_stats(const vsim_sampler *s, uint64_t *picks, uint64_t *host_picks) {
  if (!s) { set_error("sampler_stats: null sampler"); return VSIM_EINVAL; }
  if (picks) *picks = s->picks;
  if (host_picks) *host_picks = s->host_picks;
  return VSIM_OK;
}

void vsim_sampler_free(vsim_sampler *s) { delete s; }

}  // extern "C"
