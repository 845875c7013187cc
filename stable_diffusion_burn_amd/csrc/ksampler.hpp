// ksampler.hpp -- the sigma-schedule samplers (include/sdmi.h "sigma-schedule samplers"): schedules, sigma <-> t and the evaluation plan,
// host only and in f64.  ONE implementation: sdmi_ksampler_sigmas / sdmi_sigma_to_t / sdmi_ksampler_plan export it, the engine calls it.  Everything throws
// sdmi::Error(SDMI_ERR_INVALID) for what the header lists.
#pragma once
#include <cstddef>
#include <vector>

#include "../../include/sdmi.h"

namespace sdmi {

constexpr int KPLAN_COLS = 12;   // step, stage, t, sigma, cx, ce, h1, cz, cz2, qx, qe, a_end
enum { KP_STEP = 0, KP_STAGE, KP_T, KP_SIGMA, KP_CX, KP_CE, KP_H1, KP_CZ, KP_CZ2, KP_QX, KP_QE, KP_AEND };

// what sdmi_set_ksampler refuses; alphas (total entries) gives the range of the sigma bounds (null and 0: the range is not checked)
void check_ksampler(const sdmi_ksampler& k, const float* alphas, int total);
double sigma_to_t(const float* alphas, int total, double sigma);
// steps + 1 sigmas, the last 0; ts (may be null) receives the integer timesteps of schedule 0 (empty for the others)
std::vector<double> ksampler_sigmas(const sdmi_ksampler& k, const float* alphas, int total, size_t n_steps, std::vector<int>* ts = nullptr);
// KPLAN_COLS doubles per UNet evaluation of the call; *call_steps = the steps the call runs
// prediction (sdmi_set_prediction): 0 = the model output is eps, the rows are what they always were; 1 = it is v = sqrt(a) eps - sqrt(1 - a) x0.  With
// a = 1 / sqrt(1 + sigma^2), b = sigma / sqrt(1 + sigma^2) at the evaluation, eps = a v + b x, and every row is linear in x and in the model output: the row for v
// is cx += ce b, ce *= a, qx += qe b, qe *= a -- the history q keeps holding what it held (x0, eps or the start latent).
std::vector<double> ksampler_plan(const sdmi_ksampler& k, const float* alphas, int total, size_t n_steps, double strength, int* call_steps = nullptr, int prediction = 0);

}  // namespace sdmi
