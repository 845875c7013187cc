// k_sample.hpp -- device arithmetic of the sampler shared by k_elem.hip (txt2img), k_img2img.hip (img2img) and
// k_sampler.hip (sampler choice): one definition each of the N(0,1) stream, of the CFG + DDIM update and of the
// linear sampler step, so that the paths cannot draw or round differently.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.hpp"

namespace sdmi {

// splitmix64 -> Box-Muller: element i of the N(0,1) stream `seed` (launch_fill_normal; img2img's noise when the caller
// passes none).  Keyed by the element index, so any thread may draw any element.
__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

__device__ __forceinline__ float normal_draw(uint64_t seed, uint64_t i) {
    const uint64_t r = splitmix64(seed * 0xD1342543DE82EF95ull + i);
    const float u1 = ((float)(uint32_t)(r >> 40) + 1.0f) * (1.0f / 16777217.0f);
    const float u2 = (float)(uint32_t)((r >> 8) & 0xFFFFFF) * (1.0f / 16777216.0f);
    return sqrtf(-2.0f * logf(u1)) * cosf(6.283185307179586f * u2);
}

// CFG combine + DDIM update of one latent element (stablediffusion/mod.rs:152-156, 190-191): eu / ec = the
// unconditional / conditional noise predictions, x = the latent at t; returns the latent at t_prev.
__device__ __forceinline__ float cfg_ddim_update(float eu, float ec, float x, const DdimCoef& c) {
    const float e = eu + (ec - eu) * c.scale;                  // :190-191
    const float predx0 = (x - e * c.sqrt_noise) / c.sqrt_cur;  // :152
    const float dir = e * c.dir_coef;                          // :153
    return predx0 * c.sqrt_prev + dir;                         // :155 (sigma = 0)
}

// Sampler choice: one element of a DDIM(eta) / DPM-Solver++(2M) / PLMS step in the linear form of
// sdmi_sampler_coefs.  q1..q3 = the q of one / two / three steps ago (pass 0 where there is none: its weight is 0 then), z = the
// step's N(0,1) draw (0 where cz = 0).  *q = what the step pushes to history (x0 for DPM-Solver++, e for PLMS).
// Plain Euler on sigma = sqrt((1 - a) / a) is this step with DDIM's eta = 0 coefficients, Euler-ancestral with eta = 1.
// The update is the CFG combine followed by the linear step on the guided output e: CFG rescale scales e per image between the two.
__device__ __forceinline__ float sampler_combine(float eu, float ec, const SamplerStep& c) { return eu + (ec - eu) * c.scale; }

__device__ __forceinline__ float sampler_apply(float e, float x, float q1, float q2, float q3, float z, const SamplerStep& c, float* q) {
    *q = c.qx * x + c.qe * e;
    return c.cx * x + c.ce * e + c.h[0] * q1 + c.h[1] * q2 + c.h[2] * q3 + c.cz * z;
}

__device__ __forceinline__ float sampler_update(float eu, float ec, float x, float q1, float q2, float q3, float z, const SamplerStep& c, float* q) {
    return sampler_apply(sampler_combine(eu, ec, c), x, q1, q2, q3, z, c, q);
}

}  // namespace sdmi
