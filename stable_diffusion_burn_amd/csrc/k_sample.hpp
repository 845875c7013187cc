// k_sample.hpp -- device arithmetic of the sampler shared by k_elem.hip (txt2img) and k_img2img.hip (img2img):
// one definition each of the N(0,1) stream and of the CFG + DDIM update, so that the two paths cannot draw or
// round differently.
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

}  // namespace sdmi
