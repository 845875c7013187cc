// k_sampler.hip -- the per-step update of the sampler choice (sdmi_set_sampler): stochastic DDIM (eta),
// DPM-Solver++(2M) and PLMS.  No reference counterpart: the reference integrates with DDIM at sigma = 0 only
// (stablediffusion/mod.rs:142-156), which stays on cfg_ddim_kernel / cfg_ddim_masked_kernel.
//
// All three are linear in what is on the device at the end of a step -- the latent x, the two halves of the UNet output, at most
// three earlier q, one N(0,1) draw -- so ONE launch per step does the CFG combine, forms q, applies the update, draws z where the
// step has noise, blends toward the re-noised start latent under an img2img mask, writes the latent and both CFG halves of the next
// UNet input and stores q into the history slot the host rotated to.  Elementwise: one 16-byte f32x4 per latent pixel (NHWC4), a
// grid-stride loop, no LDS.  Templated on history depth, noise and mask so that DDIM(eta) carries no history loads and no form a
// dead one.
#include "kernels.hpp"
#include "k_sample.hpp"

namespace sdmi {

typedef float f32x4 __attribute__((ext_vector_type(4)));

static inline int blocks_for(long long work, int cap = 2048) {
    long long b = (work + 255) / 256;
    if (b < 1) b = 1;
    if (b > cap) b = cap;
    return (int)b;
}

#define GRID_STRIDE(i, total) \
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < (total); i += (long long)gridDim.x * blockDim.x)

struct SamplerHist { const f32x4* prev[3]; f32x4* out; };

// eps [2 pixels] (unconditional half first), latent [pixels] in place, unet_in [2 pixels]; hw pixels per image.  DEPTH history slots:
// h.prev[k] is read where k < c.n_hist, h.out is written (it may alias the oldest slot: a thread reads its pixel first).  NOISE: image
// b's element i is normal_draw(noise_key + b, i), i in NCHW order (launch_fill_normal's); NOISE = 2 (dpmpp_sde's second stage) adds
// cz2 z2, z2 drawn the same way from noise_key2, behind the update -- 0 and 1 are the arithmetic they were.  MASK: launch_cfg_ddim_masked's blend.
template <int DEPTH, int NOISE, bool MASK>
__device__ __forceinline__ void sampler_step_body(const f32x4* __restrict__ eps, f32x4* __restrict__ latent, f32x4* __restrict__ unet_in, long long pixels,
                                                  long long hw, const SamplerStep& c, const SamplerHist& h, uint64_t noise_key, uint64_t noise_key2,
                                                  const float* __restrict__ mask, const f32x4* __restrict__ z0, const f32x4* __restrict__ e0) {
    GRID_STRIDE(i, pixels) {
        const f32x4 eu = eps[i], ec = eps[pixels + i], x = latent[i];
        f32x4 q1 = f32x4{0.f, 0.f, 0.f, 0.f}, q2 = q1, q3 = q1, z = q1, z2 = q1;
        if (DEPTH >= 1 && c.n_hist >= 1) q1 = h.prev[0][i];
        if (DEPTH >= 3 && c.n_hist >= 2) q2 = h.prev[1][i];
        if (DEPTH >= 3 && c.n_hist >= 3) q3 = h.prev[2][i];
        if (NOISE) {
            const long long b = i / hw, p = i - b * hw;
            const uint64_t key = noise_key + (uint64_t)b;
            z = f32x4{normal_draw(key, (uint64_t)p), normal_draw(key, (uint64_t)(hw + p)), normal_draw(key, (uint64_t)(2 * hw + p)),
                      normal_draw(key, (uint64_t)(3 * hw + p))};
            if (NOISE == 2) {
                const uint64_t key2 = noise_key2 + (uint64_t)b;
                z2 = f32x4{normal_draw(key2, (uint64_t)p), normal_draw(key2, (uint64_t)(hw + p)), normal_draw(key2, (uint64_t)(2 * hw + p)),
                           normal_draw(key2, (uint64_t)(3 * hw + p))};
            }
        }
        f32x4 nx;
        float qx, qy, qz, qw;
        nx.x = sampler_update(eu.x, ec.x, x.x, q1.x, q2.x, q3.x, z.x, c, &qx);
        nx.y = sampler_update(eu.y, ec.y, x.y, q1.y, q2.y, q3.y, z.y, c, &qy);
        nx.z = sampler_update(eu.z, ec.z, x.z, q1.z, q2.z, q3.z, z.z, c, &qz);
        nx.w = sampler_update(eu.w, ec.w, x.w, q1.w, q2.w, q3.w, z.w, c, &qw);
        if (NOISE == 2) { nx.x += c.cz2 * z2.x; nx.y += c.cz2 * z2.y; nx.z += c.cz2 * z2.z; nx.w += c.cz2 * z2.w; }
        if (DEPTH >= 1) h.out[i] = f32x4{qx, qy, qz, qw};   // the pre-blend q
        if (MASK) {
            const f32x4 zs = z0[i], es = e0[i];
            const float m = mask[i], km = 1.0f - m;
            nx.x = m * nx.x + km * (c.blend_prev * zs.x + c.blend_dir * es.x);
            nx.y = m * nx.y + km * (c.blend_prev * zs.y + c.blend_dir * es.y);
            nx.z = m * nx.z + km * (c.blend_prev * zs.z + c.blend_dir * es.z);
            nx.w = m * nx.w + km * (c.blend_prev * zs.w + c.blend_dir * es.w);
        }
        latent[i] = nx;
        unet_in[i] = nx;
        unet_in[pixels + i] = nx;
    }
}

// the twelve forms of the sampler choice (section 9b), which the k-samplers share: history depth 0 / 1 / 3 x one draw or none x mask
template <int DEPTH, bool NOISE, bool MASK>
__global__ void sampler_step_kernel(const f32x4* __restrict__ eps, f32x4* __restrict__ latent, f32x4* __restrict__ unet_in, long long pixels,
                                    long long hw, SamplerStep c, SamplerHist h, uint64_t noise_key, const float* __restrict__ mask,
                                    const f32x4* __restrict__ z0, const f32x4* __restrict__ e0) {
    sampler_step_body<DEPTH, NOISE ? 1 : 0, MASK>(eps, latent, unet_in, pixels, hw, c, h, noise_key, 0, mask, z0, e0);
}

// dpmpp_sde's second stage (section 9i): history depth 1 and TWO draws, z from noise_key -- stage 1's, drawn again instead of stored -- and z2 from noise_key2
template <bool MASK>
__global__ void sampler_two_draw_kernel(const f32x4* __restrict__ eps, f32x4* __restrict__ latent, f32x4* __restrict__ unet_in, long long pixels,
                                        long long hw, SamplerStep c, SamplerHist h, uint64_t noise_key, uint64_t noise_key2,
                                        const float* __restrict__ mask, const f32x4* __restrict__ z0, const f32x4* __restrict__ e0) {
    sampler_step_body<1, 2, MASK>(eps, latent, unet_in, pixels, hw, c, h, noise_key, noise_key2, mask, z0, e0);
}

template <int DEPTH>
static void launch_depth(bool noise, bool mask, int blocks, hipStream_t s, const f32x4* eps, f32x4* latent, f32x4* unet_in, long long pixels, long long hw,
                         const SamplerStep& c, const SamplerHist& h, uint64_t noise_key, const float* m, const f32x4* z0, const f32x4* e0) {
#define SDMI_SAMPLER_LAUNCH(N, M) \
    hipLaunchKernelGGL((sampler_step_kernel<DEPTH, N, M>), dim3(blocks), dim3(256), 0, s, eps, latent, unet_in, pixels, hw, c, h, noise_key, m, z0, e0)
    if (noise && mask) SDMI_SAMPLER_LAUNCH(true, true);
    else if (noise) SDMI_SAMPLER_LAUNCH(true, false);
    else if (mask) SDMI_SAMPLER_LAUNCH(false, true);
    else SDMI_SAMPLER_LAUNCH(false, false);
#undef SDMI_SAMPLER_LAUNCH
}

hipError_t launch_sampler_step(const float* eps, float* latent, float* unet_in, long long per_half, long long hw, SamplerStep c, int depth,
                               const float* const q_prev[3], float* q_out, uint64_t noise_key, uint64_t noise_key2, const float* mask, const float* z0,
                               const float* e0, hipStream_t s) {
    if ((per_half & 3) || hw <= 0 || (per_half / 4) % hw) return hipErrorInvalidValue;
    if (depth != 0 && depth != 1 && depth != 3) return hipErrorInvalidValue;
    if (c.n_hist < 0 || c.n_hist > depth || (depth && !q_out)) return hipErrorInvalidValue;
    for (int k = 0; k < c.n_hist; ++k)
        if (!q_prev || !q_prev[k]) return hipErrorInvalidValue;
    if ((!mask) != (!z0) || (!mask) != (!e0)) return hipErrorInvalidValue;
    const long long pixels = per_half / 4;
    SamplerHist h{{nullptr, nullptr, nullptr}, reinterpret_cast<f32x4*>(q_out)};
    for (int k = 0; k < c.n_hist; ++k) h.prev[k] = reinterpret_cast<const f32x4*>(q_prev[k]);
    if (c.cz2 != 0.0f && (depth != 1 || c.cz == 0.0f)) return hipErrorInvalidValue;   // the second draw follows a first one, in a kind of history depth 1
    const bool noise = c.cz != 0.0f;   // z is never drawn where the step has none
    auto* e4 = reinterpret_cast<const f32x4*>(eps);
    auto* l4 = reinterpret_cast<f32x4*>(latent);
    auto* u4 = reinterpret_cast<f32x4*>(unet_in);
    auto* z4 = reinterpret_cast<const f32x4*>(z0);
    auto* n4 = reinterpret_cast<const f32x4*>(e0);
    const int blocks = blocks_for(pixels);
    if (c.cz2 != 0.0f) {
        if (mask) hipLaunchKernelGGL((sampler_two_draw_kernel<true>), dim3(blocks), dim3(256), 0, s, e4, l4, u4, pixels, hw, c, h, noise_key, noise_key2, mask, z4, n4);
        else hipLaunchKernelGGL((sampler_two_draw_kernel<false>), dim3(blocks), dim3(256), 0, s, e4, l4, u4, pixels, hw, c, h, noise_key, noise_key2, mask, z4, n4);
    }
    else if (depth == 0) launch_depth<0>(noise, mask != nullptr, blocks, s, e4, l4, u4, pixels, hw, c, h, noise_key, mask, z4, n4);
    else if (depth == 1) launch_depth<1>(noise, mask != nullptr, blocks, s, e4, l4, u4, pixels, hw, c, h, noise_key, mask, z4, n4);
    else launch_depth<3>(noise, mask != nullptr, blocks, s, e4, l4, u4, pixels, hw, c, h, noise_key, mask, z4, n4);
    return hipGetLastError();
}

}  // namespace sdmi
