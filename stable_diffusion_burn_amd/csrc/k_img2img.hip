// k_img2img.hip -- the glue between the VAE encoder and the DDIM loop for image-to-image sampling
// (no reference counterpart: the reference's sampler always starts from noise,
// stablediffusion/mod.rs:115-121).  DESIGN.md section "img2img" states the semantics.
//
//  * u8 HWC image -> the encoder's fp32 NHWC4 input, x = v / 127.5 - 1
//  * start latent x_t0 = sqrt(a_t0) z0 + sqrt(1 - a_t0) eps, written to the latent and both CFG halves
//    of the UNet input (what launch_dup_latent does for txt2img)
//  * CFG + DDIM update followed by the latent-mask blend toward the re-noised start latent
// Elementwise and tiny (one 16-byte f32x4 per latent pixel, ~64 KB per latent image): grid-stride loops,
// no LDS.
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

// rgb [pixels][3] u8 -> dst [pixels] f32x4 = (v / 127.5 - 1, .., .., 0): conv_in of the encoder runs with Cin = 4
__global__ void rgb_u8_to_nhwc4_kernel(const uint8_t* __restrict__ rgb, f32x4* __restrict__ dst, long long pixels) {
    GRID_STRIDE(i, pixels) {
        const uint8_t* s = rgb + 3 * i;
        f32x4 v;
        v.x = (float)s[0] / 127.5f - 1.0f;
        v.y = (float)s[1] / 127.5f - 1.0f;
        v.z = (float)s[2] / 127.5f - 1.0f;
        v.w = 0.f;
        dst[i] = v;
    }
}

// Start latent of n images of hw pixels.  FROM_Q8: z0 = 0.18215 * channels 0..3 of the encoder's NHWC8 quant_conv output;
// otherwise z0 comes from the caller in NCHW.  eps: the caller's NCHW noise, or image b's draw from stream seed + b at its
// NCHW element index (launch_fill_normal's order).  latent / unet_in / z0_out / eps_out are NHWC4 (one f32x4 per pixel);
// unet_in's conditional half starts `half4` pixels after the unconditional one.  z0_out / eps_out (both or neither) keep
// z0 and eps for the mask blend of every step.
template <bool FROM_Q8>
__global__ void img2img_start_kernel(const float* __restrict__ z_src, const float* __restrict__ noise, uint64_t seed, float sqrt_a, float sqrt_1ma,
                                     f32x4* __restrict__ latent, f32x4* __restrict__ unet_in, long long half4, f32x4* __restrict__ z0_out,
                                     f32x4* __restrict__ eps_out, long long hw, long long pixels) {
    GRID_STRIDE(i, pixels) {
        const long long b = i / hw, p = i - b * hw;
        f32x4 z;
        if (FROM_Q8) {
            z = reinterpret_cast<const f32x4*>(z_src)[2 * i] * 0.18215f;
        } else {
            const float* s = z_src + b * 4 * hw + p;
            z = f32x4{s[0], s[hw], s[2 * hw], s[3 * hw]};
        }
        f32x4 e;
        if (noise) {
            const float* s = noise + b * 4 * hw + p;
            e = f32x4{s[0], s[hw], s[2 * hw], s[3 * hw]};
        } else {
            const uint64_t sb = seed + (uint64_t)b;
            e = f32x4{normal_draw(sb, (uint64_t)p), normal_draw(sb, (uint64_t)(hw + p)), normal_draw(sb, (uint64_t)(2 * hw + p)),
                      normal_draw(sb, (uint64_t)(3 * hw + p))};
        }
        f32x4 x;
        x.x = sqrt_a * z.x + sqrt_1ma * e.x;
        x.y = sqrt_a * z.y + sqrt_1ma * e.y;
        x.z = sqrt_a * z.z + sqrt_1ma * e.z;
        x.w = sqrt_a * z.w + sqrt_1ma * e.w;
        latent[i] = x;
        unet_in[i] = x;
        unet_in[half4 + i] = x;
        if (z0_out) {
            z0_out[i] = z;
            eps_out[i] = e;
        }
    }
}

// cfg_ddim_kernel (k_elem.hip) followed by x <- m x + (1 - m)(sqrt(a_prev) z0 + sqrt(1 - a_prev) eps): mask [pixels] (1 = regenerate)
__global__ void cfg_ddim_masked_kernel(const f32x4* __restrict__ eps, f32x4* __restrict__ latent, f32x4* __restrict__ unet_in, long long pixels,
                                       DdimCoef c, const float* __restrict__ mask, const f32x4* __restrict__ z0, const f32x4* __restrict__ e0) {
    GRID_STRIDE(i, pixels) {
        const f32x4 eu = eps[i], ec = eps[pixels + i], x = latent[i], z = z0[i], e = e0[i];
        const float m = mask[i], km = 1.0f - m;
        f32x4 nx;
        nx.x = cfg_ddim_update(eu.x, ec.x, x.x, c);
        nx.y = cfg_ddim_update(eu.y, ec.y, x.y, c);
        nx.z = cfg_ddim_update(eu.z, ec.z, x.z, c);
        nx.w = cfg_ddim_update(eu.w, ec.w, x.w, c);
        nx.x = m * nx.x + km * (c.sqrt_prev * z.x + c.dir_coef * e.x);   // dir_coef = sqrt(1 - a_prev)
        nx.y = m * nx.y + km * (c.sqrt_prev * z.y + c.dir_coef * e.y);
        nx.z = m * nx.z + km * (c.sqrt_prev * z.z + c.dir_coef * e.z);
        nx.w = m * nx.w + km * (c.sqrt_prev * z.w + c.dir_coef * e.w);
        latent[i] = nx;
        unet_in[i] = nx;
        unet_in[pixels + i] = nx;
    }
}

// ---- launchers ---------------------------------------------------------------------------
hipError_t launch_rgb_u8_to_nhwc4(const uint8_t* rgb, float* dst, long long pixels, hipStream_t s) {
    hipLaunchKernelGGL(rgb_u8_to_nhwc4_kernel, dim3(blocks_for(pixels)), dim3(256), 0, s, rgb, reinterpret_cast<f32x4*>(dst), pixels);
    return hipGetLastError();
}

hipError_t launch_img2img_start(const float* z_src, bool from_q8, const float* noise, uint64_t seed, float sqrt_a, float sqrt_1ma, float* latent,
                                float* unet_in, long long half_elems, float* z0_out, float* eps_out, int n, long long hw, hipStream_t s) {
    if ((half_elems & 3) || (!z0_out) != (!eps_out)) return hipErrorInvalidValue;
    const long long pixels = (long long)n * hw;
    auto* lat = reinterpret_cast<f32x4*>(latent);
    auto* uin = reinterpret_cast<f32x4*>(unet_in);
    auto* zo = reinterpret_cast<f32x4*>(z0_out);
    auto* eo = reinterpret_cast<f32x4*>(eps_out);
    if (from_q8)
        hipLaunchKernelGGL(img2img_start_kernel<true>, dim3(blocks_for(pixels)), dim3(256), 0, s, z_src, noise, seed, sqrt_a, sqrt_1ma, lat, uin,
                           half_elems / 4, zo, eo, hw, pixels);
    else
        hipLaunchKernelGGL(img2img_start_kernel<false>, dim3(blocks_for(pixels)), dim3(256), 0, s, z_src, noise, seed, sqrt_a, sqrt_1ma, lat, uin,
                           half_elems / 4, zo, eo, hw, pixels);
    return hipGetLastError();
}

hipError_t launch_cfg_ddim_masked(const float* eps, float* latent, float* unet_in, long long per_half, DdimCoef c, const float* mask,
                                  const float* z0, const float* e0, hipStream_t s) {
    if (per_half & 3) return hipErrorInvalidValue;
    const long long pixels = per_half / 4;
    hipLaunchKernelGGL(cfg_ddim_masked_kernel, dim3(blocks_for(pixels)), dim3(256), 0, s, reinterpret_cast<const f32x4*>(eps),
                       reinterpret_cast<f32x4*>(latent), reinterpret_cast<f32x4*>(unet_in), pixels, c, mask,
                       reinterpret_cast<const f32x4*>(z0), reinterpret_cast<const f32x4*>(e0));
    return hipGetLastError();
}

}  // namespace sdmi
