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

#include <algorithm>

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

// ---- CFG rescale (sdmi_set_guidance_rescale) ---------------------------------------------------------------------------
// e' = f_b g with g the guided output and f_b = phi std(ec_b) / std(g_b) + (1 - phi), the statistics over image b's 4 hw elements -- so no element
// can be updated before its whole image has been read.  ONE workgroup per image (blockDim = a multiple of 64, at most 1024) makes three sweeps over
// it: the means of ec and g, the sums of squared deviations from them (two-pass: a model output may sit far from zero), the update.  Thread t owns
// pixels t, t + blockDim, ...: the first RS_REG of them stay in registers across the sweeps (all of a 64 x 64 latent at 1024 threads), the others
// are read again (L2).  Every sum has a fixed order: an fp32 partial per thread over its pixels in ascending order, merged in fp64 by a lane
// butterfly and then wave 0, 1, ... through LDS.  No atomics, nothing of another image: a result depends on neither n nor the image's position.

// One pixel of the step behind the CFG combine, sampler_step_body's arithmetic: e = the (rescaled) guided model output of pixel i (= pixel p of
// image b), x = its latent.  (sampler_step_body keeps its own statements so that the elementwise kernels stay the instructions they were.)
template <int DEPTH, int NOISE, bool MASK>
__device__ __forceinline__ void sampler_pixel(const f32x4 e, const f32x4 x, long long i, long long b, long long p, f32x4* __restrict__ latent,
                                              f32x4* __restrict__ unet_in, long long pixels, long long hw, const SamplerStep& c, const SamplerHist& h,
                                              uint64_t noise_key, uint64_t noise_key2, const float* __restrict__ mask, const f32x4* __restrict__ z0,
                                              const f32x4* __restrict__ e0) {
#pragma clang fp contract(off)
    f32x4 q1 = f32x4{0.f, 0.f, 0.f, 0.f}, q2 = q1, q3 = q1, z = q1, z2 = q1;
    if (DEPTH >= 1 && c.n_hist >= 1) q1 = h.prev[0][i];
    if (DEPTH >= 3 && c.n_hist >= 2) q2 = h.prev[1][i];
    if (DEPTH >= 3 && c.n_hist >= 3) q3 = h.prev[2][i];
    if (NOISE) {
        const uint64_t key = noise_key + (uint64_t)b;
        z = f32x4{normal_draw(key, (uint64_t)p), normal_draw(key, (uint64_t)(hw + p)), normal_draw(key, (uint64_t)(2 * hw + p)),
                  normal_draw(key, (uint64_t)(3 * hw + p))};
        if (NOISE == 2) {
            const uint64_t key2 = noise_key2 + (uint64_t)b;
            z2 = f32x4{normal_draw(key2, (uint64_t)p), normal_draw(key2, (uint64_t)(hw + p)), normal_draw(key2, (uint64_t)(2 * hw + p)),
                       normal_draw(key2, (uint64_t)(3 * hw + p))};
        }
    }
    // sampler_apply and the blend with every contraction written out, in the order the elementwise kernels compile to: where f = 1 the step is theirs bit for bit
    f32x4 nx, q;
    for (int k = 0; k < 4; ++k) {
        q[k] = fmaf(c.qx, x[k], c.qe * e[k]);
        float t = fmaf(c.cx, x[k], c.ce * e[k]);
        if (DEPTH >= 1) t = fmaf(c.h[0], q1[k], t);
        if (DEPTH >= 3) { t = fmaf(c.h[1], q2[k], t); t = fmaf(c.h[2], q3[k], t); }
        if (NOISE) t = fmaf(c.cz, z[k], t);
        if (NOISE == 2) t = fmaf(c.cz2, z2[k], t);
        nx[k] = t;
    }
    if (DEPTH >= 1) h.out[i] = q;   // the pre-blend q
    if (MASK) {
        const f32x4 zs = z0[i], es = e0[i];
        const float m = mask[i], km = 1.0f - m;
        for (int k = 0; k < 4; ++k) nx[k] = fmaf(m, nx[k], km * fmaf(c.blend_prev, zs[k], c.blend_dir * es[k]));
    }
    latent[i] = nx;
    unet_in[i] = nx;
    unet_in[pixels + i] = nx;
}

__device__ __forceinline__ f32x4 sampler_combine4(const f32x4 eu, const f32x4 ec, const SamplerStep& c) {
    return f32x4{sampler_combine(eu.x, ec.x, c), sampler_combine(eu.y, ec.y, c), sampler_combine(eu.z, ec.z, c), sampler_combine(eu.w, ec.w, c)};
}

constexpr int RS_REG = 4;
constexpr int RS_MAX_THREADS = 1024;

// sums a and b over the workgroup in fp64; every thread returns the same two totals.  sh: [2][16] doubles.
__device__ __forceinline__ void block_sum2(double& a, double& b, double* sh) {
    for (int off = 32; off > 0; off >>= 1) { a += __shfl_xor(a, off); b += __shfl_xor(b, off); }
    const int wave = threadIdx.x >> 6, n_wave = blockDim.x >> 6;
    __syncthreads();   // the last call's totals have been read
    if ((threadIdx.x & 63) == 0) { sh[wave] = a; sh[16 + wave] = b; }
    __syncthreads();
    a = 0.0; b = 0.0;
    for (int w = 0; w < n_wave; ++w) { a += sh[w]; b += sh[16 + w]; }
}

__device__ __forceinline__ float sum4(const f32x4 v) { return (v.x + v.y) + (v.z + v.w); }
__device__ __forceinline__ float sq4(const f32x4 v, float m) {
    const float a = v.x - m, b = v.y - m, c = v.z - m, d = v.w - m;
    return (a * a + b * b) + (c * c + d * d);
}

template <int DEPTH, int NOISE, bool MASK>
__global__ __launch_bounds__(RS_MAX_THREADS) void sampler_step_rescale_kernel(const f32x4* __restrict__ eps, f32x4* __restrict__ latent,
                                                                              f32x4* __restrict__ unet_in, long long pixels, long long hw, SamplerStep c,
                                                                              float rescale, SamplerHist h, uint64_t noise_key, uint64_t noise_key2,
                                                                              const float* __restrict__ mask, const f32x4* __restrict__ z0,
                                                                              const f32x4* __restrict__ e0) {
    __shared__ double sh[32];
    const long long b = blockIdx.x, base = b * hw;
    const f32x4* __restrict__ eu_img = eps + base;
    const f32x4* __restrict__ ec_img = eps + pixels + base;
    const long long nt = blockDim.x, tid = threadIdx.x, tail = tid + RS_REG * nt;
    const f32x4 zero = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 reu[RS_REG], rec[RS_REG];
#pragma unroll
    for (int k = 0; k < RS_REG; ++k) {
        const long long p = tid + k * nt;
        const bool in = p < hw;
        reu[k] = in ? eu_img[p] : zero;
        rec[k] = in ? ec_img[p] : zero;
    }
    // sweep 1: the means
    float s_c = 0.f, s_g = 0.f;
#pragma unroll
    for (int k = 0; k < RS_REG; ++k)
        if (tid + k * nt < hw) { s_c += sum4(rec[k]); s_g += sum4(sampler_combine4(reu[k], rec[k], c)); }
    for (long long p = tail; p < hw; p += nt) {
        const f32x4 eu = eu_img[p], ec = ec_img[p];
        s_c += sum4(ec); s_g += sum4(sampler_combine4(eu, ec, c));
    }
    double d_c = (double)s_c, d_g = (double)s_g;
    block_sum2(d_c, d_g, sh);
    const double inv_count = 1.0 / (4.0 * (double)hw);
    const float m_c = (float)(d_c * inv_count), m_g = (float)(d_g * inv_count);
    // sweep 2: the sums of squared deviations
    float v_c = 0.f, v_g = 0.f;
#pragma unroll
    for (int k = 0; k < RS_REG; ++k)
        if (tid + k * nt < hw) { v_c += sq4(rec[k], m_c); v_g += sq4(sampler_combine4(reu[k], rec[k], c), m_g); }
    for (long long p = tail; p < hw; p += nt) {
        const f32x4 eu = eu_img[p], ec = ec_img[p];
        v_c += sq4(ec, m_c); v_g += sq4(sampler_combine4(eu, ec, c), m_g);
    }
    double q_c = (double)v_c, q_g = (double)v_g;
    block_sum2(q_c, q_g, sh);
    // (the Bessel factor cancels in the ratio)  std(g) = 0 or a statistic that is not finite: f = 1
    double fd = (double)rescale * sqrt(q_c / q_g) + (1.0 - (double)rescale);
    if (!(q_g > 0.0) || !(q_c >= 0.0) || !(fd == fd) || fd - fd != 0.0) fd = 1.0;
    const float f = (float)fd;
    // sweep 3: the update
#pragma unroll
    for (int k = 0; k < RS_REG; ++k) {
        const long long p = tid + k * nt;
        if (p < hw) {
            const f32x4 g = sampler_combine4(reu[k], rec[k], c);
            sampler_pixel<DEPTH, NOISE, MASK>(f32x4{f * g.x, f * g.y, f * g.z, f * g.w}, latent[base + p], base + p, b, p, latent, unet_in, pixels, hw, c, h,
                                              noise_key, noise_key2, mask, z0, e0);
        }
    }
    for (long long p = tail; p < hw; p += nt) {
        const f32x4 g = sampler_combine4(eu_img[p], ec_img[p], c);
        sampler_pixel<DEPTH, NOISE, MASK>(f32x4{f * g.x, f * g.y, f * g.z, f * g.w}, latent[base + p], base + p, b, p, latent, unet_in, pixels, hw, c, h,
                                          noise_key, noise_key2, mask, z0, e0);
    }
}

template <int DEPTH>
static void launch_rescale_depth(int noise, bool mask, int images, int threads, hipStream_t s, const f32x4* eps, f32x4* latent, f32x4* unet_in, long long pixels,
                                 long long hw, const SamplerStep& c, float rescale, const SamplerHist& h, uint64_t noise_key, uint64_t noise_key2, const float* m,
                                 const f32x4* z0, const f32x4* e0) {
#define SDMI_RESCALE_LAUNCH(N, M)                                                                                                                       \
    hipLaunchKernelGGL((sampler_step_rescale_kernel<DEPTH, N, M>), dim3(images), dim3(threads), 0, s, eps, latent, unet_in, pixels, hw, c, rescale, h, \
                       noise_key, noise_key2, m, z0, e0)
    constexpr int TWO = DEPTH == 1 ? 2 : 1;   // the second draw belongs to history depth 1 (launch_sampler_step checks)
    if (noise == 2 && mask) SDMI_RESCALE_LAUNCH(TWO, true);
    else if (noise == 2) SDMI_RESCALE_LAUNCH(TWO, false);
    else if (noise && mask) SDMI_RESCALE_LAUNCH(1, true);
    else if (noise) SDMI_RESCALE_LAUNCH(1, false);
    else if (mask) SDMI_RESCALE_LAUNCH(0, true);
    else SDMI_RESCALE_LAUNCH(0, false);
#undef SDMI_RESCALE_LAUNCH
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

hipError_t launch_sampler_step(const float* eps, float* latent, float* unet_in, long long per_half, long long hw, SamplerStep c, float rescale, int depth,
                               const float* const q_prev[3], float* q_out, uint64_t noise_key, uint64_t noise_key2, const float* mask, const float* z0,
                               const float* e0, hipStream_t s) {
    if ((per_half & 3) || hw <= 0 || (per_half / 4) % hw) return hipErrorInvalidValue;
    if (depth != 0 && depth != 1 && depth != 3) return hipErrorInvalidValue;
    if (!(rescale >= 0.0f && rescale <= 1.0f)) return hipErrorInvalidValue;
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
    if (rescale != 0.0f) {   // CFG rescale: one workgroup per image
        const long long images = pixels / hw;
        if (images > 0x7fffffffLL) return hipErrorInvalidValue;
        const int threads = (int)std::min<long long>(RS_MAX_THREADS, (hw + 63) / 64 * 64);
        const int nz = c.cz2 != 0.0f ? 2 : noise ? 1 : 0;
        if (depth == 0) launch_rescale_depth<0>(nz, mask != nullptr, (int)images, threads, s, e4, l4, u4, pixels, hw, c, rescale, h, noise_key, noise_key2, mask, z4, n4);
        else if (depth == 1) launch_rescale_depth<1>(nz, mask != nullptr, (int)images, threads, s, e4, l4, u4, pixels, hw, c, rescale, h, noise_key, noise_key2, mask, z4, n4);
        else launch_rescale_depth<3>(nz, mask != nullptr, (int)images, threads, s, e4, l4, u4, pixels, hw, c, rescale, h, noise_key, noise_key2, mask, z4, n4);
        return hipGetLastError();
    }
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
