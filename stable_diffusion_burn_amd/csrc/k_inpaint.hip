// k_inpaint.hip -- a UNet with conditioning channels next to the latent (sdmi_config.unet_in_ch > 4; include/sdmi.h "conditioned UNet"),
// and the conditioning of the SD v1 inpainting checkpoints (unet_in_ch = 9).  No reference counterpart: the reference's UNet takes the 4 latent channels only
// (unet/mod.rs:109-143).
//
// The sampler's update kernels (k_elem.hip, k_img2img.hip, k_sampler.hip) write the UNet input as ONE f32x4 per pixel, [2n][hw][4], and stay as they are.  A
// conditioned model's first convolution reads pc = unet_in_ch rounded up to a multiple of 4 channels per pixel, so one launch in front of every UNet forward
// assembles its input:
//
//   assemble   unet_in [rows][hw][4] + cond [n][hw][pc - 4]  ->  unet_in_c [rows][hw][pc]:  latent | conditioning | zeros in the pad channels.
//              Row r reads cond row r mod n: both halves of a CFG batch (uncond rows, then cond rows) see their sample's conditioning.  The pad
//              channels are WRITTEN, on every launch: their weights are zero, but 0 x NaN is NaN, and the buffer is pool scratch.
//
// One thread moves one 16-byte quad (4 channels of one pixel): consecutive threads read and write consecutive quads of the output row, so a wave stores 1 KiB
// contiguous and loads the same bytes from two streams.  0.4 MB per image and step at 64 x 64: the launch is latency, not bandwidth.  Grid-stride, no LDS.
//
// The inpainting conditioning (the rule of the CompVis inpainting script, with the posterior MEAN for its posterior sample, as everywhere in this project):
//   masked picture   u8 HWC image + u8 pixel mask -> the encoder's NHWC4 input: (v / 127.5 - 1) where mask < 128, exactly 0 where mask >= 128
//   cond row         the encoder's NHWC8 moments of the masked picture + the pixel mask -> cond [hw][8]:
//                    m | 0.18215 * moments[0..3] | 0 0 0,   m[y][x] = mask_u8[8y][8x] >= 128 ? 1 : 0   (sdmi_inpaint_latent_mask is THE statement of that rule)
//   paste            rgb_out = mask_u8 >= 128 ? generated : init_rgb, byte for byte
#include "kernels.hpp"

namespace sdmi {

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

inline int blocks_for(long long work, int cap = 2048) {
    long long b = (work + 255) / 256;
    if (b < 1) b = 1;
    if (b > cap) b = cap;
    return (int)b;
}

#define GRID_STRIDE(i, total) \
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < (total); i += (long long)gridDim.x * blockDim.x)

// quads = rows * hw * qp output quads, qp = pc / 4 quads per pixel; cond_pixels = n * hw; cond has qp - 1 quads per pixel of which cond_ch channels are data
__global__ __launch_bounds__(256) void assemble_unet_in_kernel(const f32x4* __restrict__ unet_in, const f32x4* __restrict__ cond, f32x4* __restrict__ out,
                                                               long long quads, long long cond_pixels, int qp, int cond_ch) {
    GRID_STRIDE(j, quads) {
        const long long pix = j / qp;
        const int q = (int)(j - pix * qp);
        f32x4 v;
        if (q == 0) {
            v = unet_in[pix];
        } else {
            v = cond[(pix % cond_pixels) * (qp - 1) + (q - 1)];
            const int c0 = 4 * (q - 1);   // first conditioning channel of this quad: the channels past cond_ch are the pad
            v.x = c0 + 0 < cond_ch ? v.x : 0.f;
            v.y = c0 + 1 < cond_ch ? v.y : 0.f;
            v.z = c0 + 2 < cond_ch ? v.z : 0.f;
            v.w = c0 + 3 < cond_ch ? v.w : 0.f;
        }
        out[j] = v;
    }
}

// cond [n][cond_ch][hw] (NCHW, the caller's) -> [n][hw][4 qc] (qc quads per pixel, the channels past cond_ch zero)
__global__ __launch_bounds__(256) void cond_nchw_to_nhwc_kernel(const float* __restrict__ src, f32x4* __restrict__ dst, long long quads, long long hw, int qc,
                                                                int cond_ch) {
    GRID_STRIDE(j, quads) {
        const long long pix = j / qc;
        const int q = (int)(j - pix * qc);
        const long long b = pix / hw, p = pix - b * hw;
        const float* s = src + (b * cond_ch + 4 * q) * hw + p;
        f32x4 v;
        v.x = 4 * q + 0 < cond_ch ? s[0] : 0.f;
        v.y = 4 * q + 1 < cond_ch ? s[hw] : 0.f;
        v.z = 4 * q + 2 < cond_ch ? s[2 * hw] : 0.f;
        v.w = 4 * q + 3 < cond_ch ? s[3 * hw] : 0.f;
        dst[j] = v;
    }
}

// rgb [pixels][3] u8 + mask [pixels] u8 -> dst [pixels] f32x4: rgb_u8_to_nhwc4_kernel's value where the pixel is kept (mask < 128), exactly 0 where it is regenerated
__global__ __launch_bounds__(256) void rgb_u8_masked_to_nhwc4_kernel(const uint8_t* __restrict__ rgb, const uint8_t* __restrict__ mask, f32x4* __restrict__ dst,
                                                                     long long pixels) {
    GRID_STRIDE(i, pixels) {
        const uint8_t* s = rgb + 3 * i;
        f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
        if (mask[i] < 128) {
            v.x = (float)s[0] / 127.5f - 1.0f;
            v.y = (float)s[1] / 127.5f - 1.0f;
            v.z = (float)s[2] / 127.5f - 1.0f;
        }
        dst[i] = v;
    }
}

// one image: q8 [h w][8] (the encoder's moments of the masked picture), mask [8h][8w] u8 -> cond [h w][8] = m | 0.18215 * q8[0..3] | 0 0 0, and (lat_mask != null)
// the latent mask m [h w] on its own, for the blend
__global__ __launch_bounds__(256) void inpaint_cond_pack_kernel(const f32x4* __restrict__ q8, const uint8_t* __restrict__ mask, f32x4* __restrict__ cond,
                                                                float* __restrict__ lat_mask, int h, int w) {
    const long long hw = (long long)h * w;
    GRID_STRIDE(i, hw) {
        const int y = (int)(i / w), x = (int)(i - (long long)y * w);
        const float m = mask[(long long)(8 * y) * (8 * w) + 8 * x] >= 128 ? 1.0f : 0.0f;
        const f32x4 z = q8[2 * i] * 0.18215f;
        cond[2 * i] = f32x4{m, z.x, z.y, z.z};
        cond[2 * i + 1] = f32x4{z.w, 0.f, 0.f, 0.f};
        if (lat_mask) lat_mask[i] = m;
    }
}

// once per call, 3 bytes per thread: out may be gen (every thread reads its pixel before it writes it)
__global__ __launch_bounds__(256) void inpaint_paste_kernel(const uint8_t* gen, const uint8_t* __restrict__ init, const uint8_t* __restrict__ mask, uint8_t* out,
                                                            long long pixels) {
    GRID_STRIDE(i, pixels) {
        const bool g = mask[i] >= 128;
        out[3 * i + 0] = g ? gen[3 * i + 0] : init[3 * i + 0];
        out[3 * i + 1] = g ? gen[3 * i + 1] : init[3 * i + 1];
        out[3 * i + 2] = g ? gen[3 * i + 2] : init[3 * i + 2];
    }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

hipError_t launch_assemble_unet_in(const float* unet_in, const float* cond, float* out, long long rows_pixels, long long cond_pixels, int pc, int cond_ch,
                                   hipStream_t s) {
    if (!unet_in || !cond || !out || rows_pixels <= 0 || cond_pixels <= 0 || pc < 8 || pc % 4 || cond_ch < 1 || cond_ch > pc - 4 || pc - 4 - cond_ch > 3)
        return hipErrorInvalidValue;
    if (!aligned16(unet_in) || !aligned16(cond) || !aligned16(out)) return hipErrorInvalidValue;
    const long long quads = rows_pixels * (pc / 4);
    hipLaunchKernelGGL(assemble_unet_in_kernel, dim3(blocks_for(quads)), dim3(256), 0, s, reinterpret_cast<const f32x4*>(unet_in),
                       reinterpret_cast<const f32x4*>(cond), reinterpret_cast<f32x4*>(out), quads, cond_pixels, pc / 4, cond_ch);
    return hipGetLastError();
}

hipError_t launch_cond_nchw_to_nhwc(const float* cond_nchw, float* cond_nhwc, int n, int cond_ch, long long hw, int pcc, hipStream_t s) {
    if (!cond_nchw || !cond_nhwc || n <= 0 || hw <= 0 || cond_ch < 1 || pcc % 4 || pcc < cond_ch || !aligned16(cond_nhwc)) return hipErrorInvalidValue;
    const long long quads = (long long)n * hw * (pcc / 4);
    hipLaunchKernelGGL(cond_nchw_to_nhwc_kernel, dim3(blocks_for(quads)), dim3(256), 0, s, cond_nchw, reinterpret_cast<f32x4*>(cond_nhwc), quads, hw, pcc / 4, cond_ch);
    return hipGetLastError();
}

hipError_t launch_rgb_u8_masked_to_nhwc4(const uint8_t* rgb, const uint8_t* mask, float* dst, long long pixels, hipStream_t s) {
    if (!rgb || !mask || !dst || pixels <= 0 || !aligned16(dst)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rgb_u8_masked_to_nhwc4_kernel, dim3(blocks_for(pixels)), dim3(256), 0, s, rgb, mask, reinterpret_cast<f32x4*>(dst), pixels);
    return hipGetLastError();
}

hipError_t launch_inpaint_cond_pack(const float* q8, const uint8_t* mask, float* cond, float* lat_mask, int h, int w, hipStream_t s) {
    if (!q8 || !mask || !cond || h <= 0 || w <= 0 || !aligned16(q8) || !aligned16(cond)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(inpaint_cond_pack_kernel, dim3(blocks_for((long long)h * w)), dim3(256), 0, s, reinterpret_cast<const f32x4*>(q8), mask,
                       reinterpret_cast<f32x4*>(cond), lat_mask, h, w);
    return hipGetLastError();
}

hipError_t launch_inpaint_paste(const uint8_t* gen, const uint8_t* init, const uint8_t* mask, uint8_t* out, long long pixels, hipStream_t s) {
    if (!gen || !init || !mask || !out || pixels <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(inpaint_paste_kernel, dim3(blocks_for(pixels)), dim3(256), 0, s, gen, init, mask, out, pixels);
    return hipGetLastError();
}

}  // namespace sdmi
