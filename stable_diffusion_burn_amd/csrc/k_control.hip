// k_control.hip -- the two kernels ControlNet adds (include/sdmi.h "ControlNet").  No reference counterpart: the reference's UNet has
// no control input (unet/mod.rs:109-143).  Everything else a ControlNet runs -- the hint convolutions, the control encoder, the zero convolutions -- is the
// engine's own GEMM / norm / attention launches on a fourth weight group.
//
//   hint       u8 HWC picture -> the first hint convolution's NHWC4 input, v / 255 with a zero 4th channel (once per call).
//   add        y += strength * r for the 13 residuals of a step, ONE launch: the twelve skips (channel slices of the cats buffers, a row stride wider than the
//              channel count) and the middle block's output (the x slice of cats[0]).  At batch 1 the 13 tensors are 6.6 MB fp32 (SD v1.4, 64 x 64): a launch
//              boundary costs more than any one of them, hence a by-value table of segments, gridDim.y = segment, gridDim.x grid-strides over the segment.
//
// The add works in units of 16 bytes per access and touches every byte once.  fp32: a unit is chunk g (0..3) of a 32-channel slice -- channels 4g..4g+3 and
// 16+4g..16+4g+3, the pair that shares one 16-byte piece of each bf16 plane (k_split3.hpp: s3_plane_pos) -- so two f32x4 loads of y, two of r, two stores, and
// where the destination also exists as planes three 16-byte plane stores of the split of the NEW value: the planes never go through a read-modify-write, they are
// what s3_split8 makes of the fp32 result, as in the GEMM epilogues that produced the old ones.  Four consecutive lanes cover 64 contiguous bytes twice over (the
// low and the high half of the slice), a wave covers 16 slices: rows wider than the slice (the stride of a cats buffer) only move the start of the next row.
// bf16: a unit is 8 consecutive channels, one 16-byte load of y and r each, fp32 arithmetic, round to nearest even (v_cvt_pk_bf16_f32), one store.
// No LDS, no atomics; every unit is owned by one thread.
#include "kernels.hpp"
#include "k_split3.hpp"

namespace sdmi {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

namespace {

#define GRID_STRIDE(i, total) \
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < (total); i += (long long)gridDim.x * blockDim.x)

__global__ __launch_bounds__(256) void hint_u8_to_nhwc4_kernel(const uint8_t* __restrict__ rgb, f32x4* __restrict__ dst, long long pixels) {
    GRID_STRIDE(i, pixels) {
        const uint8_t* s = rgb + 3 * i;
        dst[i] = f32x4{(float)s[0] / 255.0f, (float)s[1] / 255.0f, (float)s[2] / 255.0f, 0.f};
    }
}

template <int DT>
__global__ __launch_bounds__(256) void control_add_kernel(const ControlAdd a) {
    const ControlSeg sg = a.seg[blockIdx.y];
    const float st = a.strength;
    if constexpr (DT == 0) {
        const int upr = sg.c >> 3;   // units per row: 4 per 32-channel slice
        const long long units = sg.rows * upr;
        float* const y = static_cast<float*>(sg.y);
        const float* const r = static_cast<const float*>(sg.r);
        unsigned char* const y3 = static_cast<unsigned char*>(sg.y3);
        GRID_STRIDE(u, units) {
            const long long row = u / upr;
            const int k = (int)(u - row * upr);
            const int ch = (k >> 2) * 32 + (k & 3) * 4;
            float* yp = y + row * sg.ld + ch;
            const float* rp = r + row * sg.c + ch;
            f32x4 lo = *reinterpret_cast<const f32x4*>(yp), hi = *reinterpret_cast<const f32x4*>(yp + 16);
            lo += st * *reinterpret_cast<const f32x4*>(rp);
            hi += st * *reinterpret_cast<const f32x4*>(rp + 16);
            *reinterpret_cast<f32x4*>(yp) = lo;
            *reinterpret_cast<f32x4*>(yp + 16) = hi;
            if (y3) {
                s3_u32x4 h, m, l;
                s3_split8(lo, hi, h, m, l);
                unsigned char* d = y3 + row * sg.ld3 + s3_plane_byte(ch, 0);
                *reinterpret_cast<s3_u32x4*>(d) = h;
                *reinterpret_cast<s3_u32x4*>(d + 64) = m;
                *reinterpret_cast<s3_u32x4*>(d + 128) = l;
            }
        }
    } else {
        const int upr = sg.c >> 3;   // units per row: 8 bf16 channels
        const long long units = sg.rows * upr;
        unsigned short* const y = static_cast<unsigned short*>(sg.y);
        const unsigned short* const r = static_cast<const unsigned short*>(sg.r);
        GRID_STRIDE(u, units) {
            const long long row = u / upr;
            const int k = (int)(u - row * upr);
            u32x4* yp = reinterpret_cast<u32x4*>(y + row * sg.ld + 8 * k);
            const u32x4 yv = *yp, rv = *reinterpret_cast<const u32x4*>(r + row * sg.c + 8 * k);
            u32x4 o;
#pragma unroll
            for (int i = 0; i < 4; ++i) {   // a packed pair: the low half is the even channel
                const float y0 = __builtin_bit_cast(float, yv[i] << 16), y1 = __builtin_bit_cast(float, yv[i] & 0xffff0000u);
                const float r0 = __builtin_bit_cast(float, rv[i] << 16), r1 = __builtin_bit_cast(float, rv[i] & 0xffff0000u);
                o[i] = s3_cvt_pk(y0 + st * r0, y1 + st * r1);
            }
            *yp = o;
        }
    }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

hipError_t launch_hint_u8_to_nhwc4(const uint8_t* rgb, float* dst, long long pixels, hipStream_t s) {
    if (!rgb || !dst || pixels <= 0 || !aligned16(dst)) return hipErrorInvalidValue;
    long long blocks = (pixels + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(hint_u8_to_nhwc4_kernel, dim3((unsigned)blocks), dim3(256), 0, s, rgb, reinterpret_cast<f32x4*>(dst), pixels);
    return hipGetLastError();
}

hipError_t launch_control_add(const ControlAdd& a, hipStream_t s) {
    if (a.n_seg < 1 || a.n_seg > kControlMaxSegs || (a.dt != 0 && a.dt != 1)) return hipErrorInvalidValue;
    const int es = a.dt ? 2 : 4;
    long long most = 0;
    for (int i = 0; i < a.n_seg; ++i) {
        const ControlSeg& g = a.seg[i];
        if (!g.y || !g.r || g.rows <= 0 || g.c <= 0 || g.ld < g.c) return hipErrorInvalidValue;
        if (a.dt ? (g.c % 8 || g.y3) : (g.c % 32)) return hipErrorInvalidValue;
        if (!aligned16(g.y) || !aligned16(g.r) || ((long long)g.ld * es) % 16) return hipErrorInvalidValue;
        if (g.y3 && (!aligned16(g.y3) || g.ld3 % 16 || g.ld3 < g.c / 32 * 192)) return hipErrorInvalidValue;
        most = most > g.rows * (g.c / 8) ? most : g.rows * (g.c / 8);
    }
    long long blocks = (most + 255) / 256;
    if (blocks > 512) blocks = 512;
    const dim3 grid((unsigned)blocks, (unsigned)a.n_seg);
    if (a.dt) hipLaunchKernelGGL(control_add_kernel<1>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(control_add_kernel<0>, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace sdmi
