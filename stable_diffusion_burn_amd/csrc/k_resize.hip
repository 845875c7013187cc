// k_resize.hip -- the latent resampler of the hires fix (no reference counterpart: the reference's latent is
// hard-coded 4x64x64, stablediffusion/mod.rs:116).
//
// Separable: one launch per axis, the horizontal pass first, the vertical one through a pool buffer.  The latent is the engine's own
// NHWC4 layout [n][h*w][4]: one 16-byte f32x4 per pixel per thread, consecutive threads on consecutive pixels of an output row, so the
// stores are coalesced and so are the loads of the vertical pass (the horizontal pass reads a window of the same row).  Grid-stride loop.
//
// The tap table of the axis (sdmi_resize_weights, taps rounded to f32) sits in a small device buffer of the call: at most
// out_size * (max_taps + 2) words -- 3 KB for 64 -> 128 bicubic -- that every wave of the launch reads, so it stays in the vector L1 / L2 after
// the first touch.  It is not staged into LDS: that would cost every workgroup a copy of the whole table and a barrier in a kernel that
// moves 16 bytes per thread; and it is not uniform across a wave (the output index differs per lane in the horizontal pass), so the
// scalar cache does not apply either.
//
// Taps are summed in ascending order into one accumulator per channel, no atomics: bit-identical run to run.  Nearest (GATHER) copies.
#include "kernels.hpp"

namespace sdmi {

typedef float f32x4 __attribute__((ext_vector_type(4)));

template <bool GATHER>
__global__ void resize_axis_kernel(const f32x4* __restrict__ x, f32x4* __restrict__ y, const int* __restrict__ first, const int* __restrict__ count,
                                   const float* __restrict__ taps, int max_taps, int in_size, int out_size, long long inner, long long total) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long r = i / inner, in = i - r * inner;
        const long long a = r / out_size;
        const int o = (int)(r - a * out_size);
        const f32x4* src = x + (a * in_size + first[o]) * inner + in;
        if (GATHER) {
            y[i] = src[0];
        } else {
            const float* t = taps + (long long)o * max_taps;
            const int cnt = count[o];
            f32x4 acc = src[0] * t[0];
            for (int j = 1; j < cnt; ++j) {
                const f32x4 v = src[(long long)j * inner];
                const float w = t[j];
                acc.x += w * v.x;
                acc.y += w * v.y;
                acc.z += w * v.z;
                acc.w += w * v.w;
            }
            y[i] = acc;
        }
    }
}

hipError_t launch_resize_axis(const float* x, float* y, const int* first, const int* count, const float* taps, int max_taps, long long outer,
                              int in_size, int out_size, long long inner, bool gather, hipStream_t s) {
    if (!x || !y || !first || outer <= 0 || in_size <= 0 || out_size <= 0 || inner <= 0) return hipErrorInvalidValue;
    if (!gather && (!count || !taps || max_taps <= 0)) return hipErrorInvalidValue;
    const long long total = outer * out_size * inner;
    long long blocks = (total + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    const f32x4* xs = reinterpret_cast<const f32x4*>(x);
    f32x4* ys = reinterpret_cast<f32x4*>(y);
    if (gather)
        hipLaunchKernelGGL(resize_axis_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, s, xs, ys, first, count, taps, max_taps, in_size, out_size, inner, total);
    else
        hipLaunchKernelGGL(resize_axis_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, s, xs, ys, first, count, taps, max_taps, in_size, out_size, inner, total);
    return hipGetLastError();
}

}  // namespace sdmi
