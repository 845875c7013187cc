// k_unpack.hip -- a checkpoint tensor's RAW bytes (F32 / F16 / BF16, torch layouts) -> the fp32 tensor in the reference's layout that the packing kernels
// read (sdmi_load_weights_safetensors).  No reference counterpart: the reference converts checkpoints in Python (python/dump.py).
//
// All three conversions are exact and done on the bit patterns, so no floating-point mode (denormal flushing, NaN quieting) can touch a value:
//   F32   the bits;
//   BF16  bits << 16;
//   F16   sign, exponent re-biased by 112, mantissa << 13; a subnormal is normalised with a count of leading zeros; inf / NaN keep their payload.
//
// Three forms, one launch per tensor, grid-stride, no atomics:
//   copy        16 bytes in, 16 (F32) or 32 (16-bit) bytes out per thread and step; the tail element by element.  Source and result are 16-byte aligned (the launcher refuses anything else:
//               ring offsets, arena slots and pool blocks all are).
//   transpose   [R][C] -> [C][R] (a Linear weight: torch's [out, in] -> the dump's [in, out]) through a 64 x 64 fp32 tile in LDS, 256 threads.  A wave reads
//               16-byte pieces along C (rows of the source) and writes 16-byte pieces along R (rows of the result): both sides of global memory see whole
//               contiguous 128- / 256-byte row segments.  The tile's pitch is 65 dwords: the row-wise ds_write_b32 of a 32-lane half land on banks
//               (r + c) mod 32 with r in 4 and c in 8-strided values -- 2-way, which a ds_write_b32 absorbs -- and the column-wise ds_read_b32 on banks
//               (4 k + i + c) mod 32, k = 0 .. 15 -- 2-way as well (64 rows on 32 banks).  Measured on [10240, 1280] F16: 22.0 us = 3.58 TB/s read + written, 1.5x the
//               time a device-to-device copy takes for the same output bytes, in a kernel class that is 5 % of a load.  16-byte accesses need every row of that side to start 16-byte aligned
//               (C % 8 == 0 for 16-bit, C % 4 == 0 for F32 sources; R % 4 == 0 for the result): then a piece is inside or outside the tensor as a whole
//               and edge tiles only mask pieces.  Otherwise (odd row lengths) that side goes element by element, still coalesced.
//   pad         a conv_in whose input channels are stored padded, [cout][cin][T] -> [cout][pc][T] with pc = cin rounded up to a multiple of 4 and the channels
//               cin .. pc - 1 zero (what upload_weight does on the host): the VAE encoder's RGB conv_in 3 -> 4, an inpainting UNet's conv_in 9 -> 12.
#include <algorithm>
#include <cstdint>

#include "k_widen.hpp"
#include "kernels.hpp"

namespace sdmi {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int kTile = 64, kPitch = kTile + 1;

// DT: 0 F32, 1 F16, 2 BF16; the 16-bit widenings are k_widen.hpp's
template <int DT>
__device__ __forceinline__ float load_one(const void* raw, long long i) {
    if (DT == 0) return reinterpret_cast<const float*>(raw)[i];
    return half_bits_to_f32<DT>(reinterpret_cast<const unsigned short*>(raw)[i]);
}

// the 4 (F32) or 8 (16-bit) values of one 16-byte piece
template <int DT>
__device__ __forceinline__ void widen_piece(const u32x4 v, float* f) {
    if (DT == 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) f[j] = __uint_as_float(v[j]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            f[2 * j] = half_bits_to_f32<DT>(v[j] & 0xffffu);
            f[2 * j + 1] = half_bits_to_f32<DT>(v[j] >> 16);
        }
    }
}

template <int DT>
__global__ __launch_bounds__(256) void unpack_copy_kernel(const void* __restrict__ raw, float* __restrict__ out, long long n) {
    constexpr int kPer = DT == 0 ? 4 : 8;
    const long long stride = (long long)gridDim.x * blockDim.x;
    const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long pieces = n / kPer;
    for (long long p = tid; p < pieces; p += stride) {
        float f[8];
        widen_piece<DT>(reinterpret_cast<const u32x4*>(raw)[p], f);
        f32x4* dst = reinterpret_cast<f32x4*>(out + p * kPer);
        dst[0] = f32x4{f[0], f[1], f[2], f[3]};
        if (DT != 0) dst[1] = f32x4{f[4], f[5], f[6], f[7]};
    }
    for (long long i = pieces * kPer + tid; i < n; i += stride) out[i] = load_one<DT>(raw, i);
}

template <int DT>
__global__ __launch_bounds__(256) void unpack_pad_kernel(const void* __restrict__ raw, float* __restrict__ out, long long cout, int cin, int pc, int T) {
    const long long n = cout * pc * T;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int t = (int)(i % T);
        const int c = (int)((i / T) % pc);
        const long long o = i / ((long long)pc * T);
        out[i] = c >= cin ? 0.f : load_one<DT>(raw, (o * cin + c) * T + t);
    }
}

template <int DT>
__global__ __launch_bounds__(256) void unpack_transpose_kernel(const void* __restrict__ raw, float* __restrict__ out, int R, int C, int vec_in, int vec_out) {
    __shared__ float tile[kTile][kPitch];
    constexpr int kPer = DT == 0 ? 4 : 8;          // elements of a 16-byte source piece
    constexpr int kPieces = kTile / kPer;          // pieces per tile row
    const int tid = threadIdx.x;
    const int tiles_c = (C + kTile - 1) / kTile;
    const long long tiles = (long long)((R + kTile - 1) / kTile) * tiles_c;
    for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {   // block-uniform: every thread reaches both barriers
        const int r0 = (int)(t / tiles_c) * kTile, c0 = (int)(t % tiles_c) * kTile;
        if (vec_in) {
            for (int e = tid; e < kTile * kPieces; e += 256) {
                const int r = e / kPieces, c = (e % kPieces) * kPer;
                if (r0 + r >= R || c0 + c >= C) continue;   // C % kPer == 0: the piece is inside as a whole
                float f[8];
                widen_piece<DT>(*reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(raw) + ((long long)(r0 + r) * C + c0 + c) * (DT == 0 ? 4 : 2)), f);
#pragma unroll
                for (int j = 0; j < kPer; ++j) tile[r][c + j] = f[j];
            }
        } else {
            for (int e = tid; e < kTile * kTile; e += 256) {
                const int r = e / kTile, c = e % kTile;
                if (r0 + r < R && c0 + c < C) tile[r][c] = load_one<DT>(raw, (long long)(r0 + r) * C + c0 + c);
            }
        }
        __syncthreads();
        if (vec_out) {
            for (int e = tid; e < kTile * (kTile / 4); e += 256) {
                const int c = e / (kTile / 4), r = (e % (kTile / 4)) * 4;
                if (c0 + c >= C || r0 + r >= R) continue;   // R % 4 == 0
                *reinterpret_cast<f32x4*>(out + (long long)(c0 + c) * R + r0 + r) = f32x4{tile[r][c], tile[r + 1][c], tile[r + 2][c], tile[r + 3][c]};
            }
        } else {
            for (int e = tid; e < kTile * kTile; e += 256) {
                const int c = e / kTile, r = e % kTile;
                if (c0 + c < C && r0 + r < R) out[(long long)(c0 + c) * R + r0 + r] = tile[r][c];
            }
        }
        __syncthreads();   // the tile is free for the next round
    }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

hipError_t launch_unpack_tensor(const void* raw, int dtype, int transform, long long d0, long long d1, float* out, hipStream_t s, int cin) {
    if (!raw || !out || dtype < 0 || dtype > 2 || transform < 0 || transform > 2 || d0 <= 0 || d1 <= 0) return hipErrorInvalidValue;
    if (d0 > (1ll << 40) / d1) return hipErrorInvalidValue;
    if (!aligned16(raw) || !aligned16(out)) return hipErrorInvalidValue;   // every caller hands over ring / arena / pool addresses
    const int per = dtype == 0 ? 4 : 8;
    if (transform == 0) {
        const long long n = d0 * d1;
        const unsigned blocks = (unsigned)std::min<long long>((n + 256ll * per - 1) / (256ll * per), 4096);
        if (dtype == 0) hipLaunchKernelGGL(unpack_copy_kernel<0>, dim3(blocks), dim3(256), 0, s, raw, out, n);
        else if (dtype == 1) hipLaunchKernelGGL(unpack_copy_kernel<1>, dim3(blocks), dim3(256), 0, s, raw, out, n);
        else hipLaunchKernelGGL(unpack_copy_kernel<2>, dim3(blocks), dim3(256), 0, s, raw, out, n);
    } else if (transform == 1) {
        if (d0 > INT32_MAX / 2 || d1 > INT32_MAX / 2) return hipErrorInvalidValue;
        const int R = (int)d0, C = (int)d1;
        const int vec_in = C % per == 0, vec_out = R % 4 == 0;
        const long long tiles = (long long)((R + kTile - 1) / kTile) * ((C + kTile - 1) / kTile);
        const unsigned blocks = (unsigned)std::min<long long>(tiles, 8192);
        if (dtype == 0) hipLaunchKernelGGL(unpack_transpose_kernel<0>, dim3(blocks), dim3(256), 0, s, raw, out, R, C, vec_in, vec_out);
        else if (dtype == 1) hipLaunchKernelGGL(unpack_transpose_kernel<1>, dim3(blocks), dim3(256), 0, s, raw, out, R, C, vec_in, vec_out);
        else hipLaunchKernelGGL(unpack_transpose_kernel<2>, dim3(blocks), dim3(256), 0, s, raw, out, R, C, vec_in, vec_out);
    } else {
        if (d1 > 4096 || cin < 1 || cin >= 32) return hipErrorInvalidValue;
        const int pc = (cin + 3) / 4 * 4;
        const long long n = d0 * pc * d1;
        const unsigned blocks = (unsigned)std::min<long long>((n + 255) / 256, 4096);
        if (dtype == 0) hipLaunchKernelGGL(unpack_pad_kernel<0>, dim3(blocks), dim3(256), 0, s, raw, out, d0, cin, pc, (int)d1);
        else if (dtype == 1) hipLaunchKernelGGL(unpack_pad_kernel<1>, dim3(blocks), dim3(256), 0, s, raw, out, d0, cin, pc, (int)d1);
        else hipLaunchKernelGGL(unpack_pad_kernel<2>, dim3(blocks), dim3(256), 0, s, raw, out, d0, cin, pc, (int)d1);
    }
    return hipGetLastError();
}

}  // namespace sdmi
