// k_lora.hip -- the LoRA merge (sdmi_lora_set_scale): W = W0 + sum_t coef_t (P_t Q_t) on one fp32 weight tensor seen as a
// row-major matrix [R][Cc] in the reference's layout.  No reference counterpart: the reference runs the base checkpoint only.
//
// The kernel is bound by the master's bytes (one 16-byte read and one 16-byte write per four elements); the rank-r products are vector FMAs on
// factors staged through LDS, JC = 16 rank columns at a time.  A 256-thread workgroup owns a 32 x 128 tile: thread (tx, ty) holds columns
// 4 tx .. 4 tx + 3 of rows ty, ty + 8, ty + 16, ty + 24, so a wave reads two 512-byte row segments per row step and the LDS reads are one
// conflict-free 16-byte read of Q per rank column plus broadcast reads of P.  LDS: (16 x 33 + 16 x 132) x 4 = 10.3 KB, 32 + 32 live
// accumulator registers -- occupancy is not what limits a kernel that streams each byte once.  The factors are addressed with element
// strides, so a Linear target (master [in][out], delta[i][o] = sum_j up[o][j] down[j][i]) reads up and down as stored; which index runs
// fastest while staging follows the unit stride.  No atomics, a fixed summation order: bit-identical run to run.
//
// Order of operations (the rounding bound of tests/test_lora_gpu.py rests on it): per term d = fma(P(r, j), Q(j, c), d) for j = 0 .. rank - 1
// from d = 0, then w = fma(coef, d, w), terms in the order given, w starting at W0.  Rank columns past `rank` are staged as zeros (d + 0 * 0).
#include "kernels.hpp"

namespace sdmi {

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {
constexpr int kTR = 32, kTC = 128, kJC = 16;
}

__global__ __launch_bounds__(256) void lora_merge_kernel(LoraMerge m) {
    __shared__ float Ps[kJC][kTR + 1];
    __shared__ __attribute__((aligned(16))) float Qs[kJC][kTC + 4];
    const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;
    const int r0 = blockIdx.y * kTR, c0 = blockIdx.x * kTC;
    const int c = c0 + tx * 4;
    const bool vec = (m.Cc & 3) == 0;   // then a thread's four columns are inside or outside together and every row starts 16-byte aligned

    f32x4 w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = r0 + ty + 8 * i;
        w[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (r >= m.R) continue;
        const float* src = m.W0 + (long long)r * m.Cc + c;
        if (vec) {
            if (c < m.Cc) w[i] = *reinterpret_cast<const f32x4*>(src);
        } else {
            if (c + 0 < m.Cc) w[i].x = src[0];
            if (c + 1 < m.Cc) w[i].y = src[1];
            if (c + 2 < m.Cc) w[i].z = src[2];
            if (c + 3 < m.Cc) w[i].w = src[3];
        }
    }

    for (int t = 0; t < m.n_terms; ++t) {
        const LoraTerm& lt = m.t[t];
        f32x4 d[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) d[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int j0 = 0; j0 < lt.rank; j0 += kJC) {
            __syncthreads();   // the previous chunk has been consumed
            for (int e = tid; e < kJC * kTR; e += 256) {
                int j, r;
                if (lt.p_js == 1) { j = e % kJC; r = e / kJC; } else { r = e % kTR; j = e / kTR; }
                float v = 0.f;
                if (r0 + r < m.R && j0 + j < lt.rank) v = lt.P[(long long)(r0 + r) * lt.p_rs + (long long)(j0 + j) * lt.p_js];
                Ps[j][r] = v;
            }
            for (int e = tid; e < kJC * kTC; e += 256) {
                int j, cc;
                if (lt.q_cs == 1) { cc = e % kTC; j = e / kTC; } else { j = e % kJC; cc = e / kJC; }
                float v = 0.f;
                if (c0 + cc < m.Cc && j0 + j < lt.rank) v = lt.Q[(long long)(j0 + j) * lt.q_js + (long long)(c0 + cc) * lt.q_cs];
                Qs[j][cc] = v;
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < kJC; ++j) {
                const f32x4 q = *reinterpret_cast<const f32x4*>(&Qs[j][tx * 4]);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float p = Ps[j][ty + 8 * i];
                    d[i].x = __fmaf_rn(p, q.x, d[i].x);
                    d[i].y = __fmaf_rn(p, q.y, d[i].y);
                    d[i].z = __fmaf_rn(p, q.z, d[i].z);
                    d[i].w = __fmaf_rn(p, q.w, d[i].w);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            w[i].x = __fmaf_rn(lt.coef, d[i].x, w[i].x);
            w[i].y = __fmaf_rn(lt.coef, d[i].y, w[i].y);
            w[i].z = __fmaf_rn(lt.coef, d[i].z, w[i].z);
            w[i].w = __fmaf_rn(lt.coef, d[i].w, w[i].w);
        }
    }

#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = r0 + ty + 8 * i;
        if (r >= m.R) continue;
        float* dst = m.W + (long long)r * m.Cc + c;
        if (vec) {
            if (c < m.Cc) *reinterpret_cast<f32x4*>(dst) = w[i];
        } else {
            if (c + 0 < m.Cc) dst[0] = w[i].x;
            if (c + 1 < m.Cc) dst[1] = w[i].y;
            if (c + 2 < m.Cc) dst[2] = w[i].z;
            if (c + 3 < m.Cc) dst[3] = w[i].w;
        }
    }
}

hipError_t launch_lora_merge(const LoraMerge& m, hipStream_t s) {
    if (!m.W0 || !m.W || m.R <= 0 || m.Cc <= 0 || m.n_terms < 0 || m.n_terms > kLoraMaxTerms) return hipErrorInvalidValue;
    if ((m.Cc & 3) == 0 && ((reinterpret_cast<uintptr_t>(m.W0) | reinterpret_cast<uintptr_t>(m.W)) & 15)) return hipErrorInvalidValue;
    for (int t = 0; t < m.n_terms; ++t)
        if (!m.t[t].P || !m.t[t].Q || m.t[t].rank < 1) return hipErrorInvalidValue;
    const long long gy = ((long long)m.R + kTR - 1) / kTR;
    if (gy > 65535) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((m.Cc + kTC - 1) / kTC), (unsigned)gy);
    hipLaunchKernelGGL(lora_merge_kernel, grid, dim3(256), 0, s, m);
    return hipGetLastError();
}

}  // namespace sdmi
