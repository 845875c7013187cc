// k_ipattn.hip -- the second attention of IP-Adapter's decoupled cross attention (include/sdmi.h "IP-Adapter").  No reference counterpart.
//
//     O[b, r, head] = O_text[b, r, head] + s_b * softmax_t(q[b, r, head] . K_ip[b, t, head] * scale^2) V_ip[b, t, head],     t < T <= 64 image tokens
//
// The text attention has already written O_text; this launch adds the image term to it.  With at most 64 keys there is no key loop worth a matrix pipe: the two
// products are [64 rows x d] x [d x T] with T as small as 1 (4 for one picture) -- a 16- or 32-wide MFMA tile would be three quarters padding at T = 4, and fp32
// accuracy on the bf16 pipe needs the three-way split on top.  The kernel moves 12 bytes per output element (q, O_text, O) for 4 T flops: VALU fp32 FMAs keep up with
// that traffic, so both products run on the VALU, fp32 throughout, the softmax maximum and sum in registers.
//
// One workgroup (128 threads) = 64 query rows of one (batch row, head):
//   1. K_ip / V_ip of the head ([T][d] fp32 each, rows past T zero up to a multiple of 4) and the q tile go to LDS.  Global traffic is in 16-byte pieces, consecutive
//      lanes on consecutive pieces of a row's d-wide head segment, then the next row: a wave instruction covers whole segments, never one lane per strided row.
//      A bf16 q is widened here; it arrives in log2 units (Engine::q_prescaled), an fp32 q is scaled by scale^2 log2(e) at the scores.
//   2. Two lanes per row, lane `half` owning the 4-channel chunks half, half + 2, ...: the partial dot products of four keys, one xor-shuffle each, an online
//      softmax step in exp2, four V rows accumulated.  K / V reads are LDS broadcasts (two addresses per wave).  The result, times s_b / sum, overwrites the
//      lane's own chunks of the q tile.
//   3. The tile is added to O_text with the coalesced mapping of step 1 and stored in the form the consumer reads:
//        form 0  fp32 dense;   form 1  bf16 dense (fp32 sum, one round to nearest even);
//        form 2  the fp32 engine's three bf16 planes [C / 32][3][32] per row, READ-MODIFY-WRITE: h + m + l is the fp32 value the text attention produced, exactly
//                ((h + m) has at most 17 significant bits), the new value is split by s3_store4 as every producer of planes does.  8-byte pieces: a head of
//                width 40 / 80 / 160 does not own whole 16-byte plane pieces (k_split3.hpp: a piece pairs channels 4g.. with 16 + 4g..).
// A batch row with s_b == 0 is left alone (o == o_text) or copied bit for bit.  No atomics; every output element is owned by one thread and every sum has a fixed
// order: two runs give the same bits and a sample's result does not depend on the batch it is in.
#include "kernels.hpp"
#include "k_split3.hpp"

namespace sdmi {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

namespace {

constexpr int kRows = 64, kThreads = 128;

__device__ __forceinline__ float bf_lo(unsigned w) { return __builtin_bit_cast(float, w << 16); }
__device__ __forceinline__ float bf_hi(unsigned w) { return __builtin_bit_cast(float, w & 0xffff0000u); }
__device__ __forceinline__ f32x4 widen4(u32x2 w) { return f32x4{bf_lo(w[0]), bf_hi(w[0]), bf_lo(w[1]), bf_hi(w[1])}; }

template <int D, int FORM>
__global__ __launch_bounds__(kThreads) void ip_attention_kernel(const IpAttnParams p) {
    extern __shared__ __attribute__((aligned(16))) float smem_ip[];
    constexpr int LD = D + 4;        // tile row stride in floats: 16-byte aligned, off the 32-bank period
    constexpr int Q4 = D / 4;        // 16-byte pieces of an fp32 head segment
    constexpr int NCH = D / 8;       // chunks per lane
    const int b = blockIdx.z, head = blockIdx.y, r0 = blockIdx.x * kRows, tid = threadIdx.x;
    const float sb = p.s[b];
    const bool skip = sb == 0.f;
    if (skip && p.o == p.o_text) return;
    const int C = p.n_head * D, T = p.T, T4 = (T + 3) & ~3;
    const int rows = min(kRows, p.nq - r0);
    float* const Ks = smem_ip;
    float* const Vs = Ks + T4 * D;
    float* const tile = Vs + T4 * D;

    if (!skip) {
        // ---- 1. stage K_ip / V_ip of this head and the q tile ----
        const float* kb = p.k + (long long)b * T * C + head * D;
        const float* vb = p.v + (long long)b * T * C + head * D;
        for (int u = tid; u < T4 * Q4; u += kThreads) {
            const int t = u / Q4, j = u - t * Q4;
            f32x4 kv = f32x4{0.f, 0.f, 0.f, 0.f}, vv = kv;
            if (t < T) {
                kv = *reinterpret_cast<const f32x4*>(kb + (long long)t * C + 4 * j);
                vv = *reinterpret_cast<const f32x4*>(vb + (long long)t * C + 4 * j);
            }
            *reinterpret_cast<f32x4*>(Ks + t * D + 4 * j) = kv;
            *reinterpret_cast<f32x4*>(Vs + t * D + 4 * j) = vv;
        }
        if (p.bf16) {
            constexpr int Q8 = D / 8;
            const unsigned short* qb = static_cast<const unsigned short*>(p.q) + (long long)b * p.q_bs + (long long)r0 * p.ldq + head * D;
            for (int u = tid; u < kRows * Q8; u += kThreads) {
                const int r = u / Q8, j = u - r * Q8;
                u32x4 w = u32x4{0u, 0u, 0u, 0u};
                if (r < rows) w = *reinterpret_cast<const u32x4*>(qb + (long long)r * p.ldq + 8 * j);
                *reinterpret_cast<f32x4*>(tile + r * LD + 8 * j) = widen4(u32x2{w[0], w[1]});
                *reinterpret_cast<f32x4*>(tile + r * LD + 8 * j + 4) = widen4(u32x2{w[2], w[3]});
            }
        } else {
            const float* qb = static_cast<const float*>(p.q) + (long long)b * p.q_bs + (long long)r0 * p.ldq + head * D;
            for (int u = tid; u < kRows * Q4; u += kThreads) {
                const int r = u / Q4, j = u - r * Q4;
                f32x4 w = f32x4{0.f, 0.f, 0.f, 0.f};
                if (r < rows) w = *reinterpret_cast<const f32x4*>(qb + (long long)r * p.ldq + 4 * j);
                *reinterpret_cast<f32x4*>(tile + r * LD + 4 * j) = w;
            }
        }
        __syncthreads();

        // ---- 2. two lanes per row: scores, online softmax, P V ----
        const int row = tid >> 1, half = tid & 1;
        float* const trow = tile + row * LD + 4 * half;
        f32x4 q[NCH], acc[NCH];
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            q[j] = *reinterpret_cast<const f32x4*>(trow + 8 * j);
            acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        float m = -__builtin_inff(), l = 0.f;
        const float* kl = Ks + 4 * half;
        const float* vl = Vs + 4 * half;
        for (int t0 = 0; t0 < T4; t0 += 4) {
            float sc[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                f32x4 d4 = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int j = 0; j < NCH; ++j) d4 += q[j] * *reinterpret_cast<const f32x4*>(kl + (t0 + i) * D + 8 * j);
                float d = (d4[0] + d4[1]) + (d4[2] + d4[3]);
                d += __shfl_xor(d, 1);
                sc[i] = (t0 + i < T) ? d * p.sl2 : -__builtin_inff();
            }
            const float mn = fmaxf(fmaxf(m, fmaxf(sc[0], sc[1])), fmaxf(sc[2], sc[3]));   // finite: key t0 exists
            const float alpha = __builtin_amdgcn_exp2f(m - mn);
            float pr[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) pr[i] = __builtin_amdgcn_exp2f(sc[i] - mn);
            l = l * alpha + ((pr[0] + pr[1]) + (pr[2] + pr[3]));
#pragma unroll
            for (int j = 0; j < NCH; ++j) {
                f32x4 a = acc[j] * alpha;
#pragma unroll
                for (int i = 0; i < 4; ++i) a += pr[i] * *reinterpret_cast<const f32x4*>(vl + (t0 + i) * D + 8 * j);
                acc[j] = a;
            }
            m = mn;
        }
        const float f = sb / l;
#pragma unroll
        for (int j = 0; j < NCH; ++j) *reinterpret_cast<f32x4*>(trow + 8 * j) = acc[j] * f;
        __syncthreads();
    }

    // ---- 3. O = O_text + tile, in the consumer's form (skip: the bits of O_text) ----
    if constexpr (FORM == 0) {
        const long long base = ((long long)b * p.nq + r0) * C + head * D;
        const float* ot = static_cast<const float*>(p.o_text) + base;
        float* o = static_cast<float*>(p.o) + base;
        for (int u = tid; u < rows * Q4; u += kThreads) {
            const int r = u / Q4, j = u - r * Q4;
            u32x4 raw = *reinterpret_cast<const u32x4*>(ot + (long long)r * C + 4 * j);
            if (!skip) {
                const f32x4 y = __builtin_bit_cast(f32x4, raw) + *reinterpret_cast<const f32x4*>(tile + r * LD + 4 * j);
                raw = __builtin_bit_cast(u32x4, y);
            }
            *reinterpret_cast<u32x4*>(o + (long long)r * C + 4 * j) = raw;
        }
    } else if constexpr (FORM == 1) {
        constexpr int Q8 = D / 8;
        const long long base = ((long long)b * p.nq + r0) * C + head * D;
        const unsigned short* ot = static_cast<const unsigned short*>(p.o_text) + base;
        unsigned short* o = static_cast<unsigned short*>(p.o) + base;
        for (int u = tid; u < rows * Q8; u += kThreads) {
            const int r = u / Q8, j = u - r * Q8;
            u32x4 raw = *reinterpret_cast<const u32x4*>(ot + (long long)r * C + 8 * j);
            if (!skip) {
                const f32x4 y0 = widen4(u32x2{raw[0], raw[1]}) + *reinterpret_cast<const f32x4*>(tile + r * LD + 8 * j);
                const f32x4 y1 = widen4(u32x2{raw[2], raw[3]}) + *reinterpret_cast<const f32x4*>(tile + r * LD + 8 * j + 4);
                raw = u32x4{s3_cvt_pk(y0[0], y0[1]), s3_cvt_pk(y0[2], y0[3]), s3_cvt_pk(y1[0], y1[1]), s3_cvt_pk(y1[2], y1[3])};
            }
            *reinterpret_cast<u32x4*>(o + (long long)r * C + 8 * j) = raw;
        }
    } else {
        const long long rbase = ((long long)b * p.nq + r0) * p.ldo3;
        const unsigned char* ot = static_cast<const unsigned char*>(p.o_text) + rbase;
        unsigned char* o = static_cast<unsigned char*>(p.o) + rbase;
        for (int u = tid; u < rows * Q4; u += kThreads) {
            const int r = u / Q4, j = u - r * Q4;
            const int c = head * D + 4 * j;
            const long long off = (long long)r * p.ldo3 + s3_plane_byte(c, 0);
            const u32x2 h = *reinterpret_cast<const u32x2*>(ot + off);
            const u32x2 mm = *reinterpret_cast<const u32x2*>(ot + off + 64);
            const u32x2 lo = *reinterpret_cast<const u32x2*>(ot + off + 128);
            if (skip) {
                *reinterpret_cast<u32x2*>(o + off) = h;
                *reinterpret_cast<u32x2*>(o + off + 64) = mm;
                *reinterpret_cast<u32x2*>(o + off + 128) = lo;
            } else {
                const f32x4 y = ((widen4(h) + widen4(mm)) + widen4(lo)) + *reinterpret_cast<const f32x4*>(tile + r * LD + 4 * j);
                s3_store4(o + (long long)r * p.ldo3, c, y);
            }
        }
    }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <int D, int FORM>
hipError_t launch_one(const IpAttnParams& p, hipStream_t s) {
    const int T4 = (p.T + 3) & ~3;
    const int lds = (2 * T4 * D + kRows * (D + 4)) * (int)sizeof(float);
    auto* kernel = ip_attention_kernel<D, FORM>;
    if (lds > 64 * 1024) {
        const hipError_t e = set_max_dynamic_lds(reinterpret_cast<const void*>(kernel), (2 * 64 * D + kRows * (D + 4)) * (int)sizeof(float));
        if (e != hipSuccess) return e;
    }
    const dim3 grid((unsigned)((p.nq + kRows - 1) / kRows), (unsigned)p.n_head, (unsigned)p.n);
    hipLaunchKernelGGL(kernel, grid, dim3(kThreads), (size_t)lds, s, p);
    return hipGetLastError();
}

template <int D>
hipError_t launch_form(const IpAttnParams& p, hipStream_t s) {
    switch (p.form) {
        case 0: return launch_one<D, 0>(p, s);
        case 1: return launch_one<D, 1>(p, s);
        default: return launch_one<D, 2>(p, s);
    }
}

}  // namespace

bool ip_attention_head_dim(int d) { return d == 40 || d == 64 || d == 80 || d == 160; }

hipError_t launch_ip_attention(const IpAttnParams& p_in, hipStream_t s) {
    IpAttnParams p = p_in;
    if (!p.q || !p.k || !p.v || !p.o_text || !p.o || !p.s) return hipErrorInvalidValue;
    if (p.n < 1 || p.n > 65535 || p.nq < 1 || p.n_head < 1 || p.n_head > 65535 || p.T < 1 || p.T > kIpMaxTokens || !ip_attention_head_dim(p.d_head)) return hipErrorInvalidValue;
    if (p.form < 0 || p.form > 2 || (p.form == 1) != (p.bf16 != 0)) return hipErrorInvalidValue;   // a bf16 q belongs to a bf16 output, an fp32 q to fp32 or planes
    const long long C = (long long)p.n_head * p.d_head;
    const int qa = p.bf16 ? 7 : 3;
    if (p.ldq < C || (p.ldq & qa) || (p.q_bs & qa) || p.q_bs < 0) return hipErrorInvalidValue;
    if (!aligned16(p.q) || !aligned16(p.k) || !aligned16(p.v) || !aligned16(p.o_text) || !aligned16(p.o)) return hipErrorInvalidValue;
    if (p.form == 2 && (C % 32 || p.ldo3 % 16 || p.ldo3 < C / 32 * 192)) return hipErrorInvalidValue;
    if (p.form == 1 && C % 8) return hipErrorInvalidValue;
    // scores in log2 units: a q that carries d^-1/2 log2(e) already (q_log2) needs nothing, otherwise scale^2 = d^-1/2 and the change of base
    p.sl2 = p.q_log2 ? 1.f : p.scale * p.scale * 1.4426950408889634f;
    switch (p.d_head) {
        case 40: return launch_form<40>(p, s);
        case 64: return launch_form<64>(p, s);
        case 80: return launch_form<80>(p, s);
        default: return launch_form<160>(p, s);
    }
}

}  // namespace sdmi
