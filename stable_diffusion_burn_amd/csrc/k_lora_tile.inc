// k_lora_tile.inc -- the body of the LoRA merge kernels (k_lora.hip), included once per __global__ function with DT (the factors' storage type: 0 F32, 1 F16,
// 2 BF16) and HADA (LoHa terms: two products per term, NF = 2 staged factor pairs) in scope as compile-time constants and `m` the kernel's LoraMerge argument.
// A textual body, not a __device__ function: the F32 kernel keeps the code the compiler always made of it (a call through a reference to the by-value kernel
// argument allocates registers differently).
    constexpr int NF = HADA ? 2 : 1;
    __shared__ float Ps[NF][kJC][kTR + 1];
    __shared__ __attribute__((aligned(16))) float Qs[NF][kJC][kTC + 4];
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
        f32x4 d[NF][4];
#pragma unroll
        for (int f = 0; f < NF; ++f)
#pragma unroll
            for (int i = 0; i < 4; ++i) d[f][i] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int j0 = 0; j0 < lt.rank; j0 += kJC) {
            __syncthreads();   // the previous chunk has been consumed
#pragma unroll
            for (int f = 0; f < NF; ++f) {
                const void* P = f ? lt.P2 : lt.P;
                const void* Q = f ? lt.Q2 : lt.Q;
                const long long p_rs = f ? lt.p2_rs : lt.p_rs, p_js = f ? lt.p2_js : lt.p_js, q_js = f ? lt.q2_js : lt.q_js, q_cs = f ? lt.q2_cs : lt.q_cs;
                for (int e = tid; e < kJC * kTR; e += 256) {
                    int j, r;
                    if (p_js == 1) { j = e % kJC; r = e / kJC; } else { r = e % kTR; j = e / kTR; }
                    float v = 0.f;
                    if (r0 + r < m.R && j0 + j < lt.rank) v = factor_at<DT>(P, (long long)(r0 + r) * p_rs + (long long)(j0 + j) * p_js);
                    Ps[f][j][r] = v;
                }
                for (int e = tid; e < kJC * kTC; e += 256) {
                    int j, cc;
                    if (q_cs == 1) { cc = e % kTC; j = e / kTC; } else { j = e % kJC; cc = e / kJC; }
                    float v = 0.f;
                    if (c0 + cc < m.Cc && j0 + j < lt.rank) v = factor_at<DT>(Q, (long long)(j0 + j) * q_js + (long long)(c0 + cc) * q_cs);
                    Qs[f][j][cc] = v;
                }
            }
            __syncthreads();
#pragma unroll
            for (int f = 0; f < NF; ++f)
#pragma unroll
                for (int j = 0; j < kJC; ++j) {
                    const f32x4 q = *reinterpret_cast<const f32x4*>(&Qs[f][j][tx * 4]);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float p = Ps[f][j][ty + 8 * i];
                        d[f][i].x = __fmaf_rn(p, q.x, d[f][i].x);
                        d[f][i].y = __fmaf_rn(p, q.y, d[f][i].y);
                        d[f][i].z = __fmaf_rn(p, q.z, d[f][i].z);
                        d[f][i].w = __fmaf_rn(p, q.w, d[f][i].w);
                    }
                }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            f32x4 h = d[0][i];
            if (HADA) {   // the Hadamard product of the two rank-r products: one rounding
                h.x = __fmul_rn(h.x, d[NF - 1][i].x);
                h.y = __fmul_rn(h.y, d[NF - 1][i].y);
                h.z = __fmul_rn(h.z, d[NF - 1][i].z);
                h.w = __fmul_rn(h.w, d[NF - 1][i].w);
            }
            w[i].x = __fmaf_rn(lt.coef, h.x, w[i].x);
            w[i].y = __fmaf_rn(lt.coef, h.y, w[i].y);
            w[i].z = __fmaf_rn(lt.coef, h.z, w[i].z);
            w[i].w = __fmaf_rn(lt.coef, h.w, w[i].w);
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
