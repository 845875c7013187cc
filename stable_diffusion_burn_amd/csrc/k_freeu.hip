// k_freeu.hip -- the kernels FreeU adds (include/sdmi.h "FreeU").  No reference counterpart: the reference's UNet concatenates the backbone
// and the saved skip as they are (unet/mod.rs:134).  FreeU (Si et al., "FreeU: Free Lunch in Diffusion U-Net") edits both halves of cats[i] in front of an output block:
//
//   filter     the SKIP half: Fourier_filter(hs, threshold = 1, scale = s) -- fftn over (H, W), the 2 x 2 box around the zero frequency times s, ifftn, real part.  The
//              box holds the frequencies F(H) x F(W), F(n) = {-1, 0} (n >= 2), {0} (n = 1): at most four coefficients per (sample, channel), so no FFT is run.  With
//              a = 2 pi y / H, b = 2 pi x / W the seven real sums
//                  S = sum v     Ay = sum v cos a   By = sum v sin a   Ax = sum v cos b   Bx = sum v sin b   Axy = sum v cos(a + b)   Bxy = sum v sin(a + b)
//              give   v' = v + (s - 1) / (H W) (S + [H > 1] (Ay cos a + By sin a) + [W > 1] (Ax cos b + Bx sin b) + [H > 1][W > 1] (Axy cos(a + b) + Bxy sin(a + b)))
//              (the sign of a frequency drops out of A cos + B sin).  ONE launch for every affected skip of a forward: a by-value table of segments, gridDim.y =
//              segment, one workgroup per (sample, channel slice of 32 -- bf16: 64 -- channels).  A lane owns 8 channels (16 bytes of bf16, two 16-byte pieces of fp32:
//              the pair that shares a piece of each plane, k_control.hip), the other lanes and the waves stride over the pixels; the partial sums meet through a wave
//              butterfly and four LDS rows added in wave order -- a fixed order, no atomics; then every thread re-reads exactly the elements it read (L2) and writes
//              them back in every form the buffer exists in.  cos / sin of the H + W row and column angles: sincospi in f64, once per workgroup, kept in LDS as fp32.
//   mean       version 2: m[row] = mean over the cx channels of the BACKBONE half, 16 lanes per pixel, fixed order.
//   backbone   h[:, :c] *= b (version 1) or (b - 1) (m - min m) / (max m - min m) + 1 (version 2; 1 where max m == min m), c = cx / 2.  gridDim.y = sample; in version 2
//              every workgroup finds its sample's min and max of m itself (exact whatever the order).
//
// fp32: y fp32 with a row stride, and where y3 != null the three bf16 planes of the NEW value (s3_split8): never a read-modify-write of planes.  bf16: fp32 arithmetic,
// one round to nearest even.  Every store is a 16-byte vector store of one thread's own elements.
#include "kernels.hpp"
#include "k_split3.hpp"

namespace sdmi {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int kSums = 7;
constexpr int kUnroll = 4;   // pixels of one thread loaded before the first of them is used

// the 8 channels of one thread: fp32 -- channels ch .. ch + 3 and ch + 16 .. ch + 19 of the row at p; bf16 -- 8 consecutive channels
template <int DT>
__device__ __forceinline__ void load8(const void* base, long long elem, float (&v)[8]) {
    if constexpr (DT == 0) {
        const float* p = static_cast<const float*>(base) + elem;
        const f32x4 lo = *reinterpret_cast<const f32x4*>(p), hi = *reinterpret_cast<const f32x4*>(p + 16);
#pragma unroll
        for (int i = 0; i < 4; ++i) { v[i] = lo[i]; v[4 + i] = hi[i]; }
    } else {
        const u32x4 u = *reinterpret_cast<const u32x4*>(static_cast<const unsigned short*>(base) + elem);
#pragma unroll
        for (int i = 0; i < 4; ++i) {   // a packed pair: the low half is the even channel
            v[2 * i] = __builtin_bit_cast(float, u[i] << 16);
            v[2 * i + 1] = __builtin_bit_cast(float, u[i] & 0xffff0000u);
        }
    }
}
// ch: the first of the thread's channels inside the tensor y / y3 start at (fp32: a multiple of 4 below 16 mod 32)
template <int DT>
__device__ __forceinline__ void store8(void* base, long long elem, unsigned char* y3, long long row, int ld3, int ch, const float (&v)[8]) {
    if constexpr (DT == 0) {
        float* p = static_cast<float*>(base) + elem;
        const f32x4 lo = {v[0], v[1], v[2], v[3]}, hi = {v[4], v[5], v[6], v[7]};
        *reinterpret_cast<f32x4*>(p) = lo;
        *reinterpret_cast<f32x4*>(p + 16) = hi;
        if (y3) {
            s3_u32x4 h, m, l;
            s3_split8(lo, hi, h, m, l);
            unsigned char* d = y3 + row * ld3 + s3_plane_byte(ch, 0);
            *reinterpret_cast<s3_u32x4*>(d) = h;
            *reinterpret_cast<s3_u32x4*>(d + 64) = m;
            *reinterpret_cast<s3_u32x4*>(d + 128) = l;
        }
    } else {
        u32x4 o;
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = s3_cvt_pk(v[2 * i], v[2 * i + 1]);
        *reinterpret_cast<u32x4*>(static_cast<unsigned short*>(base) + elem) = o;
    }
}

template <int DT>
__global__ __launch_bounds__(256) void freeu_filter_kernel(const FreeuFilter a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int CL = DT ? 8 : 4;         // lanes along the channels of a slice
    constexpr int SW = DT ? 64 : 32;       // channels of a slice
    constexpr int PL = 256 / CL;           // pixels in flight per workgroup
    const FreeuSeg sg = a.seg[blockIdx.y];
    const int slices = sg.c / SW;
    if ((int)blockIdx.x >= sg.n * slices) return;   // (the grid is as wide as the widest segment)
    const int sample = (int)blockIdx.x / slices, sl = (int)blockIdx.x - sample * slices;
    const int H = sg.h, W = sg.w, HW = H * W;
    float* const cy = smem; float* const sy = cy + H; float* const cx = sy + H; float* const sx = cx + W;
    float* const part = smem + ((2 * (H + W) + 3) & ~3);
    const int tid = (int)threadIdx.x, cl = tid % CL, pl = tid / CL;
    for (int i = tid; i < H + W; i += 256) {
        double s, c;
        if (i < H) { sincospi(2.0 * (double)i / (double)H, &s, &c); cy[i] = (float)c; sy[i] = (float)s; }
        else { sincospi(2.0 * (double)(i - H) / (double)W, &s, &c); cx[i - H] = (float)c; sx[i - H] = (float)s; }
    }
    __syncthreads();
    const int ch = DT ? sl * SW + cl * 8 : sl * SW + cl * 4;
    const long long row0 = (long long)sample * HW;
    float acc[kSums][8];
#pragma unroll
    for (int k = 0; k < kSums; ++k)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[k][j] = 0.f;
    // (kUnroll pixels of a thread in flight: the longest walk -- 4096 pixels, 64 per thread -- is bound by the latency of its loads; the sums keep their order)
    for (int p0 = pl; p0 < HW; p0 += kUnroll * PL) {
        float v[kUnroll][8];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u)
            if (p0 + u * PL < HW) load8<DT>(sg.y, (row0 + p0 + u * PL) * sg.ld + ch, v[u]);
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int p = p0 + u * PL;
            if (p >= HW) break;
            const int yy = p / W, xx = p - yy * W;
            const float c1 = cy[yy], s1 = sy[yy], c2 = cx[xx], s2 = sx[xx];
            const float c12 = c1 * c2 - s1 * s2, s12 = s1 * c2 + c1 * s2;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                acc[0][j] += v[u][j];
                acc[1][j] = fmaf(v[u][j], c1, acc[1][j]); acc[2][j] = fmaf(v[u][j], s1, acc[2][j]);
                acc[3][j] = fmaf(v[u][j], c2, acc[3][j]); acc[4][j] = fmaf(v[u][j], s2, acc[4][j]);
                acc[5][j] = fmaf(v[u][j], c12, acc[5][j]); acc[6][j] = fmaf(v[u][j], s12, acc[6][j]);
            }
        }
    }
    // the lanes of a wave that share cl: a butterfly (both partners add the same two numbers), then the four waves' rows in wave order
    const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
    for (int k = 0; k < kSums; ++k)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float t = acc[k][j];
#pragma unroll
            for (int off = CL; off < 64; off <<= 1) t += __shfl_xor(t, off);
            if (lane < CL) part[((wave * CL + cl) * kSums + k) * 8 + j] = t;
        }
    __syncthreads();
    const float kk = sg.k / (float)HW;
#pragma unroll
    for (int k = 0; k < kSums; ++k)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float t = part[((0 * CL + cl) * kSums + k) * 8 + j];
#pragma unroll
            for (int w = 1; w < 4; ++w) t += part[((w * CL + cl) * kSums + k) * 8 + j];
            acc[k][j] = t * kk;
        }
    const bool hy = H > 1, hx = W > 1;
    unsigned char* const y3 = static_cast<unsigned char*>(sg.y3);
    for (int p0 = pl; p0 < HW; p0 += kUnroll * PL) {
        float v[kUnroll][8];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u)
            if (p0 + u * PL < HW) load8<DT>(sg.y, (row0 + p0 + u * PL) * sg.ld + ch, v[u]);
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int p = p0 + u * PL;
            if (p >= HW) break;
            const int yy = p / W, xx = p - yy * W;
            const float c1 = cy[yy], s1 = sy[yy], c2 = cx[xx], s2 = sx[xx];
            const float c12 = c1 * c2 - s1 * s2, s12 = s1 * c2 + c1 * s2;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                float d = acc[0][j];
                if (hy) d += fmaf(acc[1][j], c1, acc[2][j] * s1);
                if (hx) d += fmaf(acc[3][j], c2, acc[4][j] * s2);
                if (hy && hx) d += fmaf(acc[5][j], c12, acc[6][j] * s12);
                v[u][j] += d;
            }
            store8<DT>(sg.y, (row0 + p) * sg.ld + ch, y3, row0 + p, sg.ld3, ch, v[u]);
        }
    }
}

// m[row] = (sum of the cx channels of the row) / cx: 16 lanes per row, lane i takes the 16-byte pieces i, i + 16, ...; then a butterfly over the 16
template <int DT>
__global__ __launch_bounds__(256) void freeu_mean_kernel(const void* __restrict__ x, float* __restrict__ m, long long rows, int cx, int ld) {
    constexpr int PE = DT ? 8 : 4;   // elements of a 16-byte piece
    const int sub = (int)threadIdx.x & 15, pieces = cx / PE;
    const float inv = 1.0f / (float)cx;
    for (long long row = (long long)blockIdx.x * 16 + (threadIdx.x >> 4); row < rows; row += (long long)gridDim.x * 16) {
        float t = 0.f;
        for (int q = sub; q < pieces; q += 16) {
            if constexpr (DT == 0) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(static_cast<const float*>(x) + row * ld + 4 * q);
                t += (v[0] + v[1]) + (v[2] + v[3]);
            } else {
                const u32x4 u = *reinterpret_cast<const u32x4*>(static_cast<const unsigned short*>(x) + row * ld + 8 * q);
                float e = 0.f;
#pragma unroll
                for (int i = 0; i < 4; ++i) e += __builtin_bit_cast(float, u[i] << 16) + __builtin_bit_cast(float, u[i] & 0xffff0000u);
                t += e;
            }
        }
#pragma unroll
        for (int off = 8; off >= 1; off >>= 1) t += __shfl_xor(t, off);   // (the 16 lanes of a row run the loop together)
        if (sub == 0) m[row] = t * inv;
    }
}

template <int DT, int VERSION>
__global__ __launch_bounds__(256) void freeu_backbone_kernel(const FreeuBackbone a) {
    __shared__ float red[8];
    const int sample = (int)blockIdx.y, tid = (int)threadIdx.x;
    const float* const m = a.mean + (long long)sample * a.hw;
    float mn = 0.f, scale = 0.f;   // m_hat = (m - mn) * scale; scale 0: max == min (or nothing finite), m_hat = 0
    if constexpr (VERSION == 2) {
        float lo = INFINITY, hi = -INFINITY;
        for (int i = tid; i < a.hw; i += 256) { const float v = m[i]; lo = fminf(lo, v); hi = fmaxf(hi, v); }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) { lo = fminf(lo, __shfl_xor(lo, off)); hi = fmaxf(hi, __shfl_xor(hi, off)); }
        if ((tid & 63) == 0) { red[tid >> 6] = lo; red[4 + (tid >> 6)] = hi; }
        __syncthreads();
        lo = fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
        hi = fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7]));
        mn = lo;
        scale = hi > lo ? 1.0f / (hi - lo) : 0.f;
    }
    const int upr = a.c >> 3;   // units of 8 channels per row
    const long long units = (long long)a.hw * upr;
    unsigned char* const y3 = static_cast<unsigned char*>(a.y3);
    for (long long u = (long long)blockIdx.x * 256 + tid; u < units; u += (long long)gridDim.x * 256) {
        const long long p = u / upr;
        const int k = (int)(u - p * upr);
        const int ch = DT ? 8 * k : (k >> 2) * 32 + (k & 3) * 4;
        const long long row = (long long)sample * a.hw + p, elem = row * a.ld + ch;
        float f = a.b;
        if constexpr (VERSION == 2) f = scale != 0.f ? fmaf(a.b - 1.0f, (m[p] - mn) * scale, 1.0f) : 1.0f;
        float v[8];
        load8<DT>(a.y, elem, v);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] *= f;
        store8<DT>(a.y, elem, y3, row, a.ld3, ch, v);
    }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// the rules both edits share: a tensor of c channels (whole slices) inside rows of ld elements, every base and stride on 16 bytes; planes are an fp32 form
bool tensor_ok(const void* y, const void* y3, int c, int ld, int ld3, int dt) {
    const int sw = dt ? 64 : 32;
    if (!y || c <= 0 || c % sw || ld < c || !aligned16(y) || ((long long)ld * (dt ? 2 : 4)) % 16) return false;
    if (y3 && (dt || !aligned16(y3) || ld3 % 16 || ld3 < c / 32 * 192)) return false;
    return true;
}

size_t filter_lds_bytes(int h, int w, int dt) { return (size_t)(((2 * (h + w) + 3) & ~3) + 4 * (dt ? 8 : 4) * kSums * 8) * sizeof(float); }

}  // namespace

bool freeu_filter_size_ok(int h, int w) { return h >= 1 && w >= 1 && filter_lds_bytes(h, w, 1) <= 65536 && (long long)h * w < (1ll << 31); }

hipError_t launch_freeu_filter(const FreeuFilter& f, hipStream_t s) {
    if (f.n_seg < 1 || f.n_seg > kFreeuMaxSegs || (f.dt != 0 && f.dt != 1)) return hipErrorInvalidValue;
    int most = 0;
    size_t lds = 0;
    for (int i = 0; i < f.n_seg; ++i) {
        const FreeuSeg& g = f.seg[i];
        if (g.n < 1 || !freeu_filter_size_ok(g.h, g.w) || !tensor_ok(g.y, g.y3, g.c, g.ld, g.ld3, f.dt) || !(g.k == g.k)) return hipErrorInvalidValue;
        const long long wgs = (long long)g.n * (g.c / (f.dt ? 64 : 32));
        if (wgs > 0x7fffffff) return hipErrorInvalidValue;
        most = most > (int)wgs ? most : (int)wgs;
        const size_t b = filter_lds_bytes(g.h, g.w, f.dt);
        lds = lds > b ? lds : b;
    }
    const dim3 grid((unsigned)most, (unsigned)f.n_seg);
    if (f.dt) hipLaunchKernelGGL(freeu_filter_kernel<1>, grid, dim3(256), lds, s, f);
    else hipLaunchKernelGGL(freeu_filter_kernel<0>, grid, dim3(256), lds, s, f);
    return hipGetLastError();
}

hipError_t launch_freeu_mean(const void* x, float* mean, long long rows, int cx, int ld, int dt, hipStream_t s) {
    if (!x || !mean || rows <= 0 || cx <= 0 || cx % (dt ? 8 : 4) || ld < cx || (dt != 0 && dt != 1)) return hipErrorInvalidValue;
    if (!aligned16(x) || ((long long)ld * (dt ? 2 : 4)) % 16) return hipErrorInvalidValue;
    long long blocks = (rows + 15) / 16;
    if (blocks > 2048) blocks = 2048;
    if (dt) hipLaunchKernelGGL(freeu_mean_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, s, x, mean, rows, cx, ld);
    else hipLaunchKernelGGL(freeu_mean_kernel<0>, dim3((unsigned)blocks), dim3(256), 0, s, x, mean, rows, cx, ld);
    return hipGetLastError();
}

hipError_t launch_freeu_backbone(const FreeuBackbone& a, hipStream_t s) {
    if ((a.version != 1 && a.version != 2) || (a.dt != 0 && a.dt != 1) || a.n < 1 || a.n > 65535 || a.hw < 1) return hipErrorInvalidValue;
    if (!tensor_ok(a.y, a.y3, a.c, a.ld, a.ld3, a.dt) || !(a.b == a.b) || (a.version == 2 && !a.mean)) return hipErrorInvalidValue;
    long long blocks = ((long long)a.hw * (a.c / 8) + 255) / 256;
    if (blocks > 256) blocks = 256;
    const dim3 grid((unsigned)blocks, (unsigned)a.n);
    if (a.dt) {
        if (a.version == 2) hipLaunchKernelGGL((freeu_backbone_kernel<1, 2>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((freeu_backbone_kernel<1, 1>), grid, dim3(256), 0, s, a);
    } else {
        if (a.version == 2) hipLaunchKernelGGL((freeu_backbone_kernel<0, 2>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((freeu_backbone_kernel<0, 1>), grid, dim3(256), 0, s, a);
    }
    return hipGetLastError();
}

}  // namespace sdmi
