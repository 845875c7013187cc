// kernels.hpp -- launch interface of the gfx950 HIP kernels of libsdmi.
//
// Layout rules (DESIGN.md "Data layout in HBM"):
//   activations  NHWC fp32 (bf16 for the *_bf16 kernels): [NB][H][W][C]  == row-major [M = NB*H*W][C]
//   conv/linear weights pre-packed "Bt": [N = Cout][K], K ordered
//       k = (cs * T + tap) * CS + ci   with channel c = cs*CS + ci, tap = ky*KW+kx,
//       T = KH*KW, CS = min(32, Cin)   (channel-slice outer, taps inner: the nine
//       taps of one 32-channel slice reuse the same 128-byte pixel segments)
// Every launcher enqueues on `stream` and returns the hipError of the launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "attn_plan.hpp"
#include "gemm_tiles.hpp"

namespace sdmi {

// ---- implicit-GEMM convolution / linear on fp32 MFMA -------------------------
// C[m][n] = sum_k A(m,k) * Bt[n][k]  (+ bias[n] + rowvec[sample(m)][n] + resid[m][n])
// A(m,k) is gathered from the NHWC source: m -> (nb, oy, ox), k -> (tap, channel).
struct ConvGemm {
    const float* A;       // source activations [NB][Hs][Ws][Cin]
    const float* Bt;      // packed weights [N][K]
    const void* Bt3;      // split kernels (k_gemm3x.hip, k_gemm3p.hip): the same weights as three bf16 planes, [N][K / 32][3][32]
    int b3_grouped;       // ... 0: that row-major layout; 1 (round 5): 16-row fragment groups, [N / 16][K / 32][3][16][32] -- a DMA piece (one plane of one group's k tile) is
                          // 1 KiB of consecutive bytes and a group's k tiles follow each other, instead of sixteen 64-byte pieces 6 K bytes apart (launch_pack_split3)
    const void* A3;       // plane kernel (k_gemm3p.hip): the source activations as three bf16 planes, [NB][Hs][Ws][a3_ld / 192 slices][3][32]
    int a3_ld;            // bytes between source pixels in A3 (192 per 32 channels of the -- possibly wider -- buffer)
    float* C;             // output [M][ldc]; may be null when C3 is set
    void* C3;             // k_gemm3x.hip / k_gemm3p.hip / launch_splitk_reduce: not null -> the output ALSO (or only) as three bf16 planes, [M][ldc3 / 192 slices][3][32]
    int ldc3;             // bytes between output rows in C3 (needs N % 4 == 0: the 16-byte epilogue)
    float* slabs;         // splits > 1: fp32 partial sums [splits][M][N]
    const float* bias;    // [N] or null
    const float* rowvec;  // per-sample per-channel add (time embedding) or null
    const float* resid;   // residual [M][ldr] or null
    int M, N, K;
    int NB, Hs, Ws, Cin;  // source dims (before the optional nearest-2x upsample)
    int Ho, Wo;           // output spatial dims
    int KH, KW, stride, pad, ups;
    int ldc, ldr;
    int a_ld;             // floats between source pixels (normally Cin)
    int b_ld;             // floats between Bt rows (normally K)
    int rowvec_stride;    // floats between samples in rowvec (0: shared by the batch)
    int CS;               // channel slice width: 32, or Cin when Cin < 32
    int kt_total;         // number of 32-wide k tiles
    int kt_per_split;     // k tiles per blockIdx.z slice
    int splits;           // gridDim.z
    long long slab_stride;  // M*N when splits > 1
    unsigned a_bytes, b_bytes;  // extents of A / Bt for the buffer-load range check (v2 kernel)
    int out_mode;               // 0: output in the kernel's storage type; 1: force fp32 (bf16 kernel); 2: bf16 from the fp32 kernel
    const void* zero_page;      // >= 16 readable zero bytes (large-tile kernels: source of padded / out-of-range lanes)
    const void* a_scale;        // fp8 kernel: E8M0 scales of A, [pixels][a_ld / 32] bytes (a_ld = padded channel count = bytes per pixel)
    const void* b_scale;        // fp8 kernel: E8M0 scales of Bt, [N][b_ld / 32] bytes
    int variant;                // k_gemm3x.hip A/B switches (option gemm3x_variant): bit 0 DMA issued in one block per k tile, 1 scalar residual subtractions,
                                // 2 two LDS stages on the 128-row tiles, 4 s_setprio 1 for waves 4-7; k_gemm_bf16x.hip (option gemm_bf16x_variant): bit 0 persistent tile loop
    int resid_acc;              // large-tile bf16 / MXFP8 kernels (round 6): the (bf16) residual is loaded INTO THE ACCUMULATORS in front of the k loop (C = R + A B) instead of
                                // being read by the epilogue one fragment group at a time -- eight exposed load latencies per 256-row tile there; set by Engine::launch_gemm / launch_fp8
    int geglu;                  // large-tile kernels: Bt holds 2 N rows (N value rows, then N gate rows; bias likewise) and the
                                // epilogue writes value * gelu_erf(gate) -- GEGLU::forward (unet/mod.rs:579-591) without the [M, 2N] tensor
    unsigned long long* probe;  // diagnostic (option gemm_probe; k_gemm3p.hip tiles 300 / 303 / 304 only): when non-null the PROBE instantiation runs and
                                // stores 24 words per workgroup (see conv_gemm3p_kernel)
    // A second problem on the slices [z_aux, splits) of a split-K launch (k_gemm3p.hip only; every other launcher refuses z_aux != 0): a 1x1 / stride-1 / pad-0 GEMM over the
    // same M output rows and the same N, its own activation planes and weight planes -- the ResBlock shortcut riding in conv_out's launch (Engine::conv_pair).  The main
    // problem must be stride 1 without upsampling (source pixel = output pixel).  Slices [0, z_aux) cover the kt_total k tiles of the main problem, slice z >= z_aux the
    // k tiles [(z - z_aux) kt_per_split, ...) of the kt_total_aux auxiliary ones: no slice holds tiles of both.  Slabs are indexed by z; launch_splitk_reduce sums all
    // `splits` of them in slice order and adds bias + bias_aux, then the residual where there is one (Engine::linear_pair; a ResBlock's pair has none: its
    // shortcut IS the residual).  The main problem may be a Linear layer (NB = 1, Hs = 1, Ws = rows, one tap).
    const void* A3_aux;         // [NB][Hs][Ws][a3_ld_aux / 192 slices][3][32]
    int a3_ld_aux;
    const void* Bt3_aux;        // [N][Cin_aux / 32][3][32], in the layout b3_grouped names (it depends on N only)
    int Cin_aux, kt_total_aux;
    int z_aux;                  // first slice of the auxiliary problem; 0: none
    const float* bias_aux;      // [N] or null
    // Phase mode (k_gemm3p.hip only; every other launcher refuses phases != 0): conv3x3(nearest_2x(x)) as four 2x2 convolutions over the SOURCE grid, one per output pixel
    // phase ph = py * 2 + px, each with its own folded weights (Engine::rebuild_folds: [4][N][4 Cin], k = (channel slice, tap a * 2 + b, 32 channels)).  The struct keeps the
    // layer's description (KH = KW = 3, ups = 1, Ho = 2 Hs, Wo = 2 Ws) except: M = NB Hs Ws, the rows of ONE phase, and K = 4 Cin, kt_total = Cin / 8.  The M tiles are laid
    // phase-major, ceil(M / BM) per phase, so no tile holds two phases; row m = (nb, y, x) of phase ph reads source pixels (y - 1 + py + a, x - 1 + px + b) and is output
    // row ups_phase_row(m, ph, Hs, Ws).  Bias only: no rowvec / resid / geglu / z_aux / probe.  splits > 1: slabs [splits][4][M][N], slab_stride = 4 M N.
    int phases;                 // 0 or 4
    long long phase_stride;     // bytes between the phase images of Bt3
};

// output row of row m = (nb, y, x) of phase ph = py * 2 + px: pixel (2 y + py, 2 x + px) of sample nb in the [NB][2 Hs][2 Ws] result.  THE row map of a phase launch:
// the epilogue (k_gemm_epi.hpp) and the split-K reduce (k_gemm.hip) both write through it.
__host__ __device__ inline long long ups_phase_row(int m, int ph, int Hs, int Ws) {
    const int hw = Hs * Ws;
    const int nb = m / hw, rem = m - nb * hw;
    const int y = rem / Ws, x = rem - y * Ws;
    return ((long long)nb * (2 * Hs) + 2 * y + (ph >> 1)) * (2 * Ws) + 2 * x + (ph & 1);
}

// capacity of ConvGemm::probe in workgroups (24 words each); launch_conv_gemm3p refuses a probe launch with a larger grid
constexpr int kGemmProbeBlocks = 1 << 13;

// launch grid of a GEMM kernel: (tiles rounded up to the 8 XCDs) x slices
inline dim3 gemm_grid(const ConvGemm& p, int tiles) {
    return dim3((unsigned)(((tiles + 7) / 8) * 8), 1, (unsigned)p.splits);
}

hipError_t launch_conv_gemm2(const ConvGemm& p, int tile_cfg, hipStream_t stream);  // k_gemm2.hip; the tile lists of every family (index = tile_cfg): gemm_tiles.hpp
size_t gemm2_tile_lds_bytes(int cfg);
// bf16 storage / fp32 accumulate (k_gemm_bf16.hip); A, Bt, resid and (unless out_mode == 1) C are bf16
hipError_t launch_conv_gemm_bf16(const ConvGemm& p, int tile_cfg, hipStream_t stream);
hipError_t launch_splitk_reduce_bf16(const ConvGemm& p, hipStream_t stream);
// large-tile (256-row, 8-wave, LDS-DMA staged) bf16 kernel (k_gemm_bf16x.hip); its own tile list
hipError_t launch_conv_gemm_bf16x(const ConvGemm& p, int tile_cfg, hipStream_t stream);
// the 256 x 320 / 256 x 256 tiles for 3x3 / stride-1 / pad-1 convolutions with the three taps of a kernel row read from one staged activation tile
// (k_gemm_bf16t.hip); bf16 tile_cfg 100 + kNumGemmTilesX + x.  launch_conv_gemm_bf16t fails (hipErrorInvalidValue) unless conv_gemm_bf16t_supported(p, p.kt_per_split).
hipError_t launch_conv_gemm_bf16t(const ConvGemm& p, int tile_cfg, hipStream_t stream);
// bf16 large tiles as one list: 100 + [0, kNumGemmTilesX) = k_gemm_bf16x.hip, then k_gemm_bf16t.hip
inline hipError_t launch_conv_gemm_bf16_large(const ConvGemm& p, int c, hipStream_t stream) {
    return c < kNumGemmTilesX ? launch_conv_gemm_bf16x(p, c, stream) : launch_conv_gemm_bf16t(p, c - kNumGemmTilesX, stream);
}
// the same structure for fp32 storage (k_gemm2x.hip; Cin % 32 == 0, fp32 output); same tile list
hipError_t launch_conv_gemm2x(const ConvGemm& p, int tile_cfg, hipStream_t stream);
// fp32 on the bf16 matrix pipe: operands as exact sums of three bf16 terms, six partial products (k_gemm3x.hip); its own tile
// list; needs p.Bt3 (launch_pack_split3 of the packed fp32 rows, once at load)
hipError_t launch_conv_gemm3x(const ConvGemm& p, int tile_cfg, hipStream_t stream);
hipError_t launch_pack_split3(const float* bt, void* w3, long long rows, int K, hipStream_t s, bool grouped = false);   // grouped needs rows % 16 == 0
// the same arithmetic with the ACTIVATIONS as planes too, written once by their producer (k_gemm3p.hip; tile_cfg 300 + x; needs p.A3)
hipError_t launch_conv_gemm3p(const ConvGemm& p, int tile_cfg, hipStream_t stream);
// fp32 rows [rows][ld] (c channels, c % 32 == 0) -> planes [rows][ld3_bytes / 192 slices][3][32] bf16 (slices [0, c / 32) written)
hipError_t launch_split3_rows(const float* x, void* y3, long long rows, int c, long long ld, long long ld3_bytes, hipStream_t s);
hipError_t launch_join3_rows(const void* x3, float* y, long long rows, int c, long long ld3_bytes, long long ld, hipStream_t s);   // planes -> fp32 (exact)
// hipFuncAttributeMaxDynamicSharedMemorySize, once per (kernel, device); safe to call from several host threads (multi.cpp)
hipError_t set_max_dynamic_lds(const void* kernel, int bytes);
// MXFP8 (e4m3 + E8M0 block scales) 256-row LDS-DMA kernel on v_mfma_scale_f32_16x16x128_f8f6f4 (k_fp8.hip); its own tile list
hipError_t launch_conv_gemm_fp8x(const ConvGemm& p, int tile_cfg, hipStream_t stream);
// fp32 OIHW -> e4m3 [Cout][Kp] + scales [Cout][Kp / 32], Kp = roundup(Cin, 128) * kh * kw, k = (slice * T + tap) * 128 + ci
hipError_t launch_pack_conv_weight_fp8(const float* w_oihw, void* bt8, void* bs, int cout, int cin, int kh, int kw, hipStream_t s);
// GroupNorm(+SiLU) of a bf16 tensor with MXFP8 output: y8 [n][hw][Cp] e4m3, y_scale [n][hw][Cp / 32], Cp = roundup(c, 128)
struct GnTune;
hipError_t launch_group_norm_fp8(const void* x, void* y8, void* y_scale, const float* gamma, const float* beta, int n, int hw, int c,
                                 int ldx, int n_group, float eps, bool silu, void* partials, hipStream_t stream, const GnTune* t = nullptr);
hipError_t launch_quantize_fp8(const float* x, void* q, void* s, long long rows, int c, hipStream_t stream);   // fp32 [rows][c] -> MXFP8
// precision = 2 beyond the ResBlock convolutions (option fp8_linear; k_fp8.hip): quantising producers and the Linear weight packer
hipError_t launch_quantize_bf16_fp8(const void* x, void* q, void* s, long long rows, int c, int ldx, hipStream_t stream);   // bf16 [rows][ldx] -> MXFP8 (c % 32 == 0)
hipError_t launch_layer_norm_fp8(const void* x, void* y8, void* y_scale, const float* gamma, const float* beta, int rows, int c, float eps, hipStream_t stream);
hipError_t launch_geglu_fp8(const void* proj, void* y8, void* y_scale, long long rows, int hidden, hipStream_t stream);
hipError_t launch_pack_linear_weight_fp8(const float* w_in_out, void* bt8, void* bs, int cin, int cout, hipStream_t s);
hipError_t launch_dequant_fp8(const void* q, const void* s, float* out, long long rows, int c, hipStream_t stream);
hipError_t launch_pack_conv_weight_bf16(const float* w_oihw, void* bt, int cout, int cin, int kh, int kw, hipStream_t s);
hipError_t launch_pack_linear_weight_bf16(const float* w_in_out, void* bt, int cin, int cout, hipStream_t s);
// sums split-K slabs in fixed order and applies the epilogue
hipError_t launch_splitk_reduce(const ConvGemm& p, hipStream_t stream);
// the 16-byte form of the split-K reduce kernels (four outputs per thread; bf16: launch_splitk_reduce_bf16): strides AND base addresses aligned for its vector
// loads and stores -- the fp32 bias / time-embedding rows 16 bytes, the residual and the output 8 (bf16) or 16 bytes (fp32); otherwise the scalar form
__host__ __device__ inline bool splitk_reduce_vec(const ConvGemm& p, bool bf16) {
    const uintptr_t ra = bf16 ? 7 : 15, ca = (bf16 && p.out_mode != 1) ? 7 : 15;
    return ((p.N | p.ldc | p.rowvec_stride) & 3) == 0 && (!p.resid || (p.ldr & 3) == 0) && (((uintptr_t)p.bias | (uintptr_t)p.rowvec) & 15) == 0 &&
           ((uintptr_t)p.resid & ra) == 0 && ((uintptr_t)p.C & ca) == 0;
}
// weight packing (done once at load)
hipError_t launch_pack_conv_weight(const float* w_oihw, float* bt, int cout, int cin, int kh, int kw, hipStream_t s);
hipError_t launch_pack_linear_weight(const float* w_in_out, float* bt, int cin, int cout, hipStream_t s);
// out [N][K] (rows ldo apart) = fp32(a [N][Cn] x b [Cn][K]) with fp64 accumulation, rounded once: the folded weights of Engine::rebuild_folds (load time only)
hipError_t launch_fold_matmul_f64(const float* a, const float* b, float* out, int N, int Cn, int K, long long lda, long long ldb, long long ldo, hipStream_t s);
// bt: a packed 3x3 weight [N][9 Cin] (Cin % 32 == 0) -> out [nph][N][4 Cin], the images of phases ph0 .. ph0 + nph - 1 of the phase image [4][N][4 Cin]: the folded 2x2 weights of the four pixel phases of conv3x3(nearest_2x(x)) (ConvGemm::phases):
// out[py * 2 + px][n][(cs * 4 + a * 2 + b) * 32 + ci] = sum of the 1, 2 or 4 taps (ky, kx) with R_py[a][ky] = R_px[b][kx] = 1, R_0 = [[1,0,0],[0,1,1]], R_1 = [[1,1,0],[0,0,1]],
// in fp64 (ky outer, kx inner), rounded once
hipError_t launch_fold_ups_phase_f64(const float* bt, float* out, int N, int Cin, int ph0, int nph, hipStream_t s);

// ---- flash-style attention on fp32 MFMA ---------------------------------------
struct AttnParams {
    const float* q; const float* k; const float* v; float* o;
    const int* kv_len;      // [n] valid keys per batch entry, or null (= nk)
    const float* mask;      // additive [>=nq][mask_ld] or null
    int mask_ld;
    int n, n_head, nq, nk, d_head;
    int ldq, ldk, ldv, ldo;             // row strides in floats
    long long q_bs, k_bs, v_bs, o_bs;   // batch strides in floats
    float scale;                        // d_head^-0.25 applied to q and to k (attention.rs:15-26)
    int bf16;                           // q/k/v/o are bf16 in HBM (strides in elements)
    int q_log2;                         // the CALLER states that q already carries d_head^-0.5 log2(e) (attn_bf16_q_scale: folded into the query weight at load, or applied by
                                        // the fp32 -> bf16 conversion): launch_attention_bf16 ignores `scale` and refuses the call without it
    void* o3;                           // fp32 kernels: not null -> the output is written as three bf16 planes instead of fp32 ([n * nq][ldo3 / 192 slices][3][32],
    int ldo3;                           // channel = head * d_head + column; bytes between rows), what the out-projection's k_gemm3p.hip launch reads
    // fp32 kernels, no mask (round 5): kv_splits = S > 1 -> blockIdx.z = key slice: workgroup z walks K / V tiles [z T / S, (z + 1) T / S) and writes its
    // UNNORMALISED output rows + (running maximum in log2 units, row sum) instead of o / o3; launch_attention_combine merges the S slices in slice order.  For the
    // batch-1 levels whose (query tile x head) grid leaves most CUs without a workgroup (32 x 32: 128 workgroups, 16 x 16: 64).
    int kv_splits;                      // = AttnPlan::kv_splits
    float* part_o;                      // [S][n][nq][n_head * d_head]
    float* part_ml;                     // [S][n][n_head][nq][2]
};
// The three fused kernels.  Which one runs, its workgroup form and the slice count are decided by plan_attention (attn_plan.hpp): a launcher only maps
// (d_head, plan.waves, form flags) to the template instantiation, takes the grid from plan.q_rows and plan.kv_splits, and keeps the argument checks the kernel's
// safety rests on.  A plan for another kernel, or one that names no instantiated form, is hipErrorInvalidValue.
// k_attn.hip: fp32 matrix instructions, fp32 or (widened) bf16 storage, additive mask in fp32
hipError_t launch_attention(const AttnParams& p, const AttnPlan& plan, hipStream_t stream);
// k_attn_split.hip: fp32 q/k/v/o on the bf16 matrix pipe, three-way split operands: d_head 40 / 80, no additive mask, 16-byte aligned rows
hipError_t launch_attention_split(const AttnParams& p, const AttnPlan& plan, hipStream_t stream);
// merges the key slices of a kv_splits > 1 launch (either fp32 kernel) into p.o / p.o3
hipError_t launch_attention_combine(const AttnParams& p, hipStream_t stream);
// k_attn_bf16.hip: p.bf16 set, no additive mask; q must arrive multiplied by attn_bf16_q_scale(d_head) (the engine folds it into the query projection's
// weight at load: Engine::q_prescaled) and the caller must say so (p.q_log2, else hipErrorInvalidValue); p.scale is not used
inline float attn_bf16_q_scale(int d_head) { return (float)(1.4426950408889634 / __builtin_sqrt((double)d_head)); }
hipError_t launch_attention_bf16(const AttnParams& p, const AttnPlan& plan, hipStream_t stream);
// row softmax (in place) for the unfused single-head VAE attention: x[rows][cols] *= scale first
hipError_t launch_softmax_rows(float* x, int rows, int cols, float scale, hipStream_t stream);

// ---- normalisation (HBM-bound class) --------------------------------------------
// GroupNorm (+SiLU) over NHWC: stats pass (per-chunk partial sums) + apply pass.
// `partials` needs gn_partials_bytes(n, hw, c) bytes of scratch.
size_t gn_partials_bytes(int n, int hw, int c, int min_wgs = 0);    // min_wgs: k_norm.hip gn_geom (option gn32_min_wgs)
// ldx: elements between pixels of x (>= c; x may be a channel slice of a wider buffer); y is dense [n][hw][c]
hipError_t launch_group_norm(const float* x, float* y, const float* gamma, const float* beta,
                             int n, int hw, int c, int ldx, int n_group, float eps, bool silu,
                             void* partials, hipStream_t stream, int min_wgs = 0);
hipError_t launch_layer_norm(const float* x, float* y, const float* gamma, const float* beta,
                             int rows, int c, float eps, hipStream_t stream);
// the same normalisations with the result written as three bf16 planes (k_split3.hpp; y3 dense: (c / 32) * 192 bytes per pixel / row),
// what the consuming k_gemm3p.hip launch reads.  c % 32 == 0.
hipError_t launch_group_norm_planes(const float* x, void* y3, const float* gamma, const float* beta, int n, int hw, int c, int ldx,
                                    int n_group, float eps, bool silu, void* partials, hipStream_t stream, int min_wgs = 0);
hipError_t launch_layer_norm_planes(const float* x, void* y3, const float* gamma, const float* beta, int rows, int c, float eps,
                                    hipStream_t stream);

// ---- elementwise / data movement ---------------------------------------------------
hipError_t launch_nchw_to_nhwc(const float* src, float* dst, int n, int c, int h, int w, float scale, hipStream_t s);
hipError_t launch_nhwc_to_nchw(const float* src, float* dst, int n, int c, int h, int w, hipStream_t s);
hipError_t launch_concat_channels(const float* a, const float* b, float* dst, long long rows, int ca, int cb, hipStream_t s);
hipError_t launch_geglu(const float* proj, float* out, long long rows, int hidden, hipStream_t s);
hipError_t launch_geglu_planes(const float* proj, void* out3, long long rows, int hidden, hipStream_t s);   // out3: planes, hidden % 32 == 0
hipError_t launch_silu(const float* x, float* y, long long n, hipStream_t s);
hipError_t launch_repeat_rows(const float* src, float* dst, int n, long long elems, hipStream_t s);   // dst[i][:] = src[:], i < n
hipError_t launch_nhwc_to_nchw_slice(const float* src, float* dst, int n, int c_src, int c_out, int h, int w, hipStream_t s);
hipError_t launch_nchw3_to_nhwc4(const float* src, float* dst, int n, int h, int w, hipStream_t s);
// CLIP text encoder pieces (clip/mod.rs): QuickGELU in place, token + position embedding, decoder mask
hipError_t launch_quick_gelu(float* x, long long n, hipStream_t s);
hipError_t launch_gelu_erf(float* x, long long n, hipStream_t s);   // x * Phi(x), the exact GELU of the OpenCLIP text tower (SD 2.x)
hipError_t launch_clip_embed(const int* tokens, const float* tok_table, const float* pos_table, float* out, int n, int T, int C,
                             hipStream_t s);
hipError_t launch_causal_mask(float* mask, int T, hipStream_t s);
// the extended CLIP forward: rows of the textual-inversion bank [rows, C] where emb_row >= 0; emphasis weights w [n][T] applied to
// z [n][T][C] in place, one workgroup per chunk, each renormalised to its unweighted sum
hipError_t launch_clip_embed_bank(const int* tokens, const int* emb_row, const float* tok_table, const float* bank, const float* pos_table, float* out, int n,
                                  int T, int C, hipStream_t s);
hipError_t launch_clip_reweight(float* z, const float* w, int n, int T, int C, hipStream_t s);
// dst[c][r] = src[r*src_ld + c]
hipError_t launch_transpose2d(const float* src, float* dst, int rows, int cols, int src_ld, hipStream_t s);
// out[s][0:half] = cos(t_s * f_i), out[s][half:dim] = sin(t_s * f_i)  (unet/mod.rs:19-30)
hipError_t launch_timestep_embedding(const int* t_dev, int n_t, int dim, float* out, hipStream_t s);
// the same at fractional timesteps (f32 on the device): an integer t gives the bits of the int form
hipError_t launch_timestep_embedding_f(const float* t_dev, int n_t, int dim, float* out, hipStream_t s);
// CFG combine + DDIM update on NHWC latents (stablediffusion/mod.rs:152-156,190-191).
// eps [2n][hw][4] (uncond rows first), latent [n][hw][4] updated in place, and
// copied twice into unet_in [2n][hw][4] for the next step.
struct DdimCoef { float scale, sqrt_noise, inv_div /*unused*/, sqrt_cur, sqrt_prev, dir_coef; };
hipError_t launch_cfg_ddim(const float* eps, float* latent, float* unet_in, long long per_half,
                           DdimCoef c, hipStream_t s);
hipError_t launch_dup_latent(const float* latent, float* unet_in, long long per_half, hipStream_t s);
// (img+1)/2*255 -> clamp -> truncating u8, NHWC in, HWC out (stablediffusion/mod.rs:79-99)
hipError_t launch_image_to_u8(const float* img_nhwc, uint8_t* out, long long n_elem, hipStream_t s);
hipError_t launch_fill_normal(float* dst, long long n, uint64_t seed, hipStream_t s);

// ---- img2img (k_img2img.hip) -----------------------------------------------------------------------------
// rgb [pixels][3] u8 (HWC, sample_image's output layout) -> dst [pixels][4] fp32 = v / 127.5 - 1, channel 3 = 0
hipError_t launch_rgb_u8_to_nhwc4(const uint8_t* rgb, float* dst, long long pixels, hipStream_t s);
// x_t0 = sqrt_a z0 + sqrt_1ma eps for n images of hw pixels -> latent [n][hw][4] and both halves of unet_in
// (the conditional half starts half_elems floats in).  z_src: from_q8 ? the encoder's NHWC8 quant_conv output
// (z0 = 0.18215 * channels 0..3) : z0 [n,4,h,w] NCHW.  noise [n,4,h,w] NCHW, or null: image b draws N(0,1) from
// stream seed + b (launch_fill_normal's element order).  z0_out / eps_out [n][hw][4] (both or neither): kept for
// launch_cfg_ddim_masked.
hipError_t launch_img2img_start(const float* z_src, bool from_q8, const float* noise, uint64_t seed, float sqrt_a, float sqrt_1ma, float* latent,
                                float* unet_in, long long half_elems, float* z0_out, float* eps_out, int n, long long hw, hipStream_t s);
// launch_cfg_ddim, then latent <- m latent + (1 - m)(c.sqrt_prev z0 + c.dir_coef eps) with m = mask[n][hw] (1 = regenerate)
hipError_t launch_cfg_ddim_masked(const float* eps, float* latent, float* unet_in, long long per_half, DdimCoef c, const float* mask,
                                  const float* z0, const float* e0, hipStream_t s);

// ---- conditioned UNet input and the inpainting conditioning (k_inpaint.hip) ------------------------------------
// unet_in [rows_pixels][4] + cond [cond_pixels][pc - 4] -> out [rows_pixels][pc]: latent | cond channels 0 .. cond_ch - 1 | zeros (written on every launch).
// Pixel i reads cond pixel i mod cond_pixels (cond_pixels = n hw: both halves of a CFG batch read their sample's row).  pc % 4 == 0, pc - 4 - cond_ch <= 3.
hipError_t launch_assemble_unet_in(const float* unet_in, const float* cond, float* out, long long rows_pixels, long long cond_pixels, int pc, int cond_ch,
                                   hipStream_t s);
// cond [n][cond_ch][hw] NCHW -> [n][hw][pcc] (pcc % 4 == 0, >= cond_ch; the channels past cond_ch zero)
hipError_t launch_cond_nchw_to_nhwc(const float* cond_nchw, float* cond_nhwc, int n, int cond_ch, long long hw, int pcc, hipStream_t s);
// launch_rgb_u8_to_nhwc4 times (mask < 128): a regenerated pixel (mask >= 128) becomes exactly 0.  mask [pixels] u8
hipError_t launch_rgb_u8_masked_to_nhwc4(const uint8_t* rgb, const uint8_t* mask, float* dst, long long pixels, hipStream_t s);
// ONE image: q8 [h w][8] (the encoder's quant_conv output for the masked picture), mask [8h][8w] u8 -> cond [h w][8] = m | 0.18215 q8[0..3] | 0 0 0 with
// m[y][x] = mask[8y][8x] >= 128 (sdmi_inpaint_latent_mask); lat_mask (may be null) [h w] receives m on its own
hipError_t launch_inpaint_cond_pack(const float* q8, const uint8_t* mask, float* cond, float* lat_mask, int h, int w, hipStream_t s);
// out = mask >= 128 ? gen : init, per pixel of 3 bytes; out may be gen
hipError_t launch_inpaint_paste(const uint8_t* gen, const uint8_t* init, const uint8_t* mask, uint8_t* out, long long pixels, hipStream_t s);

// ---- latent resampler of the hires fix (k_resize.hip) -----------------------------------
// One axis of a separable resample over NHWC4 latents (one f32x4 per pixel): x [outer][in_size][inner] -> y [outer][out_size][inner] pixels,
//     y[a][o][i] = sum_{j < count[o]} taps[o * max_taps + j] * x[a][first[o] + j][i]      (ascending j, fp32)
// inner = 1, outer = n * h: the horizontal pass; inner = the row length, outer = n: the vertical one.  first / count / taps: DEVICE arrays holding the table
// of sdmi_resize_weights (taps as f32); the caller guarantees 0 <= first[o] and first[o] + count[o] <= in_size.  gather: every row is the single tap 1.0
// (nearest): the pixel is copied, not multiplied.
hipError_t launch_resize_axis(const float* x, float* y, const int* first, const int* count, const float* taps, int max_taps, long long outer,
                              int in_size, int out_size, long long inner, bool gather, hipStream_t s);

// ---- sampler choice (k_sampler.hip) ---------------------------------------------------
// One step of DDIM(eta) / DPM-Solver++(2M) / PLMS in the linear form sdmi_sampler_coefs returns (f64 on the host, applied as f32):
//   e = eu + (ec - eu) scale;  q = qx x + qe e;  x' = cx x + ce e + h[0] q_-1 + h[1] q_-2 + h[2] q_-3 + cz z
// then the optional mask blend of launch_cfg_ddim_masked (blend_prev = sqrt(a_prev), blend_dir = sqrt(1 - a_prev)).  n_hist = how many of the
// history slots hold a q of this call (the others are not read).  Plain Euler / Euler-ancestral are DDIM at eta = 0 / 1: no kinds of their own.
// cz2 (the sigma-schedule samplers, section 9i): the weight of a SECOND draw z2, x' += cz2 z2 -- dpmpp_sde's second stage, which draws its first one again.
struct SamplerStep { float scale, cx, ce, h[3], cz, qx, qe, blend_prev, blend_dir; int n_hist; float cz2; };
// eps [2n][hw][4], latent [n][hw][4] in place, unet_in [2n][hw][4].  depth = 0 / 1 / 3 history slots: q_prev[k] = q of k + 1 steps ago
// ([n][hw][4], read where k < n_hist), q_out receives this step's q (it may be the oldest slot: every thread reads its pixel before it writes it).
// Noise (cz != 0 only): element i (NCHW order within the image) of image b is normal_draw(noise_key + b, i); z2 (cz2 != 0 only) the same from noise_key2.
// mask / z0 / e0: all or none.
// rescale (CFG rescale, sdmi_set_guidance_rescale; section 9k), in [0, 1]: 0 launches the elementwise kernels above, as always.  Otherwise e is multiplied by
// f_b = rescale std(ec_b) / std(e_b) + (1 - rescale) before q and x' are formed, the statistics over image b's 4 hw elements (f_b = 1 where std(e_b) = 0 or
// one of them is not finite): sampler_step_rescale_kernel, one workgroup per image, still ONE launch.
hipError_t launch_sampler_step(const float* eps, float* latent, float* unet_in, long long per_half, long long hw, SamplerStep c, float rescale, int depth,
                               const float* const q_prev[3], float* q_out, uint64_t noise_key, uint64_t noise_key2, const float* mask, const float* z0,
                               const float* e0, hipStream_t s);

// ---- bf16-storage variants (k_bf16.hip) ---------------------------------------------------------------
// Launch geometry of the bf16 GroupNorm passes (statistics, apply, the MXFP8 apply of k_fp8.hip): a sample's hw rows are cut into `chunks` ranges, one workgroup
// of cq x R threads each (cq = c / 8 columns of 8 channels, R pixel rows per pass).  Round 4 cut by size alone (32 KB per chunk): at the batches of
// BASELINE.json configs[2..4] that is 2 560 workgroups of 2-3 loads per thread for a 64 x 64 x 320 tensor, and every one pays the fixed tail (LDS reduction, the fp64
// merges; the apply pass re-reads all chunk partials).  target_wgs > 0 (round 5) also bounds the chunks per sample by target_wgs / n: one round of larger chunks.
// Defaults measured in round 5 (profiles/r05d_*): GroupNorm class -21 % (bf16 B = 16), -24 % (MXFP8), images/s +2.0 % / +2.6 %; {0, 1024, 1} is round 4's geometry.
struct GnTune { int target_wgs = 512; int max_threads = 512; int unroll = 2; };   // unroll: independent 16-byte loads in flight per thread (1, 2 or 4)
struct GnGeomH { int cq, R, threads, chunks, rows_per_chunk; };
GnGeomH gn_geom_bf16(int n, int hw, int c, GnTune t);
size_t gn_partials_bytes_bf16(int n, int hw, int c, GnTune t = GnTune());
hipError_t launch_group_norm_bf16(const void* x, void* y, const float* gamma, const float* beta, int n, int hw, int c, int ldx,
                                  int n_group, float eps, bool silu, void* partials, hipStream_t stream, GnTune t = GnTune());
// the statistics half of launch_group_norm_bf16 alone (shared with the fp8-output apply of k_fp8.hip)
hipError_t launch_group_norm_bf16_stats(const void* x, int n, int hw, int c, int ldx, int n_group, void* partials, hipStream_t stream, GnTune t = GnTune());
hipError_t launch_layer_norm_bf16(const void* x, void* y, const float* gamma, const float* beta, int rows, int c, float eps,
                                  hipStream_t stream);
hipError_t launch_geglu_bf16(const void* proj, void* out, long long rows, int hidden, hipStream_t s);
hipError_t launch_f32_to_bf16(const float* src, void* dst, long long n, hipStream_t s);
hipError_t launch_f32_to_bf16_scaled(const float* src, void* dst, long long n, float scale, hipStream_t s);   // dst = bf16(src * scale)
hipError_t launch_scale_f32(float* x, long long n, float scale, hipStream_t s);                                // in place
hipError_t launch_nhwc_bf16_to_nchw_f32(const void* src, float* dst, int n, int c, int h, int w, hipStream_t s);
hipError_t launch_nchw_f32_to_nhwc_bf16(const float* src, void* dst, int n, int c, int h, int w, float scale, hipStream_t s);
hipError_t launch_transpose2d_bf16(const void* src, void* dst, int rows, int cols, int src_ld, hipStream_t s);
hipError_t launch_softmax_rows_f32_to_bf16(const float* x, void* y, int rows, int cols, float scale, hipStream_t s);

// ---- LoRA merge (k_lora.hip) ---------------------------------------------------------------------------------
// W[r][c] = W0[r][c] + sum_t coef_t * sum_j P_t(r, j) Q_t(j, c) over a row-major [R][Cc] fp32 tensor, terms in order, fp32 throughout.
// P_t(r, j) = P[r * p_rs + j * p_js], Q_t(j, c) = Q[j * q_js + c * q_cs] (element strides: the factors are read as the caller stored them,
// whichever way the target's layout turns them).  W may be W0 (every element is read and written by one thread).
// dtype: what the factors are stored as -- 0 F32, 1 F16, 2 BF16 (element strides count elements of that type); a 16-bit factor is widened exactly, on its bit
// pattern (k_widen.hpp), while it is staged.  kind 0: the product above.  kind 1 (LoHa): a second pair P2 / Q2 of the same rank with strides of its own, and the
// term is coef_t * (sum_j P Q) * (sum_j P2 Q2): d1 and d2 each the FMA chain over j from 0, h = d1 * d2 rounded once, w = fma(coef, h, w).
// All terms of one launch share dtype and kind (anything else is hipErrorInvalidValue): the caller splits a mixed list into launches that continue in place,
// which leaves every element's order of operations as it is.
struct LoraTerm {
    const void* P; const void* Q; long long p_rs, p_js, q_js, q_cs; int rank; float coef;
    int dtype, kind;
    const void* P2; const void* Q2; long long p2_rs, p2_js, q2_js, q2_cs;
};
constexpr int kLoraMaxTerms = 8;
struct LoraMerge { const float* W0; float* W; int R, Cc, n_terms; LoraTerm t[kLoraMaxTerms]; };
static_assert(sizeof(LoraMerge) <= 4096, "LoraMerge is passed by value: it must fit the 4 KB kernel-argument segment (lower kLoraMaxTerms)");
hipError_t launch_lora_merge(const LoraMerge& m, hipStream_t s);

// ---- checkpoint tensors (k_unpack.hip) ---------------------------------------------------
// raw: the bytes of a checkpoint tensor on the device, dtype 0 F32 / 1 F16 / 2 BF16 (exact conversions, on the bit patterns); out: fp32.
// transform 0: out[i] = raw[i], i < d0 d1.  1: raw [d0][d1] -> out [d1][d0] (a Linear weight, torch [out, in] -> the dump's [in, out]).
// 2: raw [d0][cin][d1] -> out [d0][pc][d1], pc = cin rounded up to a multiple of 4, the input channels cin .. pc - 1 zero (a conv_in stored with padded input
// channels: the VAE encoder's RGB one, cin = 3; an inpainting UNet's, cin = 9; d1 = kh kw; cin < 32).  One launch.
hipError_t launch_unpack_tensor(const void* raw, int dtype, int transform, long long d0, long long d1, float* out, hipStream_t s, int cin = 3);

// ---- ControlNet (k_control.hip) --------------------------------------------------------------------------------
// rgb [pixels][3] u8 (HWC, sample_image's layout) -> dst [pixels][4] fp32 = v / 255, channel 3 = 0: a ControlNet hint lives in [0, 1], not in [-1, 1]
hipError_t launch_hint_u8_to_nhwc4(const uint8_t* rgb, float* dst, long long pixels, hipStream_t s);
// ONE launch for all residuals of a controlled UNet step: segment i is y[row][0 .. c) += strength * r[row][0 .. c) over `rows` rows; y has a row stride and starts at its
// channel offset (a skip slice of a cats buffer), r is dense.  Every form the destination exists in is written:
//   dt 0: y fp32 (ld elements between rows) and, where y3 != null, the three bf16 planes of the NEW fp32 value by k_split3.hpp's split (ld3 bytes between rows) --
//         bit for bit what a producer of that fp32 value writes;
//   dt 1: y and r bf16, y = rn(float(y) + strength * float(r)).
// c % 32 == 0 (dt 0) / c % 8 == 0 (dt 1); every base and row stride a multiple of 16 bytes.
struct ControlSeg { void* y; const void* r; void* y3; long long rows; int c, ld, ld3; };
constexpr int kControlMaxSegs = 13;
struct ControlAdd { ControlSeg seg[kControlMaxSegs]; int n_seg; int dt; float strength; };
hipError_t launch_control_add(const ControlAdd& a, hipStream_t s);

// ---- FreeU (k_freeu.hip) ------------------------------------------------------------------------------------------
// ONE launch for every filtered skip of a UNet forward: segment i is the tensor y [n][h w][c] inside rows of ld elements (a skip slice of a cats buffer), each
// (sample, channel) plane of it replaced by Fourier_filter(., threshold 1, scale 1 + k): v' = v + k / (h w) x (the sum of its <= 4 lowest Fourier modes; k_freeu.hip).
//   dt 0: y fp32 and, where y3 != null, the three bf16 planes of the NEW value (ld3 bytes between rows), as launch_control_add writes them;
//   dt 1: y bf16, fp32 arithmetic, one round to nearest even.
// c % 32 == 0 (dt 0) / c % 64 == 0 (dt 1); every base and row stride a multiple of 16 bytes; freeu_filter_size_ok(h, w): the row and column tables fit the LDS.
// Sums in a fixed order, no atomics: two runs give the same bits, and a sample's result does not depend on the batch it is in.
struct FreeuSeg { void* y; void* y3; int n, h, w, c, ld, ld3; float k; };
constexpr int kFreeuMaxSegs = 12;
struct FreeuFilter { FreeuSeg seg[kFreeuMaxSegs]; int n_seg; int dt; };
bool freeu_filter_size_ok(int h, int w);
hipError_t launch_freeu_filter(const FreeuFilter& f, hipStream_t s);
// version 2's map: mean[row] = the mean of the cx channels of row `row` of x (rows ld elements apart), fp32; cx % 4 == 0 (dt 0) / % 8 (dt 1)
hipError_t launch_freeu_mean(const void* x, float* mean, long long rows, int cx, int ld, int dt, hipStream_t s);
// y [n][hw][c] (c = cx / 2 channels inside rows of ld elements; the forms and rules of FreeuSeg) *= b (version 1), or *= (b - 1) m^ + 1 with
// m^ = (mean - min) / (max - min) over the sample's hw values of `mean` [n][hw] (version 2; m^ = 0 where max == min)
struct FreeuBackbone { void* y; void* y3; const float* mean; int n, hw, c, ld, ld3, dt, version; float b; };
hipError_t launch_freeu_backbone(const FreeuBackbone& a, hipStream_t s);

// ---- IP-Adapter (k_ipattn.hip) -----------------------------------------------------------------------------------
// O = O_text + s_b softmax(q K_ip^T scale^2) V_ip per batch row b and head: the image half of a decoupled cross attention, added to what the text attention wrote.
//   q        the storage type (bf16 != 0: 2-byte elements), rows ldq and batch rows q_bs elements apart, as AttnParams has them; q_log2 / scale: Engine::attention's pair
//            (a q that arrives in log2 units is used as it is, otherwise the scores are multiplied by scale^2 log2(e)); the softmax runs in exp2
//   k, v     [n][T][C] fp32 dense at every precision, C = n_head d_head, 1 <= T <= kIpMaxTokens
//   o_text/o form 0: fp32 dense [n][nq][C]; form 1 (bf16 q only): bf16 dense; form 2 (fp32 q): the three bf16 planes, ldo3 bytes between rows, read-modify-write.
//            o may be o_text.
//   s        [n] on the device: a row with s_b == 0 keeps O_text's bits
// d_head 40 / 64 / 80 / 160 (ip_attention_head_dim); bases 16-byte aligned, ldq and q_bs multiples of 4 (bf16: 8) elements.  Anything else: hipErrorInvalidValue.
constexpr int kIpMaxTokens = 64;
struct IpAttnParams {
    const void* q; const float* k; const float* v; const void* o_text; void* o; const float* s;
    int n, nq, T, n_head, d_head;
    int ldq; long long q_bs;
    int ldo3;
    int bf16, form, q_log2;
    float scale;
    float sl2;   // set by the launcher
};
bool ip_attention_head_dim(int d);
hipError_t launch_ip_attention(const IpAttnParams& p, hipStream_t s);

}  // namespace sdmi
