// engine.hpp -- host runtime of libsdmi: device pool, weight registry, the static
// UNet / VAE-decoder launch graphs and the DDIM+CFG sampler.
//
// Mirrors the reference's L4/L3 structure:
//   Engine::sample_latent   <- StableDiffusion::sample_latent  (stablediffusion/mod.rs:102-160)
//   Engine::unet_run        <- UNet::forward                   (unet/mod.rs:109-143)
//   Engine::decode          <- Autoencoder::decode_latent      (autoencoder/mod.rs:68-71,205-217)
// but is not a translation: activations are NHWC, weights are pre-packed for the
// implicit-GEMM kernel, cond+uncond run as ONE batch-2n forward, time-embedding
// projections and cross-attention K/V are hoisted out of the step loop, and all
// launches go to one HIP stream with no host synchronisation inside the loop.
#pragma once
#include "ksampler.hpp"
#include <hip/hip_runtime.h>

#include <functional>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/sdmi.h"
#include "error.hpp"
#include "gemm_plan.hpp"
#include "kernels.hpp"

namespace sdmi {

#define SDMI_HIP(expr)                                                                                   \
    do {                                                                                                 \
        hipError_t _e = (expr);                                                                          \
        if (_e != hipSuccess)                                                                            \
            throw ::sdmi::Error(SDMI_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e) + " (" + \
                                                  __FILE__ + ":" + std::to_string(__LINE__) + ")");      \
    } while (0)

// THE launch bookkeeping of Engine's members.  SDMI_LAUNCH_IN(ps, flops, expr): the launch expression is evaluated inside the open ProfScope ps -- between its two
// events -- its status checked, the kernel counted (with its flops).  A scope with a class, bytes and a tag, or two launches under one scope, open the scope
// themselves; SDMI_LAUNCH(expr) is the common case, class PC_OTHER with no bytes and no tag.
#define SDMI_LAUNCH_IN(ps, flops, expr) do { (void)static_cast<const ProfScope&>(ps); SDMI_HIP(expr); count_kernel(flops); } while (0)
#define SDMI_LAUNCH(expr) do { ProfScope ps_o(this, PC_OTHER); SDMI_LAUNCH_IN(ps_o, 0, expr); } while (0)

// ---- device memory pool: host-side first-fit allocator over big slabs -------------
// All work is on one stream, so a block may be reused as soon as it is freed
// (kernel order == program order).  Addresses are deterministic for a given call
// sequence, which keeps launches graph-capturable.
class DevPool {
public:
    ~DevPool();
    void* alloc(size_t bytes);
    void free(void* p);
    size_t reserved() const { return reserved_; }
    size_t high_water() const { return high_; }
    // blocks are numbered in allocation order; free_since(m) returns every block allocated after mark m = serial()
    // (the clean-up of a call that threw half way through a forward pass)
    unsigned long long serial() const { return serial_; }
    size_t free_since(unsigned long long mark);
    // tests (option pool_fill): byte >= 0 overwrites every block alloc hands out, over its whole rounded size, with that byte -- a hipMemsetAsync on `stream`
    // (the stream all of the pool's users work on), enqueued before alloc returns and so in front of the block's first write; -1 = off, nothing is enqueued.
    // note_fill / take_fill_counts: blocks and bytes filled since the counts were last taken (option dump_pool_fills; the engine's own persistent
    // allocations are counted here too).
    void set_stream(hipStream_t s) { stream_ = s; }
    void set_fill(int byte) { fill_ = byte; }
    int fill() const { return fill_; }
    void note_fill(size_t bytes) { ++fill_blocks_; fill_bytes_ += bytes; }
    void take_fill_counts(unsigned long long* blocks, unsigned long long* bytes) { *blocks = fill_blocks_; *bytes = fill_bytes_; fill_blocks_ = fill_bytes_ = 0; }

private:
    struct Block { size_t off, size; };
    struct Slab { char* base; size_t size; std::vector<Block> free_list; };
    std::vector<Slab> slabs_;
    struct Live { int slab; size_t size; unsigned long long serial; };
    std::map<void*, Live> live_;
    size_t reserved_ = 0, in_use_ = 0, high_ = 0;
    unsigned long long serial_ = 0;
    hipStream_t stream_ = nullptr;
    int fill_ = -1;
    unsigned long long fill_blocks_ = 0, fill_bytes_ = 0;
};

// dt: storage type of a device tensor -- 0 = fp32, 1 = bf16 (precision = 1).  `p` is typed float* for
// historical reasons; for dt == 1 it is an opaque pointer to 2-byte elements.
// ld: elements between consecutive pixels (0 = dense, i.e. c).  A channel-slice VIEW of a wider buffer (view = true, never
// freed) is how Tensor::cat (unet/mod.rs:134) is realised without a copy: producers write their slice, the consumer reads the whole.
// p3 (precision = 0 only): the same tensor as three bf16 planes [pixel][ld3 / 192 slices][h, m, l][32] (k_split3.hpp), what k_gemm3p.hip
// reads; written by the tensor's producer.  A tensor may exist as fp32 (p), as planes (p3), or as both.
struct Act {
    float* p = nullptr;
    int n = 0, h = 0, w = 0, c = 0;
    int dt = 0;
    int ld = 0;
    bool view = false;
    void* p3 = nullptr;
    int ld3 = 0;       // bytes between pixels of p3
    size_t bytes3() const { return (size_t)rows() * (size_t)(c / 32) * 192; }
    long long rows() const { return (long long)n * h * w; }
    int stride() const { return ld ? ld : c; }
    size_t bytes() const { return (size_t)rows() * c * (dt ? 2 : 4); }
};

// bt8 / bs8 (precision = 2 only): the same weight as MXFP8 -- e4m3 [cout][Kp] + E8M0 scales [cout][Kp / 32] (k_fp8.hip)
// up3 / up_fresh (fp32 engine, the 3x3 convolution of an Upsample layer; Engine::rebuild_folds): the planes of the four folded 2x2 phase weights [4][cout][4 cin]
// (kernels.hpp, ConvGemm::phases), phase images cout * cin * 24 bytes apart.  up_fresh: they are derived from what the weight entry up_entry holds NOW -- handled exactly
// like SpatialW::fold_fresh: every write or re-pack of the entry clears it (fold_touch), and a layer whose fold is not fresh runs the K = 9 cin launch.
struct ConvW {
    float* bt = nullptr; float* bias = nullptr; int cin = 0, cout = 0, k = 1; int dt = 0; float* bt8 = nullptr; float* bs8 = nullptr;
    void* up3 = nullptr; bool up_fresh = false; int up_entry = -1;
};
// an MXFP8 activation: e4m3 [n][h][w][cp] + E8M0 scales [n][h][w][cp / 32], cp = c rounded up to 128 (zero padded)
struct ActQ {
    void* q = nullptr; void* s = nullptr;
    int n = 0, h = 0, w = 0, c = 0, cp = 0;
    long long rows() const { return (long long)n * h * w; }
};
// bt8 / bs8: MXFP8 copy (precision = 2, option fp8_linear).  fused: the weights packed behind this one as further rows of ONE GEMM, itself included (3: q | k | v)
struct LinW { float* bt = nullptr; float* bias = nullptr; int cin = 0, cout = 0; int dt = 0; float* bt8 = nullptr; float* bs8 = nullptr; int fused = 1; };
struct NormW { float* gamma = nullptr; float* beta = nullptr; int c = 0; float eps = 1e-5f; };  // eps: Q3 default, overridden by the dump's eps file

struct ResW {  // UNet ResBlock (unet/mod.rs:700-734) and VAE ResnetBlock (autoencoder/mod.rs:503-528)
    NormW norm_in; ConvW conv_in; LinW lin_embed; NormW norm_out; ConvW conv_out; ConvW skip;
    bool has_skip = false, has_embed = false;
    int cin = 0, cout = 0, temb_index = -1;
};
struct MhaW { LinW q, k, v, out; };
struct SpatialW {  // SpatialTransformer + TransformerBlock (unet/mod.rs:454-527)
    NormW norm; ConvW proj_in, proj_out; NormW ln1, ln2, ln3; MhaW attn1, attn2; LinW geglu_proj, mlp_lin;
    int c = 0, ctx_index = -1;
    // fp32 engine (option proj_out_fold; Engine::rebuild_folds): fold_bt = proj_out x mlp_lin as a packed Linear weight [c][4c] with its planes, fold_bias =
    // proj_out x mlp_lin.bias [c].  fold_fresh: both are the product of what the three entries fold_entries (mlp_lin weight and bias, proj_out weight) hold NOW;
    // every re-pack or re-set of one of them clears it, and a block whose fold is not fresh runs mlp_lin and proj_out as two launches.
    float* fold_bt = nullptr; float* fold_bias = nullptr;
    bool fold_fresh = false;
    int fold_entries[3] = {-1, -1, -1};
};
enum BlockKind { BK_CONV, BK_DOWN, BK_RES, BK_RES_ST, BK_RES_UP, BK_RES_ST_UP };
struct UBlock { BlockKind kind; int cin, cout; ConvW conv; ResW res; SpatialW st; ConvW up; };
struct VaeAttnW { NormW norm; ConvW q, k, v, proj_out; int c = 0; };
struct DecBlockW { ResW res[3]; ConvW upsampler; bool has_up = false; int cin = 0, cout = 0; };

// CLIP text encoder block (ResidualDecoderAttentionBlock, clip/mod.rs:95-114); q/k/v weights and biases are
// packed for one N = 3C GEMM
struct ClipBlockW { NormW attn_ln, mlp_ln; LinW q, k, v, out, fc1, fc2; };

struct WeightEntry {
    std::string name;
    int kind;  // 0 conv (OIHW), 1 linear ([in,out]), 2 vector, 3 alphas (host)
    int ndim;
    int64_t dims[4];
    float** dst;  // where the device pointer lives (null for alphas)
    int wdt = 0;  // storage type of the packed weight: 0 fp32, 1 bf16
    int group = 0;  // 0: hot path (required); 1: CLIP text encoder, 2: VAE encoder, 3: ControlNet (each optional as a whole)
    float** dst8 = nullptr;   // precision = 2: where the MXFP8 copy of a conv weight and its scales go (null: none)
    float** dsts = nullptr;
    float pre_scale = 1.f;    // the tensor is multiplied by this in fp32 before it is packed (bf16 / MXFP8 query projections: attn_bf16_q_scale)
    bool set = false;
    int fold_st = -1;         // index in st_list_ of the SpatialTransformer whose folded weights (SpatialW::fold_bt) are derived from this entry; -1: none
    int fold_up = -1;         // index in up_list_ of the up-convolution whose phase weights (ConvW::up3) are derived from this entry; -1: none
    float* master = nullptr;  // option keep_masters, kind 0 / 1: the fp32 tensor as the packing kernels read it (reference layout, a conv_in's input channels padded by padded_cin, before pre_scale)
};

// One target of a LoRA adapter (sdmi_lora_add): the factors on the device as the caller stored them -- down [rank][in] / [rank][cin k k],
// up [out][rank] / [cout][rank] -- in one allocation.  dtype: what the factors are stored as (0 F32: sdmi_lora_add; 1 F16 / 2 BF16: the raw bytes of a file,
// sdmi_lora_load_safetensors).  kind 1 (LoHa): a second pair down2 / up2 (hada_w2_b / hada_w2_a next to hada_w1_b / hada_w1_a), the delta their Hadamard product.
struct LoraTarget { int entry; int rank; double alpha; const void* down; const void* up; int dtype = 0; int kind = 0; const void* down2 = nullptr; const void* up2 = nullptr; };

// Per-module scalar / 2-vector files of the dump tree that are not tensors (python/save.py:23-68): `store` != null: the value
// is honoured (a norm's eps); otherwise it must equal `expect` (the hyper-parameters this engine hard-wires).
struct MetaEntry { std::string name; int n; float expect[2]; float* store; };

class Engine {
public:
    explicit Engine(const sdmi_config& cfg);
    ~Engine();
    Engine(const Engine&) = delete;
    Engine& operator=(const Engine&) = delete;

    // weights
    void set_weight(const char* name, const float* data, int ndim, const int64_t* dims);
    void load_weights_dir(const char* dir);
    void load_weights_mpk(const char* path);
    void load_weights_safetensors(const char* path);   // an SD v1.x CompVis checkpoint, converted on the device
    void load_safetensors_groups(const char* path, bool control);   // the route both .safetensors loaders share
    void load_control_safetensors(const char* path);   // a ControlNet in the cldm layout -> weight group 3
    void load_weights_packed(const float* data, size_t n_floats, int groups);
    size_t packed_size(int groups) const;
    void finalize_weights();
    const std::vector<WeightEntry>& entries() const { return entries_; }
    // LoRA adapters merged into the packed weights on the device (include/sdmi.h "LoRA adapters").  Needs option keep_masters.
    sdmi_lora* lora_create();
    void lora_add(sdmi_lora* a, const char* target, const float* down, const float* up, int rank, float alpha);
    void lora_set_scale(sdmi_lora* a, double scale);
    void lora_destroy(sdmi_lora* a);
    // a kohya-ss / LyCORIS file (csrc/lora_keys.hpp): a new adapter at scale 0 holding every module of the halves `which` selects; the whole file is checked against
    // the entries' dims before the first byte is uploaded, and a refused file leaves the context as it was.  *n_skipped: modules passed over (SDMI_LORA_SKIP_UNKNOWN)
    sdmi_lora* lora_load_safetensors(const char* path, int which, int flags, int* n_skipped);
    // THE rule for a convolution's stored input channels as a function of cin alone (padded_cin(e) applies it to an entry); public for the host-only file check
    static int64_t padded_conv_cin(int64_t cin);
    void effective_weight(const char* name, float* out, size_t n);

    // hot path (device pointers, reference layouts)
    // cond_nchw: null for a 4-channel model; [n, cond_ch, h, w] for a conditioned one (unet_in_ch > 4) -- anything else is SDMI_ERR_STATE
    void unet_forward_dev(const float* x_nchw, int t, const float* context, int n, int T, float* out_nchw, const float* cond_nchw = nullptr);
    // Conditioning channels of the UNet input: cond_ch = unet_in_ch - 4 per-call channels next to the latent, stored padded to a multiple of 4 (padded_cin).
    int cond_ch() const { return cfg_.unet_in_ch - 4; }
    int unet_in_padded() const { return (cfg_.unet_in_ch + 3) / 4 * 4; }
    void check_cond(const char* entry, bool given) const;
    // CLIP::forward (clip/mod.rs:56-75): int32 tokens [n, T] on the device -> [n, T, ctx_dim] fp32 (both precisions)
    void clip_forward_dev(const int32_t* tokens, int n, int T, float* out);
    // The extended form (include/sdmi.h "web-UI prompt encoding"): emb_row [n, T] (null: none) takes rows of the embedding bank where
    // >= 0, clip_skip = s runs the first clip_layers - s + 1 blocks before the final LayerNorm, weights [n, T] (null: none) re-weights every chunk in one
    // more launch.  Device pointers; the caller has range-checked tokens and emb_row.  (null, null, 1) issues exactly the launches of the form above.
    void clip_forward_dev(const int32_t* tokens, const int32_t* emb_row, const float* weights, int n, int T, int clip_skip, float* out);
    // Textual-inversion embeddings: a device bank [rows, ctx_dim] fp32, rows numbered over the list in order.  ids = the tokenizer's encoding of the name.
    struct Embedding { std::string name; std::vector<int32_t> ids; int n_vectors; };
    const std::vector<Embedding>& embeddings() const { return embeddings_; }
    int embedding_rows() const { return emb_rows_; }
    // vectors [n_vectors, ctx_dim] fp32 on the host, or on the device (on_device; enqueued on stream_ by the caller).  SDMI_ERR_INVALID: an empty name, no
    // ids, n_vectors outside 1 .. clip_ctx - 2, a name the context already has.  SDMI_ERR_STATE: a context without a text encoder (clip_layers = 0).
    void embedding_add(const std::string& name, const std::vector<int32_t>& ids, const float* vectors, int n_vectors, bool on_device = false);
    void embedding_load_safetensors(const std::string& name, const std::vector<int32_t>& ids, const char* path);
    void embedding_remove(const std::string& name);
    bool clip_ready() const { return clip_ready_; }
    // ControlNet (include/sdmi.h "ControlNet").  control_ready: every tensor of weight group 3 is set (they may arrive before or after
    // finalize_weights, one by one or through a loader).  The control state is sticky, like the sampler: hint_dev is the caller's hint on the device.
    bool has_control() const { return cfg_.control_hint_ch != 0; }
    bool control_ready() const;
    static void check_control(const sdmi_control& c);   // SDMI_ERR_INVALID for what the header lists
    void set_control(const sdmi_control* c);
    bool control_set() const { return ctrl_.set; }
    // step i of the S steps a call runs is controlled iff start * S <= i < end * S, in f64 (THE rule; sdmi_control_step_on)
    static bool control_step_on(double start, double end, int i, int S) { return start * (double)S <= (double)i && (double)i < end * (double)S; }
    // hint_rgb: n x [hint_h, hint_w, 3] u8 on the DEVICE -> out [n, mc, hint_h / 8, hint_w / 8] fp32 NCHW (device)
    void control_hint_embed_dev(const uint8_t* hint_rgb, int n, int hint_h, int hint_w, float* out_nchw);
    // the 13 residuals of the sticky hint (strength ignored) for x [n,4,h,w], t, context [n,T,cd]: NCHW fp32, back to back (device pointers)
    void control_residuals_dev(const float* x_nchw, int t, const float* context, int n, int T, float* out);
    size_t control_residual_elems(int n) const;   // floats control_residuals_dev writes
    // FreeU (include/sdmi.h "FreeU"): sticky, like the control.  freeu_plan is THE block rule (sdmi_freeu_plan; unet_run reads it too):
    // out[5 i ..] = group (0 none, 1: b1 / s1, 2: b2 / s2), cx, cskip, h, w of output block i.  check_freeu: SDMI_ERR_INVALID for what the header lists.
    struct FreeU { int version = 0; float b1 = 1, b2 = 1, s1 = 1, s2 = 1; double start = 0, end = 1; };
    static void freeu_plan(int model_channels, int latent_h, int latent_w, int (&out)[60]);
    static void check_freeu(const FreeU& f);
    void set_freeu(const FreeU& f);   // version 0 clears; SDMI_ERR_UNSUPPORTED for a model whose widths the kernels do not take -- the state in force stays
    const FreeU& freeu() const { return freeu_; }
    // tests (sdmi_op_freeu): parent [n h w][ld] fp32 on the device, columns [0, c) = cat([h, hs]) with cx backbone channels, the others the caller's filler -> the
    // engine's storage type (+ planes at precision 0 where c and ld are multiples of 32), the model's launches, back into parent; parent3 (may be null): the joined
    // planes.  Returns whether the buffer had planes.
    bool op_freeu(float* parent, int n, int c, int h, int w, int ld, int cx, int version, float b, float s, float* parent3);
    // IP-Adapter (include/sdmi.h "IP-Adapter"): image-prompt tokens through a second, decoupled cross attention.  The adapter's weights --
    // image_proj (Linear [T ctx_dim, D] + bias, LayerNorm over ctx_dim) and one to_k_ip / to_v_ip pair [C_i, ctx_dim] per cross attention of the UNet -- live in
    // allocations of their own, packed by the loader's Linear packing for the fp32 GEMM (dt = 0) at every precision.  The setting (tokens, scale, window) is sticky,
    // like the control.  IpTensor: a HOST tensor in the file's layout and element type (0 F32, 1 F16, 2 BF16), widened on the device (k_unpack.hip).
    struct IpTensor { const void* p; int dtype; };
    static constexpr int kIpLayers = 16;
    // THE layer rule: cross attention ctx_index (st_list_ order: input blocks, middle, output blocks) -> the odd index j of "ip_adapter.<j>.to_k_ip.weight"
    // (diffusers' processor order: down, up, mid) and its width C
    static void ip_adapter_layer(int model_channels, int ctx_index, int* j, int* c);
    static std::string ip_adapter_key(int model_channels, int ctx_index, int which);   // which 0: to_k_ip, 1: to_v_ip
    void ip_set_weights(const IpTensor& proj_w, const IpTensor& proj_b, const IpTensor& norm_g, const IpTensor& norm_b, int D, int T, const IpTensor* wk, const IpTensor* wv);
    void ip_load_safetensors(const char* path);   // h94's ip-adapter_sd15 layout; the whole file is checked before anything is uploaded
    static void ip_check_safetensors(const char* path, int model_channels, int ctx_dim, int* D, int* T);   // that check alone: host only
    bool ip_ready() const { return ipw_.ready; }
    int ip_embed_dim() const { return ipw_.D; }
    int ip_tokens_per_image() const { return ipw_.T; }
    void ip_clear();                               // the weights and the setting
    void ip_image_tokens_dev(const float* embeds, int n, float* out);   // embeds [n, D] -> LayerNorm(reshape(Linear(embeds))) [n, T, ctx_dim]; device pointers, fp32
    static void check_ip_adapter(const sdmi_ip_adapter& a);             // the argument errors that need no context
    void check_ip_setting(const sdmi_ip_adapter& a) const;              // every refusal of set_ip_adapter, host only: those, then against this context's adapter
    void set_ip_adapter(const sdmi_ip_adapter* a);                      // null clears the setting (the weights stay)
    void set_ip_adapter_file(const char* path, float scale, double start, double end);   // embeds from the tensor "image_embeds" [n, D] of a .safetensors file
    bool get_ip_adapter(sdmi_ip_adapter* out) const;                    // the setting in force, pointers null; false: none
    // tests (sdmi_op_ip_attention): dense fp32 device tensors q / o_text [n, nq, C], k_ip / v_ip [n, T, C], s [n] -> the storage type of the context (bf16: q scaled as
    // the model's query weights are), the launch the model runs, out [n, nq, C] fp32.  planes (precision 0): O_text as planes, read-modify-write, joined.
    void op_ip_attention(const float* q, const float* k_ip, const float* v_ip, const float* o_text, const float* s, int n, int nq, int T, int n_state, int n_head, bool planes,
                         float* out);
    // the hoisted K_ip / V_ip of the call a forward would run, for tests: out [n_layers] concatenated [nb, T_ip, C_i] blocks, K then V per layer (device)
    size_t ip_kv_elems(int nb) const;
    void ip_kv_dev(int n_images, bool cfg_pair, float* out);
    // Autoencoder::encode_image (autoencoder/mod.rs:60-66): img [n,3,8h,8w] NCHW -> latent mean [n,4,h,w] NCHW (device pointers)
    void encode_image_dev(const float* img_nchw, int n, float* latent_nchw);
    void sample_latent_dev(const float* context, int n, int T, const float* uncond, int Tu, double scale,
                           size_t n_steps, const float* init_latent, float* latent_out, bool out_nhwc = false);   // out_nhwc: see sample_loop
    // img2img (DESIGN.md section "img2img"): the last k of sample_latent's timesteps (sdmi_img2img_timesteps), started from
    // z0 re-noised to t0 with eps = noise [n,4,h,w] or, when null, image i's N(0,1) stream seed + i; mask [n,1,h,w] or null.
    // _latent: z0 [n,4,h,w] NCHW; _image: z0 = 0.18215 * encode_image(rgb / 127.5 - 1), rgb = n x [8h,8w,3] u8 (needs the
    // encoder weights).  latent_out [n,4,h,w].  Device pointers.
    void img2img_latent_dev(const float* context, int n, int T, const float* uncond, int Tu, double scale, size_t n_steps,
                            double strength, const float* z0, const float* mask, const float* noise, uint64_t seed, float* latent_out,
                            const float* cond_nchw = nullptr);   // cond [n, cond_ch, h, w]: only the UNet sees it
    void img2img_image_dev(const float* context, int n, int T, const float* uncond, int Tu, double scale, size_t n_steps,
                           double strength, const uint8_t* init_rgb, const float* mask, const float* noise, uint64_t seed, float* latent_out,
                           const float* cond_nhwc = nullptr);    // cond rows [n][hw][padded_in_ch - 4], as inpaint_cond_nhwc writes them
    // Inpainting checkpoints (unet_in_ch = 9; include/sdmi.h "inpainting"): cond = [latent mask | 0.18215 * encode(masked picture)[:, :4]].  init_rgb n x [8h,8w,3] u8,
    // mask_u8 n x [8h,8w] u8 (>= 128: regenerate), device pointers.  inpaint_cond_dev: cond_nchw [n,5,h,w].  inpaint_image_dev: cond, z0 = 0.18215 * encode(init),
    // the img2img loop (opt->latent_blend: the latent mask as its blend mask), latent_to_image, opt->paste_back: kept pixels copied from init_rgb.
    void check_inpaint(const char* entry) const;
    void inpaint_cond_nhwc(const uint8_t* init_rgb, const uint8_t* mask_u8, int n, float* cond_nhwc, float* lat_mask);
    void inpaint_cond_dev(const uint8_t* init_rgb, const uint8_t* mask_u8, int n, float* cond_nchw);
    void inpaint_image_dev(const float* context, int n, int T, const float* uncond, int Tu, double scale, size_t n_steps, double strength,
                           const uint8_t* init_rgb, const uint8_t* mask_u8, const sdmi_inpaint* opt, const float* noise, uint64_t seed, uint8_t* rgb_out);
    // Hires fix (include/sdmi.h "hires fix"): sample_latent at hr.base_h x base_w, the NHWC latent resampled on the device to the
    // current size, img2img_latent_dev from it (no mask).  init_latent [n,4,base_h,base_w], hires_noise [n,4,H,W] or null, latent_out [n,4,H,W]: device pointers.
    // The size is switched for the first pass and restored on every way out.
    void hires_latent_dev(const float* context, int n, int T, const float* uncond, int Tu, double scale, size_t n_steps, const float* init_latent,
                          const sdmi_hires& hr, const float* hires_noise, float* latent_out);
    static void check_hires(const sdmi_hires* hr);   // the argument errors of sdmi_hires_* that need no context
    // x [n][h*w][4] -> y [n][oh*ow][4] (NHWC4, device) by the tables of sdmi_resize_weights: horizontal pass, then vertical; an unchanged axis is skipped
    void resize_nhwc4(const float* x, int n, int h, int w, int oh, int ow, int mode, int antialias, float* y);
    void op_resize(const float* x_nchw, int n, int h, int w, int oh, int ow, int mode, int antialias, float* out_nchw);
    // k_unpack.hip on its own: raw = a checkpoint tensor's bytes (dtype 0 F32 / 1 F16 / 2 BF16), transform 0 copy / 1 2-D transpose / 2 a conv_in's input channels (dims[1] < 32) padded to the next multiple of 4
    void op_unpack_tensor(const void* raw, int dtype, int ndim, const int64_t* dims, int transform, float* out);
    // sampler choice (sdmi_set_sampler): sticky, read by sample_loop -- every sampling entry point.  The default (kind 0,
    // eta 0) is the reference's DDIM on its own launches.  check_sampler throws SDMI_ERR_INVALID for what the header lists; null = the default.
    static void check_sampler(const sdmi_sampler& s);
    void set_sampler(const sdmi_sampler* s);
    const sdmi_sampler& sampler() const { return sampler_; }
    // sigma-schedule samplers (sdmi_set_ksampler; ksampler.hpp): the second sticky state, read wherever sampler_ is.  The two exclude each
    // other: setting one resets the other (set_sampler, null included, clears this one).  set_image_base: the sharded path's per-shard key offset, on whichever is set.
    void set_ksampler(const sdmi_ksampler* k);
    bool ksampler_set() const { return kset_; }
    const sdmi_ksampler& ksampler() const { return ksampler_; }
    void set_image_base(int64_t base) { sampler_.image_base = base; ksampler_.image_base = base; }
    const std::vector<float>& alphas() const { return alphas_; }
    void op_timestep_embedding_f(double t, int dim, float* out);
    void decode_latent_dev(const float* latent_nchw, int n, float in_scale, float* img_nchw, uint8_t* rgb_u8);
    // kv_len_host: null, or a HOST array [n] of per-sample key counts (1 .. nk; the CFG batch's cross attention, Engine::attention's kv_len)
    void qkv_attention_dev(const float* q, const float* k, const float* v, const float* mask, int mask_ld, int n,
                           int nq, int nk, int n_state, int n_head, float* out, const int* kv_len_host = nullptr);
    // tests (sdmi_op_qkv_attention_view): qkv_attention_dev with q, k, v scattered into parents [n][rows][ld] full of view.in_fill and the result written into
    // a slice of parent [n][out_rows][out_ld] (fp32 on the device, prefilled by the caller, returned whole) -- attention() sees the strides the model gives it
    void op_qkv_attention_view(const float* q, const float* k, const float* v, const float* mask, int mask_ld, const int* kv_len_host, int n, int nq, int nk,
                               int n_state, int n_head, const sdmi_attn_view& view, float* parent);
    // every host-side check of that call (check_attention_view, attn_plan.hpp, in the storage type the call would run in): allocates and launches nothing
    void check_qkv_attention_view(const sdmi_attn_view& view, bool has_mask, int mask_ld, const int* kv_len_host, int n, int nq, int nk, int n_state, int n_head) const;

    // operator-level (device pointers, reference layouts)
    // (defined in engine_ops.cpp, with every other op_* / bench_* member and qkv_attention_dev)
    void op_group_norm(const float* x, const float* gamma, const float* beta, int n, int c, int h, int w, int groups,
                       float eps, bool silu, float* out);
    void op_group_norm_fp8(const float* x, const float* gamma, const float* beta, int n, int c, int h, int w, int groups, float eps,
                           bool silu, float* out);
    void op_layer_norm(const float* x, const float* gamma, const float* beta, int rows, int c, float eps, float* out);
    // the time-embedding row and residual of an operator-level conv2d / Linear given by the caller (tests: sdmi_op_conv2d_epilogue / sdmi_op_linear_epilogue), as
    // HOST arrays: temb [n][cout] ([cout] with temb_stride 0: one row for the batch), resid of the output's shape (NCHW; [rows][cout] for Linear).  Staged by
    // stage_epi in the layout the model's launches read: temb rows temb_stride floats apart, the residual as NHWC rows resid_ld (0: cout) elements apart
    // in the output's storage type
    struct EpiOps { const float* temb = nullptr; int temb_stride = 0; const float* resid = nullptr; int resid_ld = 0; };
    void op_conv2d(const float* x, const float* w, const float* bias, int n, int cin, int h, int wd, int cout, int k,
                   int stride, int pad, int ups, float* out, const EpiOps* epi = nullptr);
    void op_linear(const float* x, const float* w, const float* bias, int rows, int cin, int cout, float* out, const EpiOps* epi = nullptr);
    // the tail of a ResBlock with a shortcut (tests: sdmi_op_conv2d_pair): conv3x3(h, w_out) + b_out + conv1x1(x, w_skip) + b_skip; out3: the planes output, joined
    void op_conv2d_pair(const float* x, const float* h, const float* w_skip, const float* b_skip, const float* w_out, const float* b_out, int n, int cin_x, int cout,
                        int hh, int wd, float* out, float* out3);
    // tests (sdmi_op_linear_pair): out [rows][cout] = u [rows][k_main] x w_main [k_main][cout] + b_main + h [rows][k_aux] x w_aux [k_aux][cout] + b_aux + resid, the
    // inputs as planes; option proj_out_fold = 1: linear_pair (an error where it declines), 0: two launches.  resid_ld / out_ld (0: cout): the row strides the engine
    // keeps the residual and the result at; out (may be null: planes only) / out3 (may be null): the fp32 result / the plane output of the same launch, joined
    void op_linear_pair(const float* u, const float* h, const float* w_main, const float* b_main, const float* w_aux, const float* b_aux, const float* resid, int resid_ld,
                        int rows, int k_main, int k_aux, int cout, int out_ld, float* out, float* out3);
    // tests (sdmi_op_linear_fold): w_lin [k_main][cmid] / b_lin [cmid] (a Linear in the reference layout), w_proj [cout][cmid] (a 1x1 convolution) -> wf [cout][k_main], bf [cout]
    void op_linear_fold(const float* w_lin, const float* b_lin, const float* w_proj, int k_main, int cmid, int cout, float* wf, float* bf);
    void op_geglu(const float* proj, int rows, int hidden, float* out);
    // the same operators on channel-slice VIEWS, built with slice() on real Acts as unet_run builds the halves of a Tensor::cat (tests: sdmi_op_*_view).
    // xp: the input's parent [rows][in_ld] fp32 NHWC on the device (the slice's columns hold x, the others the caller's filler); yp: the output's
    // parent [rows][out_ld] fp32 NHWC, prefilled by the caller and returned whole; yp3 (may be null): the joined plane copy when the parent exists both
    // as fp32 and as planes.  Parents take the storage type of the route (bf16 at precision >= 1; v.in_planes / v.out_planes at precision 0).
    static void check_view(const sdmi_op_view& v, int cin, int cout);
    // the output size of conv(): k x k, pad, stride over the input upsampled 2x when ups
    static void conv_out_hw(int h, int w, int k, int stride, int pad, int ups, int* ho, int* wo) {
        *ho = ((h << ups) + 2 * pad - k) / stride + 1;
        *wo = ((w << ups) + 2 * pad - k) / stride + 1;
    }
    void op_conv2d_view(const float* xp, const float* w, const float* bias, int n, int cin, int h, int wd, int cout, int k, int stride, int pad, int ups,
                        const sdmi_op_view& v, const EpiOps* epi, float* yp, float* yp3);
    void op_linear_view(const float* x, const float* w, const float* bias, int rows, int cin, int cout, const sdmi_op_view& v, const EpiOps* epi, float* yp);
    // form 0: the precision's GroupNorm (fp32 / bf16), 1: planes out (precision 0), 2: MXFP8 out, dequantised (precision 2); out [n,c,h,w]
    void op_group_norm_view(const float* xp, const float* gamma, const float* beta, int n, int c, int h, int w, int groups, float eps, bool silu,
                            const sdmi_op_view& v, int form, float* out);
    // a block boundary: conv3x3(x, w_skip) -> channels [cx, cx + cskip), conv3x3(x, w_x) -> channels [0, cx), GroupNorm(+SiLU) over all of them.
    // dense = false: both convolutions write slices of one buffer (as unet_run); true: dense results joined by launch_concat_channels.  out [n,cx+cskip,h,w]
    void op_cat_chain(const float* x, const float* w_x, const float* b_x, const float* w_skip, const float* b_skip, const float* gamma, const float* beta,
                      int n, int cin, int h, int wd, int cx, int cskip, float eps, bool silu, bool dense, float* out);
    void op_geglu_forward(const float* x, const float* wt, const float* bias, int rows, int cin, int hidden, float* out);
    void op_timestep_embedding(int t, int dim, float* out);
    double bench_conv(int n, int cin, int h, int w, int cout, int k, int stride, int ups, int tile_cfg, int splitk,
                      int iters);

    double bench_attention(int n, int nq, int nk, int n_state, int n_head, int iters);
    void set_prediction(int kind);   // 0 eps, 1 v
    // CFG rescale and zero-terminal-SNR schedules, sticky like the prediction kind.  set_guidance_rescale: phi in [0, 1], 0 = off (SDMI_ERR_INVALID
    // otherwise, the state kept).  set_zero_snr: sample on the loaded table rescaled to a_T = 0 (rescale_zero_snr); off restores the loaded one bit for bit.
    void set_guidance_rescale(double phi);
    double guidance_rescale() const { return rescale_; }
    void set_zero_snr(bool on);
    static void rescale_zero_snr(const float* in, float* out, int n);   // the paper's Algorithm 1 on sqrt(a), f64; throws SDMI_ERR_INVALID
    // the sampling entries' refusals on a table that holds a = 0, before any launch: eps does not determine x0 there (INVALID), a k-sampler's sigma_max is infinite (UNSUPPORTED)
    void check_schedule(const char* entry) const;
    // one launch_sampler_step on NCHW device tensors (sdmi_op_sampler_step): eps [2n], latent [n], q_hist [n_hist][n], mask [n][hw], z0 / e0 [n]
    void op_sampler_step(const float* eps, const float* latent, int n, int h, int w, const SamplerStep& c, float rescale, int depth, const float* q_hist,
                         uint64_t noise_key, uint64_t noise_key2, const float* mask, const float* z0, const float* e0, float* latent_out, float* q_out);
    AttnPlan attention_plan(int n, int n_head, int nq, int nk, int d_head, bool has_mask) const;   // what qkv_attention_dev would run now; host only
    void set_option(const std::string& key, const std::string& value);
    void sync();
    // Every C-ABI entry point runs inside a Call: the constructor orders the engine's stream behind the caller's work
    // (dev_inputs: the arguments are device buffers produced on another stream), finish() waits for the results and
    // records the call statistics, and a Call destroyed by an exception returns every pool block the call allocated.
    void begin_call(bool dev_inputs = false);
    void end_call();
    void abort_call() noexcept;
    struct Call {
        Engine& e; bool done = false;
        Call(Engine& e_, bool dev_inputs = false) : e(e_) { e.begin_call(dev_inputs); }
        void finish() { e.end_call(); done = true; }
        ~Call() { if (!done) e.abort_call(); }
        Call(const Call&) = delete;
        Call& operator=(const Call&) = delete;
    };
    // the stream the caller's device buffers are produced / consumed on (sdmi_set_stream); has_user_stream_ false:
    // *_dev entry points synchronise the whole device on entry instead
    void set_user_stream(hipStream_t s, bool enable) { user_stream_ = s; has_user_stream_ = enable; }
    double last_ms = 0;
    long long last_kernels = 0;
    double last_flops = 0;

    hipStream_t stream() const { return stream_; }
    DevPool& pool() { return pool_; }
    const sdmi_config& config() const { return cfg_; }
    // The CURRENT latent size (sdmi_set_latent_size): cfg_.latent_h / latent_w are its initial value.  Every entry point reads it
    // at call time and nothing is cached per size.  check_latent_size: sdmi_create's rule (positive multiples of 8), SDMI_ERR_INVALID otherwise.
    int latent_h() const { return lat_h_; }
    int latent_w() const { return lat_w_; }
    static void check_latent_size(int h, int w);
    void set_latent_size(int h, int w) { check_latent_size(h, w); lat_h_ = h; lat_w_ = w; }

    // RAII helper for pool scratch
    struct Buf {
        Engine* e; void* p;
        Buf(Engine* e_, size_t bytes) : e(e_), p(e_->pool_.alloc(bytes)) {}
        ~Buf() { if (p) e->pool_.free(p); }
        Buf(const Buf&) = delete;
        Buf& operator=(const Buf&) = delete;
        float* f() const { return reinterpret_cast<float*>(p); }
    };
    // host [rows][c] (nchw_hw > 0: NCHW with that many pixels per sample, row r = pixel r of the flattened batch) -> a new device buffer of rows x ld
    // elements, fp32 (dt 0) or bf16 rounded to nearest even (dt 1), the ld - c padding columns NaN; option op_misalign starts it one element past an
    // aligned address.  Returns the first element.
    const float* stage_epi(std::unique_ptr<Buf>& b, const float* host, long long rows, int c, int ld, int dt, long long nchw_hw = 0);

private:
    void destroy() noexcept;
    // batched weight staging (engine.cpp "weights")
    struct Stager;
    std::unique_ptr<Stager> stager_;
    static constexpr int kGroups = 4;
    bool arena_done_[kGroups] = {false, false, false, false};
    // precision = 0: every packed fp32 weight also exists as three bf16 planes (k_gemm3x.hip) in a parallel arena; the planes of
    // the weight at byte offset o of arena g start at offset 3 o / 2 of split arena g (6 bytes per weight instead of 4), so
    // weights that are adjacent rows of one GEMM (q | k | v) stay adjacent
    char* arena_base_[kGroups] = {nullptr, nullptr, nullptr, nullptr};
    size_t arena_bytes_[kGroups] = {0, 0, 0, 0};
    char* split_base_[kGroups] = {nullptr, nullptr, nullptr, nullptr};
    struct SplitRegion { char* base; size_t bytes; char* planes; };
    std::vector<SplitRegion> split_regions_;
    const void* split_planes(const float* bt) const;
    // weight planes of a tensor with `rows` rows: 16-row fragment groups (kernels.hpp, ConvGemm::b3_grouped) whenever the rows fill whole groups.  Packer and launches
    // apply the same rule; sub-views of a packed tensor (q | k | v) start and end on multiples of 16 rows.
    bool b3_grouped(long long rows) const { return opt_b3_grouped_ != 0 && rows % 16 == 0; }
    // operator-level calls (op_conv2d, op_linear, bench_conv ...) pack their weight into a pool buffer: this gives it planes for
    // the duration of the call, so that those calls run the kernels the model runs
    struct TempSplit {
        Engine* e; const float* bt; void* planes = nullptr;
        TempSplit(Engine* e_, const float* bt_, long long rows, long long K);
        ~TempSplit();
        TempSplit(const TempSplit&) = delete;
        TempSplit& operator=(const TempSplit&) = delete;
    };
    const float* temp_split_bt_[2] = {nullptr, nullptr};
    const void* temp_split_planes_[2] = {nullptr, nullptr};
    char* stage_reserve(size_t bytes, size_t* offset, int* half);
    void stage_commit(WeightEntry& e, size_t offset, int half);
    // THE packing routine, shared by the loader (stage_commit) and a LoRA re-merge (lora_repack): the device fp32 tensor `stage` (reference layout, the padded
    // element count of stage_elems; clobbered by pre_scale) -> the entry's packed slot, its MXFP8 copy and its bf16 planes.  Enqueues on stream_.
    void pack_entry(WeightEntry& e, float* stage);
    static size_t stage_elems(const WeightEntry& e);
    static int padded_cin(const WeightEntry& e);   // a conv weight's stored input channels (engine.cpp: the one rule)
    // option keep_masters: fp32 master copies of every conv / Linear tensor, one arena per weight group laid out like the packed one (ensure_arena)
    int opt_keep_masters_ = 0;
    std::vector<sdmi_lora*> loras_;      // in creation order: the order the deltas of a shared target are added in
    bool lora_owned(const sdmi_lora* a) const;
    void lora_refuse_bulk_load(const char* what) const;          // SDMI_ERR_STATE while any adapter has a non-zero scale
    bool lora_active_on(int entry) const;                       // an adapter with a non-zero scale holds this entry
    void lora_compose(int entry, float* dst);                   // dst (stage_elems floats, device) = W0, or W0 + the active adapters' deltas (launch_lora_merge)
    void lora_repack(int entry);                                // lora_compose into a pool buffer + pack_entry
    void upload_weight(WeightEntry& e, const float* data);
    void stager_release();
    void ensure_arena(int group);
    bool set_meta(const std::string& name, const float* values, size_t n);
    void add_meta(const std::string& name, int n, float e0, float e1, float* store);
    std::vector<MetaEntry> meta_;
    std::map<std::string, int> meta_index_;
    // model definition
    void add_entry(const std::string& name, int kind, std::initializer_list<int64_t> dims, float** dst, int wdt = 0);
    int cur_group_ = 0;  // weight group add_entry assigns (build_model switches it to 1 for the CLIP section)
    void build_model();

    // primitive ops on device activations (NHWC)
    Act new_act(int n, int h, int w, int c, int dt = -1);  // dt -1: the engine's activation type
    // fp32 engines: what = 1 fp32 only, 2 planes only, 3 both (c % 32 == 0 for planes)
    Act new_act3(int n, int h, int w, int c, int what);
    void release(Act& a);
    // [rows][c] tensors (what the Linear layers, LayerNorm, GEGLU and attention work on): n = h = 1, w = rows.  new_rows: what = 1 storage type dt (-1: the engine's),
    // 2 planes only, 3 fp32 + planes (new_act3's rule).  rows_view: a buffer somebody else owns (release() leaves it alone) -- p (may be null) rows ld elements apart
    // (0: dense) and / or p3, dense planes.  top: the first `rows` rows of a dense tensor, a view.
    Act new_rows(long long rows, int c, int what = 1, int dt = -1) { return (what & 2) ? new_act3(1, 1, (int)rows, c, what) : new_act(1, 1, (int)rows, c, dt); }
    static Act rows_view(const void* p, long long rows, int c, int dt, int ld = 0, void* p3 = nullptr) {
        Act a; a.p = (float*)const_cast<void*>(p); a.n = 1; a.h = 1; a.w = (int)rows; a.c = c; a.dt = dt; a.ld = ld; a.view = true; a.p3 = p3; a.ld3 = (c / 32) * 192; return a;
    }
    static Act top(const Act& a, long long rows) { if (rows > a.rows()) throw Error(SDMI_ERR_STATE, "top: more rows than the tensor has"); return rows_view(a.p, rows, a.c, a.dt, a.ld, a.p3); }
    // pad_br: zero padding on the bottom / right only (PaddingCfg::new(0, 1, 0, 1), the VAE encoder's downsampler)
    void probe_report(void* pb_dev, size_t max_blocks, int n, int cin, int h, int w, int cout, int k, int tile_cfg, int splitk);
    void conv(const ConvW& w, const Act& x, Act& y, int stride, int ups, const float* rowvec, int rowvec_stride,
              const Act* resid, bool pad_br = false);
    // conv3x3(h, w_out) + conv1x1(x, w_skip) + both biases as one split-K plane launch (ConvGemm::z_aux) + reduce; false: not launched (see engine.cpp)
    bool conv_pair(const ConvW& w_out, const Act& h, const ConvW& w_skip, const Act& x, Act& y);
    // conv_pair for a Linear main problem: C / C3 [rows][cout] = u x bt^T + bias + h x bt_aux^T + bias_aux + resid as one split-K plane launch + reduce.  u3 / h3: the
    // two activation matrices as planes (pixels u3_ld / h3_ld bytes apart), bt [cout][k_main] / bt_aux [cout][k_aux] packed weights with planes, resid (may be null)
    // rows ldr floats apart, C and / or C3 with their own strides.  false: not launched, in the situations conv_pair declines in.  plan_only: nothing is launched
    // either way; true = a call with these arguments would launch.
    struct LinearPair {
        const void* u3; int u3_ld; const float* bt; const float* bias; int k_main;
        const void* h3; int h3_ld; const float* bt_aux; const float* bias_aux; int k_aux;
        int rows, cout; const float* resid; int ldr; float* C; int ldc; void* C3; int ldc3;
        bool measured_only = false;   // decline a shape without a row in the pairs table (option proj_out_fold = 2)
    };
    bool linear_pair(const LinearPair& a, bool plan_only = false);
    // wf [cout][k_main] = proj_bt [cout][cmid] x lin_bt [cmid][k_main], bf [cout] = proj_bt x lin_bias (zeros without one): fp64 accumulation, rounded once
    void fold_weights(const float* proj_bt, const float* lin_bt, const float* lin_bias, int cout, int cmid, int k_main, float* wf, float* bf);
    void rebuild_folds();                        // every SpatialW whose fold is not fresh and whose three entries are set (precision 0 only); enqueues on stream_
    void fold_touch(const WeightEntry& e) {
        if (e.fold_st >= 0) st_list_[(size_t)e.fold_st]->fold_fresh = false;
        if (e.fold_up >= 0) up_list_[(size_t)e.fold_up]->up_fresh = false;
    }
    std::vector<ConvW*> up_list_;                // the up-convolutions (UNet Upsample, VAE decoder upsampler), in model order
    // option ups_phase (fp32 engine): conv3x3(nearest_2x(x)) as four folded 2x2 phase convolutions in one plane launch.  0 = never (the A/B arm), 1 = wherever supported
    // (tests), 2 = where the planner takes it (plan_ups_phase)
    int opt_ups_phase_ = 2;
    // planes of the four phase weights of the packed 3x3 weight bt [cout][9 cin] -> up3 (cout * cin * 96 bytes): launch_fold_ups_phase_f64 into a pool buffer, then
    // launch_pack_split3 per the layout b3_grouped(cout) names.  Enqueues on stream_.
    void build_up_fold(const float* bt, void* up3, int cout, int cin);
    bool up_fold_supported(int cin, int cout) const;
    // the phase launch of an up-convolution (+ its reduce); false: not launched, the caller runs the K = 9 cin launch (see engine.cpp)
    bool conv_ups_phase(const ConvW& w, const Act& x, Act& y, const float* rowvec, const Act* resid);
    // operator-level calls: the phase weights of a temporary 3x3 weight, for the duration of the call (like TempSplit)
    struct TempUpFold {
        Engine* e; void* up3 = nullptr;
        TempUpFold(Engine* e_, ConvW& w, int stride, int ups);
        ~TempUpFold();
        TempUpFold(const TempUpFold&) = delete;
        TempUpFold& operator=(const TempUpFold&) = delete;
    };
    static Act slice(const Act& parent, int c_off, int c);   // channel-slice view
    // operator-level entry points (engine_ops.cpp): what they share.  A new storage form is taught to the route, OpConvW / OpLinW and OpParent once.
    // OpRoute: the kernels an operator-level conv2d / Linear of the shape runs on this context -- q8: MXFP8 (input quantised, MXFP8 weight, bf16 output);
    // otherwise the storage types of the packed weight, the input and the output (0 fp32, 1 bf16)
    struct OpRoute { bool q8; int wdt, xdt, ydt; };
    // f32: option op_f32 (the dense conv entry only); refuse: throw where the context has no kernel for the shape (bench_conv leaves that to conv())
    OpRoute conv_route(int cin, int cout, int k, int stride, int ups, bool f32 = false, bool refuse = true) const;
    OpRoute lin_route(int cin, int cout) const;
    struct OpConvW;    // a reference-layout conv weight packed for a route, with its planes and phase weights, for the duration of a call
    struct OpLinW;     // ... a Linear weight
    struct OpParent;   // the parent of a channel-slice view in the route's storage type, filled from / given back to the caller's fp32 NHWC image
    Act act_from_nchw(const float* x, int n, int c, int h, int w, int dt);      // x [n,c,h,w] fp32 -> a new NHWC activation of type dt
    void act_to_nchw(const Act& a, float* out);                                 // a dense NHWC activation (fp32 or bf16) -> out [n,c,h,w] fp32
    void rows_to_f32(const void* bf16_rows, float* out, long long rows, int c);   // dense bf16 rows -> fp32
    const int* kv_len_to_dev(std::unique_ptr<Buf>& b, const int* kv_len_host, int n);   // null without per-sample key counts
    // q / k / v (dense fp32) -> bf16 in bufs[3], q in Engine::attention's convention (q_prescaled); the pointers are redirected to the copies
    void qkv_to_bf16(const float*& q, const float*& k, const float*& v, long long qe, long long ke, int dh, std::unique_ptr<Buf> (&bufs)[3]);
    // what op_conv2d and op_conv2d_view share once their input xs and output ys stand: temb and residual staged (self_resid: option op_resid's x), the weight packed
    // for the route, an MXFP8 input quantised from xs (fp32: the dense entry; bf16: a view's slice), then conv_fp8 or conv
    void op_conv_run(const OpRoute& r, const float* wt, const float* bias, int k, int stride, int ups, const EpiOps* epi, const Act& xs, Act& ys, const Act* self_resid);
    // ... op_linear and op_linear_view: x [rows][cin] dense fp32 -> C (rows ldc elements apart, the route's output type) on the MXFP8, bf16 or fp32 kernels; resid: staged
    // by the caller (may be null); self_resid (option op_resid): without one, the input in the route's storage type is the residual of the bf16 / fp32 kernels
    void op_linear_run(const OpRoute& r, const float* x, const float* wt, const float* bias, int rows, int cin, int cout, float* C, int ldc, const float* resid, int ldr,
                       bool self_resid);
    // y [rows][y.c] = x W^T + bias (+ resid).  Everything comes from the structs: in_features, bias and packing from w; the number of weight rows from y.c, which
    // must be w.cout or, for a weight with others packed behind it (q | k | v), w.fused * w.cout; rows and the storage type from x (y and resid agree); the
    // plane forms from x.p3 (input; x.p may then be null) and y.p3 (written next to, or instead of, y.p); the output's and the residual's row strides from their ld.
    // A weight that is no model entry is a LinW built in place.
    void linear(const LinW& w, const Act& x, const Act& y, const Act* resid = nullptr);
    void linear(const LinW& w, const ActQ& x, const Act& y, const Act* resid = nullptr);   // ... on MXFP8 operands (w.bt8), bf16 out
    // fp32 engine, option gemm_planes: does the GEMM cin -> cout take its activations as planes (k_gemm3p.hip)?
    bool plane_gemm(int cin, int cout) const { return !bf16_ && gopt_.gemm_planes != 0 && gopt_.gemm_f32s != 0 && cin % 32 == 0 && cout >= 32; }
    void launch_gemm(ConvGemm& p, int in_dt, int force_cfg = -1, int force_splits = 0);   // plan (gemm_plan.hpp), temporary plane / fp32 buffers, run_gemm
    GemmPlanIn gemm_plan_in(const ConvGemm& p, int in_dt, int force_cfg, int force_splits) const;
    using GemmLauncher = hipError_t (*)(const ConvGemm&, int, hipStream_t);
    struct GemmRun { GemmLauncher launch; int index; const char* what; int cfg; int pc; bool bf16_reduce, reduce_tag; double flops, bytes; };
    void record_choice(const ConvGemm& p, const char* kind, int cfg, const char* note);
    void run_gemm(ConvGemm& p, const GemmRun& r);   // kernel (+ slabs and split-K reduce), profiled and counted; shared with launch_fp8
    int edt() const { return bf16_ ? 1 : 0; }
    size_t esz() const { return bf16_ ? 2 : 4; }
    // element-wise pointer advance on an activation of type dt
    static float* adv(const float* p, long long elems, int dt) { return (float*)((char*)const_cast<float*>(p) + elems * (dt ? 2 : 4)); }
    void group_norm(const NormW& w, const Act& x, Act& y, bool silu);
    // precision = 2: GroupNorm(+SiLU) writing MXFP8, and the 3x3 convolution that consumes it (k_fp8.hip)
    ActQ new_actq(int n, int h, int w, int c);
    void release(ActQ& a);
    void group_norm_fp8(const NormW& w, const Act& x, ActQ& y, bool silu);
    // stride / ups as conv(); 3x3 (pad 1) or 1x1 (pad 0) -- whatever was packed as MXFP8 (ConvW::bt8)
    void conv_fp8(const ConvW& w, const ActQ& x, Act& y, const float* rowvec, const Act* resid, int stride = 1, int ups = 0, int rowvec_stride = 0);
    bool use_fp8(const ConvW& w, const Act& x) const;
    // option fp8_linear: the layers beyond the ResBlock 3x3 convolutions -- Linear layers, 1x1 / up / down convolutions
    bool use_fp8_wide(const float* bt8, long long rows) const { return fp8_ && opt_fp8_convs_ && opt_fp8_linear_ && bt8 && rows >= opt_fp8_min_rows_; }
    void set_resid_acc(ConvGemm& p, bool eligible, bool resid_ok) const;          // ConvGemm::resid_acc of a launch (option resid_acc, strides, base alignment)
    void launch_fp8(ConvGemm& p, double flops);                                   // tile / split-K choice + launch (+ reduce) of conv_gemm_fp8x_kernel
    void conv_raw(const ConvW& w, const Act& x, Act& y, int stride, int ups);     // conv() or, at precision = 2, quantize() + conv_fp8()
    void quantize(const Act& x, ActQ& y);                                         // bf16 activation -> MXFP8 (quantize_bf16_fp8_kernel)
    void layer_norm(const NormW& w, const Act& x, ActQ& y);                        // ... writing MXFP8
    ActQ new_rowsq(long long rows, int c) { return new_actq(1, 1, (int)rows, c); }
    void layer_norm(const NormW& w, const Act& x, const Act& y);   // dense rows of x's storage type; y.p3: the output as planes (y.p must then be null)
    // GEGLU::forward (unet/mod.rs:579-591): y[rows, hidden] = (x W + b)[:, :hidden] * gelu((x W + b)[:, hidden:]), hidden = w.cout / 2 = y.c; w.bt is the
    // packed [2 hidden][cin] weight.  Fused into a large-tile GEMM when possible, else linear() into a scratch tensor + gate kernel.  Plane forms as linear().
    void gemm_geglu(const LinW& w, const Act& x, const Act& y);
    // qkv_attention's arguments, filled by field name.  An operand is rows ld elements apart and samples bs elements apart; o.p may be null where o3 (the output
    // as planes, fp32 kernels) is given.  kv_len_dev / kv_len_host: the same per-sample key counts on both sides, or both null.  dt -1: the engine's storage type.
    struct AttnOperand { const float* p = nullptr; int ld = 0; long long bs = 0; };
    struct Attn {
        AttnOperand q, k, v, o;
        int n = 0, nq = 0, nk = 0, n_head = 0, d_head = 0;
        const int* kv_len_dev = nullptr; const int* kv_len_host = nullptr; const float* mask = nullptr; int mask_ld = 0;
        void* o3 = nullptr; int dt = -1; bool q_log2 = false;   // q_log2: see q_prescaled
    };
    // a dense-or-strided [n * rows][c] tensor as an operand, `rows` rows per sample; the three operands of a packed [n * rows][3 c] q | k | v buffer
    static AttnOperand attn_rows(const Act& a, long long rows) { return AttnOperand{a.p, a.stride(), rows * a.stride()}; }
    static void attn_packed_qkv(const Act& qkv, long long rows, Attn& a) {
        a.q = a.k = a.v = attn_rows(qkv, rows);
        a.k.p = adv(qkv.p, qkv.c / 3, qkv.dt); a.v.p = adv(qkv.p, 2 * (qkv.c / 3), qkv.dt);
    }
    void attention(const Attn& a);
    // ONE rule for "the query arrives multiplied by attn_bf16_q_scale(d_head)": bf16 storage at the head dims the fused bf16 kernel serves.  The weight loader
    // folds the factor into the query projection by it, the fp32 -> bf16 conversions of the operator entry points apply it by it, and every attention() call
    // states it as Attn::q_log2 -- the kernel launcher refuses a bf16 call that does not state it.
    // d_head = 64 follows option attn_d64 (0: as before k_attn_bf16.hip had a d = 64 instance -- plain q on k_attn.hip).
    bool q_prescaled(int dt, int d_head) const { return dt != 0 && attn_bf16_head_dim(d_head, aopt_.attn_d64); }
    // heads of a UNet attention at channel width c: n_head of them (SD v1), or c / 64 of width 64 (variant = 1, SD 2.x)
    int unet_heads(int c) const { return cfg_.variant == 1 ? c / 64 : cfg_.n_head; }

    // composite blocks
    void res_block(const ResW& w, const Act& x, Act& y, int step);
    void spatial_transformer(const SpatialW& w, const Act& x, Act& y);
    void vae_attn(const VaeAttnW& w, const Act& x, Act& y);

    // UNet driver
    // n_images (a controlled call): the images of the call, nb = n_images or 2 n_images (a CFG batch); window: false = every step is controlled (unet_forward)
    void unet_prepare(const float* ctx_packed, int nb, int t_max, const int* kv_len_host, const std::vector<int>& ts, int n_images = 0, bool window = true,
                      bool force_control = false);   // force_control: a controlled prepare whatever the strength (control_residuals_dev)
    // the k-samplers' form: one row per UNet EVALUATION at the fractional times tf (f64 narrowed once); eval_step[i] = the step of the call
    // evaluation i belongs to, of call_steps -- what the ControlNet window counts, so that both evaluations of a step agree
    void unet_prepare(const float* ctx_packed, int nb, int t_max, const int* kv_len_host, const std::vector<double>& tf, const std::vector<int>& eval_step, int call_steps,
                      int n_images);
    void unet_prepare_rows(const float* ctx_packed, int nb, int t_max, const int* kv_len_host, const int* ti, const float* tf, int S, int n_images, bool window,
                           bool force_control);
    void run_block(const UBlock& b, const Act& in, Act& y, int step);   // one UNet block; its last kernel writes y (dense or a channel slice)
    // ControlNet: the hint embedding [n][h][w][mc] fp32 of n hints on the device (the caller releases it); the control encoder on the assembled UNet input -> r[13]
    // dense, in the engine's activation type (the caller releases them); whether step `step` of the call in flight is controlled
    Act control_hint_embed(const uint8_t* hint_rgb_dev, int n, int hint_h, int hint_w);
    void control_run(const float* x_nhwc, int nb, int step, Act (&r)[13]);
    bool control_on(int step) const {
        if (!us_.ctrl || !us_.ctrl_window) return us_.ctrl;
        if (!us_.eval_step.empty()) return control_step_on(ctrl_.start, ctrl_.end, us_.eval_step[(size_t)step], us_.call_steps);
        return control_step_on(ctrl_.start, ctrl_.end, step, us_.steps);
    }
    // FreeU: is evaluation `step` of the call in flight inside the window (control_on's rule); the two edits on a block's input buffer `cat` = [cx backbone channels |
    // skip channels]: segments for the one filter launch of a forward, and the backbone launches in front of the block
    bool freeu_on(int step) const {
        if (!freeu_.version) return false;
        if (!us_.window) return true;
        if (!us_.eval_step.empty()) return control_step_on(freeu_.start, freeu_.end, us_.eval_step[(size_t)step], us_.call_steps);
        return control_step_on(freeu_.start, freeu_.end, step, us_.steps);
    }
    int freeu_granule() const { return bf16_ ? 64 : 32; }
    void freeu_filter(const Act* const* cats, const int* cx, const float* s, int n_cats);   // the entries with s != 1, one launch (none without one)
    void freeu_backbone(const Act& cat, int cx, float b, int version);
    FreeU freeu_;
    // IP-Adapter: the weights (ipw_), the sticky setting (ip_: tokens [n_sets][T_ip][cd] and negative tokens [neg_sets][T_ip][cd] on the device), whether evaluation
    // `step` of the call in flight is inside the window (control_on's rule), and the launch behind a cross attention: o (dense, the storage type) or o3 (planes)
    // += s_b softmax(q K_ip^T) V_ip.  ip_live_: the forward in flight is an adapted one (set by unet_run for its own blocks; a ControlNet's transformers are not adapted).
    struct IpWeights { bool ready = false; int D = 0, T = 0; float* proj_bt = nullptr; float* proj_b = nullptr; NormW norm; std::vector<float*> kbt, vbt; std::vector<void*> allocs; } ipw_;
    struct IpState { bool set = false; float* tokens = nullptr; float* neg = nullptr; int n_sets = 0, neg_sets = 0, T_ip = 0; bool neg_given = false; float scale = 1.f; double start = 0, end = 1; } ip_;
    bool ip_live_ = false;
    bool ip_on(int step) const {
        if (!us_.ip_want) return false;
        if (!us_.window) return true;
        if (!us_.eval_step.empty()) return control_step_on(ip_.start, ip_.end, us_.eval_step[(size_t)step], us_.call_steps);
        return control_step_on(ip_.start, ip_.end, step, us_.steps);
    }
    void ip_prepare(int nb, int n_images, const std::function<void*(size_t)>& own);
    void ip_attention(const SpatialW& w, const Act& q, const Act& o, int nb, int hw, int heads, int d);
    void unet_release();
    void unet_run(const float* x_nhwc, int nb, int step, float* out_nhwc, bool cfg_pair = false);
    void decode_one(const float* z_nhwc, int n, Act& img);
    // Encoder::forward + quant_conv of ONE image: rgb [1][8h][8w][4] fp32 (released here) -> the 8 moments [1][h][w][8] fp32 (caller releases)
    Act encode_one(Act& rgb);
    // The DDIM + CFG loop of sample_latent over `ts` (sample_latent's schedule or its tail): `start` writes x_ts[0] into the NHWC latent
    // [n][hw][4] and both halves of unet_in [2n][hw][4] (per_half floats each).  blend (img2img with a mask): after each update
    // x <- m x + (1 - m)(sqrt(a_prev) z0 + sqrt(1 - a_prev) eps), device pointers, z0 / eps NHWC.  With a non-default sampler_ the update of every step is
    // launch_sampler_step on the coefficient table of sdmi_sampler_coefs instead (one launch per step either way), its history in pool buffers of the call.
    // out_nhwc (the first pass of the hires fix): latent_out receives the NHWC latent itself (a device copy) instead of the NCHW conversion launch.
    struct Blend { const float* mask; const float* z0; const float* eps; };
    void sample_loop(const float* context, int n, int T, const float* uncond, int Tu, double scale, const std::vector<int>& ts,
                     size_t step_size, const std::function<void(float* latent, float* unet_in, long long per_half)>& start,
                     const Blend* blend, float* latent_out, bool out_nhwc = false, const float* cond_nhwc = nullptr, const std::vector<double>* kplan = nullptr);
    // kplan (a k-sampler is set): the rows of ksampler_plan for the call -- the loop walks its evaluations instead of ts, which is unused then.
    // kplan_for: the plan of a call of n_steps at `strength`, *a0 = 1 / (1 + sigma_start^2), the alpha of the img2img start.
    std::vector<double> kplan_for(size_t n_steps, double strength, double* a0) const;
    double rescale_ = 0.0;   // sdmi_set_guidance_rescale
    bool zero_snr_ = false;  // sdmi_set_zero_snr: alphas_ = rescale_zero_snr(alphas_loaded_) while on
    std::vector<float> alphas_loaded_;
    void refresh_schedule();   // alphas_ from alphas_loaded_ and zero_snr_
    int prediction_ = 0;   // sdmi_set_prediction: 0 = the UNet predicts eps, 1 = v (the coefficient tables are rewritten)
    // cond_nhwc (a conditioned model): [n][hw][padded_in_ch - 4]; every unet_run is preceded by assemble_unet_in into a buffer of the call
    float* cond_to_nhwc(const float* cond_nchw, int n);
    void assemble_unet_in(const float* unet_in, const float* cond_nhwc, int rows, int n, float* dst);
    // argument checks of both img2img entry points; returns the timesteps (rule 1) and the schedule's step size
    std::vector<int> img2img_schedule(int n, int T, int Tu, size_t n_steps, double strength, size_t* step_size);

    void count_kernel(double flops = 0) { ++n_kernels_; flops_ += flops; }
    // roctx ranges (option "roctx=1"; rocprofv3 --marker-trace shows them): one per DDIM step, UNet block, ResBlock,
    // SpatialTransformer and VAE stage.  libroctx64 is opened lazily, like RCCL.
    struct Range {
        Engine* e;
        Range(Engine* e_, const char* name) : e(e_->roctx_on_ ? e_ : nullptr) { if (e) e->roctx_push(name); }
        Range(Engine* e_, const std::string& name) : Range(e_, name.c_str()) {}
        ~Range() { if (e) e->roctx_pop(); }
        Range(const Range&) = delete;
        Range& operator=(const Range&) = delete;
    };
    bool roctx_on_ = false;
    void roctx_enable(bool on);
    void roctx_push(const char* name);
    void roctx_pop();
    void check_batch(int n) const {
        if (cfg_.max_batch > 0 && n > cfg_.max_batch)
            throw Error(SDMI_ERR_INVALID, "batch of " + std::to_string(n) + " exceeds sdmi_config.max_batch = " + std::to_string(cfg_.max_batch));
    }

public:
    // per-kernel-class timing (option "profile=1"): HIP events around every launch on the
    // engine's stream, accumulated per class.  Used by bench.py for the roofline line.
    enum ProfClass { PC_CONV_GEMM, PC_SPLITK_REDUCE, PC_ATTENTION, PC_GROUP_NORM, PC_LAYER_NORM, PC_CONV_FP8, PC_CONV_SPLIT, PC_SPLIT_ROWS, PC_OTHER, PC_GEGLU, PC_COUNT };
    struct ProfStat { double ms = 0; long long launches = 0; double flops = 0; double bytes = 0; };
    ProfStat prof_[PC_COUNT];
    void prof_flush();
    void prof_calibrate();
    double prof_overhead_ms_ = 0;    // what an empty event pair reads (subtracted from every sample)
    void prof_reset() { prof_flush(); for (auto& p : prof_) p = ProfStat{}; prof_tags_.clear(); }
    // option "profile=2": the same samples also accumulated per launch TAG (class + shape + tile choice), option dump_profile_tags writes them:
    // where inside a class the time goes (tools/shape_times.py)
    std::map<std::string, ProfStat> prof_tags_;

private:
    struct ProfScope {
        Engine* e; int cls; double flops, bytes; int n_launch; hipEvent_t a = nullptr, b = nullptr; int tag = -1;
        ProfScope(Engine* e_, int cls_, double flops_ = 0, double bytes_ = 0, int n_launch_ = 1);    // n_launch: kernels inside the scope (GroupNorm: statistics + apply)
        ~ProfScope();
        void set_tag(const char* fmt, ...) __attribute__((format(printf, 2, 3)));   // no-op unless profile=2
    };
    struct ProfPending { int cls; hipEvent_t a, b; double flops, bytes; int n_launch; int tag; };
    bool prof_tagging_ = false;
    std::vector<std::string> prof_tag_names_;
    std::map<std::string, int> prof_tag_ids_;
    hipEvent_t prof_event();
    bool profiling_ = false;
    std::vector<hipEvent_t> prof_free_;
    std::vector<ProfPending> prof_pending_;

    sdmi_config cfg_;
    int lat_h_ = 0, lat_w_ = 0;   // current latent size
    bool bf16_ = false;  // precision >= 1: bf16 activations / weights, fp32 accumulate
    bool fp8_ = false;   // precision = 2: additionally the ResBlock / ResnetBlock 3x3 convs in MXFP8 (k_fp8.hip)
    int opt_fp8_convs_ = 1;          // 0: run the fp8-capable convs on the bf16 kernels (A/B, accuracy comparison)
    int opt_fp8_min_rows_ = 1024;    // GEMMs with fewer output rows stay bf16 (256-row tiles need rows to fill the chip)
    int opt_fp8_tile_ = -1;
    int opt_gn32_min_wgs_ = 256 | ((64 + 1) << 16);   // precision = 0, GroupNorm launch geometry (k_norm.hip gn_geom): low 16 bits = at least this many workgroups in the APPLY pass over
                                     // the call's samples (a batch-1 tensor cut by size alone leaves CUs without a workgroup); bits 16.. = 1 + the same for the STATISTICS pass, which
                                     // is cut coarser (every apply workgroup merges all chunk partials).  Options gn32_min_wgs / gn32_stats_min_wgs / gn32_stats_chunk_kb;
                                     // measured at batch 1: GroupNorm class 21.3 -> 17.3 ms per image (profiles/r05d, r05f, r05o, r05p)
    GnTune gn_tune_;                 // launch geometry of the bf16 / MXFP8 GroupNorm passes (kernels.hpp; options gn_target_wgs, gn_max_threads, gn_unroll)
    int opt_b3_grouped_ = 1;         // precision 0: weight planes in 16-row fragment groups (1 KiB DMA pieces, sequential per group); 0 = row-major planes.  Before the weights are loaded.
    std::vector<int> q64_entries_;   // bf16 query weights of 64-wide UNet heads: their pre_scale follows option attn_d64
    AttnPlanOpts aopt_;              // options attn_split, attn_bf16, attn_bf16_variant, attn_pack_tail, attn_kv_splits, attn_kv_prefer8 (attn_plan.hpp)
    int opt_cfg_share_ = 1;          // sample_latent: the part of the UNet in front of the first cross attention is computed once for the two identical halves of a CFG step (unet_run)
    int opt_skip_slices_ = 1;        // fp32 ResBlocks with a 1x1 shortcut: 1 = the shortcut runs on extra K slices of conv_out's split-K launch (conv_pair); 0 = its own launches
    // fp32 transformer blocks: mlp_lin + proj_out as one paired launch on the folded weight (linear_pair).  0 = their own launches; 1 = every
    // shape the pair planner pairs; 2 = only shapes with a measured row in the pairs table (an unmeasured pair has not been shown to beat its two launches)
    int opt_proj_out_fold_ = 2;
    int opt_splitk_aux_ = 0;         // tests (with splitk): requested slice count of the auxiliary problem of a paired launch; 0 = planned
    int opt_op_resid_ = 0;           // tests: op_conv2d / op_linear add their input as the residual (cin == cout) through the GEMM epilogue
    int opt_op_misalign_ = 0;        // tests: stage_epi starts the device copies of bias, time-embedding row and residual one element past an aligned address
    int opt_fp8_ops_ = 0;            // tests: op_linear / op_layer_norm / op_geglu run the fp8_linear path's kernels (outputs dequantised)
    int opt_fp8_linear_ = 0;         // precision = 2: 0 (default: the accuracy budget of 6e-2 final-latent relative RMS) = MXFP8 on the ResBlock / ResnetBlock 3x3
                                     // convolutions only; 1 = also the transformer blocks' Linear layers and the 1x1 / up / down convolutions (8.1e-2)
    sdmi_sampler sampler_{};          // all zero: kind 0, eta 0
    sdmi_ksampler ksampler_{};        // the k-sampler in force where kset_
    bool kset_ = false;
    struct Control { bool set = false; uint8_t* hint_dev = nullptr; size_t hint_bytes = 0; int n_hint = 0, hint_h = 0, hint_w = 0; double strength = 1, start = 0, end = 1; } ctrl_;
    int opt_op_f32_ = 0;             // tests: op_conv2d runs the fp32 route (fp32 weight, input and output) at every precision -- the route of the ControlNet hint convolutions
    hipStream_t stream_ = nullptr;
    hipEvent_t ev0_ = nullptr, ev1_ = nullptr, ev_user_ = nullptr;
    hipStream_t user_stream_ = nullptr;
    bool has_user_stream_ = false;
    bool call_dev_ = false;
    unsigned long long call_mark_ = 0;
    DevPool pool_;
    std::vector<WeightEntry> entries_;
    std::map<std::string, int> entry_index_;
    std::vector<void*> weight_allocs_;
    // every hipMalloc of persistent device data (weight arenas, planes, masters, fused q | k | v weights, MXFP8 copies, LoRA factors) goes through here, so that option
    // pool_fill reaches what the pool does not hold: the allocation is filled like a pool block when the option is on at that moment.  weight_buffer: written on
    // stream_ only, and remembered, so that pool_fill set before the first weight is loaded also fills the buffers the constructor made; false (the LoRA factors, copied
    // on the null stream): the fill is complete on return.  The caller records the pointer for the matching hipFree.
    void* persistent_alloc(size_t bytes, bool weight_buffer = true);
    struct PersistentBlock { void* p; size_t bytes; };
    std::vector<PersistentBlock> persistent_blocks_;
    bool finalized_ = false;
    std::vector<float> alphas_;

    // UNet
    LinW lin1_time_, lin2_time_;
    std::vector<UBlock> in_blocks_, out_blocks_;
    ResW mid_res1_, mid_res2_;
    SpatialW mid_st_;
    NormW unet_norm_out_;
    ConvW unet_conv_out_;
    size_t n_res_unet_ = 0, n_st_unet_ = 0;   // res_list_ / st_list_ entries of the UNet itself; the ControlNet's follow
    // ControlNet (optional weight group 3): its own time MLP, encoder and middle block, the hint convolutions, the zero convolutions
    LinW ctl_lin1_time_, ctl_lin2_time_;
    std::vector<UBlock> ctl_blocks_;
    ResW ctl_mid_res1_, ctl_mid_res2_;
    SpatialW ctl_mid_st_;
    ConvW ctl_hint_[8], ctl_zero_[12], ctl_mid_out_;
    std::vector<ResW*> res_list_;       // index = temb_index
    std::vector<SpatialW*> st_list_;    // index = ctx_index
    // VAE decoder
    ConvW post_quant_, dec_conv_in_, dec_conv_out_;
    ResW dec_mid1_, dec_mid2_;
    VaeAttnW dec_attn_;
    DecBlockW dec_blocks_[4];
    NormW dec_norm_out_;
    // CLIP text encoder (optional weight group)
    float* clip_tok_ = nullptr;
    float* clip_pos_ = nullptr;
    std::vector<ClipBlockW> clip_blocks_;
    NormW clip_ln_;
    bool clip_ready_ = false;
    std::vector<Embedding> embeddings_;
    float* emb_bank_ = nullptr;   // [emb_rows_, ctx_dim], one allocation, rebuilt by embedding_add / embedding_remove
    int emb_rows_ = 0;
    // VAE encoder (optional weight group)
    struct EncBlockW { ResW res[2]; ConvW down; bool has_down = false; int cin = 0, cout = 0; };
    ConvW enc_conv_in_, enc_conv_out_, quant_conv_;
    EncBlockW enc_blocks_[4];
    ResW enc_mid1_, enc_mid2_;
    VaeAttnW enc_attn_;
    NormW enc_norm_out_;
    bool enc_ready_ = false;

    // per-call UNet state
    struct UNetState {
        int nb = 0, t_max = 0, steps = 0;
        std::vector<int> eval_step;   // a k-sampler's call: the step of the call each evaluation (row) belongs to, of call_steps; empty otherwise
        int call_steps = 0;
        std::vector<float*> temb;   // per ResBlock [steps][cout]
        std::vector<float*> kc, vc; // per SpatialTransformer [nb][t_max][c]
        int* kv_len_dev = nullptr;
        std::vector<int> kv_len_host;
        std::vector<void*> owned;
        bool window = true;                      // the call counts steps (the sampling entries); false: sdmi_unet_forward*, where the control and FreeU are simply on
        bool ctrl = false, ctrl_window = true;   // a controlled call: the control blocks' tables are prepared, hint_rows holds the hint embedding
        float* hint_rows = nullptr;              // [nb][h][w][mc] fp32: row block i = the embedding of hint (i mod n_images) mod n_hint
        bool ip_want = false;                    // an adapted call (IP-Adapter): an adapter is set with a scale other than 0
        int n_images = 0;
        std::vector<float*> kip, vip;            // per cross attention of the UNet [nb][T_ip][c] fp32, made by the first adapted step of the call; empty before
        float* ip_s = nullptr;                   // [nb] the adapter's scale per batch row
        std::vector<float> ip_s_host;
    } us_;

    // options
    int opt_resid_acc_ = 3;     // precision >= 1, large-tile kernels without split-K (ConvGemm::resid_acc): bit 0 = the residual, bit 1 = bias + time-embedding row are the accumulators'
                                // initial value, loaded in front of the k loop; 0 = added by the epilogue (round 5)
    int opt_geglu_fuse_ = 1;    // GEGLU gate in the projection GEMM's epilogue: 0 never, 1 where there are >= 4 rounds of tiles, 2 / 3 always (256x128 / 256x256 tiles; tests)
    static constexpr int kGemm3xVariantDefault = 2;
    int opt_gemm3x_variant_ = kGemm3xVariantDefault;     // k_gemm3x.hip: bit 0: DMA in one block per k tile; bit 1: scalar residual subtractions (+0.7 %); bit 2: two LDS stages on the 128-row tiles
                                     // (default three: +5..10 % on long K); bit 4: s_setprio 1 for waves 4-7 (measured: no gain)
    int opt_gemm_probe_ = 0;    // bench_conv: 1 = one extra launch with per-workgroup phase stamps (ConvGemm::probe), summary on stderr
    unsigned long long* probe_buf_ = nullptr;
    int opt_bench_cold_ = 0;    // bench_conv: 1 = evict the weights from the Infinity Cache between timed launches (what a layer sees inside the model)
    static constexpr int kGemmBf16xVariantDefault = 5;
    int opt_gemm_bf16x_variant_ = kGemmBf16xVariantDefault; // precision >= 1, k_gemm_bf16x.hip / k_gemm_bf16t.hip: bit 2 (round 6) = waves 4 - 7 issue their DMA pieces between a tile's two k steps (one-tile forms and the kernel-row convolution); bit 0 = persistent tile loop (launches without split-K or residual and with more tiles than CUs;
                                     // bit-identical results, +0.4 ... 0.7 % per image: profiles/r05a_*)
    void* zero_page_ = nullptr;
    GemmPlanOpts gopt_;   // options gemm_tile, splitk, gemm_x32, gemm_f32s, gemm_bf16x, gemm_planes, conv3_reuse
    GemmTuning tuning_;   // measured per-shape tile choices: tuning/gfx950_*.txt, options tune / tune_bf16 / tune_clear
    bool record_shapes_ = false;
    std::map<std::string, long long> shape_counts_;  // "n,cin,h,w,cout,k,stride,ups" -> launches
    std::map<std::string, long long> choice_counts_;   // "M,N,K cfg=.. splits=.." -> launches (record_shapes)

    long long n_kernels_ = 0;
    double flops_ = 0;
};

// One output index of a resampling axis (include/sdmi.h, sdmi_resize_weights): y[o] = sum_j w[j] x[first + j].  resize_rows is THE implementation of the rule
// (sdmi_capi.cpp); throws SDMI_ERR_INVALID for what sdmi_resize_weights refuses.
struct ResizeRow { int first = 0; std::vector<double> w; };
std::vector<ResizeRow> resize_rows(int in_size, int out_size, int mode, bool antialias);

void set_last_error(const std::string& msg);   // the thread-local message behind sdmi_last_error() (sdmi_capi.cpp)

}  // namespace sdmi

// the opaque handles of include/sdmi.h
struct sdmi_ctx {
    sdmi::Engine* engine;
};
struct sdmi_lora {
    sdmi::Engine* engine;
    double scale = 0;
    std::vector<sdmi::LoraTarget> targets;
    std::vector<void*> allocs;   // device memory of the factors
    size_t factor_bytes = 0;     // of a file's raw factors (sdmi_lora_load_safetensors); 0 for sdmi_lora_add targets
};
