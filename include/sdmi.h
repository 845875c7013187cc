/*
 * sdmi.h -- C ABI of libsdmi.so: the MI355X (gfx950) Stable Diffusion v1.4
 * sampling hot path (UNet DDIM+CFG loop and VAE decoder) that sits behind the
 * `StableDiffusion::sample_image` surface of Gadersd/stable-diffusion-burn.
 *
 * Every entry point below names the reference interface it replaces
 * (file:line relative to the reference repo).  The reference has no FFI of its
 * own -- its "plugin" seam is the Burn `Backend` type parameter
 * (src/bin/sample/main.rs:59-83) plus the commented-out operator-override
 * trait in src/backend.rs:4-84 -- so this header is what a Rust shim
 * (ffi/sdmi.rs) binds with `extern "C"`.
 *
 * Conventions
 *  - plain pointers and sizes only; no C++/torch types
 *  - host-pointer functions take row-major fp32 in the REFERENCE's logical
 *    layouts (NCHW images/latents, [n, tokens, channels] sequences); the
 *    library copies in/out and blocks until results are in host memory.
 *    NHWC and packed weights are internal.
 *  - *_dev functions take DEVICE pointers (same logical layouts).  The context
 *    works on a private non-blocking HIP stream, so on entry it must be ordered
 *    behind whatever produced those buffers: if sdmi_set_stream() named the
 *    caller's stream, the context waits for an event on it (and makes that
 *    stream wait for the results on return); otherwise the call starts with a
 *    hipDeviceSynchronize().  All entry points return after the results are
 *    complete (they block on the context's stream).
 *  - every function returns 0 (SDMI_OK) or a negative sdmi_status; the
 *    message is available from sdmi_last_error() (thread-local).  The
 *    reference's hot path is infallible by type and panics on shape errors
 *    (stablediffusion/mod.rs:86, unet/mod.rs:134); the Rust shim panics on a
 *    non-zero status to keep that contract.
 *  - a context is not re-entrant: one call at a time per context.
 *  - the caller owns every in/out buffer; the context owns device weights,
 *    activation pool and stream.  Nothing returned needs freeing but the ctx.
 */
#ifndef SDMI_H
#define SDMI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sdmi_ctx sdmi_ctx;

typedef enum sdmi_status {
    SDMI_OK = 0,
    SDMI_ERR_INVALID = -1,     /* bad argument / shape (reference: panic)      */
    SDMI_ERR_HIP = -2,         /* a hip* call failed                           */
    SDMI_ERR_WEIGHTS = -3,     /* missing / mis-shaped weight tensor           */
    SDMI_ERR_IO = -4,          /* weight file / directory unreadable           */
    SDMI_ERR_UNSUPPORTED = -5, /* valid in the reference, not built here yet   */
    SDMI_ERR_STATE = -6        /* call order (e.g. forward before finalize)    */
} sdmi_status;

/* Model / device configuration.  Defaults (sdmi_default_config) are the
 * reference's hard-coded hyper-parameters: UNetConfig::init unet/mod.rs:36-92,
 * AutoencoderConfig::init autoencoder/mod.rs:30-36, latent 4x64x64
 * stablediffusion/mod.rs:116.  Tests shrink them; nothing else should. */
typedef struct sdmi_config {
    int32_t device;          /* HIP device ordinal                              */
    int32_t model_channels;  /* 320                                             */
    int32_t n_head;          /* 8                                               */
    int32_t ctx_dim;         /* 768  (CLIP text width)                          */
    int32_t latent_h;        /* 64   (image = 8x)                               */
    int32_t latent_w;        /* 64                                              */
    int32_t vae_ch;          /* 128  (decoder channels 4c,4c,2c,c)              */
    int32_t max_batch;       /* largest n a call may pass; 0 = no limit          */
    int32_t precision;       /* 0 = fp32; 1 = bf16 storage, fp32 accumulate; 2 = 1 + MXFP8 operands for the ResBlock / ResnetBlock 3x3 convolutions (20-step latent 5.2e-2 relative RMS
                              * of the exact one; option "fp8_linear=1": also the transformer blocks' Linear layers and the 1x1 / up / down convolutions, 8.1e-2 for +5 %).
                              * ATTENTION IS NOT ON FP8 OPERANDS at any precision (BASELINE.json configs[4] names "fp8 conv+attn"): qkv_attention runs bf16 at precision 1 and 2 --
                              * formally dropped, DESIGN.md section 8: Q K^T contracts over d_head = 40 (no gain on the K = 128 MX instruction), P V would return at most 2.5 % of an
                              * image (measured ablation), at the price of an e4m3 P with block scales inside the softmax loop. */
    /* CLIP text encoder, CLIPConfig::new(49408, 768, 12, 77, 12) stablediffusion/mod.rs:29;
     * its width is ctx_dim.  clip_layers = 0 builds a context without it.              */
    int32_t clip_layers;     /* 12                                              */
    int32_t clip_heads;      /* 12                                              */
    int32_t clip_vocab;      /* 49408                                           */
    int32_t clip_ctx;        /* 77                                              */
    int32_t unet_in_ch;      /* 4; input channels of the UNet's first convolution: 4 = the latent alone, 5..12 = the latent + (unet_in_ch - 4)
                              * conditioning channels given per call (the *_cond entry points; 9 = the SD v1 inpainting checkpoints, 8 = instruct-pix2pix-shaped
                              * UNets).  0 means 4, so that a zeroed struct keeps working; anything else is SDMI_ERR_INVALID from sdmi_create. */
    int32_t control_hint_ch; /* 0; channels of a ControlNet's hint picture: 0 = no ControlNet (the tensor list, sdmi_weight_count and every launch are those of a context
                              * without the field), 3 = an RGB hint: the model gets a fourth weight group "controlnet/..." (section "ControlNet" below).  Anything else is
                              * SDMI_ERR_INVALID from sdmi_create; control_hint_ch != 0 with unet_in_ch != 4 is SDMI_ERR_UNSUPPORTED (the control encoder's first convolution
                              * takes the 4 latent channels). */
    int32_t variant;         /* 0 = SD v1 (a zeroed field keeps meaning what it meant), 1 = SD 2.x: every UNet attention has model_channels-level width / 64 heads of width 64
                              * (n_head is ignored; model_channels % 64 != 0 is SDMI_ERR_INVALID; the ".../n_head" metadata entries carry the per-level count), the text
                              * encoder's MLP uses the exact (erf) GELU and sdmi_encode_prompt pads each chunk behind its <|endoftext|> with token id 0 (OpenCLIP), and option
                              * "attn_d64" defaults to 2 (head dim 64 on the bf16-pipe attention kernels where measured faster).  Anything else is SDMI_ERR_INVALID from sdmi_create; variant = 1 with control_hint_ch != 0 is SDMI_ERR_UNSUPPORTED.
                              * The OpenCLIP ViT-H tower of SD 2.x is ctx_dim = 1024, clip_layers = 23, clip_heads = 16: 23 blocks + the final LayerNorm are its "penultimate"
                              * output.  Whether a checkpoint predicts eps (512-base) or v (768-v) is not in the file: the caller chooses, sdmi_set_prediction. */
} sdmi_config;

int sdmi_default_config(sdmi_config* cfg);

/* ---- lifecycle ------------------------------------------------------------ */
int sdmi_create(sdmi_ctx** out, const sdmi_config* cfg);
void sdmi_destroy(sdmi_ctx* ctx);
const char* sdmi_last_error(void);
int sdmi_synchronize(sdmi_ctx* ctx);
/* Names the HIP stream (a hipStream_t passed as void*; NULL = the legacy default stream) on which the caller
 * produces the inputs and consumes the outputs of the *_dev entry points; enable = 0 returns to the default
 * (device-wide synchronisation on entry).  The reference has no counterpart: Burn tensors are ordered by the
 * backend's own queue. */
int sdmi_set_stream(sdmi_ctx* ctx, void* hip_stream, int32_t enable);
/* library / build identification, e.g. "sdmi 0.1 gfx950 fp32" */
const char* sdmi_version(void);

/* ---- weights -------------------------------------------------------------
 * Names are the reference's npy-dump tree paths (src/model/unet/load.rs:217-305,
 * src/model/autoencoder/load.rs:135-157, src/model/stablediffusion/load.rs:20-24),
 * e.g. "unet/input_blocks/rt1/res/conv_in/weight", "autoencoder/post_quant_conv/bias",
 * "alphas_cumprod".  Shapes are the reference's: Conv2d weight [Cout,Cin,kh,kw],
 * Linear weight [in,out] (python/save.py:19), norms [C].  Replaces
 * load_stable_diffusion (stablediffusion/load.rs:16-33) for the hot-path
 * subset (UNet, VAE decoder + post_quant_conv, alphas_cumprod). */
int sdmi_set_weight(sdmi_ctx* ctx, const char* name, const float* data, int32_t ndim, const int64_t* dims);
/* number of tensors the configured model needs / name + shape of the i-th */
int sdmi_weight_count(sdmi_ctx* ctx);
int sdmi_weight_info(sdmi_ctx* ctx, int32_t index, const char** name, int32_t* ndim, int64_t dims[4]);
/* reads the npy-dump directory written by the reference's python/ exporters
 * (format: src/model/load.rs:17-28 -- 1-D float32 .npy whose first D values
 * are the shape). */
int sdmi_load_weights_dir(sdmi_ctx* ctx, const char* dump_dir);
/* load_stable_diffusion_model_file (src/bin/sample/main.rs:27-34): reads a Burn NamedMpkFileRecorder<FullPrecisionSettings>
 * record (the reference's "SDv1-4.mpk") natively -- a MessagePack walker over the memory-mapped file, tensors staged
 * straight from the mapping.  The burn 0.14 layout it assumes is spelled out in csrc/mpk_reader.hpp (UNPINNED against a
 * real record: none exists offline).  Tensors the configured model lacks are skipped; call sdmi_finalize_weights after. */
int sdmi_load_weights_mpk(sdmi_ctx* ctx, const char* mpk_path);
/* Host only (no context): the tensors of a record as text, one "name<TAB>d0,d1,..<TAB>file offset" line each (dump-tree
 * names), after a "# format=.. float=.." line.  *needed = bytes incl. the terminator; out may be NULL to query it. */
int sdmi_mpk_list(const char* mpk_path, char* out, size_t capacity, size_t* needed);
/* An SD v1.x checkpoint in the CompVis layout -- ONE .safetensors file with keys "model.diffusion_model.…", "first_stage_model.…",
 * "cond_stage_model.transformer.text_model.…" and "alphas_cumprod", F32 / F16 / BF16, Linear weights as torch's [out, in] -- read natively (DESIGN.md
 * section 9e): the file is memory-mapped, every tensor of the configured model is looked up under sdmi_checkpoint_key(its dump name), its RAW bytes are
 * moved to the device and converted there (csrc/k_unpack.hip: exact widening to fp32, the Linear transpose, the zero 4th input channel of the VAE
 * encoder's RGB conv_in), and packed like every other loader's tensors.  Keys the model has no tensor for (model_ema.*, position_ids, ...) are skipped
 * whatever their dtype.  alphas_cumprod is taken from the file (F64 accepted) or, when absent, computed (sdmi_default_alphas_cumprod).
 * SDMI_ERR_IO / SDMI_ERR_WEIGHTS: an unreadable / malformed file (csrc/safetensors_reader.hpp lists what is refused); SDMI_ERR_WEIGHTS: a hot-path
 * tensor without a source (the message names the dump name and the key), a shape other than the model's (key, file's shape, expected shape: a 9-channel
 * inpainting conv_in into a 4-channel context, or the reverse, is refused here), no
 * matching key at all; SDMI_ERR_UNSUPPORTED: F64 or an integer dtype on a tensor of the model; SDMI_ERR_STATE: a LoRA adapter with a non-zero
 * scale.  Everything is checked before the first tensor is staged: a refused file leaves the context as it was.  The CLIP and VAE-encoder groups are
 * all-or-nothing by sdmi_finalize_weights' rule; call it after.  Out of scope: .ckpt pickles, diffusers-layout and sharded checkpoints, SDXL.
 * On a variant = 1 context the file is an SD 2.x checkpoint in Stability's layout: the UNet and VAE keys of v1 -- the transformers' proj_in /
 * proj_out as Linear [C, C], taken as [C, C, 1, 1] -- and the OpenCLIP text encoder under "cond_stage_model.model." (sdmi_checkpoint_key_ex), whose fused
 * attn.in_proj_weight [3C, C] / in_proj_bias [3C] is uploaded as three views of the mapped bytes: rows 0..C-1 query, C..2C-1 key, 2C..3C-1 value.  A file of the other
 * family (sdmi_safetensors_model_family) is SDMI_ERR_WEIGHTS before anything is looked up, naming the key that gives it away. */
int sdmi_load_weights_safetensors(sdmi_ctx* ctx, const char* path);
/* Host only.  *family = 1: an SD v1 checkpoint (the file has "cond_stage_model.transformer.text_model.final_layer_norm.weight"), 2: SD 2.x
 * ("cond_stage_model.model.ln_final.weight"), 0: neither key (a bare UNet, a ControlNet, a LoRA ...).  Errors as sdmi_safetensors_list. */
int sdmi_safetensors_model_family(const char* path, int32_t* family);
/* Host only (no context): the tensors of a .safetensors file as text, one "key<TAB>dtype<TAB>d0,d1,..<TAB>file offset<TAB>dump name or -" line each, in
 * header order.  A backslash, tab, newline or other control character inside a key is written as its JSON escape, so that a key stays one field.  The dump
 * name is the one whose sdmi_checkpoint_key is the key (SD v1.4's tensor set), "-" for any other key.  *needed = bytes incl. the terminator; out may be
 * NULL to query it. */
int sdmi_safetensors_list(const char* path, char* out, size_t capacity, size_t* needed);
/* Host only.  Writes the CompVis checkpoint key of `dump_name`, e.g. "unet/input_blocks/rt1/res/conv_in/weight" ->
 * "model.diffusion_model.input_blocks.1.0.in_layers.2.weight" (derived by rule, csrc/ckpt_keys.cpp; pinned against the reference's Python model and
 * exporters by tests/golden/sd14_ckpt_keys.txt).  *transposed = 1 where the checkpoint holds torch's [out,in] of a dump [in,out].  *needed = bytes
 * incl. the terminator; out may be NULL to query it.
 * SDMI_ERR_INVALID for a name that has no checkpoint source: module metadata such as eps / n_group, n_steps. */
int sdmi_checkpoint_key(const char* dump_name, char* out, size_t capacity, size_t* needed, int32_t* transposed);
/* The same for sdmi_config.variant `variant` (0: exactly the above; 1: SD 2.x, tests/golden/sd2_ckpt_keys.txt; anything else SDMI_ERR_INVALID).  *slice (may be NULL):
 * -1 = the key's whole tensor, 0 / 1 / 2 = the first / second / third third of its rows (query / key / value of a fused attn.in_proj_weight or in_proj_bias). */
int sdmi_checkpoint_key_ex(const char* dump_name, int32_t variant, char* out, size_t capacity, size_t* needed, int32_t* transposed, int32_t* slice);
/* Host only.  The schedule sdmi_load_weights_safetensors installs when the file has no alphas_cumprod: the LDM "scaled linear" one,
 * float32(cumprod(1 - linspace(sqrt(0.00085), sqrt(0.012), n)^2)) computed in f64.  out [n], n >= 1. */
int sdmi_default_alphas_cumprod(float* out, int32_t n);
/* One flat image of every tensor: `data` holds, for each entry i of the configured model in
 * sdmi_weight_info() order and restricted to the weight groups selected by `groups` (bit 0: hot path = UNet,
 * VAE decoder, alphas_cumprod; bit 1: CLIP; bit 2: VAE encoder), the tensor's fp32 values in the reference's
 * layout, back to back, no headers.  `n_floats` must equal the sum of their sizes (sdmi_packed_size).  Staged
 * through one pinned buffer and one stream: the batched replacement of load_stable_diffusion's ~1100 file reads
 * (stablediffusion/load.rs:16-33, model/load.rs:17-160). */
int sdmi_load_weights_packed(sdmi_ctx* ctx, const float* data, size_t n_floats, int32_t groups);
/* number of floats sdmi_load_weights_packed expects for `groups` */
int64_t sdmi_packed_size(sdmi_ctx* ctx, int32_t groups);
/* packs everything into the device layouts; fails listing the first missing tensor */
int sdmi_finalize_weights(sdmi_ctx* ctx);

/* ---- hot path, host pointers ------------------------------------------------ */

/* UNet::forward (src/model/unet/mod.rs:109-143).
 * x [n,4,h,w] NCHW, t scalar timestep (the reference passes a 1-element Int
 * tensor shared by the batch), context [n,T,ctx_dim] -> out [n,4,h,w]. */
int sdmi_unet_forward(sdmi_ctx* ctx, const float* x, int32_t t, const float* context,
                      int32_t n, int32_t T, float* out);

/* StableDiffusion::sample_latent (src/model/stablediffusion/mod.rs:102-160),
 * DDIM eta=0 with classifier-free guidance (forward_diffuser :162-192).
 * context [n,T,ctx_dim]; uncond [Tu,ctx_dim] (broadcast over the batch);
 * init_latent [n,4,h,w] = x_T (the reference draws it from an unseeded backend
 * RNG, :115-121; here it is an explicit input) or NULL to draw N(0,1) from
 * `seed` (image i uses stream seed+i); latent_out [n,4,h,w]. */
int sdmi_sample_latent(sdmi_ctx* ctx, const float* context, int32_t n, int32_t T,
                       const float* uncond, int32_t Tu, double scale, size_t n_steps,
                       const float* init_latent, uint64_t seed, float* latent_out);

/* Autoencoder::decode_latent (src/model/autoencoder/mod.rs:68-71):
 * latent [n,4,h,w] (already divided by 0.18215 by the caller, as in
 * latent_to_image) -> img_out [n,3,8h,8w] fp32 NCHW. */
int sdmi_decode_latent(sdmi_ctx* ctx, const float* latent, int32_t n, float* img_out);

/* Autoencoder::encode_image (src/model/autoencoder/mod.rs:60-66): img [n,3,8h,8w]
 * fp32 NCHW -> latent_out [n,4,h,w] (Encoder::forward, quant_conv, first 4 channels = the
 * posterior mean; the reference does not sample).  Not on the txt2img path;
 * needs the optional weight group autoencoder/encoder/..., autoencoder/quant_conv
 * (SDMI_ERR_STATE otherwise).  Autoencoder::forward (:56-58) = decode_latent(encode_image(x)). */
int sdmi_encode_image(sdmi_ctx* ctx, const float* img, int32_t n, float* latent_out);

/* StableDiffusion::latent_to_image (stablediffusion/mod.rs:69-100):
 * latent [n,4,h,w] -> rgb_out n x [8h,8w,3] uint8 (HWC, truncating cast). */
int sdmi_latent_to_image(sdmi_ctx* ctx, const float* latent, int32_t n, uint8_t* rgb_out);

/* StableDiffusion::sample_image (stablediffusion/mod.rs:51-67). */
int sdmi_sample_image(sdmi_ctx* ctx, const float* context, int32_t n, int32_t T,
                      const float* uncond, int32_t Tu, double scale, size_t n_steps,
                      const float* init_latent, uint64_t seed, uint8_t* rgb_out);

/* ---- img2img: sampling from an init image, optionally masked (no reference counterpart) ----
 * The DDIM + CFG loop of sdmi_sample_latent run over the LAST k of its timesteps ts (L entries, quirk Q5 included),
 * k = min(L, (size_t)(strength * L)), t0 = ts[L - k], started from
 *     x_t0 = sqrt(a_t0) z0 + sqrt(1 - a_t0) eps        (a = alphas_cumprod; coefficients in f64, applied as f32)
 * eps = noise [n,4,h,w], or when noise is NULL image i's N(0,1) stream seed + i (the draws of sdmi_sample_latent's
 * seed path, same elements).  Each step is sample_latent's update, unchanged.  mask [n,1,h,w] fp32 (1 = regenerate,
 * 0 = keep, values between blend) or NULL: after each step's update to t_prev,
 *     x <- m x + (1 - m)(sqrt(a_prev) z0 + sqrt(1 - a_prev) eps)   (same eps; not applied at t0)
 * so m = 0 ends exactly at z0.  context [n,T,ctx_dim], uncond [Tu,ctx_dim] broadcast, as in sample_latent.
 * SDMI_ERR_INVALID unless 0 < strength <= 1 and k >= 1. */

/* Host only, needs no device: the timesteps ts[L - k ..] the call runs for `total` = len(alphas_cumprod) (1000).
 * *count is always set to k when the arguments are valid; SDMI_ERR_INVALID if capacity < k (nothing written). */
int sdmi_img2img_timesteps(int32_t total, size_t n_steps, double strength, int32_t* timesteps, int32_t capacity, int32_t* count);
/* z0 [n,4,h,w]: the start latent in the sampler's space (= 0.18215 x the VAE posterior mean); latent_out [n,4,h,w].
 * Does not need the encoder weights. */
int sdmi_img2img_latent(sdmi_ctx* ctx, const float* context, int32_t n, int32_t T, const float* uncond, int32_t Tu,
                        double scale, size_t n_steps, double strength, const float* z0, const float* mask,
                        const float* noise, uint64_t seed, float* latent_out);
/* init_rgb n x [8h,8w,3] uint8 HWC (sdmi_sample_image's output layout): z0 = 0.18215 * encode_image(v / 127.5 - 1).
 * rgb_out = latent_to_image of the final latent, as sdmi_sample_image.  Pixels of the kept (m = 0) region go through
 * one VAE round trip: they are NOT pasted back from init_rgb.  Needs the encoder weight group (SDMI_ERR_STATE otherwise). */
int sdmi_img2img_image(sdmi_ctx* ctx, const float* context, int32_t n, int32_t T, const float* uncond, int32_t Tu,
                       double scale, size_t n_steps, double strength, const uint8_t* init_rgb, const float* mask,
                       const float* noise, uint64_t seed, uint8_t* rgb_out);

/* ---- sampler choice: stochastic DDIM (eta), DPM-Solver++(2M), PLMS (no reference counterpart) ----
 * The reference integrates with DDIM at sigma = 0 only (stablediffusion/mod.rs:142-156); that stays the default, on the same launches.
 * A sampler set on a context applies to every sampling entry point above and below (sample_latent / sample_image / img2img, host and
 * device pointers, sharded) until it is changed: sticky, like sdmi_set_stream.  Schedule (ts, step_size, prev, quirk Q5) and, for
 * img2img, the tail sdmi_img2img_timesteps selects are unchanged; with cur = a[ts_j], prev = a[ts_j - step_size] (1 past the end),
 * e = eu + (ec - eu) scale and x0 = (x - sqrt(1 - cur) e) / sqrt(cur):
 *   kind 0, DDIM(eta), 0 <= eta <= 1: sigma = eta sqrt((1 - prev) / (1 - cur)) sqrt(1 - cur / prev),
 *       x' = sqrt(prev) x0 + sqrt(1 - prev - sigma^2) e + sigma z.  eta = 0 is the default path, bit for bit.  Plain Euler on
 *       sigma_k = sqrt((1 - a) / a) IS eta = 0 and Euler-ancestral IS eta = 1 (sqrt(prev) sigma_up = sigma): no kinds of their own.
 *   kind 1, DPM-Solver++(2M) (data prediction, k-diffusion's sample_dpmpp_2m): lambda(a) = log(a / (1 - a)) / 2, h = lambda(prev) - lambda(cur),
 *       D = x0 on the first step of a call and where prev = 1, else (1 + 1/(2r)) x0 - x0_last / (2r) with r = (lambda(cur) - lambda(cur_last)) / h;
 *       x' = sqrt((1 - prev) / (1 - cur)) x - sqrt(prev) expm1(-h) D; where prev = 1 the step is its limit x' = x0.
 *   kind 2, PLMS: Adams-Bashforth on e with warm-up orders 1, 2, 3, then 4 -- e' = e, (3e - e1)/2, (23e - 16e1 + 5e2)/12,
 *       (55e - 59e1 + 37e2 - 9e3)/24 -- and the eta = 0 update with e' for e.  One UNet evaluation per step (CompVis plms.py spends a
 *       second one on its first step; this variant does not).
 * Step noise z (only where its weight is not 0): element i (NCHW order) of image b at index s of the FULL schedule ts is element i of the
 * N(0,1) stream  noise_seed + image_base + b + ((uint64_t)(s + 1) << 32)  (the stream of sdmi_sample_latent's seed path; uint64 wraparound).
 * image_base = the global index of the call's first image: a batch split into smaller calls draws the same noise per image.
 * The img2img mask blend follows the update of any kind, unchanged. */
typedef struct sdmi_sampler {
    int32_t kind;          /* 0 DDIM(eta), 1 DPM-Solver++(2M), 2 PLMS                              */
    int32_t reserved0;
    double eta;            /* kind 0 only: 0 (deterministic, the default) .. 1; must be 0 otherwise */
    uint64_t noise_seed;
    int64_t image_base;
    int64_t reserved[4];
} sdmi_sampler;
/* NULL restores the default (kind 0, eta 0).  SDMI_ERR_INVALID -- and nothing changes -- for an unknown kind, eta outside [0, 1] or NaN,
 * eta != 0 with kind != 0. */
int sdmi_set_sampler(sdmi_ctx* ctx, const sdmi_sampler* sampler);
int sdmi_get_sampler(sdmi_ctx* ctx, sdmi_sampler* out);

/* ---- sigma-schedule samplers: Karras / exponential / uniform spacing, Heun, DPM2, DPM++ 2S / SDE / 2M SDE (no reference counterpart;
 * DESIGN.md section 9i) ----
 * The samplers of k-diffusion on a continuous sigma schedule, sigma(a) = sqrt((1 - a) / a), with fractional timesteps.  The engine keeps the VP latent
 * x = x_k / sqrt(1 + sigma^2); in k-space, with D = x_k - sigma e, a step s -> s' and anc(s, s', eta): up = min(s', eta sqrt(s'^2 (s^2 - s'^2) / s^2)),
 * down = sqrt(s'^2 - up^2):
 *   0 euler(eta)        (d, u) = anc(s, s', eta); x_k' = x_k + e (d - s) + u z             (eta 0: Euler, eta 1: Euler-ancestral)
 *   1 dpmpp_2m          sdmi_sampler's kind 1 on the schedule's sigmas, h = ln s - ln s'
 *   2 heun              x2 = x_k + e1 (s' - s); e2 at s'; x_k' = x_k + (e1 + e2) / 2 (s' - s)
 *   3 dpm2              s_m = sqrt(s s'); x2 = x_k + e1 (s_m - s); e2 at s_m; x_k' = x_k + e2 (s' - s)
 *   4 dpmpp_2s(eta)     (d, u) = anc(s, s', eta), s_m = sqrt(s d); x2 = (s_m / s) x_k + (1 - s_m / s) D1; D2 at s_m; x_k' = (d / s) x_k + (1 - d / s) D2 + u z
 *   5 dpmpp_sde(eta)    s_m = sqrt(s s'); (d1, u1) = anc(s, s_m, eta): x2 = (d1 / s) x_k + (1 - d1 / s) D1 + u1 z_a; D2 at s_m; (d2, u2) = anc(s, s', eta):
 *                       x_k' = (d2 / s) x_k + (1 - d2 / s) D2 + u2 (alpha z_a + beta z_b), alpha = sqrt((s - s_m) / (s - s')), beta = sqrt((s_m - s') / (s - s')):
 *                       the two increments of one Brownian path in sigma (k-diffusion's law at r = 1/2, not its numbers)
 *   6 dpmpp_2m_sde(eta) h = ln s - ln s', g = eta h, B = -expm1(-h - g): x_k' = (s' / s) e^-g x_k + B D + [B / (2r) (D - D_last), r = h_last / h] + s' sqrt(-expm1(-2g)) z
 * Where s' = 0 every kind takes the single evaluation x_k' = D, without noise.  Kinds 2 - 5 spend two UNet evaluations on each of the other steps.  History (depth 1,
 * empty at the first step of a call): D for kinds 1 and 6, stage 1's e for 2 and 3, the step's start latent for 4 and 5.
 * Schedules: n steps give n + 1 sigmas, the last 0.  With S_j = sigma(a[j]), smax / smin = sigma_max / sigma_min or S_total-1 / S_0:
 *   0 model        sigma(a[ts_j]) over sdmi_sample_latent's own timesteps (quirk Q5: more than n of them where n does not divide total); sigma_min / sigma_max unused
 *   1 karras       (smax^(1/rho) + i / (n - 1) (smin^(1/rho) - smax^(1/rho)))^rho, i = 0 .. n - 1 (n = 1: smax alone)
 *   2 exponential  exp(linspace(ln smax, ln smin, n))
 *   3 uniform      k-diffusion's get_sigmas: t = linspace(total - 1, 0, n), ln sigma = ln S interpolated linearly in t; sigma_min / sigma_max unused
 * The UNet is evaluated at t = sdmi_sigma_to_t(sigma), a fraction (on schedule 0 the integer ts_j itself).
 * Step noise: draw r of step s of the FULL schedule is the stream  noise_seed + image_base + b + ((uint64_t)(s + 1) << 32) + ((uint64_t)r << 62);  r = 0 is
 * sdmi_sampler's rule, z_b of kind 5 is r = 1 (its z_a is drawn again from r = 0 in the second stage, never stored).
 * img2img: with L steps the call runs the last k = min(L, (size_t)(strength L)) of them from x = sqrt(a0) z0 + sqrt(1 - a0) eps, a0 = 1 / (1 + sigma_start^2); the mask
 * blend follows a step's LAST evaluation, with 1 / (1 + s'^2) for a_prev.  sdmi_sample_latent's init_latent is the VP latent at the schedule's first sigma.
 * The two sticky states exclude each other: a successful sdmi_set_ksampler(non-NULL) resets the sdmi_sampler to its default, and any sdmi_set_sampler call (NULL included)
 * clears the k-sampler.  With no k-sampler set every call runs the launches and gives the bits it gave before.  A ControlNet window counts the call's STEPS: both
 * evaluations of a step agree.  Out of scope: LMS / PLMS on non-uniform schedules, UniPC, s_churn, bit-compatibility with k-diffusion's noise.  (v-prediction: sdmi_set_prediction.) */
typedef struct sdmi_ksampler {
    int32_t kind;      /* 0 euler (eta), 1 dpmpp_2m, 2 heun, 3 dpm2, 4 dpmpp_2s (eta), 5 dpmpp_sde (eta), 6 dpmpp_2m_sde (eta) */
    int32_t schedule;  /* 0 model (the reference's integer timesteps), 1 karras, 2 exponential, 3 uniform */
    double eta;        /* 0..1; must be 0 for kinds 1, 2, 3 */
    double rho;        /* karras only; 0 = 7 */
    double sigma_min, sigma_max;   /* 0 = the model's sigma(a[0]) / sigma(a[total-1]); else inside that range, min < max */
    uint64_t noise_seed; int64_t image_base; int64_t reserved[4];
} sdmi_ksampler;
/* Sticky; NULL clears.  SDMI_ERR_INVALID -- and nothing changes -- for an unknown kind or schedule, eta outside [0, 1] or NaN, eta != 0 for kinds 1 - 3, rho < 0 or
 * not finite, a sigma bound that is negative, not finite, outside the model's range or min >= max. */
int sdmi_set_ksampler(sdmi_ctx* ctx, const sdmi_ksampler* ksampler);
/* *is_set = 1 and *out = the k-sampler in force, or *is_set = 0 and *out zeroed */
int sdmi_get_ksampler(sdmi_ctx* ctx, sdmi_ksampler* out, int32_t* is_set);
/* Host only, f64, no device: THE implementation of the schedules and samplers above (the engine calls it).
 * sigmas: the *count = steps + 1 sigmas of n_steps, the last 0.  sigma_to_t: k-diffusion's rule -- low = the last j <= total - 2 with ln S_j <= ln sigma,
 * w = clamp((ln S_low - ln sigma) / (ln S_low - ln S_low+1), 0, 1), t = low + w; exactly j at S_j.
 * plan: one row of 12 doubles per UNet evaluation of the call (strength 1: txt2img; else the img2img tail),
 *     step (index in the full schedule), stage (0 / 1), t, sigma, cx, ce, h1, cz, cz2, qx, qe, a_end:
 *     q = qx x + qe e (pushed to the one history slot);  x' = cx x + ce e + h1 q_-1 + cz z + cz2 z2  on the VP latent, z = draw 0 and z2 = draw 1 of the row's step;
 *     a_end = 1 / (1 + s'^2) on a step's last evaluation, -1 otherwise.
 * SDMI_ERR_INVALID: a struct sdmi_set_ksampler refuses, n_steps outside 1 .. total, strength outside (0, 1] or leaving no step, capacity too small (in entries of the
 * output: sigmas, or rows; *count still receives the number needed), a null pointer. */
int sdmi_ksampler_sigmas(const sdmi_ksampler* ksampler, const float* alphas_cumprod, int32_t total, size_t n_steps, double* sigmas, int32_t capacity, int32_t* count);
int sdmi_sigma_to_t(const float* alphas_cumprod, int32_t total, double sigma, double* t);
int sdmi_ksampler_plan(const sdmi_ksampler* ksampler, const float* alphas_cumprod, int32_t total, size_t n_steps, double strength, double* rows, int32_t capacity,
                       int32_t* count);

/* ---- what the model predicts: eps or v (no reference counterpart) ----
 * SD 2.x's 768 models predict v = sqrt(a) eps - sqrt(1 - a) x0 instead of eps.  kind: 0 = eps (the default), 1 = v; sticky; anything else is SDMI_ERR_INVALID and
 * changes nothing.  Every update the engine launches is linear in x and in the guided model output, and so is classifier-free guidance: with a = sqrt(a_t),
 * b = sqrt(1 - a_t) at the evaluation's (possibly fractional) timestep, eps = a v + b x, and the step for v is the step for eps with its coefficient row rewritten --
 * cx += ce b, ce *= a, qx += qe b, qe *= a.  No kernel changes and no launch is added.  It holds for every sdmi_set_sampler and sdmi_set_ksampler kind (there
 * a = 1 / sqrt(1 + sigma^2), b = sigma / sqrt(1 + sigma^2)) and for the default path, which under v runs DDIM(eta = 0) through the sampler-choice step kernel on that
 * table (the default path's own update divides by sqrt(a_t) and is kept as it is) -- and with them for img2img, masks, the hires pass, inpainting and the sharded loop.
 * With eps set every call runs the launches and gives the bits it gave before.  A checkpoint does not say what it predicts (512-base: eps, 768-v: v; the .yaml that says
 * so is not read): the caller chooses.  The _ex forms of the host-only table functions take the same `prediction`. */
int sdmi_set_prediction(sdmi_ctx* ctx, int32_t kind);
int sdmi_sampler_coefs_ex(const sdmi_sampler* sampler, const float* alphas_cumprod, int32_t total, const int32_t* ts, int32_t count,
                          int64_t step_size, int32_t prediction, double* coefs);
int sdmi_ksampler_plan_ex(const sdmi_ksampler* ksampler, const float* alphas_cumprod, int32_t total, size_t n_steps, double strength, int32_t prediction, double* rows,
                          int32_t capacity, int32_t* count);

/* ---- CFG rescale and zero-terminal-SNR schedules (no reference counterpart) ----
 * The other two parts of the recipe v-prediction models are trained by (Lin et al., "Common Diffusion Noise Schedules and Sample Steps are Flawed"); the third,
 * trailing spacing, is the reference's step_by rule wherever n_steps divides the table.
 *
 * sdmi_set_guidance_rescale: phi in [0, 1], sticky, 0 = off (the default).  NaN or a value outside [0, 1] is SDMI_ERR_INVALID and the value in force stays.  With
 * phi != 0 the guided model output g = eu + (ec - eu) scale (eps or v alike) of every evaluation is multiplied, per image b, by
 *     f_b = phi std(ec_b) / std(g_b) + (1 - phi)            (std over the image's 4 h w elements; f_b = 1 where std(g_b) = 0 or a statistic is not finite)
 * before the sampler's linear step -- diffusers' rescale_noise_cfg.  It holds for every sampler, k-sampler, img2img, mask, hires pass, inpainting call and for the
 * sharded loop, still with ONE update launch per UNet evaluation: a step kernel with one workgroup per image, which sweeps the image three times (means, squared
 * deviations, update) with fixed-order sums, so that an image's result depends neither on the batch size nor on its place in the batch.  With phi = 0 every call runs
 * the launches and gives the bits it gave before.
 *
 * sdmi_rescale_zero_snr (host only, f64): s = sqrt(a); s <- (s - s_T) s_0 / (s_0 - s_T); out = float(s^2).  out[n - 1] is exactly 0, out[0] has in[0]'s bits.
 * SDMI_ERR_INVALID for n < 2, entries outside [0, 1], or in[0] <= in[n - 1].  in and out may be the same array.
 * sdmi_set_zero_snr: sticky; the context keeps the table it loaded and samples on the rescaled one, whether set before or after a loader; 0 restores the loaded table
 * bit for bit.  sdmi_schedule reads the table in force (out NULL: *count alone; capacity below the count is SDMI_ERR_INVALID).
 * On a table that holds a = 0: sdmi_sampler_coefs_ex writes the rows with a_t = 0 from x0 = -v, eps = x (nothing is singular under v) and leaves every other row as it
 * was; eps-prediction is SDMI_ERR_INVALID there -- from sdmi_sampler_coefs(_ex) and from every sampling entry, before any launch: eps does not determine x0 at a = 0 --
 * and a sigma-schedule sampler is SDMI_ERR_UNSUPPORTED (sigma_max is infinite), from sdmi_set_ksampler, sdmi_ksampler_sigmas / _plan(_ex) or the sampling call,
 * whichever comes last.  The context stays as it was either way.  img2img at strength 1 starts from x = noise there.
 *
 * sdmi_op_sampler_step: one update launch on host NCHW tensors.  eps [2n][4][h][w] (unconditional half first), latent [n][4][h][w]; row[9] = cx ce h1 h2 h3 cz cz2
 * qx qe; depth 0 / 1 / 3, q_hist [n_hist][n][4][h][w] (NULL where n_hist = 0), q_out [n][4][h][w] (NULL where depth = 0); mask [n][h][w], z0, e0 [n][4][h][w]: all
 * three or none.  rescale = 0 launches the elementwise kernels of the sampler choice. */
int sdmi_set_guidance_rescale(sdmi_ctx* ctx, double phi);
int sdmi_rescale_zero_snr(const float* in, float* out, int32_t n);
int sdmi_set_zero_snr(sdmi_ctx* ctx, int32_t on);
int sdmi_schedule(sdmi_ctx* ctx, float* out, int32_t capacity, int32_t* count);
int sdmi_op_sampler_step(sdmi_ctx* ctx, const float* eps, const float* latent, int32_t n, int32_t h, int32_t w, double scale, double rescale, const double* row,
                         int32_t depth, int32_t n_hist, const float* q_hist, uint64_t noise_key, uint64_t noise_key2, const float* mask, const float* z0,
                         const float* e0, double blend_prev, double blend_dir, float* latent_out, float* q_out);

/* ---- ControlNet (SD v1; no reference counterpart) -----------------------------------------------------
 * A context created with sdmi_config.control_hint_ch = 3 has a fourth weight group, "controlnet/...": a second copy of the UNet's time MLP
 * (controlnet/lin1_time_embed, lin2_time_embed), its 12 input blocks and its middle block under the UNet's own names, the eight hint convolutions
 * controlnet/hint/c0 .. c7 (3x3, pad 1: 3->16, 16->16, 16->32 stride 2, 32->32, 32->96 stride 2, 96->96, 96->256 stride 2, 256->model_channels, SiLU after all but
 * the last; fp32 at every precision), the 1x1 zero convolutions controlnet/zero_convs/0 .. 11 and controlnet/middle_block_out.  The group is all or nothing
 * (sdmi_finalize_weights refuses a partial one); its tensors arrive through sdmi_set_weight (before or after sdmi_finalize_weights), a controlnet/ subtree of the dump
 * directory or sdmi_load_control_safetensors -- never through sdmi_load_weights_packed, whose groups stay 1..7.  Loading another ControlNet does not touch the base model.
 *
 * sdmi_load_control_safetensors: ONE .safetensors file in the ControlNet ("cldm") layout -- keys "control_model.…", F32 / F16 / BF16 -- by the route of
 * sdmi_load_weights_safetensors: memory-mapped, raw bytes to the device, widening and the Linear transpose there, everything checked before the first tensor is
 * staged (a refused file leaves the context as it was).  Key rule (sdmi_checkpoint_key; tests/golden/controlnet_ckpt_keys.txt): the encoder, middle block and time MLP
 * as the UNet's with "control_model." for "model.diffusion_model."; hint/c<i> = control_model.input_hint_block.<2i>; zero_convs/<j> = control_model.zero_convs.<j>.0;
 * middle_block_out = control_model.middle_block_out.0.  The last three families are stated from ControlNet's cldm.py and UNPINNED: no ControlNet file exists offline.
 * Every tensor of the group must be in the file; keys the group has no tensor for are skipped.  Statuses as sdmi_load_weights_safetensors, plus SDMI_ERR_STATE on a
 * context with control_hint_ch = 0.  Out of scope: diffusers-layout ControlNets, .pth pickles, T2I-Adapter, SD 2.x / SDXL ControlNets. */
int sdmi_load_control_safetensors(sdmi_ctx* ctx, const char* path);
/* 1: every tensor of the ControlNet group is set; 0: not (also on a context without one) */
int sdmi_control_ready(sdmi_ctx* ctx);
/* The control state: sticky, like sdmi_set_sampler.  It applies to every later sdmi_unet_forward*, sdmi_sample_* and sdmi_img2img_* call of the context, host-pointer
 * and _dev forms alike.  Per call the hint goes through the hint convolutions once; on every controlled step the control encoder runs on the UNet's own input (the hint
 * embedding enters as the residual of its first convolution; image i of both halves of a CFG batch reads hint i mod n_hint -- both halves are controlled, there is
 * no "guess mode"), the zero convolutions give 13 residuals, and ONE launch (csrc/k_control.hip) adds strength x residual to the UNet's 12 saved skips and to its middle
 * block's output.  The UNet's encoder runs on the unmodified activations.  In sdmi_unet_forward* the step window does not apply: the control is on.  With the state
 * cleared, with strength == 0, or on a step outside the window the forward is the plain one: the same launches, the same bits. */
typedef struct sdmi_control {
    const uint8_t* hint_rgb;   /* HOST, n_hint x [hint_h, hint_w, 3] u8, sample_image's layout; values / 255; copied to the device by the call */
    int32_t n_hint;            /* 1 = one hint for every image of a call, or the n of the later calls */
    int32_t hint_h, hint_w;    /* must be 8 x the latent size in force when a forward runs */
    double strength;           /* multiplies all 13 residuals; finite */
    double start, end;         /* 0 <= start <= end <= 1: step i (0-based) of the S steps a call runs is controlled iff start*S <= i < end*S, in f64 */
    int64_t reserved[4];
} sdmi_control;
/* NULL clears.  SDMI_ERR_STATE: a context without a ControlNet, or one whose group is not completely set.  SDMI_ERR_INVALID -- and nothing changes --: a NULL hint,
 * n_hint < 1, hint_h / hint_w not positive multiples of 64, a non-finite strength, start > end or a bound outside [0, 1].  Later, from the call that runs a forward:
 * SDMI_ERR_INVALID when the latent size in force is not hint / 8, or the call's n is not n_hint (n_hint != 1) -- the message names both sizes.  While a control is set
 * sdmi_hires_* (its first pass runs at another size) and sdmi_sample_image_sharded return SDMI_ERR_UNSUPPORTED. */
int sdmi_set_control(sdmi_ctx* ctx, const sdmi_control* control);
/* Host only: THE window rule of sdmi_control -- 1 when step `step` of `n_steps` is controlled, 0 when not; SDMI_ERR_INVALID for a bad window or step. */
int sdmi_control_step_on(double start, double end, int32_t step, int32_t n_steps);
/* The pieces, for tests and for callers who want them (host pointers).  hint_embed: n hints -> out [n, model_channels, hint_h / 8, hint_w / 8] fp32.
 * residuals: the 13 residual tensors of the sticky hint (strength and window ignored) for x [n,4,h,w], timestep t, context [n,T,ctx_dim] -- NCHW fp32, back to back,
 * zero_convs 0 .. 11 then middle_block_out; sdmi_control_residuals_size(n) floats in all. */
int sdmi_control_hint_embed(sdmi_ctx* ctx, const uint8_t* hint_rgb, int32_t n, int32_t hint_h, int32_t hint_w, float* out);
int64_t sdmi_control_residuals_size(sdmi_ctx* ctx, int32_t n);
int sdmi_control_residuals(sdmi_ctx* ctx, const float* x, int32_t t, const float* context, int32_t n, int32_t T, float* out);
/* Host only, needs no device: THE implementation of the rules above (the engine calls it).  For the `count` timesteps ts a call runs
 * (sample_latent's schedule or its img2img tail; ts[0] is the call's first step) it writes 8 doubles per step,
 *     cx, ce, h1, h2, h3, cz, qx, qe:    q = qx x + qe e  (pushed to history: x0 for kind 1, e for kind 2, unused for kind 0)
 *                                        x' = cx x + ce e + h1 q_-1 + h2 q_-2 + h3 q_-3 + cz z
 * computed in f64 (the engine applies them as f32).  alphas_cumprod has `total` entries; SDMI_ERR_INVALID for a sampler sdmi_set_sampler
 * refuses, a timestep outside [0, total), step_size < 1 or a null pointer. */
int sdmi_sampler_coefs(const sdmi_sampler* sampler, const float* alphas_cumprod, int32_t total, const int32_t* ts, int32_t count,
                       int64_t step_size, double* coefs);

/* ---- FreeU (no reference counterpart) -----------------------------------------------------
 * Si et al., "FreeU: Free Lunch in Diffusion U-Net", as ComfyUI's FreeU / FreeU_V2 nodes ship it: in front of every output block of the UNet the two halves of
 * torch.cat([h, hs]) are re-balanced -- no weights, no training.  The rule is PER BLOCK, keyed on the channel count cx of the backbone tensor h entering the block
 * (mc = model_channels):    cx == 4 mc (output blocks 0..6): (b, s) = (b1, s1);    cx == 2 mc (blocks 7..9): (b2, s2);    otherwise (blocks 10, 11) nothing happens.
 * (diffusers' enable_freeu keys on the resolution instead -- its resolution_idx rule touches other blocks, and is NOT what runs here.)
 *   skip      hs <- Fourier_filter(hs, threshold 1, scale s): fftn over (H, W), fftshift, the box [H/2-1 : H/2+1, W/2-1 : W/2+1] times s, ifftshift, ifftn, real part.
 *             The box holds at most four coefficients, so the engine evaluates it in closed form (csrc/k_freeu.hip) -- one launch per forward for all filtered skips.
 *   backbone  version 1: h[:, :cx/2] *= b.   version 2: m = mean of h over its cx channels, per sample m^ = (m - min m) / (max m - min m),
 *             h[:, :cx/2] *= (b - 1) m^ + 1.  The one deviation from the published code: where max m == min m (a 1 x 1 level) it divides by zero; here m^ = 0.
 *             One launch (version 1) or two (version 2) per affected block.
 * A ControlNet adds to the saved skips and to the middle block's output first; FreeU works on the sums.  Both halves of a CFG batch are treated alike.  fp32
 * arithmetic at every precision; at precision 0 the fp32 tensor and its bf16 planes are both rewritten, at precisions 1 / 2 the bf16 value is rounded once.
 *
 * sdmi_set_freeu: sticky, like sdmi_set_sampler; it applies to every later forward of the context (sdmi_unet_forward*: every call; the sampling entries: the steps
 * of the window start * S <= i < end * S, sdmi_control_step_on's rule and step index -- both evaluations of a two-evaluation sampler's step agree).  version 0
 * clears the state (the other arguments are ignored).  SDMI_ERR_INVALID -- and the state in force stays --: a version outside 0..2, a non-finite parameter, b <= 0,
 * s < 0, start > end or a bound outside [0, 1].  SDMI_ERR_UNSUPPORTED -- likewise --: a model whose cx / 2 or skip widths of the affected blocks are no multiples of
 * 32 (precisions 1 and 2: 64).  A group whose b == 1 runs no backbone launch, one whose s == 1 filters nothing: with all four at 1, with an empty window or with
 * the state cleared every call runs the launches and gives the bits it gave before.
 * sdmi_get_freeu: the state in force (version 0: the other outputs hold the defaults 1, 1, 1, 1, 0, 1); any output may be NULL.
 * sdmi_freeu_plan (host only, needs no context): THE block rule.  For output block i of a model with cfg's model_channels at latent_h x latent_w it writes
 * out[5 i .. 5 i + 4] = group (0 none, 1: b1 / s1, 2: b2 / s2), cx, cskip, h, w -- the shape of the concatenation the block reads.  SDMI_ERR_INVALID: a NULL
 * pointer, model_channels < 1, a latent size sdmi_set_latent_size refuses.
 * sdmi_op_freeu (tests): x [n, c, h, w] = cat([h, hs]) with cx backbone channels, laid out as the engine keeps a block's input -- its precision's storage type, rows
 * wider than c, at precision 0 with bf16 planes beside the fp32 copy where c % 32 == 0 -- through the launches the model runs (the filter where s != 1, the backbone
 * where b != 1), back as y [n, c, h, w].  y_from_planes (may be NULL): h + m + l of the planes.  Returns 1 when the buffer had planes and y_from_planes (if given)
 * was written, 0 when it had none and y_from_planes was left alone, a negative status on an error. */
int sdmi_set_freeu(sdmi_ctx* ctx, int32_t version, float b1, float b2, float s1, float s2, double start, double end);
int sdmi_get_freeu(sdmi_ctx* ctx, int32_t* version, float* b1, float* b2, float* s1, float* s2, double* start, double* end);
int sdmi_freeu_plan(const sdmi_config* cfg, int32_t latent_h, int32_t latent_w, int32_t* out /* 12 x 5 */);
int sdmi_op_freeu(sdmi_ctx* ctx, const float* x, int32_t n, int32_t c, int32_t h, int32_t w, int32_t cx, int32_t version, float b, float s, float* y,
                  float* y_from_planes);

/* ---- IP-Adapter (SD v1; no reference counterpart) ----------------------------------------------------------
 * Ye et al., "IP-Adapter", as diffusers' IPAdapterAttnProcessor runs it: an image prompt enters every cross attention of the UNet through a SECOND attention on
 * the same queries,     a = Attn(q, K_text, V_text) + scale * Attn(q, K_ip, V_ip),     K_ip = tokens Wk_i^T, V_ip = tokens Wv_i^T (no bias),
 * with the same heads and d_head^-1/2 score scale and a softmax of its own over the T_ip image tokens; attn2's output projection then runs on a as before.  The text
 * attention launches exactly as without an adapter; one small launch per cross attention (csrc/k_ipattn.hip) adds the image term to its output.  The ControlNet's
 * transformers are not adapted.  K_ip / V_ip are made once per call, next to the text K / V; they and the adapter's arithmetic are fp32 at every precision.
 *   tokens = image_proj(embeds) = LayerNorm(reshape(Linear(embeds), [T, ctx_dim])): embeds [n, D] is the CALLER's CLIP image embedding (the image encoder is out of
 *   scope, like the ControlNet hint preprocessor); D = 1024 and T = 4 for the published SD 1.5 adapters; eps 1e-5.  Several pictures concatenate along the token axis:
 *   T_ip = T * pictures, 1 <= T_ip <= 64.  The unconditional half of a CFG batch reads image_proj(0) (diffusers' zeros_like negative) unless negative tokens are given.
 * Out of scope: the image encoder, the "plus" / "full-face" / FaceID Resampler (project outside and pass tokens), several adapters at once, per-region image prompts.
 *
 * The adapter's weights (not a weight group: they arrive whole, through one of two calls, before or after sdmi_finalize_weights):
 * sdmi_ip_adapter_load_safetensors: ONE file in h94's ip-adapter_sd15.safetensors layout, F32 / F16 / BF16, through the mapped reader, widened on the device:
 *   image_proj.proj.weight [T ctx_dim, D], image_proj.proj.bias, image_proj.norm.weight, image_proj.norm.bias [ctx_dim],
 *   ip_adapter.<j>.to_k_ip.weight / ip_adapter.<j>.to_v_ip.weight [C, ctx_dim], j odd, counting the cross attentions in diffusers' processor order -- down blocks
 *   (UNet input blocks 1, 2, 4, 5, 7, 8 -> 1 .. 11), up blocks (output blocks 3 .. 11 -> 13 .. 29), then mid (31); sdmi_ip_adapter_key is the rule
 *   (tests/golden/ip_adapter_keys.txt).  The rule is written from the published code and UNPINNED against a real file: none exists offline.
 *   Refused with the key named, before anything is uploaded (SDMI_ERR_WEIGHTS; the adapter in force stays): a missing or extra layer, a shape that does not match the
 *   model, a dtype other than the three; SDMI_ERR_UNSUPPORTED: image_proj.latents / image_proj.layers.* (the "plus" Resampler), a .bin / pickle file.
 * sdmi_ip_adapter_set_weights: the same tensors as HOST fp32 arrays in the file's layouts; wk / wv: 16 pointers, in the engine's order (sdmi_ip_adapter_key's
 *   ctx_index).  SDMI_ERR_INVALID: a null pointer, T < 1, T > 64, D < 32 or D % 32 != 0.  SDMI_ERR_UNSUPPORTED: a model whose UNet head widths are not 40 / 64 / 80 / 160.
 * sdmi_ip_adapter_ready: 1 when an adapter is loaded, else 0.  sdmi_ip_adapter_dims: its D and T (SDMI_ERR_STATE without one).  sdmi_ip_adapter_clear: frees the weights and clears the setting.
 * sdmi_ip_image_tokens: image_proj alone, embeds [n, D] -> out [n, T, ctx_dim] (host pointers).  SDMI_ERR_STATE without an adapter, SDMI_ERR_INVALID: D is not the adapter's.
 * sdmi_ip_adapter_key (host only): cross attention ctx_index (0 .. 15: the input blocks' six, the middle block's, the output blocks' nine) of a model with cfg's
 *   model_channels -> the file key of its to_k_ip (which 0) / to_v_ip (which 1) weight, *j its index in the file and *c its width C; text by the sdmi_checkpoint_key
 *   convention (capacity / needed). */
typedef struct sdmi_ip_adapter {
    const float* tokens;       /* HOST [n_sets, T_ip, token_dim], or NULL when embeds is given */
    const float* embeds;       /* HOST [n_sets, T_ip / T, embed_dim], or NULL: projected by image_proj; exactly one of tokens / embeds */
    const float* neg_tokens;   /* HOST [n_sets, T_ip, token_dim] or NULL: image_proj(0) per picture */
    int32_t n_sets;            /* image i of either half of a CFG batch reads token set i mod n_sets */
    int32_t T_ip;              /* image tokens per set, 1 .. 64 */
    int32_t token_dim;         /* width of tokens / neg_tokens: must be ctx_dim (ignored when neither is given) */
    int32_t embed_dim;         /* width of embeds: must be the adapter's D (ignored without embeds) */
    float scale;               /* finite; 0: the plain forward */
    double start, end;         /* the step window, sdmi_control's rule (sdmi_control_step_on); sdmi_unet_forward*: the adapter is simply on */
    int64_t reserved[4];
} sdmi_ip_adapter;
/* sdmi_set_ip_adapter: sticky, like sdmi_set_control; it applies to every later sdmi_unet_forward* / sdmi_sample_* / sdmi_img2img_* / sdmi_hires_* / sdmi_inpaint_*
 * call, controlled or not, and to each device of a multi-context.  NULL clears the setting (the weights stay).  With no adapter, a cleared setting, scale == 0 or on a
 * step outside the window a forward runs the launches and gives the bits it gave before.  SDMI_ERR_STATE: no adapter is loaded.  SDMI_ERR_INVALID -- the setting in
 * force stays --: both or neither of tokens / embeds, n_sets < 1, T_ip < 1, T_ip not a multiple of T with embeds, token_dim != ctx_dim, embed_dim != D, a non-finite
 * scale, start > end or a bound outside [0, 1].  SDMI_ERR_UNSUPPORTED: T_ip > 64.
 * sdmi_set_ip_adapter_file: sdmi_set_ip_adapter with embeds read from the tensor "image_embeds" [n, D] (F32 / F16 / BF16) of a .safetensors file: one set of n pictures
 * (what the sdmi_sample twin's SDMI_IP_EMBEDS uses).  SDMI_ERR_WEIGHTS: no such tensor, or another dtype.
 * sdmi_get_ip_adapter: the setting in force (pointers NULL); returns 1 when one is set, 0 when none (out untouched).
 * sdmi_op_ip_attention (tests): the operator alone on dense HOST tensors -- q, o_text [n, nq, n_state], k_ip, v_ip [n, T_ip, n_state], scale [n] -- brought to the
 * device in the context's storage type as sdmi_op_qkv_attention_view does (a bf16 q carries the score scale, as the model's), through the launch the model runs, out
 * [n, nq, n_state] fp32.  planes != 0 (precision 0 only, n_state % 32 == 0): O_text goes in as the three bf16 planes and out is what they hold afterwards.
 * sdmi_ip_kv (tests): the per-call K_ip / V_ip a call with n images would hoist (cfg_pair != 0: 2 n batch rows, the unconditional half first), per cross attention
 * i = 0 .. 15 the blocks K_i, V_i [nb, T_ip, C_i] back to back; sdmi_ip_kv_size: floats in all. */
int sdmi_ip_adapter_load_safetensors(sdmi_ctx* ctx, const char* path);
/* host only, needs no context: every check sdmi_ip_adapter_load_safetensors makes, against a model with cfg's model_channels and ctx_dim; *D / *T (may be NULL): the file's */
int sdmi_ip_adapter_check_safetensors(const sdmi_config* cfg, const char* path, int32_t* D, int32_t* T);
int sdmi_ip_adapter_set_weights(sdmi_ctx* ctx, const float* proj_w, const float* proj_b, const float* norm_g, const float* norm_b, int32_t D, int32_t T,
                                const float* const* wk, const float* const* wv);
int sdmi_ip_adapter_ready(sdmi_ctx* ctx);
int sdmi_ip_adapter_dims(sdmi_ctx* ctx, int32_t* D, int32_t* T);
int sdmi_ip_adapter_clear(sdmi_ctx* ctx);
int sdmi_ip_image_tokens(sdmi_ctx* ctx, const float* embeds, int32_t n, int32_t D, float* out);
int sdmi_set_ip_adapter(sdmi_ctx* ctx, const sdmi_ip_adapter* adapter);
int sdmi_set_ip_adapter_file(sdmi_ctx* ctx, const char* embeds_path, float scale, double start, double end);
int sdmi_get_ip_adapter(sdmi_ctx* ctx, sdmi_ip_adapter* out);
int sdmi_ip_adapter_key(const sdmi_config* cfg, int32_t ctx_index, int32_t which, char* out, size_t capacity, size_t* needed, int32_t* j, int32_t* c);
int sdmi_op_ip_attention(sdmi_ctx* ctx, const float* q, const float* k_ip, const float* v_ip, const float* o_text, const float* scale, int32_t n, int32_t nq,
                         int32_t T_ip, int32_t n_state, int32_t n_head, int32_t planes, float* out);
int64_t sdmi_ip_kv_size(sdmi_ctx* ctx, int32_t n, int32_t cfg_pair);
int sdmi_ip_kv(sdmi_ctx* ctx, int32_t n, int32_t cfg_pair, float* out);

/* ---- latent size per call, and the two-pass "hires fix" (no reference counterpart: its latent is hard-coded 4x64x64, stablediffusion/mod.rs:116;
 * DESIGN.md section 9d) ----
 * The weights do not depend on the picture size and the context caches nothing per size, so one context serves any size.  sdmi_config.latent_h / latent_w are
 * the INITIAL size; sdmi_set_latent_size changes it for every later call of the context -- unet_forward, sample_*, img2img_*, decode / encode / latent_to_image,
 * host and device pointers: each reads the current size for its shapes and buffers -- until it is changed again: sticky, like sdmi_set_sampler and
 * sdmi_set_stream.  The rule is sdmi_create's: positive multiples of 8; anything else is SDMI_ERR_INVALID and changes nothing.  The contexts of an sdmi_multi
 * are set one by one (sdmi_multi_ctx); sdmi_sample_image_sharded returns SDMI_ERR_STATE when they disagree. */
int sdmi_set_latent_size(sdmi_ctx* ctx, int32_t h, int32_t w);
int sdmi_get_latent_size(sdmi_ctx* ctx, int32_t* h, int32_t* w);

/* Host only, needs no device: THE resampling rule of one axis (the engine calls it once per axis and applies the table as f32).  Output index o is
 *     y[o] = sum_{j < count[o]} taps[o * *max_taps + j] * x[first[o] + j]          (ascending j; 0 <= first[o], first[o] + count[o] <= in_size)
 * mode 0 nearest-exact (one tap 1.0), 1 bilinear, 2 bicubic; antialias != 0 (modes 1 and 2 only) selects the antialiased filters.  The definition is
 * torch.nn.functional.interpolate(x, size = out_size, mode = ..., align_corners = False, antialias = ...) on the CPU in float64, its border rule and its
 * bicubic constants (A = -0.75; -0.5 antialiased) included; a tap torch clamps to the border is folded onto the border index, so every index is in range.
 * Mode 0: torch keeps two nearest-exact rules, floorf((o + 0.5) * scale) with scale = in / out held in float or in double, which differ where scale (o + 0.5) is
 * an integer in exact arithmetic, and picks by the output size of the whole call (float where out_h + out_w <= 128).  One axis cannot see the other: the table
 * is torch's on a one-axis tensor [1,1,1,in_size] -> (1, out_size), i.e. the float rule where out_size + 1 <= 128, the double rule above.
 * in_size == out_size gives the single tap 1.0 at first[o] = o in every mode.  *max_taps (may be NULL) = the largest count; *needed (may be NULL) = the number
 * of doubles `taps` must hold = out_size * *max_taps; both are always set when the arguments are valid.  first / count hold out_size entries.  With first,
 * count and taps all NULL the call is the capacity query.  SDMI_ERR_INVALID: a size < 1, a mode outside 0..2, antialias with mode 0, some but not all
 * outputs NULL, capacity < *needed (nothing is written). */
int sdmi_resize_weights(int32_t in_size, int32_t out_size, int32_t mode, int32_t antialias, int32_t* first, int32_t* count, double* taps,
                        int32_t capacity, int32_t* max_taps, int32_t* needed);

/* Hires fix: sample at the size the model was trained for, enlarge the latent on the device, re-noise it part-way and finish the schedule at the context's
 * size H x W (the output size, as for every other call):
 *   1. sdmi_sample_latent at base_h x base_w: init_latent [n,4,base_h,base_w] = x_T, or NULL: image i draws from stream seed + i at that size.
 *   2. its final latent resampled to H x W by the rule of sdmi_resize_weights(mode, antialias), rows then columns (csrc/k_resize.hip).
 *   3. sdmi_img2img_latent at H x W, unchanged, without a mask: timesteps sdmi_img2img_timesteps(total, hires_steps ? hires_steps : n_steps, strength),
 *      x_t0 = sqrt(a_t0) z0 + sqrt(1 - a_t0) eps with z0 = the result of 2 and eps = hires_noise [n,4,H,W], or NULL: image i's stream hires_seed + i.
 * The sticky sampler applies to both passes; its history starts empty in the second pass, as in any img2img tail, and both passes key their step noise by the
 * same noise_seed (rule of sdmi_set_sampler: the index in each pass's own full schedule).  Nothing leaves the device between the passes.  The result equals,
 * bit for bit, the composition of the public calls set_latent_size(base), sample_latent, set_latent_size(H, W), sdmi_op_resize, img2img_latent.
 * SDMI_ERR_INVALID: hires NULL, a base size that breaks the size rule, mode outside 0..2, antialias with mode 0, strength outside (0, 1], a schedule that
 * leaves no step (k < 1).  After any error the context's size is what it was.  The GEMM tile tables hold no entries tuned for other sizes than 64 x 64:
 * the planner's fallbacks serve them. */
typedef struct sdmi_hires {
    int32_t base_h, base_w;   /* latent size of the first pass                          */
    int32_t mode;             /* 0 nearest-exact, 1 bilinear, 2 bicubic                 */
    int32_t antialias;        /* modes 1 and 2                                          */
    int64_t hires_steps;      /* schedule length of the second pass; 0 = n_steps        */
    double strength;          /* 0 < strength <= 1                                      */
    uint64_t hires_seed;
    int64_t reserved[4];
} sdmi_hires;
int sdmi_hires_latent(sdmi_ctx* ctx, const float* context, int32_t n, int32_t T, const float* uncond, int32_t Tu, double scale, size_t n_steps,
                      const float* init_latent, uint64_t seed, const sdmi_hires* hires, const float* hires_noise, float* latent_out);
/* rgb_out = sdmi_latent_to_image of sdmi_hires_latent's result: n x [8H,8W,3] uint8 */
int sdmi_hires_image(sdmi_ctx* ctx, const float* context, int32_t n, int32_t T, const float* uncond, int32_t Tu, double scale, size_t n_steps,
                     const float* init_latent, uint64_t seed, const sdmi_hires* hires, const float* hires_noise, uint8_t* rgb_out);

/* ---- a UNet with conditioning channels, and the SD v1 inpainting checkpoints (no reference counterpart: its UNet takes the 4 latent channels, unet/mod.rs:109-143;
 * DESIGN.md section 9f) ----
 * sdmi_config.unet_in_ch = 4 + cond_ch builds a UNet whose first convolution, unet/input_blocks/conv/weight [model_channels, unet_in_ch, 3, 3], reads the latent and
 * cond_ch conditioning channels: 9 = sd-v1-5-inpainting and its derivatives (1 mask channel + the 4-channel latent of the masked picture), 8 = instruct-pix2pix-shaped
 * UNets.  Every loader takes the weight in that shape; the context stores it with its input channels zero-padded to a multiple of 4.  The conditioning is an input of
 * the call, constant over its steps: cond [n, cond_ch, h, w] fp32 NCHW; both halves of a CFG batch -- the unconditional and the conditional forward of sample b --
 * read cond[b].  Only the UNet sees it: schedule, start latent, noise, sampler and mask blend are those of the unconditioned entry.
 * A context with cond_ch > 0 answers the entries that take no cond -- sdmi_unet_forward, sdmi_sample_*, sdmi_img2img_*, sdmi_hires_* -- with SDMI_ERR_STATE (the
 * message names the _cond entry) and sdmi_sample_image_sharded with SDMI_ERR_UNSUPPORTED; the _cond entries and sdmi_inpaint_cond / sdmi_inpaint_image on a
 * 4-channel context, and sdmi_inpaint_* where unet_in_ch != 9, are SDMI_ERR_STATE.  A NULL cond is SDMI_ERR_INVALID. */

/* sdmi_unet_forward with x [n,4,h,w] joined by cond [n,cond_ch,h,w] in front of the first convolution (torch.cat([x, cond], 1)). */
int sdmi_unet_forward_cond(sdmi_ctx* ctx, const float* x, int32_t t, const float* context, const float* cond /* [n,cond_ch,h,w] */, int32_t n, int32_t T,
                           float* out);
/* sdmi_img2img_latent -- timesteps, x_t0, noise streams, the sticky sampler and the optional latent `mask` blend unchanged -- on a conditioned UNet: every forward
 * of the loop reads [x | cond]. */
int sdmi_img2img_latent_cond(sdmi_ctx* ctx, const float* context, int32_t n, int32_t T, const float* uncond, int32_t Tu, double scale, size_t n_steps,
                             double strength, const float* z0, const float* mask, const float* noise, uint64_t seed, const float* cond, float* latent_out);
int sdmi_img2img_latent_cond_dev(sdmi_ctx* ctx, const float* context, int32_t n, int32_t T, const float* uncond, int32_t Tu, double scale, size_t n_steps,
                                 double strength, const float* z0, const float* mask, const float* noise, uint64_t seed, const float* cond, float* latent_out);

/* Host only, needs no device: THE rule that takes a pixel mask to the latent mask.  mask_u8 n x [8h, 8w] uint8, >= 128 = regenerate; out [n, h, w] fp32,
 *     out[b][y][x] = mask_u8[b][8y][8x] >= 128 ? 1 : 0
 * which is torch.nn.functional.interpolate((mask >= 128).float(), size = (h, w)) in its default (legacy) "nearest" mode at the exact scale 8.  The device kernel
 * (csrc/k_inpaint.hip) agrees with it.  SDMI_ERR_INVALID: a NULL pointer, n, h or w < 1. */
int sdmi_inpaint_latent_mask(const uint8_t* mask_u8, int32_t n, int32_t h, int32_t w, float* out);
/* The conditioning of an inpainting checkpoint (unet_in_ch = 9), by the rule of the CompVis inpainting script with the posterior mean for its posterior sample:
 *     masked picture = (v / 127.5 - 1) where mask_u8 < 128, exactly 0 elsewhere          (init_rgb n x [8h,8w,3] uint8 HWC, mask_u8 n x [8h,8w] uint8)
 *     cond_out [n,5,h,w] = [ sdmi_inpaint_latent_mask(mask_u8) | 0.18215 * sdmi_encode_image(masked picture) ]
 * Host pointers.  Needs the encoder weight group and unet_in_ch == 9 (SDMI_ERR_STATE otherwise). */
int sdmi_inpaint_cond(sdmi_ctx* ctx, const uint8_t* init_rgb, const uint8_t* mask_u8, int32_t n, float* cond_out);
/* Inpainting from a picture and a pixel mask in one call: cond = sdmi_inpaint_cond(init_rgb, mask_u8), z0 = 0.18215 * sdmi_encode_image(init_rgb / 127.5 - 1) (the
 * WHOLE picture), sdmi_img2img_latent_cond from z0 with `strength`, `noise` [n,4,h,w] or NULL (stream seed + i) and -- latent_blend = 1 -- the latent mask as its
 * blend mask (NULL mask otherwise), sdmi_latent_to_image, and -- paste_back = 1 -- one last kernel: rgb_out = mask_u8 >= 128 ? generated : init_rgb, byte for byte.
 * Nothing leaves the device between the stages; the result is, bit for bit, the composition of those public calls plus the paste.  opt NULL: both 0. */
typedef struct sdmi_inpaint {
    int32_t latent_blend;   /* 1: blend the kept region toward the re-noised init latent after every step (sdmi_img2img_latent's mask)  */
    int32_t paste_back;     /* 1: pixels with mask_u8 < 128 are copied from init_rgb into rgb_out                                        */
    int64_t reserved[4];
} sdmi_inpaint;
int sdmi_inpaint_image(sdmi_ctx* ctx, const float* context, int32_t n, int32_t T, const float* uncond, int32_t Tu, double scale, size_t n_steps, double strength,
                       const uint8_t* init_rgb, const uint8_t* mask_u8, const sdmi_inpaint* opt, const float* noise, uint64_t seed, uint8_t* rgb_out);
/* device pointers (noise may be NULL) */
int sdmi_inpaint_image_dev(sdmi_ctx* ctx, const float* context, int32_t n, int32_t T, const float* uncond, int32_t Tu, double scale, size_t n_steps, double strength,
                           const uint8_t* init_rgb, const uint8_t* mask_u8, const sdmi_inpaint* opt, const float* noise, uint64_t seed, uint8_t* rgb_out);

/* ---- LoRA adapters: low-rank deltas merged into the packed weights on the device (no reference counterpart) ----
 * The reference runs the base checkpoint only.  An adapter is a set of targets -- conv or Linear weights named by their dump-tree path -- each
 * with two factors; at scale s the context computes with
 *     W = W0 + sum_a c_a (up_a . down_a),   c_a = (float)(s_a alpha_a / rank_a) formed in f64,   a = the adapters on that tensor with c_a != 0,
 * in creation order, all arithmetic fp32 (csrc/k_lora.hip), and re-packs W through the routine the loader uses: at every precision the result is,
 * bit for bit, what sdmi_set_weight of that fp32 W packs.  W0 is the fp32 tensor as loaded, which the context keeps only under the engine option
 * "keep_masters=1" (set before the first weight is loaded; about 3.4 GB for the UNet, 0.5 GB for CLIP at full size): at precision 1 / 2 the device
 * otherwise holds W0 already rounded to bf16 / MXFP8, to which no delta can be added exactly.  A merge is not part of sampling: no launch of a
 * sampling call changes, and a tensor without an active adapter is re-packed from W0 itself (scale 0 restores the loaded model bit for bit).
 * Factor shapes: Linear [in,out]: down [rank,in], up [out,rank].  Conv [cout,cin,k,k]: down [rank,cin,k,k], up [cout,rank].
 * Adapters belong to one context (with sdmi_multi: attach to every sdmi_multi_ctx); several may share a target, their deltas add.
 * An adapter is built target by target from fp32 factors (sdmi_lora_add) or read from a kohya-ss / LyCORIS .safetensors file (sdmi_lora_load_safetensors). */
typedef struct sdmi_lora sdmi_lora;      /* owned by its context; freed by sdmi_lora_destroy or sdmi_destroy */
/* A new adapter with no targets at scale 0.  SDMI_ERR_STATE unless the weights are finalized and "keep_masters=1" was set before they were loaded. */
int sdmi_lora_create(sdmi_ctx* ctx, sdmi_lora** out);
/* Adds one target and copies its factors to the device.  Only while the adapter's scale is 0 (SDMI_ERR_STATE otherwise).  SDMI_ERR_INVALID: an unknown
 * target, a norm / bias / embedding, rank outside 1..256, a non-finite alpha, a target this adapter already has (the factor shapes are the caller's
 * to get right: the pointers carry none).  SDMI_ERR_UNSUPPORTED: a conv_in packed with padded input channels -- the 3-channel RGB one of the VAE encoder, the
 * 9-channel one of an inpainting UNet (an 8-channel one is stored as it is: an ordinary target). */
int sdmi_lora_add(sdmi_lora* a, const char* target, const float* down, const float* up, int32_t rank, float alpha);
/* A kohya-ss / LyCORIS LoRA file (.safetensors), the format adapters are distributed in (DESIGN.md section 9c "files"): a new adapter at scale 0 with one target per
 * module of the file.  Modules are named after the *diffusers* module path -- "lora_unet_down_blocks_0_attentions_0_transformer_blocks_0_attn1_to_q",
 * "lora_te_text_model_encoder_layers_11_mlp_fc2" -- or, by some tools, after the CompVis key ("lora_unet_input_blocks_1_1_proj_in"); both are looked up in a table
 * made from this model's conv / Linear entries (sdmi_lora_module_name; tests/golden/kohya_lora_keys.txt).  Keys of a module X:
 *   X.lora_down.weight [r, in] / [r, cin, k, k], X.lora_up.weight [out, r] / [out, r, 1, 1]                     LoRA, LoCon
 *   X.hada_w1_a, X.hada_w2_a [out, r]; X.hada_w1_b, X.hada_w2_b [r, in] / [r, cin k k] / [r, cin, k, k]         LoHa: delta = (w1_a . w1_b) o (w2_a . w2_b)
 *   X.alpha                    one number of any float dtype; absent: alpha = r                                  c = (float)(s alpha / r), as above
 * in F32, F16 or BF16.  The RAW bytes of each factor go to the device as the file holds them -- one allocation per target, no host widening, no transposed copy:
 * half the memory of sdmi_lora_add's fp32 copies for an F16 file -- and the merge kernel widens them exactly while it reads, so the result is, bit for bit, what
 * sdmi_lora_add of the host-widened factors gives.  A LoHa product is d1 = sum_j w1_a w1_b, d2 = sum_j w2_a w2_b (each an fp32 FMA chain), d1 * d2 rounded once.
 * `which`: SDMI_LORA_UNET, SDMI_LORA_TE or both; modules of the other half are passed over (two adapters from one file carry the two scales of "<lora:name:unet:te>").
 * The whole file is checked against the entries' dims before anything is uploaded, and a refused file leaves the context as it was:
 *   SDMI_ERR_UNSUPPORTED  (the first offending key is named) a Tucker core (lora_mid, hada_t1 / hada_t2), lokr_*, dora_scale, diff / diff_b or any other key kind; a dtype
 *                         other than the three; a rank above 256; a padded conv_in (sdmi_lora_add); a module no entry of THIS model answers to -- a text-encoder layer
 *                         beyond clip_layers, an SDXL name -- unless flags has SDMI_LORA_SKIP_UNKNOWN, which passes such modules (and modules of a weight group that is
 *                         not loaded) over and counts them in *n_skipped;
 *   SDMI_ERR_WEIGHTS      a factor whose shape does not fit the entry, a module with half its factors, a non-finite alpha, a malformed file;
 *   SDMI_ERR_IO           an unreadable file;  SDMI_ERR_STATE  as sdmi_lora_create, and a target whose weight group is not loaded (without the skip flag).
 * The call selects the context's device itself (hipSetDevice), like sdmi_lora_add and sdmi_lora_set_scale: with an sdmi_multi it may be made for one sdmi_multi_ctx after
 * the other from one thread.  n_targets / n_skipped may be NULL.  Not read: Tucker, LoKr, DoRA, the PEFT lora_A / lora_B spelling, SDXL / SD 2 names, pickle files. */
#define SDMI_LORA_UNET 1
#define SDMI_LORA_TE 2
#define SDMI_LORA_SKIP_UNKNOWN 1
int sdmi_lora_load_safetensors(sdmi_ctx* ctx, const char* path, int32_t which, int32_t flags, sdmi_lora** out, int32_t* n_targets, int32_t* n_skipped);
/* device bytes held by the raw factors of a file-loaded adapter (0 for one built with sdmi_lora_add) */
int sdmi_lora_factor_bytes(sdmi_lora* a, size_t* bytes);
/* Host only: the kohya module name of the conv / Linear weight `dump_name` ("unet/.../weight", "clip/.../weight") into buf[n], terminator included.
 * SDMI_ERR_INVALID: any other name (a bias, a norm, an embedding, the VAE, a ControlNet), or n too small. */
int sdmi_lora_module_name(const char* dump_name, char* buf, size_t n);
/* Host only, no context: the checks of sdmi_lora_load_safetensors that need no device, against a caller's list of entries -- names[i] a dump name with ndims[i]
 * (4: conv, 2: Linear) dims at dims[4 i ..].  Statuses as above; *n_targets / *n_skipped what a load would report. */
int sdmi_lora_check_safetensors(const char* path, const char* const* names, const int32_t* ndims, const int64_t* dims, int32_t n_entries, int32_t which, int32_t flags,
                                int32_t* n_targets, int32_t* n_skipped);
/* Re-merges and re-packs every target of `a` with ALL adapters active on it; blocks until done.  A non-finite scale is SDMI_ERR_INVALID and changes nothing. */
int sdmi_lora_set_scale(sdmi_lora* a, double scale);
int sdmi_lora_get_scale(sdmi_lora* a, double* scale, int32_t* n_targets);
/* = sdmi_lora_set_scale(a, 0) + free; `a` is invalid afterwards */
int sdmi_lora_destroy(sdmi_lora* a);
/* The fp32 tensor (reference layout) that is currently packed for the conv / Linear weight `name`: W0, or the merge above.  n = its element count
 * (SDMI_ERR_INVALID otherwise, and for names that are no conv / Linear weight); SDMI_ERR_STATE without "keep_masters=1".  While an adapter with a
 * non-zero scale holds a tensor, sdmi_set_weight on it is SDMI_ERR_STATE; otherwise sdmi_set_weight replaces W0 as well. */
int sdmi_lora_effective_weight(sdmi_ctx* ctx, const char* name, float* out, size_t n);

/* qkv_attention (src/model/attention.rs:5-45 == src/backend.rs:88-128; the
 * operator seam of the commented-out `trait Backend`, backend.rs:4-84).
 * q [n,nq,n_state], k,v [n,nk,n_state], mask [>=nq, mask_ld>=nk] additive or
 * NULL -> out [n,nq,n_state].
 * The mask is added to the scaled scores before the softmax, in natural-log units
 * (softmax(q k^T s^2 + mask)), and is shared by every sample and head: row r of the
 * mask, mask[r * mask_ld .. + nk), serves query r of all of them.  nq rows of mask_ld
 * floats are read, so the array must cover at least nq rows (the library cannot see
 * where it ends); mask_ld < nk is SDMI_ERR_INVALID, a mask on a head dim without a
 * fused kernel (not 40 / 64 / 80 / 160) SDMI_ERR_UNSUPPORTED.  -inf entries are
 * allowed; a row without a live key yields NaN, as the reference's softmax does.
 * A masked call runs the fp32 kernel at every precision
 * (tests/test_attention_mask_gpu.py). */
int sdmi_qkv_attention(sdmi_ctx* ctx, const float* q, const float* k, const float* v,
                       const float* mask, int32_t mask_ld, int32_t n, int32_t nq, int32_t nk,
                       int32_t n_state, int32_t n_head, float* out);

/* ---- prompt -> context: tokenizer + CLIP text encoder ---------
 * The step before the hot path.  The CLIP weights (dump subtree clip/...) are an
 * optional group: without them these two functions return SDMI_ERR_STATE and the
 * sampling functions above work unchanged on caller-supplied embeddings. */
typedef struct sdmi_tokenizer sdmi_tokenizer;

/* SimpleTokenizer::new (src/tokenizer.rs:85-120).  The reference opens
 * "bpe_simple_vocab_16e6.txt" in the working directory; here the path is explicit. */
int sdmi_tokenizer_create(sdmi_tokenizer** out, const char* merges_path);
void sdmi_tokenizer_destroy(sdmi_tokenizer* tok);
/* number of vocabulary entries (49408 with the reference's merges file) */
int sdmi_tokenizer_vocab_size(const sdmi_tokenizer* tok);
/* SimpleTokenizer::encode (tokenizer.rs:168-189): UTF-8 text -> ids.  *n_ids is
 * always set to the number of ids the text has; SDMI_ERR_INVALID if capacity is
 * smaller (nothing is written then). */
int sdmi_tokenizer_encode(const sdmi_tokenizer* tok, const char* text, int32_t* ids, int32_t capacity, int32_t* n_ids);
/* SimpleTokenizer::decode (tokenizer.rs:191-196): ids -> UTF-8 (no terminator is
 * written; *n_bytes is always set to the length). */
int sdmi_tokenizer_decode(const sdmi_tokenizer* tok, const int32_t* ids, int32_t n, char* out, int32_t capacity, int32_t* n_bytes);

/* CLIP::forward (src/model/clip/mod.rs:56-75): tokens [n, seq_len] int32 ->
 * out [n, seq_len, ctx_dim]; seq_len <= clip_ctx; causal mask = attn_decoder_mask
 * (src/backend.rs:130-139). */
int sdmi_clip_forward(sdmi_ctx* ctx, const int32_t* tokens, int32_t n, int32_t seq_len, float* out);

/* StableDiffusion::context (src/model/stablediffusion/mod.rs:198-210): tokenises
 * "<|startoftext|>{text}<|endoftext|>" (no padding, no truncation: T = tokens + 2)
 * and runs CLIP.  out holds capacity_tokens x ctx_dim floats; *T is always set;
 * SDMI_ERR_INVALID if T > capacity_tokens or T > clip_ctx.  unconditional_context
 * (:194-196) is context(""), T = 2. */
int sdmi_context(sdmi_ctx* ctx, const sdmi_tokenizer* tok, const char* text, float* out, int32_t capacity_tokens, int32_t* T);

/* ---- web-UI prompt encoding: padded chunks, emphasis, textual-inversion embeddings, CLIP skip (no reference counterpart) ----
 * sdmi_context keeps the reference's rule (unpadded, at most clip_ctx tokens).  The calls below encode a prompt the way the SD v1 front-ends do: the text is
 * parsed for emphasis, cut into chunks of clip_ctx - 2 content tokens, every chunk is "<|startoftext|>" + content + "<|endoftext|>" padded to clip_ctx, all
 * chunks go through CLIP in one batch and their outputs follow one another: T = k * clip_ctx context rows, which every sampling call takes as they are.
 *
 * sdmi_prompt_parse (host only): the A1111 web UI's parse_prompt_attention.  "(" opens a x1.1 span, "[" a /1.1 span, ":<number>)" closes the innermost round
 * span with that factor, "\(", "\)", "\[", "\]", "\\" are literal, a lone "\" is dropped, spans open at the end run to the end, "BREAK" as a word of its own
 * outside every span gives the marker ("BREAK", -1), neighbours of equal weight are merged, weights are f64.  Writes one "weight<TAB>fragment" line per item
 * ("%.17g"; backslash, tab, newline and control characters of the fragment as JSON escapes) by the convention of sdmi_mpk_list: *needed is always set to the
 * bytes required, terminator included; out may be NULL with capacity 0.  SDMI_ERR_INVALID for a weight that is no complete number ("(y:.)"). */
int sdmi_prompt_parse(const char* text, char* out, size_t capacity, size_t* needed);
/* The chunks of a prompt (host only): ids, weights, emb_row [k, clip_ctx].  emphasis = 0: the text is one fragment of weight 1, brackets and BREAK are literal.
 * Fragments are tokenised one by one and every token takes its fragment's weight; start, end and padding positions have weight 1 and emb_row -1.  A chunk that is
 * full closes when the next token arrives; every BREAK marker closes the current chunk, an empty one too; after the last fragment the current chunk closes if it
 * has content or no chunk exists; then empty chunks are appended until k >= min_chunks.  The n_emb embeddings (name, vectors) are matched on the token ids of
 * their names, the longest name first: a match takes emb_vectors[i] content positions with ids = <|endoftext|>, emb_row = first_row(i) + j (rows numbered over
 * the list in order) and the fragment's weight, and moves to a new chunk when it does not fit the current one.  *n_chunks is always set; SDMI_ERR_INVALID for a
 * smaller capacity_chunks (nothing is written), clip_ctx < 3, an empty name, a name without tokens, emb_vectors[i] outside 1 .. clip_ctx - 2. */
int sdmi_prompt_chunks(const sdmi_tokenizer* tok, const char* text, int32_t clip_ctx, int32_t emphasis, int32_t min_chunks, const char* const* emb_names,
                       const int32_t* emb_vectors, int32_t n_emb, int32_t* ids, float* weights, int32_t* emb_row, int32_t capacity_chunks, int32_t* n_chunks);
/* sdmi_clip_forward with three additions; tokens, emb_row (or NULL), weights (or NULL): host arrays [n, seq_len].
 *   emb_row >= 0: that position's token vector is row emb_row of the context's embedding bank (sdmi_embedding_add) instead of the token table's row;
 *   clip_skip = s, 1 <= s <= clip_layers: the first clip_layers - s + 1 blocks, then the final LayerNorm (the web UI's "CLIP skip"; 1 = sdmi_clip_forward);
 *   weights: out[b][t][c] = (z[b][t][c] * w[b][t]) * r_b with r_b = (float)(sum z[b] / sum (z[b] * w[b])) over the seq_len x ctx_dim elements of chunk b --
 *   products fp32, sums f64, r_b = 1 where the weighted sum is exactly 0.  One more launch, and only when some weight differs from 1.
 * With no row >= 0, every weight 1 and clip_skip 1 the call issues the launches of sdmi_clip_forward and returns its bits.  SDMI_ERR_INVALID: a token id or a
 * row out of range (rows: -1 .. bank rows - 1), clip_skip outside 1 .. clip_layers, seq_len > clip_ctx. */
int sdmi_clip_forward_ex(sdmi_ctx* ctx, const int32_t* tokens, const int32_t* emb_row, const float* weights, int32_t n, int32_t seq_len, int32_t clip_skip,
                         float* out);
/* Textual-inversion embeddings of a context: vectors [n_vectors, ctx_dim] fp32 copied to the device bank, the name recorded with its token ids.  Rows are
 * numbered over the embeddings in the order they were added.  SDMI_ERR_INVALID: an empty name, a name without tokens, n_vectors outside 1 .. clip_ctx - 2, a
 * name the context already has.  SDMI_ERR_STATE: clip_layers = 0. */
int sdmi_embedding_add(sdmi_ctx* ctx, const sdmi_tokenizer* tok, const char* name, const float* vectors, int32_t n_vectors);
/* The same from a .safetensors file: the tensor "emb_params", or else the file's only tensor, of shape [ctx_dim] or [v, ctx_dim] in F32 / F16 / BF16, widened on
 * the device.  Another last dimension is SDMI_ERR_INVALID; a malformed file is refused as a checkpoint is (SDMI_ERR_WEIGHTS / SDMI_ERR_IO). */
int sdmi_embedding_load_safetensors(sdmi_ctx* ctx, const sdmi_tokenizer* tok, const char* name, const char* path);
int sdmi_embedding_remove(sdmi_ctx* ctx, const char* name);   /* SDMI_ERR_INVALID: no such name.  Later embeddings move down in the bank. */
/* one "name<TAB>n_vectors" line per embedding, in bank order (convention of sdmi_mpk_list) */
int sdmi_embedding_list(sdmi_ctx* ctx, char* out, size_t capacity, size_t* needed);
typedef struct sdmi_prompt_opts {
    int32_t emphasis;      /* 1: parse brackets, weights and BREAK; 0: the text is literal                                  */
    int32_t clip_skip;     /* 1 .. clip_layers                                                                              */
    int32_t min_chunks;    /* empty chunks are appended up to this count (a negative prompt brought to the positive's length) */
    int32_t reserved[5];   /* must be zero                                                                                  */
} sdmi_prompt_opts;
/* prompt -> context: sdmi_prompt_chunks with the context's embeddings, one batched sdmi_clip_forward_ex over the k chunks.  out holds capacity_tokens x ctx_dim
 * floats and receives [k * clip_ctx, ctx_dim]; *T = k * clip_ctx is always set; SDMI_ERR_INVALID if it exceeds capacity_tokens.  opts NULL: {1, 1, 1}.
 * SDMI_ERR_STATE without the CLIP weights, like sdmi_context. */
int sdmi_encode_prompt(sdmi_ctx* ctx, const sdmi_tokenizer* tok, const char* text, const sdmi_prompt_opts* opts, float* out, int32_t capacity_tokens, int32_t* T);

/* save_images (src/bin/sample/main.rs:118-125; image::save_buffer(.., Rgb8)): one 8-bit RGB image
 * [height, width, 3] -> PNG file.  Host code. */
int sdmi_write_png(const char* path, const uint8_t* rgb, int32_t width, int32_t height);

/* ---- hot path, device pointers (zero-copy; same layouts) ---------------------- */
int sdmi_sample_latent_dev(sdmi_ctx* ctx, const float* context, int32_t n, int32_t T,
                           const float* uncond, int32_t Tu, double scale, size_t n_steps,
                           const float* init_latent, float* latent_out);
int sdmi_latent_to_image_dev(sdmi_ctx* ctx, const float* latent, int32_t n, uint8_t* rgb_out);
int sdmi_sample_image_dev(sdmi_ctx* ctx, const float* context, int32_t n, int32_t T,
                          const float* uncond, int32_t Tu, double scale, size_t n_steps,
                          const float* init_latent, uint8_t* rgb_out);
/* img2img with device pointers (mask / noise may be NULL) */
int sdmi_img2img_latent_dev(sdmi_ctx* ctx, const float* context, int32_t n, int32_t T, const float* uncond, int32_t Tu,
                            double scale, size_t n_steps, double strength, const float* z0, const float* mask,
                            const float* noise, uint64_t seed, float* latent_out);
int sdmi_img2img_image_dev(sdmi_ctx* ctx, const float* context, int32_t n, int32_t T, const float* uncond, int32_t Tu,
                           double scale, size_t n_steps, double strength, const uint8_t* init_rgb, const float* mask,
                           const float* noise, uint64_t seed, uint8_t* rgb_out);
/* hires fix with device pointers: init_latent [n,4,base_h,base_w] is required (as in sdmi_sample_latent_dev); hires_noise may be NULL */
int sdmi_hires_latent_dev(sdmi_ctx* ctx, const float* context, int32_t n, int32_t T, const float* uncond, int32_t Tu, double scale, size_t n_steps,
                          const float* init_latent, const sdmi_hires* hires, const float* hires_noise, float* latent_out);
int sdmi_hires_image_dev(sdmi_ctx* ctx, const float* context, int32_t n, int32_t T, const float* uncond, int32_t Tu, double scale, size_t n_steps,
                         const float* init_latent, const sdmi_hires* hires, const float* hires_noise, uint8_t* rgb_out);

/* ---- multi-GPU: the image batch sharded over the devices of one node ----------------------
 * The reference's caller asks one StableDiffusion for n images of one prompt (src/bin/sample/main.rs:104-109).
 * The path shards over independent images, so a multi-context is: one weights replica + stream + host thread per
 * device inside ONE process, an RCCL communicator over the device list (ncclCommInitAll; librccl is opened
 * lazily here, libsdmi itself links only the HIP runtime), ONE ncclBroadcast over xGMI of the packed prompt
 * embedding [cond | uncond] from the first device per call, contiguous image ranges per device, noise keyed by
 * the GLOBAL image index -- results do not depend on the device count -- and no other collective. */
typedef struct sdmi_multi sdmi_multi;
int sdmi_create_multi(sdmi_multi** out, const sdmi_config* cfg /* .device ignored */, const int32_t* devices, int32_t n_devices);
void sdmi_destroy_multi(sdmi_multi* m);
int32_t sdmi_multi_size(sdmi_multi* m);
/* the per-device context (owned by m): for sdmi_set_weight / sdmi_load_weights_* / sdmi_set_option per device */
sdmi_ctx* sdmi_multi_ctx(sdmi_multi* m, int32_t index);
/* load_stable_diffusion / load_stable_diffusion_model_file / sdmi_load_weights_safetensors on every device in parallel + finalize;
 * kind = "dump" | "burn" | "safetensors" */
int sdmi_multi_load_weights(sdmi_multi* m, const char* kind, const char* path);
/* StableDiffusion::sample_image for n_images of ONE prompt: context [T, ctx_dim], uncond [Tu, ctx_dim] (host);
 * init_latents [n_images,4,h,w] or NULL (image i draws N(0,1) from stream seed + i); rgb_out n_images x [8h,8w,3] (host). */
int sdmi_sample_image_sharded(sdmi_multi* m, const float* context, int32_t T, const float* uncond, int32_t Tu,
                              double scale, size_t n_steps, int32_t n_images, const float* init_latents, uint64_t seed,
                              uint8_t* rgb_out);
/* sdmi_set_sampler on every device context; each shard's image_base is overridden with the global index of its first image, so the
 * step noise, like the start noise, does not depend on the device count.  NULL restores the default. */
int sdmi_multi_set_sampler(sdmi_multi* m, const sdmi_sampler* sampler);
/* sdmi_set_ksampler on every device context (checked once; NULL clears); image_base per shard, as sdmi_multi_set_sampler */
int sdmi_multi_set_ksampler(sdmi_multi* m, const sdmi_ksampler* ksampler);
/* sdmi_set_guidance_rescale / sdmi_set_zero_snr on every device context: the statistic is per image, so sharding needs nothing else */
int sdmi_multi_set_guidance_rescale(sdmi_multi* m, double phi);
int sdmi_multi_set_zero_snr(sdmi_multi* m, int32_t on);
/* sdmi_set_freeu on every device context (checked by each; a refusal leaves every context as it was): the edits are per sample, so sharding needs nothing else */
int sdmi_multi_set_freeu(sdmi_multi* m, int32_t version, float b1, float b2, float s1, float s2, double start, double end);
/* sdmi_set_ip_adapter on every device context (each holds its own copy of the adapter's weights, loaded through sdmi_multi_ctx).  Every context checks the
 * setting before any takes it, so a refusal, such as SDMI_ERR_STATE from a context without an adapter, leaves every context as it was.
 * Each shard numbers its own images from 0 when it picks a token set, as a control's hints are picked. */
int sdmi_multi_set_ip_adapter(sdmi_multi* m, const sdmi_ip_adapter* adapter);
/* the contiguous global image range [begin, end) device `rank` of `n_ranks` samples (host only): the partition rule of
 * sdmi_sample_image_sharded, and of the one-process-per-GPU launcher (bench.py / sharding.py use the same rule) */
int sdmi_shard_range(int32_t n_images, int32_t rank, int32_t n_ranks, int32_t* begin, int32_t* end);
/* number of RCCL broadcasts issued so far (one per sdmi_sample_image_sharded call) */
int64_t sdmi_multi_broadcast_count(sdmi_multi* m);
/* Diagnostic, needs no device: drives the multi-context's rank runner (one host thread per rank, csrc/multi_ranks.hpp) with n_ranks
 * ranks of which `failing_rank` throws (none if out of range).  Returns SDMI_OK when nothing failed; otherwise the failing rank's status
 * with "rank <r>: injected failure" as the last error -- after verifying that every healthy rank ran to completion and that the
 * drain hook (MultiEngine: synchronise every device's stream) ran exactly once before the error surfaced.  The reference has no
 * multi-device path (src/bin/sample/main.rs:104-109 runs one backend); this pins the error contract of sdmi_sample_image_sharded. */
int sdmi_selftest_rank_errors(int32_t n_ranks, int32_t failing_rank);

/* ---- operator-level entry points (parity tests, profiling) -------------------
 * Same math as the Burn primitives / reference modules named; host pointers
 * in reference layouts.  These let tests/ compare each HIP kernel with the
 * oracle at the op boundary (SURVEY.md section 8c "per-op KATs"). */

/* GroupNorm::forward (+ optional SILU::forward): groupnorm/mod.rs:53-82, silu.rs:14-16.
 * x,out [n,c,h,w]; gamma,beta [c]. */
int sdmi_op_group_norm(sdmi_ctx* ctx, const float* x, const float* gamma, const float* beta,
                       int32_t n, int32_t c, int32_t h, int32_t w, int32_t n_group, float eps,
                       int32_t fuse_silu, float* out);
/* precision = 2 only: the same GroupNorm(+SiLU) with its output quantised to MXFP8 (e4m3 elements, one E8M0 scale per 32
 * channels) as the ResBlock convolutions consume it (unet/mod.rs:713-733); `out` is the DEQUANTISED tensor. */
int sdmi_op_group_norm_fp8(sdmi_ctx* ctx, const float* x, const float* gamma, const float* beta,
                           int32_t n, int32_t c, int32_t h, int32_t w, int32_t n_group, float eps,
                           int32_t fuse_silu, float* out);
/* Burn nn::LayerNorm (unet/mod.rs:523-525): x,out [rows,c]. */
int sdmi_op_layer_norm(sdmi_ctx* ctx, const float* x, const float* gamma, const float* beta,
                       int32_t rows, int32_t c, float eps, float* out);
/* Burn nn::conv::Conv2d::forward: x [n,cin,h,w], weight [cout,cin,k,k], bias [cout] or NULL,
 * symmetric zero padding `pad`, `stride`; upsample2x != 0 applies the reference's
 * nearest-2x (unet/mod.rs:392-396) to x first.  out [n,cout,ho,wo]. */
int sdmi_op_conv2d(sdmi_ctx* ctx, const float* x, const float* weight, const float* bias,
                   int32_t n, int32_t cin, int32_t h, int32_t w, int32_t cout, int32_t k,
                   int32_t stride, int32_t pad, int32_t upsample2x, float* out);
/* Burn nn::Linear::forward: x [rows,cin] @ weight [cin,cout] + bias. */
int sdmi_op_linear(sdmi_ctx* ctx, const float* x, const float* weight, const float* bias,
                   int32_t rows, int32_t cin, int32_t cout, float* out);
/* sdmi_op_conv2d with the other two terms a UNet convolution adds in its GEMM epilogue (no reference counterpart; for tests):
 * out = conv(x) + bias + temb[sample] + resid, any of the three NULL.  temb is [n,cout], or [cout] with temb_stride = 0 (one row
 * for the batch, as the UNet's ResBlocks); resid has the output's shape [n,cout,ho,wo].  The engine keeps them the way the model's
 * launches read them: temb as fp32 rows temb_stride (>= cout) floats apart, resid as NHWC rows resid_ld (0: cout) elements apart in
 * the output's storage type (bf16 at precision >= 1), the padding columns NaN. */
int sdmi_op_conv2d_epilogue(sdmi_ctx* ctx, const float* x, const float* weight, const float* bias, const float* temb,
                            int32_t temb_stride, const float* resid, int32_t resid_ld, int32_t n, int32_t cin, int32_t h,
                            int32_t w, int32_t cout, int32_t k, int32_t stride, int32_t pad, int32_t upsample2x, float* out);
/* The tail of a ResBlock whose shortcut is a 1x1 convolution (no reference counterpart; for tests; precision 0 only, cin_x and cout multiples of 32):
 * out = conv3x3(h, w_out, pad 1) + b_out + conv1x1(x, w_skip) + b_skip.  x [n,cin_x,hh,ww], h [n,cout,hh,ww], w_skip [cout,cin_x,1,1], w_out [cout,cout,3,3],
 * biases [cout] or NULL, out [n,cout,hh,ww].  Both inputs reach the engine as bf16 planes, as in the model.  Option skip_slices = 1: ONE split-K launch whose extra
 * K slices compute the shortcut, plus its reduce (an error where that form does not apply); 0: the shortcut's launch, then conv_out with it as the residual.
 * Options gemm_tile / splitk / splitk_aux force the tile and request the (main, auxiliary) slice counts.  out_planes (NULL: none) receives the result the same
 * launch wrote as bf16 planes, joined back to fp32. */
int sdmi_op_conv2d_pair(sdmi_ctx* ctx, const float* x, const float* h, const float* w_skip, const float* b_skip, const float* w_out,
                        const float* b_out, int32_t n, int32_t cin_x, int32_t cout, int32_t hh, int32_t ww, float* out, float* out_planes);
/* The tail of a transformer block with proj_out folded into the MLP's output Linear (no reference counterpart; for tests; precision 0 only, k_main and k_aux
 * multiples of 32): out = u x w_main + b_main + h x w_aux + b_aux + resid.  u [rows,k_main], h [rows,k_aux], w_main [k_main,cout] and w_aux [k_aux,cout] in the
 * Linear layout, biases [cout] or NULL, resid [rows,cout] or NULL, kept as rows resid_ld (0: cout) elements apart.  Both inputs reach the engine as bf16 planes,
 * as in the model.  Option proj_out_fold = 1: ONE split-K launch whose extra K slices compute h x w_aux, plus its reduce, which adds both biases and the residual
 * (an error where that form does not apply); 0: the auxiliary Linear with the residual, then the main one with that as its residual (out_ld must be 0 or cout).
 * Options gemm_tile / splitk / splitk_aux force the tile and request the (main, auxiliary) slice counts.  The engine keeps the result as rows out_ld (0: cout)
 * elements apart; out [rows,cout] (NULL: none) receives the fp32 result, out_planes (NULL: none; cout and out_ld multiples of 32) the one the same launch wrote
 * as bf16 planes, joined back to fp32.  At least one of the two is given. */
int sdmi_op_linear_pair(sdmi_ctx* ctx, const float* u, const float* h, const float* w_main, const float* b_main, const float* w_aux, const float* b_aux,
                        const float* resid, int32_t resid_ld, int32_t rows, int32_t k_main, int32_t k_aux, int32_t cout, int32_t out_ld, float* out,
                        float* out_planes);
/* The folded weights of a transformer block's tail, through the kernel the loader uses (for tests): w_lin [k_main,cmid] and b_lin [cmid] (NULL: zeros) a Linear
 * in the reference layout, w_proj [cout,cmid] a 1x1 convolution -> wf [cout,k_main] = w_proj x w_lin^T (the packed layout) and bf [cout] = w_proj x b_lin, both
 * accumulated in fp64 and rounded once to fp32. */
int sdmi_op_linear_fold(sdmi_ctx* ctx, const float* w_lin, const float* b_lin, const float* w_proj, int32_t k_main, int32_t cmid, int32_t cout, float* wf,
                        float* bf);
/* sdmi_op_linear + resid [rows,cout] (NULL: none), kept as rows resid_ld (0: cout) elements apart like sdmi_op_conv2d_epilogue's. */
int sdmi_op_linear_epilogue(sdmi_ctx* ctx, const float* x, const float* weight, const float* bias, const float* resid,
                            int32_t resid_ld, int32_t rows, int32_t cin, int32_t cout, float* out);
/* ---- the same operators on channel-slice VIEWS (no reference counterpart; for tests) ----
 * The UNet realises Tensor::cat (unet/mod.rs:134) without a copy: the input of an output block is ONE buffer [x channels | skip channels], its
 * producers write channel slices of it and the consumers of a skip read one.  These entries run the operator the same way: the engine allocates
 * the parent buffers, cuts them with its own slice (row stride = the parent's width, base advanced by the offset) and calls the routines the model
 * calls.  Input: x occupies columns [in_off, in_off + cin) of a parent in_ld (>= cin) channels wide whose other columns hold in_fill (NaN in the
 * tests).  Output: the result goes to columns [out_off, out_off + cout) of a parent out_ld wide; the caller passes that parent PREFILLED as
 * NHWC rows [pixels][out_ld] and gets the whole of it back (through the parent's storage type: bf16 at precision >= 1, when cout > 4), so the
 * columns next to the slice are the caller's to judge.  in_planes / out_planes (precision 0): how the parent exists -- 0 or 1 fp32, 2 the three
 * bf16 planes only, 3 both (cuts on multiples of 32 channels); a plane parent is returned joined (exact).  A view with ld < c, off < 0 or
 * off + c > ld is SDMI_ERR_INVALID before anything is launched; a cut the engine's slice refuses (planes off a multiple of 32 channels, a base
 * off a 16-byte boundary) is its SDMI_ERR_STATE.  On an error the parent still comes back as the device left it. */
typedef struct sdmi_op_view {
    int32_t in_ld, in_off;
    int32_t out_ld, out_off;
    float in_fill;
    int32_t in_planes, out_planes;
} sdmi_op_view;
/* sdmi_op_conv2d_epilogue on views: x [n,cin,h,w]; parent [n*ho*wo, out_ld] in and out; parent_planes (NULL unless out_planes = 3): the joined
 * plane copy of the parent, parent then being the fp32 copy. */
int sdmi_op_conv2d_view(sdmi_ctx* ctx, const float* x, const float* weight, const float* bias, const float* temb, int32_t temb_stride,
                        const float* resid, int32_t resid_ld, int32_t n, int32_t cin, int32_t h, int32_t w, int32_t cout, int32_t k,
                        int32_t stride, int32_t pad, int32_t upsample2x, const sdmi_op_view* view, float* parent, float* parent_planes);
/* sdmi_op_linear_epilogue writing a slice (the engine's Linear reads dense rows: in_ld = cin, in_off = 0): parent [rows, out_ld] in and out. */
int sdmi_op_linear_view(sdmi_ctx* ctx, const float* x, const float* weight, const float* bias, const float* resid, int32_t resid_ld,
                        int32_t rows, int32_t cin, int32_t cout, const sdmi_op_view* view, float* parent);
/* GroupNorm (32 groups) reading a slice (in_ld, in_off, in_fill, in_planes of view): x, out [n,c,h,w].  form 0: the context's GroupNorm (fp32 /
 * bf16), 1: the plane-writing form (precision 0), 2: MXFP8 output, dequantised (precision 2). */
int sdmi_op_group_norm_view(sdmi_ctx* ctx, const float* x, const float* gamma, const float* beta, int32_t n, int32_t c, int32_t h, int32_t w,
                            int32_t n_group, float eps, int32_t fuse_silu, const sdmi_op_view* view, int32_t form, float* out);
/* A block boundary: conv3x3(x, w_skip) -> channels [cx, cx + cskip), conv3x3(x, w_x) -> channels [0, cx) of one buffer, GroupNorm(+SiLU) over
 * all cx + cskip.  dense = 0: the convolutions write slices (the model's way); 1: dense results joined by a copy.  out [n,cx+cskip,h,w]. */
int sdmi_op_cat_chain(sdmi_ctx* ctx, const float* x, const float* w_x, const float* b_x, const float* w_skip, const float* b_skip,
                      const float* gamma, const float* beta, int32_t n, int32_t cin, int32_t h, int32_t w, int32_t cx, int32_t cskip,
                      float eps, int32_t fuse_silu, int32_t dense, float* out);
/* GEGLU gate (unet/mod.rs:579-591): proj [rows,2*hidden] -> out [rows,hidden] = a*gelu_erf(gate). */
int sdmi_op_geglu(sdmi_ctx* ctx, const float* proj, int32_t rows, int32_t hidden, float* out);
/* qkv_attention with a per-sample key count (the CFG batch's cross attention; for tests): q [n,nq,n_state],
 * k,v [n,nk,n_state], kv_len [n] with 1 <= kv_len[b] <= nk; row b attends to keys 0 .. kv_len[b]-1 only and never reads
 * the others. No mask. out [n,nq,n_state]. */
int sdmi_op_qkv_attention_ragged(sdmi_ctx* ctx, const float* q, const float* k, const float* v, const int32_t* kv_len,
                                 int32_t n, int32_t nq, int32_t nk, int32_t n_state, int32_t n_head, float* out);
/* qkv_attention on strided and packed VIEWS (no reference counterpart; for tests).  The model never hands attention dense tensors where it matters: the
 * UNet's self attention and every CLIP layer read q, k and v out of ONE buffer written by one GEMM (row stride 3C, bases at +0 / +C / +2C, batch stride
 * rows * 3C), cross attention reads K and V from the per-call context buffers.  This entry runs the operator the same way: q [n,nq,n_state] and
 * k, v [n,nk,n_state] arrive dense, are brought to the device exactly as sdmi_qkv_attention brings them (fp32 at precision 0 and whenever a mask is
 * given, bf16 otherwise, q pre-scaled where the engine's convention says so) and are scattered into parent buffers [n][rows][ld] at columns
 * [off, off + n_state); every other cell of a parent holds in_fill (NaN in the tests).  The batch stride is rows * ld.  packed = 1: q, k and v are
 * slices of one parent (equal ld and rows, disjoint columns); 0: three parents.  The engine then calls the routine the model calls with these
 * pointers, row strides and batch strides.  mask, mask_ld as sdmi_qkv_attention; kv_len as sdmi_op_qkv_attention_ragged, or NULL.
 * Output: the result goes to rows [0, nq) and columns [out_off, out_off + n_state) of every sample of a parent [n][out_rows][out_ld]; the caller
 * passes that parent PREFILLED as fp32 and gets the whole of it back (through the call's storage type: bf16 at precision >= 1 without a mask), so
 * the cells around the slice are the caller's to judge.  out_planes = 1 (precision 0, a fused head dim, n_state a multiple of 32): the kernels'
 * plane-writing epilogue, joined back (exact) -- a dense output only (out_ld = n_state, out_off = 0, out_rows = nq).
 * SDMI_ERR_INVALID, on the host before anything is allocated or launched: ld < off + n_state, rows below nq / nk, packed slices that overlap or
 * differ in ld / rows, an output slice that leaves its parent, a strided plane output, and any ld or off that is no multiple of 16 bytes (4 fp32 /
 * 8 bf16 elements: the kernels load 16 bytes at a time). */
typedef struct sdmi_attn_view {
    int32_t q_ld, q_off, q_rows;
    int32_t k_ld, k_off, k_rows;
    int32_t v_ld, v_off, v_rows;
    int32_t packed;
    float in_fill;
    int32_t out_ld, out_off, out_rows, out_planes;
} sdmi_attn_view;
int sdmi_op_qkv_attention_view(sdmi_ctx* ctx, const float* q, const float* k, const float* v, const float* mask, int32_t mask_ld,
                               const int32_t* kv_len, int32_t n, int32_t nq, int32_t nk, int32_t n_state, int32_t n_head, sdmi_attn_view view,
                               float* parent);
/* The resampler of the hires fix on its own (csrc/k_resize.hip; no reference counterpart): x [n,4,h,w] -> out [n,4,out_h,out_w] by the tables of
 * sdmi_resize_weights(mode, antialias), applied as f32: the horizontal pass, then the vertical one, taps summed in ascending order (bit-identical run to
 * run); an axis whose size does not change is skipped.  Any positive sizes. */
int sdmi_op_resize(sdmi_ctx* ctx, const float* x, int32_t n, int32_t h, int32_t w, int32_t out_h, int32_t out_w, int32_t mode, int32_t antialias,
                   float* out);
/* The checkpoint conversion kernel on its own (csrc/k_unpack.hip; no reference counterpart).
 * raw = ndim-D tensor of `dtype` (0 F32, 1 F16, 2 BF16) in host memory.
 * transform: 0 copy, 1 2-D transpose ([d0,d1] -> [d1,d0]), 2 conv [cout,cin,kh,kw], cin < 32 and no multiple of 4, with cin padded to the next multiple of 4
 * (-> [cout,pc,kh,kw], the added input channels zero: 3 -> 4 the VAE encoder's RGB conv_in, 9 -> 12 an inpainting UNet's; a cin that needs no padding is transform 0's).
 * out = the fp32 stage tensor.  Exact, on the bit patterns: f16 subnormals, infinities and NaN payloads included. */
int sdmi_op_unpack_tensor(sdmi_ctx* ctx, const void* raw, int32_t dtype, int32_t ndim, const int64_t* dims, int32_t transform, float* out);
/* timestep_embedding (unet/mod.rs:19-30): out [dim] for timestep t. */
/* GEGLU::forward (src/model/unet/mod.rs:579-591): x [rows, cin], weight [cin, 2*hidden] (Burn Linear layout), bias
 * [2*hidden] or NULL -> out [rows, hidden] = a * gelu(b), a | b = the halves of x W + bias.  One fused kernel when the
 * shape allows (engine option geglu_fuse), else projection GEMM + gate kernel. */
int sdmi_op_geglu_forward(sdmi_ctx* ctx, const float* x, const float* weight, const float* bias, int32_t rows, int32_t cin,
                          int32_t hidden, float* out);
int sdmi_op_timestep_embedding(sdmi_ctx* ctx, int32_t t, int32_t dim, float* out);
/* the same for a fractional t (the k-samplers' evaluation times): t is narrowed to f32 once on the host; at an integer t the bits of the call above */
int sdmi_op_timestep_embedding_f(sdmi_ctx* ctx, double t, int32_t dim, float* out);

/* ---- tuning / introspection ---------------------------------------------------- */
/* "key=value" option of one context (Engine::set_option), e.g. "profile=1", "gemm_tile=auto".  No reference counterpart (the
 * reference's knobs are Burn backend type parameters, sample/main.rs:59-83).  An unknown key returns SDMI_ERR_INVALID.  The
 * defaults are the measured configuration; the option table -- arithmetic selectors (gemm_f32s, attn_split, gemm_planes and
 * the fp32 semantics of the split kernels at the edges of the range), the precision >= 1 / = 2 selectors, launch geometry,
 * profiling and dump switches -- is DESIGN.md section 11, one line per key. */
int sdmi_set_option(sdmi_ctx* ctx, const char* key, const char* value);
/* time (ms, HIP events on the context stream) and kernel count of the last
 * hot-path call; flops = the FLOPs it EXECUTED (2*MAC of conv/GEMM/attention as launched: an
 * up-convolution run as four folded 2x2 phase convolutions -- option ups_phase -- counts 4/9 of the
 * layer's 2*MAC, a paired launch both of its problems). */
int sdmi_last_call_stats(sdmi_ctx* ctx, double* gpu_ms, int64_t* n_kernels, double* flops);
/* Per-kernel-class timing collected while option "profile" = "1": HIP events around every
 * launch on the context stream.  cls: 0 conv_gemm (implicit-GEMM conv/linear), 1 splitk_reduce,
 * 2 attention, 3 group_norm(+silu), 4 layer_norm, 5 conv_gemm_fp8 (the MXFP8 convs of precision = 2),
 * 6 conv_gemm_split (precision = 0: the conv/linear launches that run on the bf16 matrix pipe with three-way split fp32
 * operands, k_gemm3x.hip / k_gemm3p.hip; class 0 then holds the launches left on the fp32 matrix instruction), 7 split_rows (fp32 tensors
 * converted to bf16 planes for a plane GEMM outside their producer), 8 other (every launch of the path that is in no other class: layout converters, the
 * CFG + DDIM update, the sampler-choice step (k_sampler.hip), img2img's u8 -> fp32 input conversion, start latent and masked CFG + DDIM update, the conditioned UNet's input assembly and the inpainting conditioning / paste kernels (k_inpaint.hip), the resampler of the hires fix (k_resize.hip), timestep embedding, SiLU of the embedding, row softmax / transposes of the unfused VAE attention, u8 conversion), 9 geglu (the GEGLU gate kernels
 * where the gate is not fused into its GEMM; the quantising gate of precision = 2 included).  flops / bytes are the ALGORITHMIC work of
 * those launches (2*M*N*K; one read + one write of the tensor).  "profile_reset" clears. */
int sdmi_profile_stats(sdmi_ctx* ctx, int32_t cls, double* ms, int64_t* launches, double* flops, double* bytes);
/* What an empty HIP-event pair reads on the context stream (ms): calibrated when "profile" is switched on and already subtracted from
 * every sample of sdmi_profile_stats, so that the classes add up to kernel time and not to kernel time + two event records per launch.
 * (No reference counterpart: the reference has no profiler; bench.py reports it next to the roofline block.) */
int sdmi_profile_overhead(sdmi_ctx* ctx, double* ms);
/* micro-benchmark one implicit-GEMM conv shape on device-resident synthetic
 * data: returns average kernel ms over `iters` launches (HIP events). */
int sdmi_bench_conv(sdmi_ctx* ctx, int32_t n, int32_t cin, int32_t h, int32_t w, int32_t cout,
                    int32_t k, int32_t stride, int32_t upsample2x, int32_t tile_cfg, int32_t splitk,
                    int32_t iters, double* ms_out);

/* micro-benchmark qkv_attention on device-resident synthetic q/k/v [n, nq|nk, n_state]:
 * average kernel ms over `iters` launches (HIP events). */
int sdmi_bench_attention(sdmi_ctx* ctx, int32_t n, int32_t nq, int32_t nk, int32_t n_state, int32_t n_head,
                         int32_t iters, double* ms_out);
/* What the context WOULD run for a qkv_attention of this shape under its current options: host only, no launch.  The call planned is the one
 * sdmi_qkv_attention makes (and the UNet's transformer blocks): dense rows of n_head * d_head elements, the context's storage type (fp32 when has_mask is set:
 * the masked path is fp32 at every precision), the three-plane output where option gemm_planes takes it.  Errors are the planner's (SDMI_ERR_UNSUPPORTED for
 * a head dim no kernel serves). */
typedef struct sdmi_attn_plan {
    int32_t kernel;      /* 0 = unfused (GEMM kernels), 1 = k_attn.hip (fp32 matrix instructions), 2 = k_attn_split.hip (fp32 on the bf16 pipe), 3 = k_attn_bf16.hip */
    int32_t waves;       /* per workgroup; 0 for the unfused path                                                                             */
    int32_t q_rows;      /* query rows per workgroup                                                                                          */
    int32_t kv_tile;     /* keys per K / V tile                                                                                               */
    int32_t kv_splits;   /* key slices; > 1: partial results + a merge launch                                                                 */
    int32_t reserved[3];
} sdmi_attn_plan;
int sdmi_attention_plan(sdmi_ctx* ctx, int32_t n, int32_t n_head, int32_t nq, int32_t nk, int32_t d_head, int32_t has_mask, sdmi_attn_plan* out);

#ifdef __cplusplus
}
#endif
#endif /* SDMI_H */
