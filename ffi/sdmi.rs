//! Rust shim over libsdmi.so for Gadersd/stable-diffusion-burn (SOURCE ONLY: there is no Rust
//! toolchain in the build environment, so this file is kept small and obviously correct; it is
//! what a maintainer drops into `src/` next to `src/backend.rs` -- see INTEGRATION.md).
//!
//! It gives `src/bin/sample/main.rs` a `StableDiffusionMi355` with the same four method
//! signatures it already uses on `StableDiffusion<B>` (src/model/stablediffusion/mod.rs:51-67,
//! 69-100, 102-160) but over plain `Vec<f32>` / slices instead of Burn tensors, so the hot path
//! (DDIM + CFG UNet loop, VAE decode) runs in the HIP library.  CLIP and the tokenizer can stay
//! Burn/Rust, or -- when the dump tree holds the clip/ subtree -- run in the library too
//! (`TokenizerMi355`, `StableDiffusionMi355::context`, mirroring stablediffusion/mod.rs:194-210).  Shape errors panic, exactly like the reference's `.unwrap()`s
//! (stablediffusion/mod.rs:86, unet/mod.rs:134); loader errors are `Box<dyn Error>` like
//! `load_stable_diffusion` (stablediffusion/load.rs:16-33).
use std::error::Error;
use std::ffi::{c_char, c_double, c_float, c_int, c_void, CStr, CString};

#[repr(C)]
pub struct SdmiConfig {
    pub device: i32,
    pub model_channels: i32,
    pub n_head: i32,
    pub ctx_dim: i32,
    pub latent_h: i32,
    pub latent_w: i32,
    pub vae_ch: i32,
    pub max_batch: i32,
    pub precision: i32,
    pub clip_layers: i32,
    pub clip_heads: i32,
    pub clip_vocab: i32,
    pub clip_ctx: i32,
    pub unet_in_ch: i32,
    pub reserved: [i32; 2],
}

/// `sdmi_config.control_hint_ch` (0 = no ControlNet, 3 = an RGB hint) is the first of the two reserved words of earlier versions: the field list above keeps
/// the shape the tests pin, the name is served here.
impl SdmiConfig {
    pub fn control_hint_ch(&self) -> i32 { self.reserved[0] }
    pub fn set_control_hint_ch(&mut self, v: i32) { self.reserved[0] = v; }
    /// `sdmi_config.variant` (0 = SD v1, 1 = SD 2.x: 64-wide UNet heads, OpenCLIP text tower) is the second of them.
    pub fn variant(&self) -> i32 { self.reserved[1] }
    pub fn set_variant(&mut self, v: i32) { self.reserved[1] = v; }
}

/// `sdmi_attn_plan` (`sdmi_attention_plan`): kernel 0 = unfused, 1 = k_attn.hip, 2 = k_attn_split.hip, 3 = k_attn_bf16.hip.
#[repr(C)]
#[derive(Default, Debug, Clone, Copy)]
pub struct SdmiAttnPlan {
    pub kernel: i32,
    pub waves: i32,
    pub q_rows: i32,
    pub kv_tile: i32,
    pub kv_splits: i32,
    pub reserved: [i32; 3],
}

/// `sdmi_control` (include/sdmi.h "ControlNet"): the sticky control of a context built with `control_hint_ch = 3`.  `hint_rgb`: HOST, `n_hint` pictures of
/// `[hint_h, hint_w, 3]` u8 (values / 255), copied by the call; step i of the S steps a call runs is controlled iff `start * S <= i < end * S`.
#[repr(C)]
pub struct SdmiControl {
    pub hint_rgb: *const u8,
    pub n_hint: i32,
    pub hint_h: i32,
    pub hint_w: i32,
    pub strength: f64,
    pub start: f64,
    pub end: f64,
    pub reserved: [i64; 4],
}

/// `sdmi_ip_adapter` (include/sdmi.h "IP-Adapter"): the sticky image prompt of a context with a loaded adapter.  Exactly one of `tokens`
/// (`[n_sets, T_ip, token_dim]`, projected outside) and `embeds` (`[n_sets, T_ip / T, embed_dim]`, projected by image_proj) is non-null; `neg_tokens` (may be null:
/// image_proj(0)) is what the unconditional half of a CFG batch reads.  HOST pointers, copied by the call.
#[repr(C)]
pub struct SdmiIpAdapter {
    pub tokens: *const c_float,
    pub embeds: *const c_float,
    pub neg_tokens: *const c_float,
    pub n_sets: i32,
    pub t_ip: i32,
    pub token_dim: i32,
    pub embed_dim: i32,
    pub scale: c_float,
    pub start: f64,
    pub end: f64,
    pub reserved: [i64; 4],
}

/// `sdmi_sampler` (include/sdmi.h "sampler choice"): kind 0 DDIM(eta) -- eta 0 = the reference's sampler = plain Euler, eta 1 =
/// Euler-ancestral --, 1 DPM-Solver++(2M), 2 PLMS.
#[repr(C)]
pub struct SdmiSampler {
    pub kind: i32,
    pub reserved0: i32,
    pub eta: f64,
    pub noise_seed: u64,
    pub image_base: i64,
    pub reserved: [i64; 4],
}

/// `sdmi_ksampler` (include/sdmi.h "sigma-schedule samplers"): kind 0 euler (eta), 1 dpmpp_2m, 2 heun, 3 dpm2, 4 dpmpp_2s (eta), 5 dpmpp_sde (eta),
/// 6 dpmpp_2m_sde (eta); schedule 0 model, 1 karras, 2 exponential, 3 uniform; rho 0 = 7; sigma_min / sigma_max 0 = the model's.
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct SdmiKSampler {
    pub kind: i32,
    pub schedule: i32,
    pub eta: f64,
    pub rho: f64,
    pub sigma_min: f64,
    pub sigma_max: f64,
    pub noise_seed: u64,
    pub image_base: i64,
    pub reserved: [i64; 4],
}

/// `sdmi_hires` (include/sdmi.h "hires fix"): the first pass's latent size, the resampling mode (0 nearest-exact, 1 bilinear, 2 bicubic;
/// antialias for modes 1 and 2) and the img2img tail of the second pass (`hires_steps` 0 = n_steps, 0 < strength <= 1, noise stream `hires_seed + i`).
#[repr(C)]
pub struct SdmiHires {
    pub base_h: i32,
    pub base_w: i32,
    pub mode: i32,
    pub antialias: i32,
    pub hires_steps: i64,
    pub strength: f64,
    pub hires_seed: u64,
    pub reserved: [i64; 4],
}

/// `sdmi_inpaint` (include/sdmi.h "inpainting"): the options of `sdmi_inpaint_image`; all zero = neither.
#[repr(C)]
pub struct SdmiInpaint {
    pub latent_blend: i32,
    pub paste_back: i32,
    pub reserved: [i64; 4],
}

#[link(name = "sdmi")]
extern "C" {
    fn sdmi_default_config(cfg: *mut SdmiConfig) -> c_int;
    fn sdmi_create(out: *mut *mut c_void, cfg: *const SdmiConfig) -> c_int;
    fn sdmi_destroy(ctx: *mut c_void);
    fn sdmi_last_error() -> *const c_char;
    fn sdmi_set_weight(ctx: *mut c_void, name: *const c_char, data: *const c_float, ndim: i32, dims: *const i64) -> c_int;
    fn sdmi_load_weights_dir(ctx: *mut c_void, dump_dir: *const c_char) -> c_int;
    fn sdmi_load_weights_mpk(ctx: *mut c_void, mpk_path: *const c_char) -> c_int;
    fn sdmi_load_weights_safetensors(ctx: *mut c_void, path: *const c_char) -> c_int;
    fn sdmi_safetensors_list(path: *const c_char, out: *mut c_char, capacity: usize, needed: *mut usize) -> c_int;
    fn sdmi_checkpoint_key(dump_name: *const c_char, out: *mut c_char, capacity: usize, needed: *mut usize, transposed: *mut i32) -> c_int;
    fn sdmi_default_alphas_cumprod(out: *mut c_float, n: i32) -> c_int;
    fn sdmi_op_unpack_tensor(ctx: *mut c_void, raw: *const c_void, dtype: i32, ndim: i32, dims: *const i64, transform: i32, out: *mut c_float) -> c_int;
    fn sdmi_op_conv2d_pair(ctx: *mut c_void, x: *const c_float, h: *const c_float, w_skip: *const c_float, b_skip: *const c_float, w_out: *const c_float,
                           b_out: *const c_float, n: i32, cin_x: i32, cout: i32, hh: i32, ww: i32, out: *mut c_float, out_planes: *mut c_float) -> c_int;
    fn sdmi_op_linear_pair(ctx: *mut c_void, u: *const c_float, h: *const c_float, w_main: *const c_float, b_main: *const c_float, w_aux: *const c_float,
                           b_aux: *const c_float, resid: *const c_float, resid_ld: i32, rows: i32, k_main: i32, k_aux: i32, cout: i32, out_ld: i32,
                           out: *mut c_float, out_planes: *mut c_float) -> c_int;
    fn sdmi_op_linear_fold(ctx: *mut c_void, w_lin: *const c_float, b_lin: *const c_float, w_proj: *const c_float, k_main: i32, cmid: i32, cout: i32,
                           wf: *mut c_float, bf: *mut c_float) -> c_int;
    fn sdmi_finalize_weights(ctx: *mut c_void) -> c_int;
    fn sdmi_set_option(ctx: *mut c_void, key: *const c_char, value: *const c_char) -> c_int;
    fn sdmi_create_multi(out: *mut *mut c_void, cfg: *const SdmiConfig, devices: *const i32, n_devices: i32) -> c_int;
    fn sdmi_destroy_multi(m: *mut c_void);
    fn sdmi_multi_load_weights(m: *mut c_void, kind: *const c_char, path: *const c_char) -> c_int;
    fn sdmi_sample_image_sharded(m: *mut c_void, context: *const c_float, t_len: i32, uncond: *const c_float, tu: i32, scale: c_double,
                                 n_steps: usize, n_images: i32, init_latents: *const c_float, seed: u64, rgb_out: *mut u8) -> c_int;
    fn sdmi_unet_forward(ctx: *mut c_void, x: *const c_float, t: i32, context: *const c_float, n: i32, t_len: i32, out: *mut c_float) -> c_int;
    fn sdmi_sample_latent(ctx: *mut c_void, context: *const c_float, n: i32, t_len: i32, uncond: *const c_float, tu: i32,
                          scale: c_double, n_steps: usize, init_latent: *const c_float, seed: u64, latent_out: *mut c_float) -> c_int;
    fn sdmi_decode_latent(ctx: *mut c_void, latent: *const c_float, n: i32, img_out: *mut c_float) -> c_int;
    fn sdmi_latent_to_image(ctx: *mut c_void, latent: *const c_float, n: i32, rgb_out: *mut u8) -> c_int;
    fn sdmi_sample_image(ctx: *mut c_void, context: *const c_float, n: i32, t_len: i32, uncond: *const c_float, tu: i32,
                         scale: c_double, n_steps: usize, init_latent: *const c_float, seed: u64, rgb_out: *mut u8) -> c_int;
    fn sdmi_img2img_timesteps(total: i32, n_steps: usize, strength: c_double, timesteps: *mut i32, capacity: i32, count: *mut i32) -> c_int;
    fn sdmi_img2img_latent(ctx: *mut c_void, context: *const c_float, n: i32, t_len: i32, uncond: *const c_float, tu: i32, scale: c_double,
                           n_steps: usize, strength: c_double, z0: *const c_float, mask: *const c_float, noise: *const c_float, seed: u64,
                           latent_out: *mut c_float) -> c_int;
    fn sdmi_img2img_image(ctx: *mut c_void, context: *const c_float, n: i32, t_len: i32, uncond: *const c_float, tu: i32, scale: c_double,
                          n_steps: usize, strength: c_double, init_rgb: *const u8, mask: *const c_float, noise: *const c_float, seed: u64,
                          rgb_out: *mut u8) -> c_int;
    fn sdmi_unet_forward_cond(ctx: *mut c_void, x: *const c_float, t: i32, context: *const c_float, cond: *const c_float, n: i32, t_len: i32,
                              out: *mut c_float) -> c_int;
    fn sdmi_img2img_latent_cond(ctx: *mut c_void, context: *const c_float, n: i32, t_len: i32, uncond: *const c_float, tu: i32, scale: c_double,
                                n_steps: usize, strength: c_double, z0: *const c_float, mask: *const c_float, noise: *const c_float, seed: u64,
                                cond: *const c_float, latent_out: *mut c_float) -> c_int;
    fn sdmi_img2img_latent_cond_dev(ctx: *mut c_void, context: *const c_float, n: i32, t_len: i32, uncond: *const c_float, tu: i32, scale: c_double,
                                    n_steps: usize, strength: c_double, z0: *const c_float, mask: *const c_float, noise: *const c_float, seed: u64,
                                    cond: *const c_float, latent_out: *mut c_float) -> c_int;
    fn sdmi_inpaint_latent_mask(mask_u8: *const u8, n: i32, h: i32, w: i32, out: *mut c_float) -> c_int;
    fn sdmi_inpaint_cond(ctx: *mut c_void, init_rgb: *const u8, mask_u8: *const u8, n: i32, cond_out: *mut c_float) -> c_int;
    fn sdmi_inpaint_image(ctx: *mut c_void, context: *const c_float, n: i32, t_len: i32, uncond: *const c_float, tu: i32, scale: c_double,
                          n_steps: usize, strength: c_double, init_rgb: *const u8, mask_u8: *const u8, opt: *const SdmiInpaint, noise: *const c_float,
                          seed: u64, rgb_out: *mut u8) -> c_int;
    fn sdmi_inpaint_image_dev(ctx: *mut c_void, context: *const c_float, n: i32, t_len: i32, uncond: *const c_float, tu: i32, scale: c_double,
                              n_steps: usize, strength: c_double, init_rgb: *const u8, mask_u8: *const u8, opt: *const SdmiInpaint, noise: *const c_float,
                              seed: u64, rgb_out: *mut u8) -> c_int;
    fn sdmi_img2img_latent_dev(ctx: *mut c_void, context: *const c_float, n: i32, t_len: i32, uncond: *const c_float, tu: i32, scale: c_double,
                               n_steps: usize, strength: c_double, z0: *const c_float, mask: *const c_float, noise: *const c_float, seed: u64,
                               latent_out: *mut c_float) -> c_int;
    fn sdmi_img2img_image_dev(ctx: *mut c_void, context: *const c_float, n: i32, t_len: i32, uncond: *const c_float, tu: i32, scale: c_double,
                              n_steps: usize, strength: c_double, init_rgb: *const u8, mask: *const c_float, noise: *const c_float, seed: u64,
                              rgb_out: *mut u8) -> c_int;
    fn sdmi_set_latent_size(ctx: *mut c_void, h: i32, w: i32) -> c_int;
    fn sdmi_get_latent_size(ctx: *mut c_void, h: *mut i32, w: *mut i32) -> c_int;
    fn sdmi_hires_image(ctx: *mut c_void, context: *const c_float, n: i32, t_len: i32, uncond: *const c_float, tu: i32, scale: c_double,
                        n_steps: usize, init_latent: *const c_float, seed: u64, hires: *const SdmiHires, hires_noise: *const c_float,
                        rgb_out: *mut u8) -> c_int;
    fn sdmi_set_sampler(ctx: *mut c_void, sampler: *const SdmiSampler) -> c_int;
    fn sdmi_get_sampler(ctx: *mut c_void, out: *mut SdmiSampler) -> c_int;
    fn sdmi_set_ksampler(ctx: *mut c_void, ksampler: *const SdmiKSampler) -> c_int;
    fn sdmi_get_ksampler(ctx: *mut c_void, out: *mut SdmiKSampler, is_set: *mut i32) -> c_int;
    fn sdmi_multi_set_ksampler(m: *mut c_void, ksampler: *const SdmiKSampler) -> c_int;
    fn sdmi_ksampler_sigmas(ksampler: *const SdmiKSampler, alphas_cumprod: *const c_float, total: i32, n_steps: usize, sigmas: *mut c_double, capacity: i32,
                            count: *mut i32) -> c_int;
    fn sdmi_sigma_to_t(alphas_cumprod: *const c_float, total: i32, sigma: c_double, t: *mut c_double) -> c_int;
    fn sdmi_ksampler_plan(ksampler: *const SdmiKSampler, alphas_cumprod: *const c_float, total: i32, n_steps: usize, strength: c_double, rows: *mut c_double,
                          capacity: i32, count: *mut i32) -> c_int;
    fn sdmi_ksampler_plan_ex(ksampler: *const SdmiKSampler, alphas_cumprod: *const c_float, total: i32, n_steps: usize, strength: c_double, prediction: i32,
                             rows: *mut c_double, capacity: i32, count: *mut i32) -> c_int;
    fn sdmi_sampler_coefs_ex(sampler: *const SdmiSampler, alphas_cumprod: *const c_float, total: i32, ts: *const i32, count: i32, step_size: i64, prediction: i32,
                             coefs: *mut c_double) -> c_int;
    fn sdmi_set_prediction(ctx: *mut c_void, kind: i32) -> c_int;
    fn sdmi_set_guidance_rescale(ctx: *mut c_void, phi: c_double) -> c_int;
    fn sdmi_rescale_zero_snr(input: *const c_float, out: *mut c_float, n: i32) -> c_int;
    fn sdmi_set_zero_snr(ctx: *mut c_void, on: i32) -> c_int;
    fn sdmi_schedule(ctx: *mut c_void, out: *mut c_float, capacity: i32, count: *mut i32) -> c_int;
    fn sdmi_op_sampler_step(ctx: *mut c_void, eps: *const c_float, latent: *const c_float, n: i32, h: i32, w: i32, scale: c_double, rescale: c_double,
                            row: *const c_double, depth: i32, n_hist: i32, q_hist: *const c_float, noise_key: u64, noise_key2: u64, mask: *const c_float,
                            z0: *const c_float, e0: *const c_float, blend_prev: c_double, blend_dir: c_double, latent_out: *mut c_float, q_out: *mut c_float) -> c_int;
    fn sdmi_multi_set_guidance_rescale(m: *mut c_void, phi: c_double) -> c_int;
    fn sdmi_multi_set_zero_snr(m: *mut c_void, on: i32) -> c_int;
    fn sdmi_set_freeu(ctx: *mut c_void, version: i32, b1: c_float, b2: c_float, s1: c_float, s2: c_float, start: c_double, end: c_double) -> c_int;
    fn sdmi_get_freeu(ctx: *mut c_void, version: *mut i32, b1: *mut c_float, b2: *mut c_float, s1: *mut c_float, s2: *mut c_float, start: *mut c_double,
                      end: *mut c_double) -> c_int;
    fn sdmi_freeu_plan(cfg: *const SdmiConfig, latent_h: i32, latent_w: i32, out: *mut i32) -> c_int;
    fn sdmi_op_freeu(ctx: *mut c_void, x: *const c_float, n: i32, c: i32, h: i32, w: i32, cx: i32, version: i32, b: c_float, s: c_float, y: *mut c_float,
                     y_from_planes: *mut c_float) -> c_int;
    fn sdmi_multi_set_freeu(m: *mut c_void, version: i32, b1: c_float, b2: c_float, s1: c_float, s2: c_float, start: c_double, end: c_double) -> c_int;
    fn sdmi_attention_plan(ctx: *mut c_void, n: i32, n_head: i32, nq: i32, nk: i32, d_head: i32, has_mask: i32, out: *mut SdmiAttnPlan) -> c_int;
    fn sdmi_checkpoint_key_ex(dump_name: *const c_char, variant: i32, out: *mut c_char, capacity: usize, needed: *mut usize, transposed: *mut i32, slice: *mut i32) -> c_int;
    fn sdmi_safetensors_model_family(path: *const c_char, family: *mut i32) -> c_int;
    fn sdmi_op_timestep_embedding_f(ctx: *mut c_void, t: c_double, dim: i32, out: *mut c_float) -> c_int;
    fn sdmi_load_control_safetensors(ctx: *mut c_void, path: *const c_char) -> c_int;
    fn sdmi_control_ready(ctx: *mut c_void) -> c_int;
    fn sdmi_set_control(ctx: *mut c_void, control: *const SdmiControl) -> c_int;
    fn sdmi_ip_adapter_load_safetensors(ctx: *mut c_void, path: *const c_char) -> c_int;
    fn sdmi_ip_adapter_check_safetensors(cfg: *const SdmiConfig, path: *const c_char, d: *mut i32, t: *mut i32) -> c_int;
    fn sdmi_ip_adapter_set_weights(ctx: *mut c_void, proj_w: *const c_float, proj_b: *const c_float, norm_g: *const c_float, norm_b: *const c_float, d: i32, t: i32,
                                   wk: *const *const c_float, wv: *const *const c_float) -> c_int;
    fn sdmi_ip_adapter_ready(ctx: *mut c_void) -> c_int;
    fn sdmi_ip_adapter_dims(ctx: *mut c_void, d: *mut i32, t: *mut i32) -> c_int;
    fn sdmi_ip_adapter_clear(ctx: *mut c_void) -> c_int;
    fn sdmi_ip_image_tokens(ctx: *mut c_void, embeds: *const c_float, n: i32, d: i32, out: *mut c_float) -> c_int;
    fn sdmi_set_ip_adapter(ctx: *mut c_void, adapter: *const SdmiIpAdapter) -> c_int;
    fn sdmi_set_ip_adapter_file(ctx: *mut c_void, embeds_path: *const c_char, scale: c_float, start: c_double, end: c_double) -> c_int;
    fn sdmi_get_ip_adapter(ctx: *mut c_void, out: *mut SdmiIpAdapter) -> c_int;
    fn sdmi_ip_adapter_key(cfg: *const SdmiConfig, ctx_index: i32, which: i32, out: *mut c_char, capacity: usize, needed: *mut usize, j: *mut i32, c: *mut i32) -> c_int;
    fn sdmi_op_ip_attention(ctx: *mut c_void, q: *const c_float, k_ip: *const c_float, v_ip: *const c_float, o_text: *const c_float, scale: *const c_float, n: i32,
                            nq: i32, t_ip: i32, n_state: i32, n_head: i32, planes: i32, out: *mut c_float) -> c_int;
    fn sdmi_ip_kv_size(ctx: *mut c_void, n: i32, cfg_pair: i32) -> i64;
    fn sdmi_ip_kv(ctx: *mut c_void, n: i32, cfg_pair: i32, out: *mut c_float) -> c_int;
    fn sdmi_multi_set_ip_adapter(m: *mut c_void, adapter: *const SdmiIpAdapter) -> c_int;
    fn sdmi_control_step_on(start: c_double, end: c_double, step: i32, n_steps: i32) -> c_int;
    fn sdmi_control_hint_embed(ctx: *mut c_void, hint_rgb: *const u8, n: i32, hint_h: i32, hint_w: i32, out: *mut c_float) -> c_int;
    fn sdmi_control_residuals_size(ctx: *mut c_void, n: i32) -> i64;
    fn sdmi_control_residuals(ctx: *mut c_void, x: *const c_float, t: i32, context: *const c_float, n: i32, t_len: i32, out: *mut c_float) -> c_int;
    fn sdmi_multi_set_sampler(m: *mut c_void, sampler: *const SdmiSampler) -> c_int;
    fn sdmi_sampler_coefs(sampler: *const SdmiSampler, alphas_cumprod: *const c_float, total: i32, ts: *const i32, count: i32, step_size: i64,
                          coefs: *mut c_double) -> c_int;
    fn sdmi_lora_create(ctx: *mut c_void, out: *mut *mut c_void) -> c_int;
    fn sdmi_lora_add(a: *mut c_void, target: *const c_char, down: *const c_float, up: *const c_float, rank: i32, alpha: c_float) -> c_int;
    fn sdmi_lora_load_safetensors(ctx: *mut c_void, path: *const c_char, which: i32, flags: i32, out: *mut *mut c_void, n_targets: *mut i32, n_skipped: *mut i32) -> c_int;
    fn sdmi_lora_factor_bytes(a: *mut c_void, bytes: *mut usize) -> c_int;
    fn sdmi_lora_module_name(dump_name: *const c_char, buf: *mut c_char, n: usize) -> c_int;
    fn sdmi_lora_check_safetensors(path: *const c_char, names: *const *const c_char, ndims: *const i32, dims: *const i64, n_entries: i32, which: i32, flags: i32,
                                   n_targets: *mut i32, n_skipped: *mut i32) -> c_int;
    fn sdmi_lora_set_scale(a: *mut c_void, scale: c_double) -> c_int;
    fn sdmi_lora_get_scale(a: *mut c_void, scale: *mut c_double, n_targets: *mut i32) -> c_int;
    fn sdmi_lora_destroy(a: *mut c_void) -> c_int;
    fn sdmi_lora_effective_weight(ctx: *mut c_void, name: *const c_char, out: *mut c_float, n: usize) -> c_int;
    fn sdmi_tokenizer_create(out: *mut *mut c_void, merges_path: *const c_char) -> c_int;
    fn sdmi_tokenizer_destroy(tok: *mut c_void);
    fn sdmi_tokenizer_encode(tok: *const c_void, text: *const c_char, ids: *mut i32, capacity: i32, n_ids: *mut i32) -> c_int;
    fn sdmi_context(ctx: *mut c_void, tok: *const c_void, text: *const c_char, out: *mut c_float, capacity_tokens: i32, t: *mut i32) -> c_int;
    // web-UI prompt encoding (include/sdmi.h).  opts: *const SdmiPromptOpts = [emphasis, clip_skip, min_chunks, 0, 0, 0, 0, 0] as [i32; 8], or null
    fn sdmi_prompt_parse(text: *const c_char, out: *mut c_char, capacity: usize, needed: *mut usize) -> c_int;
    fn sdmi_prompt_chunks(tok: *const c_void, text: *const c_char, clip_ctx: i32, emphasis: i32, min_chunks: i32, emb_names: *const *const c_char,
                          emb_vectors: *const i32, n_emb: i32, ids: *mut i32, weights: *mut c_float, emb_row: *mut i32, capacity_chunks: i32, n_chunks: *mut i32) -> c_int;
    fn sdmi_clip_forward_ex(ctx: *mut c_void, tokens: *const i32, emb_row: *const i32, weights: *const c_float, n: i32, seq_len: i32, clip_skip: i32,
                            out: *mut c_float) -> c_int;
    fn sdmi_embedding_add(ctx: *mut c_void, tok: *const c_void, name: *const c_char, vectors: *const c_float, n_vectors: i32) -> c_int;
    fn sdmi_embedding_load_safetensors(ctx: *mut c_void, tok: *const c_void, name: *const c_char, path: *const c_char) -> c_int;
    fn sdmi_embedding_remove(ctx: *mut c_void, name: *const c_char) -> c_int;
    fn sdmi_embedding_list(ctx: *mut c_void, out: *mut c_char, capacity: usize, needed: *mut usize) -> c_int;
    fn sdmi_encode_prompt(ctx: *mut c_void, tok: *const c_void, text: *const c_char, opts: *const [i32; 8], out: *mut c_float, capacity_tokens: i32,
                          t: *mut i32) -> c_int;
    fn sdmi_write_png(path: *const c_char, rgb: *const u8, width: i32, height: i32) -> c_int;
    fn sdmi_qkv_attention(ctx: *mut c_void, q: *const c_float, k: *const c_float, v: *const c_float, mask: *const c_float,
                          mask_ld: i32, n: i32, nq: i32, nk: i32, n_state: i32, n_head: i32, out: *mut c_float) -> c_int;
}

fn last_error() -> String {
    unsafe { CStr::from_ptr(sdmi_last_error()).to_string_lossy().into_owned() }
}

fn check(status: c_int) {
    if status != 0 {
        panic!("libsdmi status {}: {}", status, last_error()); // the reference's hot path is infallible by type
    }
}

/// `SimpleTokenizer` (src/tokenizer.rs:74-196) inside the library.
pub struct TokenizerMi355 {
    tok: *mut c_void,
}

impl TokenizerMi355 {
    /// `SimpleTokenizer::new()` reads "bpe_simple_vocab_16e6.txt" from the working directory (tokenizer.rs:91).
    pub fn new(merges_path: &str) -> Result<Self, Box<dyn Error>> {
        let p = CString::new(merges_path)?;
        let mut tok: *mut c_void = std::ptr::null_mut();
        if unsafe { sdmi_tokenizer_create(&mut tok, p.as_ptr()) } != 0 {
            return Err(last_error().into());
        }
        Ok(Self { tok })
    }

    pub fn encode(&self, text: &str) -> Vec<u32> {
        let t = CString::new(text).expect("prompt contains a NUL byte");
        let cap = 4 * text.len() + 8;
        let mut ids = vec![0i32; cap];
        let mut n = 0i32;
        check(unsafe { sdmi_tokenizer_encode(self.tok, t.as_ptr(), ids.as_mut_ptr(), cap as i32, &mut n) });
        ids[..n as usize].iter().map(|&v| v as u32).collect()
    }
}

impl Drop for TokenizerMi355 {
    fn drop(&mut self) {
        unsafe { sdmi_tokenizer_destroy(self.tok) }
    }
}

pub const LORA_UNET: i32 = 1;
pub const LORA_TE: i32 = 2;
pub const LORA_SKIP_UNKNOWN: i32 = 1;

/// One attached LoRA adapter (`sdmi_lora`).  It borrows its context, so it cannot outlive it; dropping it detaches it (`sdmi_lora_destroy` = scale 0 + free).
pub struct LoraMi355<'a> {
    a: *mut c_void,
    _ctx: std::marker::PhantomData<&'a StableDiffusionMi355>,
}

impl<'a> LoraMi355<'a> {
    /// Re-merges and re-packs every target of the adapter (`sdmi_lora_set_scale`); blocks until done.
    pub fn set_scale(&self, scale: f64) -> Result<(), Box<dyn Error>> {
        if unsafe { sdmi_lora_set_scale(self.a, scale) } != 0 { Err(last_error().into()) } else { Ok(()) }
    }

    /// Device bytes held by the raw factors of a file-loaded adapter (`sdmi_lora_factor_bytes`).
    pub fn factor_bytes(&self) -> Result<usize, Box<dyn Error>> {
        let mut b = 0usize;
        if unsafe { sdmi_lora_factor_bytes(self.a, &mut b) } != 0 { Err(last_error().into()) } else { Ok(b) }
    }

    /// (scale, number of targets) (`sdmi_lora_get_scale`).
    pub fn scale(&self) -> Result<(f64, i32), Box<dyn Error>> {
        let (mut s, mut n) = (0f64, 0i32);
        if unsafe { sdmi_lora_get_scale(self.a, &mut s, &mut n) } != 0 { Err(last_error().into()) } else { Ok((s, n)) }
    }
}

impl<'a> Drop for LoraMi355<'a> {
    fn drop(&mut self) {
        unsafe { sdmi_lora_destroy(self.a); }
    }
}

pub struct StableDiffusionMi355 {
    ctx: *mut c_void,
    ctx_dim: usize,
    clip_ctx: usize,
    latent: usize, // 4 * h * w
}

impl StableDiffusionMi355 {
    /// `load_stable_diffusion(path, device)` (stablediffusion/load.rs:16-33) for the npy dump tree.
    pub fn load(dump_dir: &str, device: i32) -> Result<Self, Box<dyn Error>> {
        unsafe {
            let mut cfg: SdmiConfig = std::mem::zeroed();
            sdmi_default_config(&mut cfg);
            cfg.device = device;
            let mut ctx: *mut c_void = std::ptr::null_mut();
            if sdmi_create(&mut ctx, &cfg) != 0 {
                return Err(last_error().into());
            }
            let dir = CString::new(dump_dir)?;
            if sdmi_load_weights_dir(ctx, dir.as_ptr()) != 0 || sdmi_finalize_weights(ctx) != 0 {
                let e = last_error();
                sdmi_destroy(ctx);
                return Err(e.into());
            }
            Ok(Self { ctx, ctx_dim: cfg.ctx_dim as usize, clip_ctx: cfg.clip_ctx as usize,
                      latent: 4 * (cfg.latent_h * cfg.latent_w) as usize })
        }
    }

    /// An engine option (`sdmi_set_option`; INTEGRATION.md "Options"), e.g. `("gemm_f32s", "0")` + `("attn_split", "0")` for the fp32 matrix
    /// instruction everywhere, or `("fp8_linear", "0")` for round 2's MXFP8 set.  Unknown keys are an error, not ignored.
    pub fn set_option(&mut self, key: &str, value: &str) -> Result<(), Box<dyn Error>> {
        let (k, v) = (CString::new(key)?, CString::new(value)?);
        if unsafe { sdmi_set_option(self.ctx, k.as_ptr(), v.as_ptr()) } != 0 {
            return Err(last_error().into());
        }
        Ok(())
    }

    /// What the loaded UNet predicts (`sdmi_set_prediction`, sticky): 0 = eps (the default), 1 = v (SD 2.x's 768-v models).  The checkpoint does not say: the caller chooses.
    pub fn set_prediction(&mut self, kind: i32) -> Result<(), Box<dyn Error>> {
        if unsafe { sdmi_set_prediction(self.ctx, kind) } != 0 {
            return Err(last_error().into());
        }
        Ok(())
    }

    /// CFG rescale (`sdmi_set_guidance_rescale`, sticky): the guided model output of every evaluation is multiplied per image by
    /// phi * std(cond) / std(guided) + (1 - phi).  phi in [0, 1]; 0 (the default) is off.
    pub fn set_guidance_rescale(&mut self, phi: f64) -> Result<(), Box<dyn Error>> {
        if unsafe { sdmi_set_guidance_rescale(self.ctx, phi) } != 0 {
            return Err(last_error().into());
        }
        Ok(())
    }

    /// FreeU (`sdmi_set_freeu`, sticky): the backbone half of every decoder concatenation scaled by b1 / b2, the low frequencies of its skip
    /// half by s1 / s2 -- the rule keyed on the backbone's channel count, as ComfyUI ships it.  `version` 0 clears, 1 is FreeU, 2 FreeU_V2; `start` / `end`: the
    /// step window of a sampling call.
    #[allow(clippy::too_many_arguments)]
    pub fn set_freeu(&mut self, version: i32, b1: f32, b2: f32, s1: f32, s2: f32, start: f64, end: f64) -> Result<(), Box<dyn Error>> {
        if unsafe { sdmi_set_freeu(self.ctx, version, b1, b2, s1, s2, start, end) } != 0 {
            return Err(last_error().into());
        }
        Ok(())
    }

    /// Sample on the loaded schedule rescaled to zero terminal SNR (`sdmi_set_zero_snr`, sticky); `false` restores the loaded table bit for bit.
    pub fn set_zero_snr(&mut self, on: bool) -> Result<(), Box<dyn Error>> {
        if unsafe { sdmi_set_zero_snr(self.ctx, on as i32) } != 0 {
            return Err(last_error().into());
        }
        Ok(())
    }

    /// The alphas_cumprod table in force (`sdmi_schedule`).
    pub fn schedule(&self) -> Result<Vec<f32>, Box<dyn Error>> {
        let mut count = 0i32;
        if unsafe { sdmi_schedule(self.ctx, std::ptr::null_mut(), 0, &mut count) } != 0 {
            return Err(last_error().into());
        }
        let mut out = vec![0f32; count as usize];
        if count > 0 && unsafe { sdmi_schedule(self.ctx, out.as_mut_ptr(), count, &mut count) } != 0 {
            return Err(last_error().into());
        }
        Ok(out)
    }

    /// What this context would run for a qkv_attention of the shape under its current options (`sdmi_attention_plan`; host only, no launch).
    pub fn attention_plan(&self, n: i32, n_head: i32, nq: i32, nk: i32, d_head: i32, has_mask: bool) -> Result<SdmiAttnPlan, Box<dyn Error>> {
        let mut p = SdmiAttnPlan::default();
        if unsafe { sdmi_attention_plan(self.ctx, n, n_head, nq, nk, d_head, has_mask as i32, &mut p) } != 0 {
            return Err(last_error().into());
        }
        Ok(p)
    }

    /// The latent size [h, w] of every later call (`sdmi_set_latent_size`, sticky; no reference counterpart: the reference's latent is 4x64x64):
    /// positive multiples of 8, pictures are 8x.  The weights do not depend on it.
    pub fn set_latent_size(&mut self, h: i32, w: i32) -> Result<(), Box<dyn Error>> {
        if unsafe { sdmi_set_latent_size(self.ctx, h, w) } != 0 {
            return Err(last_error().into());
        }
        self.latent = 4 * (h * w) as usize;
        Ok(())
    }

    /// The latent size in force (`sdmi_get_latent_size`).
    pub fn latent_size(&self) -> (i32, i32) {
        let (mut h, mut w) = (0i32, 0i32);
        check(unsafe { sdmi_get_latent_size(self.ctx, &mut h, &mut w) });
        (h, w)
    }

    /// Hires fix (include/sdmi.h "hires fix"; no reference counterpart): `sample_image` at `hires.base_h x base_w`, the latent resampled on the
    /// device to the current size, re-noised to the last `strength` of the `hires_steps` schedule and finished there.  Seeds replace the noise tensors.
    pub fn sample_image_hires(&self, context: &[f32], n_batch: usize, unconditional_context: &[f32], unconditional_guidance_scale: f64,
                              n_steps: usize, seed: u64, hires: &SdmiHires) -> Vec<Vec<u8>> {
        let t = context.len() / (n_batch * self.ctx_dim);
        let tu = unconditional_context.len() / self.ctx_dim;
        assert_eq!(context.len(), n_batch * t * self.ctx_dim);
        let per = self.latent / 4 * 64 * 3;
        let mut flat = vec![0u8; n_batch * per];
        check(unsafe {
            sdmi_hires_image(self.ctx, context.as_ptr(), n_batch as i32, t as i32, unconditional_context.as_ptr(), tu as i32,
                             unconditional_guidance_scale, n_steps, std::ptr::null(), seed, hires, std::ptr::null(), flat.as_mut_ptr())
        });
        flat.chunks(per).map(|c| c.to_vec()).collect()
    }

    /// The sampler of every later sampling call (`sdmi_set_sampler`, sticky; no reference counterpart: the reference is DDIM at eta = 0).
    /// kind 0 DDIM with 0 <= eta <= 1, 1 DPM-Solver++(2M), 2 PLMS; `noise_seed` keys the step noise of eta > 0.  `None` restores the default.
    pub fn set_sampler(&mut self, sampler: Option<(i32, f64, u64)>) -> Result<(), Box<dyn Error>> {
        let st = match sampler {
            None => unsafe { sdmi_set_sampler(self.ctx, std::ptr::null()) },
            Some((kind, eta, noise_seed)) => {
                let s = SdmiSampler { kind, reserved0: 0, eta, noise_seed, image_base: 0, reserved: [0; 4] };
                unsafe { sdmi_set_sampler(self.ctx, &s) }
            }
        };
        if st != 0 { Err(last_error().into()) } else { Ok(()) }
    }

    /// A ControlNet in the cldm layout -> the weight group `controlnet/...` (`sdmi_load_control_safetensors`; no reference counterpart).
    pub fn load_control_safetensors(&mut self, path: &str) -> Result<(), Box<dyn Error>> {
        let p = CString::new(path)?;
        if unsafe { sdmi_load_control_safetensors(self.ctx, p.as_ptr()) } != 0 { Err(last_error().into()) } else { Ok(()) }
    }

    /// Whether every tensor of the ControlNet group is set (`sdmi_control_ready`).
    pub fn control_ready(&self) -> bool {
        unsafe { sdmi_control_ready(self.ctx) == 1 }
    }

    /// Load an IP-Adapter in h94's `ip-adapter_sd15.safetensors` layout (`sdmi_ip_adapter_load_safetensors`).
    pub fn load_ip_adapter_safetensors(&mut self, path: &str) -> Result<(), Box<dyn Error>> {
        let p = std::ffi::CString::new(path)?;
        if unsafe { sdmi_ip_adapter_load_safetensors(self.ctx, p.as_ptr()) } != 0 {
            return Err(last_error().into());
        }
        Ok(())
    }

    /// The image prompt of every later forward / sampling call (`sdmi_set_ip_adapter`, sticky): `embeds` = `n_img` CLIP image embeddings of width `embed_dim` back to
    /// back (one set, concatenated along the token axis), `t` = the adapter's tokens per picture; `None` clears.
    pub fn set_ip_adapter(&mut self, prompt: Option<(&[f32], i32, i32, i32, f32, f64, f64)>) -> Result<(), Box<dyn Error>> {
        let st = match prompt {
            None => unsafe { sdmi_set_ip_adapter(self.ctx, std::ptr::null()) },
            Some((embeds, n_img, embed_dim, t, scale, start, end)) => {
                if embeds.len() != (n_img as usize) * (embed_dim as usize) { return Err("set_ip_adapter: embeds must hold n_img * embed_dim values".into()); }
                let a = SdmiIpAdapter { tokens: std::ptr::null(), embeds: embeds.as_ptr(), neg_tokens: std::ptr::null(), n_sets: 1, t_ip: n_img * t, token_dim: 0, embed_dim,
                                        scale, start, end, reserved: [0; 4] };
                unsafe { sdmi_set_ip_adapter(self.ctx, &a) }
            }
        };
        if st != 0 { Err(last_error().into()) } else { Ok(()) }
    }

    /// The control of every later forward / sampling call (`sdmi_set_control`, sticky): `hint` = `n_hint` pictures `[hint_h, hint_w, 3]` u8 back to back,
    /// (strength, start, end) as `sdmi_control` states them.  `None` clears.
    pub fn set_control(&mut self, control: Option<(&[u8], i32, i32, i32, f64, f64, f64)>) -> Result<(), Box<dyn Error>> {
        let st = match control {
            None => unsafe { sdmi_set_control(self.ctx, std::ptr::null()) },
            Some((hint, n_hint, hint_h, hint_w, strength, start, end)) => {
                if hint.len() != (n_hint as usize) * (hint_h as usize) * (hint_w as usize) * 3 { return Err("set_control: hint length".into()); }
                let c = SdmiControl { hint_rgb: hint.as_ptr(), n_hint, hint_h, hint_w, strength, start, end, reserved: [0; 4] };
                unsafe { sdmi_set_control(self.ctx, &c) }
            }
        };
        if st != 0 { Err(last_error().into()) } else { Ok(()) }
    }

    /// The hint embedding `[n, model_channels, hint_h / 8, hint_w / 8]` (`sdmi_control_hint_embed`).
    pub fn control_hint_embed(&self, hint: &[u8], n: i32, hint_h: i32, hint_w: i32, model_channels: i32) -> Result<Vec<f32>, Box<dyn Error>> {
        if hint.len() != (n as usize) * (hint_h as usize) * (hint_w as usize) * 3 { return Err("control_hint_embed: hint length".into()); }
        let mut out = vec![0f32; (n as usize) * (model_channels as usize) * ((hint_h / 8) as usize) * ((hint_w / 8) as usize)];
        if unsafe { sdmi_control_hint_embed(self.ctx, hint.as_ptr(), n, hint_h, hint_w, out.as_mut_ptr()) } != 0 { Err(last_error().into()) } else { Ok(out) }
    }

    /// The 13 residuals of the set control, NCHW back to back (`sdmi_control_residuals`; `sdmi_control_residuals_size` floats).
    pub fn control_residuals(&self, x: &[f32], t: i32, context: &[f32], n: i32, t_len: i32) -> Result<Vec<f32>, Box<dyn Error>> {
        let total = unsafe { sdmi_control_residuals_size(self.ctx, n) };
        if total < 0 { return Err(last_error().into()); }
        let mut out = vec![0f32; total as usize];
        if unsafe { sdmi_control_residuals(self.ctx, x.as_ptr(), t, context.as_ptr(), n, t_len, out.as_mut_ptr()) } != 0 { Err(last_error().into()) } else { Ok(out) }
    }

    /// The sampler in force (`sdmi_get_sampler`).
    pub fn sampler(&self) -> SdmiSampler {
        let mut s = SdmiSampler { kind: 0, reserved0: 0, eta: 0.0, noise_seed: 0, image_base: 0, reserved: [0; 4] };
        check(unsafe { sdmi_get_sampler(self.ctx, &mut s) });
        s
    }

    /// A sigma-schedule sampler for every later sampling call (`sdmi_set_ksampler`, sticky; `None` clears).  It resets `set_sampler`'s choice, and any
    /// `set_sampler` call clears it.
    pub fn set_ksampler(&mut self, ksampler: Option<&SdmiKSampler>) -> Result<(), Box<dyn Error>> {
        let st = unsafe { sdmi_set_ksampler(self.ctx, ksampler.map_or(std::ptr::null(), |k| k as *const SdmiKSampler)) };
        if st != 0 { Err(last_error().into()) } else { Ok(()) }
    }

    /// The k-sampler in force, if one is set (`sdmi_get_ksampler`).
    pub fn ksampler(&self) -> Option<SdmiKSampler> {
        let mut k = SdmiKSampler::default();
        let mut is_set = 0i32;
        check(unsafe { sdmi_get_ksampler(self.ctx, &mut k, &mut is_set) });
        if is_set != 0 { Some(k) } else { None }
    }

    /// The steps + 1 sigmas of `n_steps`, the last 0 (`sdmi_ksampler_sigmas`, host only).
    pub fn ksampler_sigmas(ksampler: &SdmiKSampler, alphas_cumprod: &[f32], n_steps: usize) -> Result<Vec<f64>, Box<dyn Error>> {
        let mut out = vec![0f64; alphas_cumprod.len() + 2];
        let mut count = 0i32;
        let st = unsafe { sdmi_ksampler_sigmas(ksampler, alphas_cumprod.as_ptr(), alphas_cumprod.len() as i32, n_steps, out.as_mut_ptr(), out.len() as i32, &mut count) };
        if st != 0 { return Err(last_error().into()); }
        out.truncate(count as usize);
        Ok(out)
    }

    /// The fractional timestep of `sigma` (`sdmi_sigma_to_t`, host only).
    pub fn sigma_to_t(alphas_cumprod: &[f32], sigma: f64) -> Result<f64, Box<dyn Error>> {
        let mut t = 0f64;
        if unsafe { sdmi_sigma_to_t(alphas_cumprod.as_ptr(), alphas_cumprod.len() as i32, sigma, &mut t) } != 0 { Err(last_error().into()) } else { Ok(t) }
    }

    /// One row per UNet evaluation: step, stage, t, sigma, cx, ce, h1, cz, cz2, qx, qe, a_end (`sdmi_ksampler_plan`, host only).
    pub fn ksampler_plan(ksampler: &SdmiKSampler, alphas_cumprod: &[f32], n_steps: usize, strength: f64) -> Result<Vec<[f64; 12]>, Box<dyn Error>> {
        let cap = 2 * (alphas_cumprod.len() + 1);
        let mut out = vec![[0f64; 12]; cap];
        let mut count = 0i32;
        let st = unsafe {
            sdmi_ksampler_plan(ksampler, alphas_cumprod.as_ptr(), alphas_cumprod.len() as i32, n_steps, strength, out.as_mut_ptr() as *mut c_double, cap as i32, &mut count)
        };
        if st != 0 { return Err(last_error().into()); }
        out.truncate(count as usize);
        Ok(out)
    }

    /// timestep_embedding at a fractional `t` (`sdmi_op_timestep_embedding_f`).
    pub fn op_timestep_embedding_f(&mut self, t: f64, dim: i32) -> Result<Vec<f32>, Box<dyn Error>> {
        let mut out = vec![0f32; dim.max(0) as usize];
        if unsafe { sdmi_op_timestep_embedding_f(self.ctx, t, dim, out.as_mut_ptr()) } != 0 { Err(last_error().into()) } else { Ok(out) }
    }

    /// A LoRA adapter merged into the packed weights on the device (`sdmi_lora_*`; no reference counterpart).  The context must
    /// have been given the option `("keep_masters", "1")` before its weights were loaded.  `targets`: (dump-tree name of a conv / Linear weight,
    /// down `[rank, in]` / `[rank, cin, k, k]`, up `[out, rank]`, rank, alpha).  The adapter is returned at `scale`; it borrows this context (the
    /// sampling methods take `&self`, so they stay usable while it lives).
    pub fn lora_attach(&self, targets: &[(&str, &[f32], &[f32], i32, f32)], scale: f64) -> Result<LoraMi355<'_>, Box<dyn Error>> {
        let mut a: *mut c_void = std::ptr::null_mut();
        if unsafe { sdmi_lora_create(self.ctx, &mut a) } != 0 {
            return Err(last_error().into());
        }
        let lora = LoraMi355 { a, _ctx: std::marker::PhantomData };
        for (name, down, up, rank, alpha) in targets {
            let n = CString::new(*name)?;
            if unsafe { sdmi_lora_add(lora.a, n.as_ptr(), down.as_ptr(), up.as_ptr(), *rank, *alpha) } != 0 {
                return Err(last_error().into());   // dropping `lora` frees what was added
            }
        }
        lora.set_scale(scale)?;
        Ok(lora)
    }

    /// A kohya-ss / LyCORIS `.safetensors` adapter (`sdmi_lora_load_safetensors`) merged at `scale`: `which` = `LORA_UNET`, `LORA_TE` or both,
    /// `flags` = 0 or `LORA_SKIP_UNKNOWN`.  Returns the adapter and the number of modules passed over.
    pub fn lora_load_safetensors(&self, path: &str, which: i32, flags: i32, scale: f64) -> Result<(LoraMi355<'_>, i32), Box<dyn Error>> {
        let p = CString::new(path)?;
        let mut a: *mut c_void = std::ptr::null_mut();
        let (mut n, mut skipped) = (0i32, 0i32);
        if unsafe { sdmi_lora_load_safetensors(self.ctx, p.as_ptr(), which, flags, &mut a, &mut n, &mut skipped) } != 0 {
            return Err(last_error().into());
        }
        let lora = LoraMi355 { a, _ctx: std::marker::PhantomData };
        lora.set_scale(scale)?;
        Ok((lora, skipped))
    }

    /// The kohya module name of a conv / Linear weight of the UNet or the text encoder (`sdmi_lora_module_name`, host only).
    pub fn lora_module_name(dump_name: &str) -> Result<String, Box<dyn Error>> {
        let c = CString::new(dump_name)?;
        let mut buf = vec![0 as c_char; 256];
        if unsafe { sdmi_lora_module_name(c.as_ptr(), buf.as_mut_ptr(), buf.len()) } != 0 {
            return Err(last_error().into());
        }
        Ok(unsafe { CStr::from_ptr(buf.as_ptr()) }.to_string_lossy().into_owned())
    }

    /// The fp32 tensor (reference layout, `n` elements) currently packed for a conv / Linear weight (`sdmi_lora_effective_weight`).
    pub fn effective_weight(&self, name: &str, n: usize) -> Result<Vec<f32>, Box<dyn Error>> {
        let c = CString::new(name)?;
        let mut out = vec![0f32; n];
        if unsafe { sdmi_lora_effective_weight(self.ctx, c.as_ptr(), out.as_mut_ptr(), n) } != 0 {
            return Err(last_error().into());
        }
        Ok(out)
    }

    /// The per-step coefficients `[ts.len()][8]` = cx, ce, h1, h2, h3, cz, qx, qe of a sampler (`sdmi_sampler_coefs`, host only).
    pub fn sampler_coefs(sampler: &SdmiSampler, alphas_cumprod: &[f32], ts: &[i32], step_size: i64) -> Result<Vec<[f64; 8]>, Box<dyn Error>> {
        let mut out = vec![[0f64; 8]; ts.len()];
        let st = unsafe {
            sdmi_sampler_coefs(sampler, alphas_cumprod.as_ptr(), alphas_cumprod.len() as i32, ts.as_ptr(), ts.len() as i32, step_size,
                               out.as_mut_ptr() as *mut c_double)
        };
        if st != 0 { Err(last_error().into()) } else { Ok(out) }
    }

    /// `load_stable_diffusion_model_file(filename, device)` (src/bin/sample/main.rs:27-34): the Burn
    /// `NamedMpkFileRecorder<FullPrecisionSettings>` record, read natively by the library (the recorder appends ".mpk").
    /// `precision`: 0 fp32 (the reference's arithmetic), 1 bf16, 2 bf16 + MXFP8 convolutions and Linear layers (INTEGRATION.md "Precision").
    pub fn load_record(model_name: &str, device: i32, precision: i32) -> Result<Self, Box<dyn Error>> {
        unsafe {
            let mut cfg: SdmiConfig = std::mem::zeroed();
            sdmi_default_config(&mut cfg);
            cfg.device = device;
            cfg.precision = precision;
            let mut ctx: *mut c_void = std::ptr::null_mut();
            if sdmi_create(&mut ctx, &cfg) != 0 {
                return Err(last_error().into());
            }
            let file = if model_name.ends_with(".mpk") { model_name.to_string() } else { format!("{}.mpk", model_name) };
            let path = CString::new(file)?;
            if sdmi_load_weights_mpk(ctx, path.as_ptr()) != 0 || sdmi_finalize_weights(ctx) != 0 {
                let e = last_error();
                sdmi_destroy(ctx);
                return Err(e.into());
            }
            Ok(Self { ctx, ctx_dim: cfg.ctx_dim as usize, clip_ctx: cfg.clip_ctx as usize,
                      latent: 4 * (cfg.latent_h * cfg.latent_w) as usize })
        }
    }

    /// An SD v1.x checkpoint in the CompVis layout, one `.safetensors` file (F32 / F16 / BF16), converted on the device
    /// (`sdmi_load_weights_safetensors`; no reference counterpart: the reference converts checkpoints in Python).
    pub fn load_safetensors(path: &str, device: i32, precision: i32) -> Result<Self, Box<dyn Error>> {
        unsafe {
            let mut cfg: SdmiConfig = std::mem::zeroed();
            sdmi_default_config(&mut cfg);
            cfg.device = device;
            cfg.precision = precision;
            let mut ctx: *mut c_void = std::ptr::null_mut();
            if sdmi_create(&mut ctx, &cfg) != 0 {
                return Err(last_error().into());
            }
            let p = CString::new(path)?;
            if sdmi_load_weights_safetensors(ctx, p.as_ptr()) != 0 || sdmi_finalize_weights(ctx) != 0 {
                let e = last_error();
                sdmi_destroy(ctx);
                return Err(e.into());
            }
            Ok(Self { ctx, ctx_dim: cfg.ctx_dim as usize, clip_ctx: cfg.clip_ctx as usize,
                      latent: 4 * (cfg.latent_h * cfg.latent_w) as usize })
        }
    }

    /// The CompVis checkpoint key of a dump-tree tensor name and whether the checkpoint holds its transpose (`sdmi_checkpoint_key`, host only).
    pub fn checkpoint_key(dump_name: &str) -> Result<(String, bool), Box<dyn Error>> {
        let name = CString::new(dump_name)?;
        let mut buf = vec![0u8; 512];
        let (mut needed, mut transposed) = (0usize, 0i32);
        let st = unsafe { sdmi_checkpoint_key(name.as_ptr(), buf.as_mut_ptr() as *mut c_char, buf.len(), &mut needed, &mut transposed) };
        if st != 0 { return Err(last_error().into()); }
        buf.truncate(needed.saturating_sub(1));
        Ok((String::from_utf8(buf)?, transposed != 0))
    }

    /// The same for a model variant (`sdmi_checkpoint_key_ex`): 1 = SD 2.x in Stability's layout.  The third element is -1 for the key's whole tensor, 0 / 1 / 2 for the
    /// query / key / value third of a fused `attn.in_proj_weight` / `in_proj_bias`.
    pub fn checkpoint_key_ex(dump_name: &str, variant: i32) -> Result<(String, bool, i32), Box<dyn Error>> {
        let name = CString::new(dump_name)?;
        let mut buf = vec![0u8; 512];
        let (mut needed, mut transposed, mut slice) = (0usize, 0i32, -1i32);
        let st = unsafe { sdmi_checkpoint_key_ex(name.as_ptr(), variant, buf.as_mut_ptr() as *mut c_char, buf.len(), &mut needed, &mut transposed, &mut slice) };
        if st != 0 { return Err(last_error().into()); }
        buf.truncate(needed.saturating_sub(1));
        Ok((String::from_utf8(buf)?, transposed != 0, slice))
    }

    /// 1 = an SD v1 checkpoint, 2 = SD 2.x, 0 = neither text encoder's final LayerNorm is in the file (`sdmi_safetensors_model_family`, host only).
    pub fn safetensors_model_family(path: &str) -> Result<i32, Box<dyn Error>> {
        let p = CString::new(path)?;
        let mut family = 0i32;
        if unsafe { sdmi_safetensors_model_family(p.as_ptr(), &mut family) } != 0 { return Err(last_error().into()); }
        Ok(family)
    }

    /// `key\tdtype\tshape\tfile offset\tdump name or -` lines of a `.safetensors` file (`sdmi_safetensors_list`, host only).
    pub fn safetensors_list(path: &str) -> Result<String, Box<dyn Error>> {
        let p = CString::new(path)?;
        let mut needed = 0usize;
        if unsafe { sdmi_safetensors_list(p.as_ptr(), std::ptr::null_mut(), 0, &mut needed) } != 0 { return Err(last_error().into()); }
        let mut buf = vec![0u8; needed];
        if unsafe { sdmi_safetensors_list(p.as_ptr(), buf.as_mut_ptr() as *mut c_char, buf.len(), &mut needed) } != 0 { return Err(last_error().into()); }
        buf.truncate(needed.saturating_sub(1));
        Ok(String::from_utf8(buf)?)
    }

    /// The LDM schedule a checkpoint without `alphas_cumprod` gets (`sdmi_default_alphas_cumprod`, host only).
    pub fn default_alphas_cumprod(n: usize) -> Result<Vec<f32>, Box<dyn Error>> {
        let mut out = vec![0f32; n];
        if unsafe { sdmi_default_alphas_cumprod(out.as_mut_ptr(), n as i32) } != 0 { return Err(last_error().into()); }
        Ok(out)
    }

    /// A schedule rescaled to zero terminal SNR (`sdmi_rescale_zero_snr`, host only): the last entry is exactly 0, the first keeps its bits.
    pub fn rescale_zero_snr(alphas_cumprod: &[f32]) -> Result<Vec<f32>, Box<dyn Error>> {
        let mut out = vec![0f32; alphas_cumprod.len()];
        if unsafe { sdmi_rescale_zero_snr(alphas_cumprod.as_ptr(), out.as_mut_ptr(), alphas_cumprod.len() as i32) } != 0 { return Err(last_error().into()); }
        Ok(out)
    }

    /// The checkpoint conversion kernel on its own (`sdmi_op_unpack_tensor`): `raw` = the tensor's bytes, dtype 0 F32 / 1 F16 / 2 BF16,
    /// transform 0 copy / 1 2-D transpose / 2 `[cout,3,kh,kw]` padded to 4 input channels.
    pub fn op_unpack_tensor(&self, raw: &[u8], dtype: i32, dims: &[i64], transform: i32) -> Result<Vec<f32>, Box<dyn Error>> {
        let count: i64 = dims.iter().product();
        if count <= 0 || raw.len() != count as usize * if dtype == 0 { 4 } else { 2 } { return Err("op_unpack_tensor: raw does not match dims".into()); }
        let mut out = vec![0f32; if transform == 2 { count as usize / 3 * 4 } else { count as usize }];
        let st = unsafe { sdmi_op_unpack_tensor(self.ctx, raw.as_ptr() as *const c_void, dtype, dims.len() as i32, dims.as_ptr(), transform, out.as_mut_ptr()) };
        if st != 0 { Err(last_error().into()) } else { Ok(out) }
    }

    /// The tail of a ResBlock with a 1x1 shortcut (`sdmi_op_conv2d_pair`): `conv3x3(h, w_out) + b_out + conv1x1(x, w_skip) + b_skip`, NCHW, `[n, cout, hh, ww]`.
    /// Option `skip_slices` = 1: one split-K launch carrying the shortcut on extra K slices; 0: two launches.
    #[allow(clippy::too_many_arguments)]
    pub fn op_conv2d_pair(&self, x: &[f32], h: &[f32], w_skip: &[f32], b_skip: &[f32], w_out: &[f32], b_out: &[f32], n: i32, cin_x: i32, cout: i32, hh: i32,
                          ww: i32) -> Result<Vec<f32>, Box<dyn Error>> {
        let px = (n * hh * ww) as usize;
        if x.len() != px * cin_x as usize || h.len() != px * cout as usize || w_skip.len() != (cout * cin_x) as usize || w_out.len() != (cout * cout * 9) as usize
            || b_skip.len() != cout as usize || b_out.len() != cout as usize { return Err("op_conv2d_pair: slices do not match the dims".into()); }
        let mut out = vec![0f32; px * cout as usize];
        let st = unsafe { sdmi_op_conv2d_pair(self.ctx, x.as_ptr(), h.as_ptr(), w_skip.as_ptr(), b_skip.as_ptr(), w_out.as_ptr(), b_out.as_ptr(), n, cin_x, cout, hh, ww,
                                              out.as_mut_ptr(), std::ptr::null_mut()) };
        if st != 0 { Err(last_error().into()) } else { Ok(out) }
    }

    /// The tail of a transformer block with `proj_out` folded into the MLP's output Linear (`sdmi_op_linear_pair`): `u w_main + b_main + h w_aux + b_aux + resid`,
    /// row-major `[rows, cout]`.  Option `proj_out_fold` = 1: one split-K launch carrying `h w_aux` on extra K slices; 0: two launches.
    #[allow(clippy::too_many_arguments)]
    pub fn op_linear_pair(&self, u: &[f32], h: &[f32], w_main: &[f32], b_main: &[f32], w_aux: &[f32], b_aux: &[f32], resid: Option<&[f32]>, rows: i32, k_main: i32,
                          k_aux: i32, cout: i32) -> Result<Vec<f32>, Box<dyn Error>> {
        let (r, km, ka, n) = (rows as usize, k_main as usize, k_aux as usize, cout as usize);
        if u.len() != r * km || h.len() != r * ka || w_main.len() != km * n || w_aux.len() != ka * n || b_main.len() != n || b_aux.len() != n
            || resid.map_or(false, |x| x.len() != r * n) { return Err("op_linear_pair: slices do not match the dims".into()); }
        let mut out = vec![0f32; r * n];
        let st = unsafe { sdmi_op_linear_pair(self.ctx, u.as_ptr(), h.as_ptr(), w_main.as_ptr(), b_main.as_ptr(), w_aux.as_ptr(), b_aux.as_ptr(),
                                              resid.map_or(std::ptr::null(), |x| x.as_ptr()), 0, rows, k_main, k_aux, cout, 0, out.as_mut_ptr(), std::ptr::null_mut()) };
        if st != 0 { Err(last_error().into()) } else { Ok(out) }
    }

    /// The folded weights of that tail (`sdmi_op_linear_fold`): `(w_proj w_lin^T [cout, k_main], w_proj b_lin [cout])`, fp64 accumulation, rounded once.
    pub fn op_linear_fold(&self, w_lin: &[f32], b_lin: &[f32], w_proj: &[f32], k_main: i32, cmid: i32, cout: i32) -> Result<(Vec<f32>, Vec<f32>), Box<dyn Error>> {
        let (km, c, n) = (k_main as usize, cmid as usize, cout as usize);
        if w_lin.len() != km * c || b_lin.len() != c || w_proj.len() != n * c { return Err("op_linear_fold: slices do not match the dims".into()); }
        let (mut wf, mut bf) = (vec![0f32; n * km], vec![0f32; n]);
        let st = unsafe { sdmi_op_linear_fold(self.ctx, w_lin.as_ptr(), b_lin.as_ptr(), w_proj.as_ptr(), k_main, cmid, cout, wf.as_mut_ptr(), bf.as_mut_ptr()) };
        if st != 0 { Err(last_error().into()) } else { Ok((wf, bf)) }
    }

    /// `context(&tokenizer, text)` (stablediffusion/mod.rs:198-210): `[T, ctx_dim]` row-major, T = tokens + 2.
    /// Needs the clip/ subtree in the dump; `unconditional_context` (:194-196) is `context(tok, "")`.
    pub fn context(&self, tokenizer: &TokenizerMi355, text: &str) -> Vec<f32> {
        let t = CString::new(text).expect("prompt contains a NUL byte");
        let mut out = vec![0f32; self.clip_ctx * self.ctx_dim];
        let mut n_tok = 0i32;
        check(unsafe { sdmi_context(self.ctx, tokenizer.tok, t.as_ptr(), out.as_mut_ptr(), self.clip_ctx as i32, &mut n_tok) });
        out.truncate(n_tok as usize * self.ctx_dim);
        out
    }

    /// `save_images` (src/bin/sample/main.rs:118-125) without the `image` crate.
    pub fn save_images(images: &[Vec<u8>], basepath: &str, width: u32, height: u32) -> Result<(), Box<dyn Error>> {
        for (index, img) in images.iter().enumerate() {
            let p = CString::new(format!("{}{}.png", basepath, index))?;
            if unsafe { sdmi_write_png(p.as_ptr(), img.as_ptr(), width as i32, height as i32) } != 0 {
                return Err(last_error().into());
            }
        }
        Ok(())
    }

    /// One tensor of a Burn record / npy dump, by its dump-tree name (unet/load.rs, autoencoder/load.rs).
    pub fn set_weight(&mut self, name: &str, data: &[f32], dims: &[i64]) -> Result<(), Box<dyn Error>> {
        let n = CString::new(name)?;
        let st = unsafe { sdmi_set_weight(self.ctx, n.as_ptr(), data.as_ptr(), dims.len() as i32, dims.as_ptr()) };
        if st != 0 { Err(last_error().into()) } else { Ok(()) }
    }

    /// `sample_image(context [n,T,768], unconditional_context [Tu,768], scale, n_steps) -> Vec<Vec<u8>>`
    /// (stablediffusion/mod.rs:51-67).  `seed` replaces the reference's unseeded `Tensor::random`.
    pub fn sample_image(&self, context: &[f32], n_batch: usize, unconditional_context: &[f32],
                        unconditional_guidance_scale: f64, n_steps: usize, seed: u64) -> Vec<Vec<u8>> {
        let t = context.len() / (n_batch * self.ctx_dim);
        let tu = unconditional_context.len() / self.ctx_dim;
        assert_eq!(context.len(), n_batch * t * self.ctx_dim);
        let per = self.latent / 4 * 64 * 3; // 512*512*3
        let mut flat = vec![0u8; n_batch * per];
        check(unsafe {
            sdmi_sample_image(self.ctx, context.as_ptr(), n_batch as i32, t as i32, unconditional_context.as_ptr(), tu as i32,
                              unconditional_guidance_scale, n_steps, std::ptr::null(), seed, flat.as_mut_ptr())
        });
        flat.chunks(per).map(|c| c.to_vec()).collect()
    }

    /// img2img (include/sdmi.h "img2img"; no reference counterpart): `sample_image` started from `init_images`
    /// (n x [512,512,3] u8, sample_image's output layout) re-noised to the last `strength` of the schedule.
    /// `mask` [n,1,64,64] (1 = regenerate, 0 = keep) or None; the noise is image i's stream `seed + i`.
    pub fn sample_image_from(&self, context: &[f32], n_batch: usize, unconditional_context: &[f32],
                             unconditional_guidance_scale: f64, n_steps: usize, strength: f64, init_images: &[Vec<u8>],
                             mask: Option<&[f32]>, seed: u64) -> Vec<Vec<u8>> {
        let t = context.len() / (n_batch * self.ctx_dim);
        let tu = unconditional_context.len() / self.ctx_dim;
        assert_eq!(context.len(), n_batch * t * self.ctx_dim);
        let per = self.latent / 4 * 64 * 3; // 512*512*3
        assert_eq!(init_images.len(), n_batch);
        let init: Vec<u8> = init_images.iter().flat_map(|im| { assert_eq!(im.len(), per); im.iter().copied() }).collect();
        let m = mask.map_or(std::ptr::null(), |s| { assert_eq!(s.len(), n_batch * self.latent / 4); s.as_ptr() });
        let mut flat = vec![0u8; n_batch * per];
        check(unsafe {
            sdmi_img2img_image(self.ctx, context.as_ptr(), n_batch as i32, t as i32, unconditional_context.as_ptr(), tu as i32,
                               unconditional_guidance_scale, n_steps, strength, init.as_ptr(), m, std::ptr::null(), seed, flat.as_mut_ptr())
        });
        flat.chunks(per).map(|c| c.to_vec()).collect()
    }

    /// `sample_latent` (stablediffusion/mod.rs:102-160) -> [n,4,64,64] row-major.
    pub fn sample_latent(&self, context: &[f32], n_batch: usize, unconditional_context: &[f32],
                         unconditional_guidance_scale: f64, n_steps: usize, init_latent: Option<&[f32]>, seed: u64) -> Vec<f32> {
        let t = context.len() / (n_batch * self.ctx_dim);
        let tu = unconditional_context.len() / self.ctx_dim;
        let mut out = vec![0f32; n_batch * self.latent];
        let x0 = init_latent.map_or(std::ptr::null(), |s| { assert_eq!(s.len(), n_batch * self.latent); s.as_ptr() });
        check(unsafe {
            sdmi_sample_latent(self.ctx, context.as_ptr(), n_batch as i32, t as i32, unconditional_context.as_ptr(), tu as i32,
                               unconditional_guidance_scale, n_steps, x0, seed, out.as_mut_ptr())
        });
        out
    }

    /// `latent_to_image` (stablediffusion/mod.rs:69-100).
    pub fn latent_to_image(&self, latent: &[f32]) -> Vec<Vec<u8>> {
        let n = latent.len() / self.latent;
        assert_eq!(latent.len(), n * self.latent);
        let per = self.latent / 4 * 64 * 3;
        let mut flat = vec![0u8; n * per];
        check(unsafe { sdmi_latent_to_image(self.ctx, latent.as_ptr(), n as i32, flat.as_mut_ptr()) });
        flat.chunks(per).map(|c| c.to_vec()).collect()
    }

    /// `UNet::forward(x, timesteps, context)` (unet/mod.rs:109-143), single shared timestep.
    pub fn unet_forward(&self, x: &[f32], timestep: i32, context: &[f32]) -> Vec<f32> {
        let n = x.len() / self.latent;
        let t = context.len() / (n * self.ctx_dim);
        let mut out = vec![0f32; x.len()];
        check(unsafe { sdmi_unet_forward(self.ctx, x.as_ptr(), timestep, context.as_ptr(), n as i32, t as i32, out.as_mut_ptr()) });
        out
    }

    /// `Autoencoder::decode_latent` (autoencoder/mod.rs:68-71) -> [n,3,512,512].
    pub fn decode_latent(&self, latent: &[f32]) -> Vec<f32> {
        let n = latent.len() / self.latent;
        let mut out = vec![0f32; n * self.latent / 4 * 64 * 3];
        check(unsafe { sdmi_decode_latent(self.ctx, latent.as_ptr(), n as i32, out.as_mut_ptr()) });
        out
    }

    /// The operator seam of the commented-out `trait Backend` (backend.rs:4-84):
    /// `qkv_attention(q, k, v, mask, n_head)` with q [n,nq,c], k/v [n,nk,c].
    pub fn qkv_attention(&self, q: &[f32], k: &[f32], v: &[f32], mask: Option<(&[f32], usize)>,
                         n: usize, nq: usize, nk: usize, n_state: usize, n_head: usize) -> Vec<f32> {
        let mut out = vec![0f32; q.len()];
        let (mp, ld) = mask.map_or((std::ptr::null(), 0), |(m, ld)| (m.as_ptr(), ld));
        check(unsafe {
            sdmi_qkv_attention(self.ctx, q.as_ptr(), k.as_ptr(), v.as_ptr(), mp, ld as i32, n as i32, nq as i32, nk as i32,
                               n_state as i32, n_head as i32, out.as_mut_ptr())
        });
        out
    }
}

impl Drop for StableDiffusionMi355 {
    fn drop(&mut self) {
        unsafe { sdmi_destroy(self.ctx) }
    }
}

/// `sd.sample_image(context, unconditional_context, scale, n_steps)` for `n_images` images of ONE prompt, sharded over the
/// GPUs of a node inside the library (sdmi_create_multi): one weights replica, stream and host thread per device, ONE RCCL
/// broadcast of the packed prompt embedding per call, contiguous image ranges, noise keyed by the global image index
/// (seed + i) -- the result does not depend on the device count.  What `main.rs:104-109` calls when more than one image
/// is wanted.
pub struct StableDiffusionMi355Node {
    m: *mut c_void,
    ctx_dim: usize,
    image_bytes: usize,
}

impl StableDiffusionMi355Node {
    /// kind = "dump" (npy tree, load_stable_diffusion) | "burn" (.mpk record, load_stable_diffusion_model_file) | "safetensors" (CompVis checkpoint)
    pub fn load(kind: &str, path: &str, devices: &[i32], precision: i32) -> Result<Self, Box<dyn Error>> {
        unsafe {
            let mut cfg: SdmiConfig = std::mem::zeroed();
            sdmi_default_config(&mut cfg);
            cfg.precision = precision;
            let mut m: *mut c_void = std::ptr::null_mut();
            if sdmi_create_multi(&mut m, &cfg, devices.as_ptr(), devices.len() as i32) != 0 {
                return Err(last_error().into());
            }
            let (k, p) = (CString::new(kind)?, CString::new(path)?);
            if sdmi_multi_load_weights(m, k.as_ptr(), p.as_ptr()) != 0 {
                let e = last_error();
                sdmi_destroy_multi(m);
                return Err(e.into());
            }
            Ok(Self { m, ctx_dim: cfg.ctx_dim as usize, image_bytes: 3 * 64 * (cfg.latent_h * cfg.latent_w) as usize })
        }
    }

    /// `StableDiffusionMi355::set_guidance_rescale` on every device (`sdmi_multi_set_guidance_rescale`): the statistic is per image, sharding changes nothing.
    pub fn set_guidance_rescale(&mut self, phi: f64) -> Result<(), Box<dyn Error>> {
        let st = unsafe { sdmi_multi_set_guidance_rescale(self.m, phi) };
        if st != 0 { Err(last_error().into()) } else { Ok(()) }
    }

    /// `StableDiffusionMi355::set_freeu` on every device (`sdmi_multi_set_freeu`): the edits are per sample, sharding changes nothing.
    #[allow(clippy::too_many_arguments)]
    pub fn set_freeu(&mut self, version: i32, b1: f32, b2: f32, s1: f32, s2: f32, start: f64, end: f64) -> Result<(), Box<dyn Error>> {
        let st = unsafe { sdmi_multi_set_freeu(self.m, version, b1, b2, s1, s2, start, end) };
        if st != 0 { Err(last_error().into()) } else { Ok(()) }
    }

    /// `StableDiffusionMi355::set_zero_snr` on every device (`sdmi_multi_set_zero_snr`).
    pub fn set_zero_snr(&mut self, on: bool) -> Result<(), Box<dyn Error>> {
        let st = unsafe { sdmi_multi_set_zero_snr(self.m, on as i32) };
        if st != 0 { Err(last_error().into()) } else { Ok(()) }
    }

    /// `StableDiffusionMi355::set_ksampler` on every device (`sdmi_multi_set_ksampler`); image_base per shard, as `set_sampler`.
    pub fn set_ksampler(&mut self, ksampler: Option<&SdmiKSampler>) -> Result<(), Box<dyn Error>> {
        let st = unsafe { sdmi_multi_set_ksampler(self.m, ksampler.map_or(std::ptr::null(), |k| k as *const SdmiKSampler)) };
        if st != 0 { Err(last_error().into()) } else { Ok(()) }
    }

    /// `StableDiffusionMi355::set_sampler` on every device; each shard's image_base is the global index of its first image.
    pub fn set_sampler(&mut self, sampler: Option<(i32, f64, u64)>) -> Result<(), Box<dyn Error>> {
        let st = match sampler {
            None => unsafe { sdmi_multi_set_sampler(self.m, std::ptr::null()) },
            Some((kind, eta, noise_seed)) => {
                let s = SdmiSampler { kind, reserved0: 0, eta, noise_seed, image_base: 0, reserved: [0; 4] };
                unsafe { sdmi_multi_set_sampler(self.m, &s) }
            }
        };
        if st != 0 { Err(last_error().into()) } else { Ok(()) }
    }

    pub fn sample_image(&self, context: &[f32], unconditional_context: &[f32], unconditional_guidance_scale: f64, n_steps: usize,
                        n_images: usize, seed: u64) -> Vec<Vec<u8>> {
        assert!(context.len() % self.ctx_dim == 0 && unconditional_context.len() % self.ctx_dim == 0, "embedding width");
        let mut rgb = vec![0u8; n_images * self.image_bytes];
        let st = unsafe {
            sdmi_sample_image_sharded(self.m, context.as_ptr(), (context.len() / self.ctx_dim) as i32, unconditional_context.as_ptr(),
                                      (unconditional_context.len() / self.ctx_dim) as i32, unconditional_guidance_scale, n_steps,
                                      n_images as i32, std::ptr::null(), seed, rgb.as_mut_ptr())
        };
        if st != 0 {
            panic!("sdmi_sample_image_sharded: {}", last_error());
        }
        rgb.chunks(self.image_bytes).map(|c| c.to_vec()).collect()
    }
}

impl Drop for StableDiffusionMi355Node {
    fn drop(&mut self) {
        unsafe { sdmi_destroy_multi(self.m) }
    }
}
