"""stable_diffusion_burn_amd -- MI355X (gfx950) native SD v1.4 sampling hot path.

The package is a thin host layer over `libsdmi.so` (hand-written HIP kernels +
C++ engine, C ABI in include/sdmi.h).  It exposes the reference's
`StableDiffusion` surface (Gadersd/stable-diffusion-burn,
src/model/stablediffusion/mod.rs) and nothing else; there is no CPU or PyTorch
fallback -- importing the pipeline without a built library raises.
"""
from .pipeline import CLIP, LORA_SKIP_UNKNOWN, LORA_TE, LORA_UNET, Autoencoder, LoraAdapter, LoraFileAdapter, ModelConfig, MultiStableDiffusion, SdmiError, SimpleTokenizer, StableDiffusion, UNet, checkpoint_key, control_residual_shapes, control_step_on, default_alphas_cumprod, freeu_plan, img2img_timesteps, ip_adapter_check_safetensors, ip_adapter_key, inpaint_latent_mask, load_lora_npz, lora_check_safetensors, lora_module_name, mpk_list, parse_prompt, qkv_attention, resize_weights, safetensors_list, safetensors_model_family, sampler_coefs, save_lora_npz, ksampler_plan, ksampler_sigmas, sigma_to_t, rescale_zero_snr  # noqa: F401
from . import synthetic  # noqa: F401

__all__ = ["StableDiffusion", "MultiStableDiffusion", "UNet", "Autoencoder", "CLIP", "SimpleTokenizer", "ModelConfig", "SdmiError", "qkv_attention", "mpk_list", "parse_prompt", "safetensors_list", "safetensors_model_family", "checkpoint_key", "default_alphas_cumprod", "control_step_on", "control_residual_shapes", "freeu_plan", "img2img_timesteps", "ip_adapter_check_safetensors", "ip_adapter_key", "inpaint_latent_mask", "sampler_coefs", "ksampler_sigmas", "sigma_to_t", "ksampler_plan", "rescale_zero_snr", "resize_weights", "load_lora_npz", "save_lora_npz", "lora_module_name", "lora_check_safetensors", "LoraAdapter", "LoraFileAdapter", "LORA_UNET", "LORA_TE", "LORA_SKIP_UNKNOWN", "synthetic"]
