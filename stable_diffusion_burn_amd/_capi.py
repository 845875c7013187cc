"""ctypes binding of libsdmi.so (include/sdmi.h).

There is NO fallback: if the shared library is missing or a call fails, an
exception is raised.  The product path never routes through oracle/ or any
CPU implementation.
"""
from __future__ import annotations

import ctypes as C
import os
import sys
from pathlib import Path

_PKG = Path(__file__).resolve().parent
LIB_PATH = _PKG / "lib" / "libsdmi.so"


class SdmiError(RuntimeError):
    def __init__(self, status: int, message: str):
        super().__init__(f"sdmi status {status}: {message}")
        self.status = status


class SdmiConfig(C.Structure):
    _fields_ = [
        ("device", C.c_int32), ("model_channels", C.c_int32), ("n_head", C.c_int32), ("ctx_dim", C.c_int32),
        ("latent_h", C.c_int32), ("latent_w", C.c_int32), ("vae_ch", C.c_int32), ("max_batch", C.c_int32),
        ("precision", C.c_int32), ("clip_layers", C.c_int32), ("clip_heads", C.c_int32), ("clip_vocab", C.c_int32),
        ("clip_ctx", C.c_int32), ("unet_in_ch", C.c_int32), ("reserved", C.c_int32 * 2),
    ]

    # sdmi_config.control_hint_ch is the first of the two reserved words of earlier versions: the field list above keeps its pinned shape
    # (tests/test_inpaint_cpu.py), the name is served here
    @property
    def control_hint_ch(self) -> int:
        return int(self.reserved[0])

    @control_hint_ch.setter
    def control_hint_ch(self, v: int) -> None:
        self.reserved[0] = int(v)

    # sdmi_config.variant (0 = SD v1, 1 = SD 2.x) is the second of them
    @property
    def variant(self) -> int:
        return int(self.reserved[1])

    @variant.setter
    def variant(self, v: int) -> None:
        self.reserved[1] = int(v)


class SdmiAttnPlan(C.Structure):
    """sdmi_attn_plan: what a context would run for an attention shape (sdmi_attention_plan; host only)"""
    _fields_ = [("kernel", C.c_int32), ("waves", C.c_int32), ("q_rows", C.c_int32), ("kv_tile", C.c_int32), ("kv_splits", C.c_int32), ("reserved", C.c_int32 * 3)]


class SdmiOpView(C.Structure):
    """sdmi_op_view: where an operator's input and output sit inside wider parent buffers (sdmi_op_*_view; tests)"""
    _fields_ = [("in_ld", C.c_int32), ("in_off", C.c_int32), ("out_ld", C.c_int32), ("out_off", C.c_int32), ("in_fill", C.c_float),
                ("in_planes", C.c_int32), ("out_planes", C.c_int32)]


class SdmiAttnView(C.Structure):
    """sdmi_attn_view: where q, k, v and the result of an attention call sit inside wider parent buffers (sdmi_op_qkv_attention_view; tests)"""
    _fields_ = [("q_ld", C.c_int32), ("q_off", C.c_int32), ("q_rows", C.c_int32), ("k_ld", C.c_int32), ("k_off", C.c_int32), ("k_rows", C.c_int32),
                ("v_ld", C.c_int32), ("v_off", C.c_int32), ("v_rows", C.c_int32), ("packed", C.c_int32), ("in_fill", C.c_float),
                ("out_ld", C.c_int32), ("out_off", C.c_int32), ("out_rows", C.c_int32), ("out_planes", C.c_int32)]


class SdmiSampler(C.Structure):
    """sdmi_sampler: the sampler choice of a context (sdmi_set_sampler)"""
    _fields_ = [("kind", C.c_int32), ("reserved0", C.c_int32), ("eta", C.c_double), ("noise_seed", C.c_uint64), ("image_base", C.c_int64),
                ("reserved", C.c_int64 * 4)]


class SdmiKSampler(C.Structure):
    """sdmi_ksampler: a sigma-schedule sampler (sdmi_set_ksampler)"""
    _fields_ = [("kind", C.c_int32), ("schedule", C.c_int32), ("eta", C.c_double), ("rho", C.c_double), ("sigma_min", C.c_double), ("sigma_max", C.c_double),
                ("noise_seed", C.c_uint64), ("image_base", C.c_int64), ("reserved", C.c_int64 * 4)]


class SdmiIpAdapter(C.Structure):
    """sdmi_ip_adapter (include/sdmi.h "IP-Adapter")"""
    _fields_ = [("tokens", C.POINTER(C.c_float)), ("embeds", C.POINTER(C.c_float)), ("neg_tokens", C.POINTER(C.c_float)), ("n_sets", C.c_int32), ("T_ip", C.c_int32),
                ("token_dim", C.c_int32), ("embed_dim", C.c_int32), ("scale", C.c_float), ("start", C.c_double), ("end", C.c_double), ("reserved", C.c_int64 * 4)]


class SdmiControl(C.Structure):
    """sdmi_control: the sticky ControlNet state of a context (sdmi_set_control)"""
    _fields_ = [("hint_rgb", C.POINTER(C.c_uint8)), ("n_hint", C.c_int32), ("hint_h", C.c_int32), ("hint_w", C.c_int32), ("strength", C.c_double),
                ("start", C.c_double), ("end", C.c_double), ("reserved", C.c_int64 * 4)]


class SdmiInpaint(C.Structure):
    """sdmi_inpaint: the options of sdmi_inpaint_image"""
    _fields_ = [("latent_blend", C.c_int32), ("paste_back", C.c_int32), ("reserved", C.c_int64 * 4)]


class SdmiHires(C.Structure):
    """sdmi_hires: the second pass of the hires fix (sdmi_hires_latent / sdmi_hires_image)"""
    _fields_ = [("base_h", C.c_int32), ("base_w", C.c_int32), ("mode", C.c_int32), ("antialias", C.c_int32), ("hires_steps", C.c_int64),
                ("strength", C.c_double), ("hires_seed", C.c_uint64), ("reserved", C.c_int64 * 4)]


class SdmiPromptOpts(C.Structure):
    """sdmi_prompt_opts: the options of sdmi_encode_prompt"""
    _fields_ = [("emphasis", C.c_int32), ("clip_skip", C.c_int32), ("min_chunks", C.c_int32), ("reserved", C.c_int32 * 5)]


_F = C.POINTER(C.c_float)
_HIRES = C.POINTER(SdmiHires)
_SAMPLER = C.POINTER(SdmiSampler)
_KSAMPLER = C.POINTER(SdmiKSampler)
_F64 = C.POINTER(C.c_double)
_VIEW = C.POINTER(SdmiOpView)
_U8 = C.POINTER(C.c_uint8)
_CTX = C.c_void_p
_TOK = C.c_void_p
_I32 = C.POINTER(C.c_int32)

# name -> (restype, argtypes); every symbol include/sdmi.h declares
SIGNATURES = {
    "sdmi_default_config": (C.c_int, [C.POINTER(SdmiConfig)]),
    "sdmi_create": (C.c_int, [C.POINTER(_CTX), C.POINTER(SdmiConfig)]),
    "sdmi_destroy": (None, [_CTX]),
    "sdmi_last_error": (C.c_char_p, []),
    "sdmi_synchronize": (C.c_int, [_CTX]),
    "sdmi_version": (C.c_char_p, []),
    "sdmi_set_stream": (C.c_int, [_CTX, C.c_void_p, C.c_int32]),
    "sdmi_set_weight": (C.c_int, [_CTX, C.c_char_p, _F, C.c_int32, C.POINTER(C.c_int64)]),
    "sdmi_weight_count": (C.c_int, [_CTX]),
    "sdmi_weight_info": (C.c_int, [_CTX, C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    "sdmi_load_weights_dir": (C.c_int, [_CTX, C.c_char_p]),
    "sdmi_load_weights_mpk": (C.c_int, [_CTX, C.c_char_p]),
    "sdmi_mpk_list": (C.c_int, [C.c_char_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "sdmi_load_weights_safetensors": (C.c_int, [_CTX, C.c_char_p]),
    "sdmi_safetensors_list": (C.c_int, [C.c_char_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "sdmi_checkpoint_key": (C.c_int, [C.c_char_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_int32)]),
    "sdmi_checkpoint_key_ex": (C.c_int, [C.c_char_p, C.c_int32, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "sdmi_safetensors_model_family": (C.c_int, [C.c_char_p, C.POINTER(C.c_int32)]),
    "sdmi_default_alphas_cumprod": (C.c_int, [_F, C.c_int32]),
    "sdmi_load_weights_packed": (C.c_int, [_CTX, _F, C.c_size_t, C.c_int32]),
    "sdmi_packed_size": (C.c_int64, [_CTX, C.c_int32]),
    "sdmi_finalize_weights": (C.c_int, [_CTX]),
    "sdmi_unet_forward": (C.c_int, [_CTX, _F, C.c_int32, _F, C.c_int32, C.c_int32, _F]),
    "sdmi_sample_latent": (C.c_int, [_CTX, _F, C.c_int32, C.c_int32, _F, C.c_int32, C.c_double, C.c_size_t, _F, C.c_uint64, _F]),
    "sdmi_decode_latent": (C.c_int, [_CTX, _F, C.c_int32, _F]),
    "sdmi_latent_to_image": (C.c_int, [_CTX, _F, C.c_int32, _U8]),
    "sdmi_sample_image": (C.c_int, [_CTX, _F, C.c_int32, C.c_int32, _F, C.c_int32, C.c_double, C.c_size_t, _F, C.c_uint64, _U8]),
    "sdmi_img2img_timesteps": (C.c_int, [C.c_int32, C.c_size_t, C.c_double, _I32, C.c_int32, _I32]),
    "sdmi_img2img_latent": (C.c_int, [_CTX, _F, C.c_int32, C.c_int32, _F, C.c_int32, C.c_double, C.c_size_t, C.c_double, _F, _F, _F, C.c_uint64, _F]),
    "sdmi_img2img_image": (C.c_int, [_CTX, _F, C.c_int32, C.c_int32, _F, C.c_int32, C.c_double, C.c_size_t, C.c_double, _U8, _F, _F, C.c_uint64, _U8]),
    "sdmi_unet_forward_cond": (C.c_int, [_CTX, _F, C.c_int32, _F, _F, C.c_int32, C.c_int32, _F]),
    "sdmi_img2img_latent_cond": (C.c_int, [_CTX, _F, C.c_int32, C.c_int32, _F, C.c_int32, C.c_double, C.c_size_t, C.c_double, _F, _F, _F, C.c_uint64, _F, _F]),
    "sdmi_img2img_latent_cond_dev": (C.c_int, [_CTX, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_double, C.c_size_t, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    "sdmi_inpaint_latent_mask": (C.c_int, [_U8, C.c_int32, C.c_int32, C.c_int32, _F]),
    "sdmi_inpaint_cond": (C.c_int, [_CTX, _U8, _U8, C.c_int32, _F]),
    "sdmi_inpaint_image": (C.c_int, [_CTX, _F, C.c_int32, C.c_int32, _F, C.c_int32, C.c_double, C.c_size_t, C.c_double, _U8, _U8, C.POINTER(SdmiInpaint), _F, C.c_uint64, _U8]),
    "sdmi_inpaint_image_dev": (C.c_int, [_CTX, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_double, C.c_size_t, C.c_double, C.c_void_p, C.c_void_p, C.POINTER(SdmiInpaint), C.c_void_p, C.c_uint64, C.c_void_p]),
    "sdmi_set_sampler": (C.c_int, [_CTX, _SAMPLER]),
    "sdmi_get_sampler": (C.c_int, [_CTX, _SAMPLER]),
    "sdmi_set_ksampler": (C.c_int, [_CTX, _KSAMPLER]),
    "sdmi_get_ksampler": (C.c_int, [_CTX, _KSAMPLER, C.POINTER(C.c_int32)]),
    "sdmi_ksampler_sigmas": (C.c_int, [_KSAMPLER, _F, C.c_int32, C.c_size_t, _F64, C.c_int32, C.POINTER(C.c_int32)]),
    "sdmi_sigma_to_t": (C.c_int, [_F, C.c_int32, C.c_double, _F64]),
    "sdmi_ksampler_plan": (C.c_int, [_KSAMPLER, _F, C.c_int32, C.c_size_t, C.c_double, _F64, C.c_int32, C.POINTER(C.c_int32)]),
    "sdmi_ksampler_plan_ex": (C.c_int, [_KSAMPLER, _F, C.c_int32, C.c_size_t, C.c_double, C.c_int32, _F64, C.c_int32, C.POINTER(C.c_int32)]),
    "sdmi_load_control_safetensors": (C.c_int, [_CTX, C.c_char_p]),
    "sdmi_control_ready": (C.c_int, [_CTX]),
    "sdmi_set_control": (C.c_int, [_CTX, C.POINTER(SdmiControl)]),
    "sdmi_control_step_on": (C.c_int, [C.c_double, C.c_double, C.c_int32, C.c_int32]),
    "sdmi_control_hint_embed": (C.c_int, [_CTX, _U8, C.c_int32, C.c_int32, C.c_int32, _F]),
    "sdmi_control_residuals_size": (C.c_int64, [_CTX, C.c_int32]),
    "sdmi_control_residuals": (C.c_int, [_CTX, _F, C.c_int32, _F, C.c_int32, C.c_int32, _F]),
    "sdmi_sampler_coefs": (C.c_int, [_SAMPLER, _F, C.c_int32, _I32, C.c_int32, C.c_int64, C.POINTER(C.c_double)]),
    "sdmi_sampler_coefs_ex": (C.c_int, [_SAMPLER, _F, C.c_int32, _I32, C.c_int32, C.c_int64, C.c_int32, C.POINTER(C.c_double)]),
    "sdmi_set_prediction": (C.c_int, [_CTX, C.c_int32]),
    "sdmi_set_guidance_rescale": (C.c_int, [_CTX, C.c_double]),
    "sdmi_rescale_zero_snr": (C.c_int, [_F, _F, C.c_int32]),
    "sdmi_set_zero_snr": (C.c_int, [_CTX, C.c_int32]),
    "sdmi_schedule": (C.c_int, [_CTX, _F, C.c_int32, _I32]),
    "sdmi_op_sampler_step": (C.c_int, [_CTX, _F, _F, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double, C.POINTER(C.c_double), C.c_int32, C.c_int32, _F,
                                       C.c_uint64, C.c_uint64, _F, _F, _F, C.c_double, C.c_double, _F, _F]),
    "sdmi_multi_set_guidance_rescale": (C.c_int, [C.c_void_p, C.c_double]),
    "sdmi_multi_set_zero_snr": (C.c_int, [C.c_void_p, C.c_int32]),
    "sdmi_set_freeu": (C.c_int, [_CTX, C.c_int32, C.c_float, C.c_float, C.c_float, C.c_float, C.c_double, C.c_double]),
    "sdmi_get_freeu": (C.c_int, [_CTX, _I32, _F, _F, _F, _F, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "sdmi_freeu_plan": (C.c_int, [C.POINTER(SdmiConfig), C.c_int32, C.c_int32, _I32]),
    "sdmi_op_freeu": (C.c_int, [_CTX, _F, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float, _F, _F]),
    "sdmi_multi_set_freeu": (C.c_int, [C.c_void_p, C.c_int32, C.c_float, C.c_float, C.c_float, C.c_float, C.c_double, C.c_double]),
    "sdmi_ip_adapter_load_safetensors": (C.c_int, [_CTX, C.c_char_p]),
    "sdmi_ip_adapter_check_safetensors": (C.c_int, [C.POINTER(SdmiConfig), C.c_char_p, _I32, _I32]),
    "sdmi_ip_adapter_set_weights": (C.c_int, [_CTX, _F, _F, _F, _F, C.c_int32, C.c_int32, C.POINTER(_F), C.POINTER(_F)]),
    "sdmi_ip_adapter_ready": (C.c_int, [_CTX]),
    "sdmi_ip_adapter_dims": (C.c_int, [_CTX, _I32, _I32]),
    "sdmi_ip_adapter_clear": (C.c_int, [_CTX]),
    "sdmi_ip_image_tokens": (C.c_int, [_CTX, _F, C.c_int32, C.c_int32, _F]),
    "sdmi_set_ip_adapter": (C.c_int, [_CTX, C.POINTER(SdmiIpAdapter)]),
    "sdmi_set_ip_adapter_file": (C.c_int, [_CTX, C.c_char_p, C.c_float, C.c_double, C.c_double]),
    "sdmi_get_ip_adapter": (C.c_int, [_CTX, C.POINTER(SdmiIpAdapter)]),
    "sdmi_ip_adapter_key": (C.c_int, [C.POINTER(SdmiConfig), C.c_int32, C.c_int32, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t), _I32, _I32]),
    "sdmi_op_ip_attention": (C.c_int, [_CTX, _F, _F, _F, _F, _F, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _F]),
    "sdmi_ip_kv_size": (C.c_int64, [_CTX, C.c_int32, C.c_int32]),
    "sdmi_ip_kv": (C.c_int, [_CTX, C.c_int32, C.c_int32, _F]),
    "sdmi_multi_set_ip_adapter": (C.c_int, [C.c_void_p, C.POINTER(SdmiIpAdapter)]),
    "sdmi_set_latent_size": (C.c_int, [_CTX, C.c_int32, C.c_int32]),
    "sdmi_get_latent_size": (C.c_int, [_CTX, _I32, _I32]),
    "sdmi_resize_weights": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, _I32, _I32, C.POINTER(C.c_double), C.c_int32, _I32, _I32]),
    "sdmi_hires_latent": (C.c_int, [_CTX, _F, C.c_int32, C.c_int32, _F, C.c_int32, C.c_double, C.c_size_t, _F, C.c_uint64, _HIRES, _F, _F]),
    "sdmi_hires_image": (C.c_int, [_CTX, _F, C.c_int32, C.c_int32, _F, C.c_int32, C.c_double, C.c_size_t, _F, C.c_uint64, _HIRES, _F, _U8]),
    "sdmi_hires_latent_dev": (C.c_int, [_CTX, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_double, C.c_size_t, C.c_void_p, _HIRES, C.c_void_p, C.c_void_p]),
    "sdmi_hires_image_dev": (C.c_int, [_CTX, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_double, C.c_size_t, C.c_void_p, _HIRES, C.c_void_p, C.c_void_p]),
    "sdmi_op_resize": (C.c_int, [_CTX, _F, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _F]),
    "sdmi_op_unpack_tensor": (C.c_int, [_CTX, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.c_int32, _F]),
    "sdmi_multi_set_sampler": (C.c_int, [C.c_void_p, _SAMPLER]),
    "sdmi_multi_set_ksampler": (C.c_int, [C.c_void_p, _KSAMPLER]),
    "sdmi_lora_create": (C.c_int, [_CTX, C.POINTER(C.c_void_p)]),
    "sdmi_lora_add": (C.c_int, [C.c_void_p, C.c_char_p, _F, _F, C.c_int32, C.c_float]),
    "sdmi_lora_load_safetensors": (C.c_int, [_CTX, C.c_char_p, C.c_int32, C.c_int32, C.POINTER(C.c_void_p), _I32, _I32]),
    "sdmi_lora_factor_bytes": (C.c_int, [C.c_void_p, C.POINTER(C.c_size_t)]),
    "sdmi_lora_module_name": (C.c_int, [C.c_char_p, C.c_char_p, C.c_size_t]),
    "sdmi_lora_check_safetensors": (C.c_int, [C.c_char_p, C.POINTER(C.c_char_p), _I32, C.POINTER(C.c_int64), C.c_int32, C.c_int32, C.c_int32, _I32, _I32]),
    "sdmi_lora_set_scale": (C.c_int, [C.c_void_p, C.c_double]),
    "sdmi_lora_get_scale": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), _I32]),
    "sdmi_lora_destroy": (C.c_int, [C.c_void_p]),
    "sdmi_lora_effective_weight": (C.c_int, [_CTX, C.c_char_p, _F, C.c_size_t]),
    "sdmi_qkv_attention": (C.c_int, [_CTX, _F, _F, _F, _F, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _F]),
    "sdmi_tokenizer_create": (C.c_int, [C.POINTER(_TOK), C.c_char_p]),
    "sdmi_tokenizer_destroy": (None, [_TOK]),
    "sdmi_tokenizer_vocab_size": (C.c_int, [_TOK]),
    "sdmi_tokenizer_encode": (C.c_int, [_TOK, C.c_char_p, _I32, C.c_int32, _I32]),
    "sdmi_tokenizer_decode": (C.c_int, [_TOK, _I32, C.c_int32, C.c_char_p, C.c_int32, _I32]),
    "sdmi_clip_forward": (C.c_int, [_CTX, _I32, C.c_int32, C.c_int32, _F]),
    "sdmi_context": (C.c_int, [_CTX, _TOK, C.c_char_p, _F, C.c_int32, _I32]),
    "sdmi_prompt_parse": (C.c_int, [C.c_char_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "sdmi_prompt_chunks": (C.c_int, [_TOK, C.c_char_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_char_p), _I32, C.c_int32, _I32, _F, _I32, C.c_int32, _I32]),
    "sdmi_clip_forward_ex": (C.c_int, [_CTX, _I32, _I32, _F, C.c_int32, C.c_int32, C.c_int32, _F]),
    "sdmi_embedding_add": (C.c_int, [_CTX, _TOK, C.c_char_p, _F, C.c_int32]),
    "sdmi_embedding_load_safetensors": (C.c_int, [_CTX, _TOK, C.c_char_p, C.c_char_p]),
    "sdmi_embedding_remove": (C.c_int, [_CTX, C.c_char_p]),
    "sdmi_embedding_list": (C.c_int, [_CTX, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "sdmi_encode_prompt": (C.c_int, [_CTX, _TOK, C.c_char_p, C.POINTER(SdmiPromptOpts), _F, C.c_int32, _I32]),
    "sdmi_encode_image": (C.c_int, [_CTX, _F, C.c_int32, _F]),
    "sdmi_write_png": (C.c_int, [C.c_char_p, _U8, C.c_int32, C.c_int32]),
    "sdmi_sample_latent_dev": (C.c_int, [_CTX, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_double, C.c_size_t, C.c_void_p, C.c_void_p]),
    "sdmi_latent_to_image_dev": (C.c_int, [_CTX, C.c_void_p, C.c_int32, C.c_void_p]),
    "sdmi_sample_image_dev": (C.c_int, [_CTX, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_double, C.c_size_t, C.c_void_p, C.c_void_p]),
    "sdmi_img2img_latent_dev": (C.c_int, [_CTX, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_double, C.c_size_t, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
    "sdmi_img2img_image_dev": (C.c_int, [_CTX, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_double, C.c_size_t, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
    "sdmi_create_multi": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(SdmiConfig), _I32, C.c_int32]),
    "sdmi_destroy_multi": (None, [C.c_void_p]),
    "sdmi_multi_size": (C.c_int32, [C.c_void_p]),
    "sdmi_multi_ctx": (C.c_void_p, [C.c_void_p, C.c_int32]),
    "sdmi_multi_load_weights": (C.c_int, [C.c_void_p, C.c_char_p, C.c_char_p]),
    "sdmi_sample_image_sharded": (C.c_int, [C.c_void_p, _F, C.c_int32, _F, C.c_int32, C.c_double, C.c_size_t, C.c_int32, _F, C.c_uint64, _U8]),
    "sdmi_shard_range": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _I32, _I32]),
    "sdmi_multi_broadcast_count": (C.c_int64, [C.c_void_p]),
    "sdmi_selftest_rank_errors": (C.c_int, [C.c_int32, C.c_int32]),
    "sdmi_op_group_norm": (C.c_int, [_CTX, _F, _F, _F, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32, _F]),
    "sdmi_op_group_norm_fp8": (C.c_int, [_CTX, _F, _F, _F, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32, _F]),
    "sdmi_op_layer_norm": (C.c_int, [_CTX, _F, _F, _F, C.c_int32, C.c_int32, C.c_float, _F]),
    "sdmi_op_conv2d": (C.c_int, [_CTX, _F, _F, _F, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _F]),
    "sdmi_op_linear": (C.c_int, [_CTX, _F, _F, _F, C.c_int32, C.c_int32, C.c_int32, _F]),
    "sdmi_op_conv2d_epilogue": (C.c_int, [_CTX, _F, _F, _F, _F, C.c_int32, _F, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                          C.c_int32, C.c_int32, _F]),
    "sdmi_op_conv2d_pair": (C.c_int, [_CTX, _F, _F, _F, _F, _F, _F, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _F, _F]),
    "sdmi_op_linear_pair": (C.c_int, [_CTX, _F, _F, _F, _F, _F, _F, _F, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _F, _F]),
    "sdmi_op_linear_fold": (C.c_int, [_CTX, _F, _F, _F, C.c_int32, C.c_int32, C.c_int32, _F, _F]),
    "sdmi_op_linear_epilogue": (C.c_int, [_CTX, _F, _F, _F, _F, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _F]),
    "sdmi_op_conv2d_view": (C.c_int, [_CTX, _F, _F, _F, _F, C.c_int32, _F, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                      C.c_int32, C.c_int32, _VIEW, _F, _F]),
    "sdmi_op_linear_view": (C.c_int, [_CTX, _F, _F, _F, _F, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _VIEW, _F]),
    "sdmi_op_group_norm_view": (C.c_int, [_CTX, _F, _F, _F, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32, _VIEW, C.c_int32, _F]),
    "sdmi_op_cat_chain": (C.c_int, [_CTX, _F, _F, _F, _F, _F, _F, _F, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32,
                                    C.c_int32, _F]),
    "sdmi_op_geglu_forward": (C.c_int, [_CTX, _F, _F, _F, C.c_int32, C.c_int32, C.c_int32, _F]),
    "sdmi_op_geglu": (C.c_int, [_CTX, _F, C.c_int32, C.c_int32, _F]),
    "sdmi_op_qkv_attention_ragged": (C.c_int, [_CTX, _F, _F, _F, _I32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _F]),
    "sdmi_op_qkv_attention_view": (C.c_int, [_CTX, _F, _F, _F, _F, C.c_int32, _I32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, SdmiAttnView, _F]),
    "sdmi_op_timestep_embedding": (C.c_int, [_CTX, C.c_int32, C.c_int32, _F]),
    "sdmi_op_timestep_embedding_f": (C.c_int, [_CTX, C.c_double, C.c_int32, _F]),
    "sdmi_set_option": (C.c_int, [_CTX, C.c_char_p, C.c_char_p]),
    "sdmi_last_call_stats": (C.c_int, [_CTX, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_double)]),
    "sdmi_profile_stats": (C.c_int, [_CTX, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "sdmi_profile_overhead": (C.c_int, [_CTX, C.POINTER(C.c_double)]),
    "sdmi_bench_conv": (C.c_int, [_CTX, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_double)]),
    "sdmi_bench_attention": (C.c_int, [_CTX, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_double)]),
    "sdmi_attention_plan": (C.c_int, [_CTX, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(SdmiAttnPlan)]),
}

_lib = None


def load_library() -> C.CDLL:
    """dlopen libsdmi.so and bind every declared symbol; raises if anything is missing.

    If torch is already imported its bundled libamdhip64 (same SONAME) is
    reused by the loader, so device pointers from torch tensors are valid in
    libsdmi; when torch will be used in the process, import it BEFORE this.
    """
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -m stable_diffusion_burn_amd.build` "
            "(libsdmi has no CPU or PyTorch fallback)")
    lib = C.CDLL(str(LIB_PATH), mode=C.RTLD_GLOBAL if "torch" in sys.modules else C.RTLD_LOCAL)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(status: int) -> None:
    if status != 0:
        msg = load_library().sdmi_last_error()
        raise SdmiError(status, msg.decode("utf-8", "replace") if msg else "")
