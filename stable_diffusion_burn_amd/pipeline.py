"""Host-side mirror of the reference's `StableDiffusion` surface over libsdmi.

The reference's caller (src/bin/sample/main.rs:100-109) uses
    sd.sample_image(context, unconditional_context, scale, n_steps) -> Vec<Vec<u8>>
and the public-but-unused `sample_latent`, `latent_to_image`
(src/model/stablediffusion/mod.rs:69,102), `UNet::forward` (unet/mod.rs:109),
`Autoencoder::decode_latent` (autoencoder/mod.rs:68) and `qkv_attention`
(attention.rs:5).  This module keeps those names, argument order and meaning;
tensors are numpy float32 arrays in the reference's layouts (NCHW latents,
[n, tokens, channels] sequences).  The Rust toolchain is absent here, so this
Python layer plays the part of the Rust shim in ffi/sdmi.rs; both only marshal
arguments into the C ABI -- all arithmetic happens in the HIP library.

Errors: the reference panics on shape errors; here they raise SdmiError (from
the C status) or ValueError (caught before the call).
"""
from __future__ import annotations

import ctypes as C
import os
import re
from dataclasses import dataclass

import numpy as np

from . import _capi
from ._capi import SdmiAttnPlan, SdmiAttnView, SdmiConfig, SdmiControl, SdmiIpAdapter, SdmiError, SdmiHires, SdmiInpaint, SdmiKSampler, SdmiOpView, SdmiPromptOpts, SdmiSampler, check, load_library

def mpk_list(path) -> list:
    """[(dump name, shape, file offset)] of a Burn .mpk record, parsed by the C++ reader (host only, no GPU)."""
    lib = load_library()
    need = C.c_size_t()
    check(lib.sdmi_mpk_list(str(path).encode(), None, 0, C.byref(need)))
    buf = C.create_string_buffer(need.value)
    check(lib.sdmi_mpk_list(str(path).encode(), buf, need.value, C.byref(need)))
    out = []
    for line in buf.value.decode().splitlines():
        if line.startswith("#") or not line:
            continue
        name, shape, off = line.split("\t")
        out.append((name, tuple(int(v) for v in shape.split(",")) if shape else (), int(off)))
    return out


def _text_query(fn, *args) -> str:
    """the query-then-fill convention of the listing entry points: fn(*args, out, capacity, &needed)"""
    need = C.c_size_t()
    check(fn(*args, None, 0, C.byref(need)))
    buf = C.create_string_buffer(need.value)
    check(fn(*args, buf, need.value, C.byref(need)))
    return buf.value.decode()


def safetensors_list(path) -> list:
    """[(key, dtype, shape, file offset, dump name or None)] of a .safetensors file, parsed by the C++ reader (host only, no GPU)."""
    out = []
    for line in _text_query(load_library().sdmi_safetensors_list, str(path).encode()).split("\n"):
        if not line:
            continue
        key, dtype, shape, off, name = line.rsplit("\t", 4)
        key = re.sub(r"\\(u[0-9a-f]{4}|.)", lambda m: {"t": "\t", "n": "\n"}.get(m.group(1), chr(int(m.group(1)[1:], 16)) if len(m.group(1)) == 5 else m.group(1)), key)
        out.append((key, dtype, tuple(int(v) for v in shape.split(",")) if shape else (), int(off), None if name == "-" else name))
    return out


def _listing_unescape(field: str) -> str:
    """a field of a tab-separated listing line: the JSON escapes of backslash and control characters undone"""
    return re.sub(r"\\(u[0-9a-f]{4}|.)", lambda m: {"t": "\t", "n": "\n"}.get(m.group(1), chr(int(m.group(1)[1:], 16)) if len(m.group(1)) == 5 else m.group(1)), field)


def parse_prompt(text: str) -> list:
    """[(fragment, weight)] of a prompt with the web UI's emphasis syntax -- "(a)", "[a]", "(a:1.3)", backslash escapes, BREAK -- parsed by the C++
    parser (sdmi_prompt_parse, host only, no GPU).  A BREAK marker is ("BREAK", -1).  SdmiError for a weight that is no number."""
    out = []
    for line in _text_query(load_library().sdmi_prompt_parse, text.encode("utf-8")).split("\n")[:-1]:
        w, frag = line.split("\t", 1)
        out.append((_listing_unescape(frag), float(w)))
    return out


def checkpoint_key(name: str, variant: int = 0, with_slice: bool = False) -> tuple:
    """(checkpoint key, transposed?) of a dump-tree tensor name (sdmi_checkpoint_key_ex, host only, no GPU); SdmiError for a name without one.
    variant: ModelConfig.variant -- 0 the CompVis SD v1 layout, 1 Stability's SD 2.x layout (OpenCLIP text encoder under cond_stage_model.model.).
    with_slice: a third element -- None = the key's whole tensor, 0 / 1 / 2 = the first / second / third third of its rows (the query / key / value parts of
    SD 2.x's fused attn.in_proj_weight / in_proj_bias)."""
    lib = load_library()
    need, tr, sl = C.c_size_t(), C.c_int32(), C.c_int32()
    check(lib.sdmi_checkpoint_key_ex(name.encode(), int(variant), None, 0, C.byref(need), C.byref(tr), C.byref(sl)))
    buf = C.create_string_buffer(need.value)
    check(lib.sdmi_checkpoint_key_ex(name.encode(), int(variant), buf, need.value, C.byref(need), C.byref(tr), C.byref(sl)))
    if with_slice:
        return buf.value.decode(), bool(tr.value), None if sl.value < 0 else int(sl.value)
    return buf.value.decode(), bool(tr.value)


def safetensors_model_family(path):
    """"sd1" | "sd2" | None: the checkpoint family of a .safetensors file (sdmi_safetensors_model_family, host only) -- decided by which text encoder's final
    LayerNorm it holds: cond_stage_model.transformer.text_model.final_layer_norm.weight (SD v1) or cond_stage_model.model.ln_final.weight (SD 2.x)."""
    fam = C.c_int32()
    check(load_library().sdmi_safetensors_model_family(str(path).encode(), C.byref(fam)))
    return {1: "sd1", 2: "sd2"}.get(fam.value)


def control_step_on(start: float, end: float, step: int, n_steps: int) -> bool:
    """THE step-window rule of a control (sdmi_control_step_on, host only, no GPU): start * n_steps <= step < end * n_steps, in f64."""
    r = load_library().sdmi_control_step_on(float(start), float(end), int(step), int(n_steps))
    if r < 0:
        check(r)
    return bool(r)


def freeu_plan(cfg, latent_h: int, latent_w: int) -> list:
    """THE block rule of FreeU (sdmi_freeu_plan, host only, no GPU): for each of the 12 output blocks of a model with cfg.model_channels at
    latent_h x latent_w, (group, cx, cskip, h, w) -- group 0: untouched, 1: (b1, s1), 2: (b2, s2); cx backbone and cskip skip channels of the h x w concatenation."""
    lib = load_library()
    c = SdmiConfig()
    check(lib.sdmi_default_config(C.byref(c)))
    c.model_channels = int(cfg.model_channels)
    out = (C.c_int32 * 60)()
    check(lib.sdmi_freeu_plan(C.byref(c), int(latent_h), int(latent_w), out))
    return [tuple(int(v) for v in out[5 * i:5 * i + 5]) for i in range(12)]


def ip_adapter_key(cfg, ctx_index: int, which: str = "k", with_shape: bool = False):
    """THE layer rule of an IP-Adapter file (sdmi_ip_adapter_key, host only, no GPU): cross attention ctx_index (0 .. 15: the input blocks'
    six, the middle block's, the output blocks' nine) of a model with cfg.model_channels -> "ip_adapter.<j>.to_k_ip.weight" (which = "k") or "...to_v_ip.weight"
    ("v").  with_shape: (key, j, C) -- the tensor is [C, ctx_dim]."""
    if which not in ("k", "v"):
        raise ValueError("which must be 'k' or 'v'")
    lib = load_library()
    c = SdmiConfig()
    check(lib.sdmi_default_config(C.byref(c)))
    c.model_channels = int(cfg.model_channels)
    need, j, cc = C.c_size_t(), C.c_int32(), C.c_int32()
    w = 0 if which == "k" else 1
    check(lib.sdmi_ip_adapter_key(C.byref(c), int(ctx_index), w, None, 0, C.byref(need), C.byref(j), C.byref(cc)))
    buf = C.create_string_buffer(need.value)
    check(lib.sdmi_ip_adapter_key(C.byref(c), int(ctx_index), w, buf, need.value, C.byref(need), C.byref(j), C.byref(cc)))
    return (buf.value.decode(), int(j.value), int(cc.value)) if with_shape else buf.value.decode()


def ip_adapter_check_safetensors(cfg, path) -> tuple:
    """Every check load_ip_adapter_safetensors makes, host only (sdmi_ip_adapter_check_safetensors): the file against a model with cfg.model_channels and
    cfg.ctx_dim.  Returns the file's (D, T); SdmiError names the offending key."""
    lib = load_library()
    c = SdmiConfig()
    check(lib.sdmi_default_config(C.byref(c)))
    c.model_channels, c.ctx_dim = int(cfg.model_channels), int(cfg.ctx_dim)
    d, t = C.c_int32(), C.c_int32()
    check(lib.sdmi_ip_adapter_check_safetensors(C.byref(c), str(path).encode(), C.byref(d), C.byref(t)))
    return int(d.value), int(t.value)


def _ip_adapter_struct(keep, embeds, tokens, negative_tokens, scale, start, end):
    """sdmi_ip_adapter of Python arrays; `keep` receives the arrays the struct points into"""
    if (embeds is None) == (tokens is None):
        raise ValueError("set_ip_adapter: give exactly one of embeds and tokens")
    a = SdmiIpAdapter()
    if tokens is not None:
        t = _f32(tokens)
        if t.ndim == 2:
            t = t[None]
        if t.ndim != 3:
            raise ValueError(f"tokens must be [n_sets, T_ip, ctx_dim] or [T_ip, ctx_dim], got {t.shape}")
        keep.append(t)
        a.tokens = _fp(t)
        a.n_sets, a.T_ip, a.token_dim = int(t.shape[0]), int(t.shape[1]), int(t.shape[2])
    else:
        e = _f32(embeds)
        if e.ndim == 2:     # [n_img, D]: one set of n_img pictures
            e = e[None]
        if e.ndim != 3:
            raise ValueError(f"embeds must be [n_sets, n_img, D] or [n_img, D], got {e.shape}")
        keep.append(e)
        a.embeds = _fp(e)
        a.n_sets, a.embed_dim = int(e.shape[0]), int(e.shape[2])
        a.T_ip = -int(e.shape[1])   # pictures; the caller multiplies by the adapter's T
    if negative_tokens is not None:
        g = _f32(negative_tokens)
        if g.ndim == 2:
            g = g[None]
        if g.ndim != 3:
            raise ValueError(f"negative_tokens must be [n_sets, T_ip, ctx_dim] or [T_ip, ctx_dim], got {g.shape}")
        if tokens is not None and g.shape != keep[0].shape:
            raise ValueError(f"negative_tokens {g.shape} must have the shape of tokens {keep[0].shape}")
        keep.append(g)
        a.neg_tokens = _fp(g)
        a.token_dim = int(g.shape[2])
    a.scale, a.start, a.end = float(scale), float(start), float(end)
    return a


def control_residual_shapes(model_channels: int) -> list:
    """[(channels, log2 of the downscale)] of the 13 ControlNet residuals: the 12 input blocks' outputs, then the middle block's."""
    mc = model_channels
    return [(mc, 0)] * 3 + [(mc, 1), (2 * mc, 1), (2 * mc, 1), (2 * mc, 2), (4 * mc, 2), (4 * mc, 2), (4 * mc, 3), (4 * mc, 3), (4 * mc, 3), (4 * mc, 3)]


def default_alphas_cumprod(n: int = 1000) -> np.ndarray:
    """The LDM schedule a checkpoint without alphas_cumprod gets (sdmi_default_alphas_cumprod, host only, no GPU)."""
    out = np.empty(int(n), np.float32)
    check(load_library().sdmi_default_alphas_cumprod(_fp(out), int(n)))
    return out


def inpaint_latent_mask(mask, h: int, w: int) -> np.ndarray:
    """sdmi_inpaint_latent_mask (host only): mask uint8 [n,8h,8w] (>= 128: regenerate) -> [n,h,w] float32 of 0 / 1, out[y][x] = mask[8y][8x] >= 128."""
    m = np.ascontiguousarray(mask)
    if m.dtype != np.uint8 or m.ndim != 3 or m.shape[1:] != (8 * int(h), 8 * int(w)):
        raise ValueError(f"mask must be uint8 [n,{8 * int(h)},{8 * int(w)}], got {m.dtype} {m.shape}")
    out = np.empty((m.shape[0], int(h), int(w)), dtype=np.float32)
    check(load_library().sdmi_inpaint_latent_mask(m.ctypes.data_as(C.POINTER(C.c_uint8)), m.shape[0], int(h), int(w), _fp(out)))
    return out


def img2img_timesteps(n_steps: int, strength: float, total: int = 1000) -> list:
    """The timesteps an img2img call runs (sdmi_img2img_timesteps, host only, no GPU): the last
    k = min(L, int(strength * L)) of sample_latent's L timesteps.  Raises SdmiError unless 0 < strength <= 1 and k >= 1."""
    lib = load_library()
    buf = (C.c_int32 * max(1, int(total)))()
    count = C.c_int32()
    check(lib.sdmi_img2img_timesteps(int(total), int(n_steps), float(strength), buf, len(buf), C.byref(count)))
    return list(buf[:count.value])


SAMPLER_KINDS = ("ddim", "dpmpp_2m", "plms")   # sdmi_sampler.kind 0, 1, 2 (plain Euler = "ddim" at eta 0, Euler-ancestral = "ddim" at eta 1)


def _sampler_struct(kind, eta=0.0, noise_seed=0, image_base=0) -> SdmiSampler:
    if kind not in SAMPLER_KINDS:
        raise ValueError(f"sampler kind must be one of {SAMPLER_KINDS}, got {kind!r}")
    eta = float(eta)
    if not 0.0 <= eta <= 1.0:   # NaN fails too
        raise ValueError(f"eta must satisfy 0 <= eta <= 1, got {eta}")
    if eta != 0.0 and kind != "ddim":
        raise ValueError("eta belongs to the ddim sampler only")
    s = SdmiSampler()
    s.kind, s.eta, s.noise_seed, s.image_base = SAMPLER_KINDS.index(kind), eta, int(noise_seed) & 0xFFFFFFFFFFFFFFFF, int(image_base)
    return s


PREDICTIONS = ("eps", "v")   # sdmi_set_prediction's kind 0, 1


def _prediction(p) -> int:
    if p not in PREDICTIONS:
        raise ValueError(f"prediction must be one of {PREDICTIONS}, got {p!r}")
    return PREDICTIONS.index(p)


def sampler_coefs(kind: str, eta: float, alphas_cumprod, ts, step_size: int, prediction: str = "eps") -> np.ndarray:
    """The per-step coefficients [len(ts), 8] = (cx, ce, h1, h2, h3, cz, qx, qe) of a sampler over the timesteps `ts` a call runs
    (sdmi_sampler_coefs_ex, host only, no GPU; float64):  q = qx x + qe e,  x' = cx x + ce e + h1 q_-1 + h2 q_-2 + h3 q_-3 + cz z.
    prediction "v": e is the model's v output, the table is the eps table rewritten."""
    lib = load_library()
    s = _sampler_struct(kind, eta)
    a = np.ascontiguousarray(alphas_cumprod, dtype=np.float32)
    t = np.ascontiguousarray(ts, dtype=np.int32)
    out = np.empty((t.size, 8), dtype=np.float64)
    check(lib.sdmi_sampler_coefs_ex(C.byref(s), _fp(a), a.size, t.ctypes.data_as(C.POINTER(C.c_int32)), t.size, int(step_size), _prediction(prediction),
                                    out.ctypes.data_as(C.POINTER(C.c_double))))
    return out


def rescale_zero_snr(alphas_cumprod) -> np.ndarray:
    """The schedule rescaled to zero terminal SNR (sdmi_rescale_zero_snr; host only, no GPU): Algorithm 1 of Lin et al. on sqrt(alphas_cumprod) in float64,
    narrowed to float32.  The last entry is exactly 0, the first keeps its bits."""
    lib = load_library()
    a = np.ascontiguousarray(alphas_cumprod, dtype=np.float32)
    if a.ndim != 1:
        raise ValueError(f"alphas_cumprod must be one-dimensional, got {a.shape}")
    out = np.empty_like(a)
    check(lib.sdmi_rescale_zero_snr(_fp(a), _fp(out), a.size))
    return out


KSAMPLER_KINDS = ("euler", "dpmpp_2m", "heun", "dpm2", "dpmpp_2s", "dpmpp_sde", "dpmpp_2m_sde")   # sdmi_ksampler.kind 0 .. 6
KSAMPLER_SCHEDULES = ("model", "karras", "exponential", "uniform")                                # sdmi_ksampler.schedule 0 .. 3
KSAMPLER_PLAN_COLUMNS = ("step", "stage", "t", "sigma", "cx", "ce", "h1", "cz", "cz2", "qx", "qe", "a_end")


def _ksampler_struct(kind, schedule="karras", eta=0.0, rho=7.0, sigma_min=None, sigma_max=None, noise_seed=0, image_base=0) -> SdmiKSampler:
    """Names -> sdmi_ksampler.  Only the names are checked here: the numbers are the library's to refuse (SdmiError)."""
    if kind not in KSAMPLER_KINDS:
        raise ValueError(f"k-sampler kind must be one of {KSAMPLER_KINDS}, got {kind!r}")
    if schedule not in KSAMPLER_SCHEDULES:
        raise ValueError(f"k-sampler schedule must be one of {KSAMPLER_SCHEDULES}, got {schedule!r}")
    k = SdmiKSampler()
    k.kind, k.schedule, k.eta, k.rho = KSAMPLER_KINDS.index(kind), KSAMPLER_SCHEDULES.index(schedule), float(eta), float(rho)
    k.sigma_min, k.sigma_max = float(sigma_min or 0.0), float(sigma_max or 0.0)
    k.noise_seed, k.image_base = int(noise_seed) & 0xFFFFFFFFFFFFFFFF, int(image_base)
    return k


def ksampler_sigmas(kind: str, alphas_cumprod, n_steps: int, schedule: str = "karras", **kw) -> np.ndarray:
    """The steps + 1 sigmas (float64, the last 0) of a k-sampler's schedule for n_steps (sdmi_ksampler_sigmas; host only, no GPU)."""
    lib = load_library()
    k = _ksampler_struct(kind, schedule, **kw)
    a = np.ascontiguousarray(alphas_cumprod, dtype=np.float32)
    out = np.empty(a.size + 2, dtype=np.float64)
    count = C.c_int32()
    check(lib.sdmi_ksampler_sigmas(C.byref(k), _fp(a), a.size, int(n_steps), out.ctypes.data_as(C.POINTER(C.c_double)), out.size, C.byref(count)))
    return out[:count.value].copy()


def sigma_to_t(alphas_cumprod, sigma: float) -> float:
    """The fractional timestep of sigma by k-diffusion's rule (sdmi_sigma_to_t; host only): exactly j at sigma(alphas_cumprod[j])."""
    lib = load_library()
    a = np.ascontiguousarray(alphas_cumprod, dtype=np.float32)
    t = C.c_double()
    check(lib.sdmi_sigma_to_t(_fp(a), a.size, float(sigma), C.byref(t)))
    return t.value


def ksampler_plan(kind: str, alphas_cumprod, n_steps: int, schedule: str = "karras", strength: float = 1.0, prediction: str = "eps", **kw) -> np.ndarray:
    """The evaluation plan [evaluations, 12] (KSAMPLER_PLAN_COLUMNS, float64) of a call of n_steps at `strength` (sdmi_ksampler_plan_ex; host only):
    one row per UNet evaluation,  q = qx x + qe e,  x' = cx x + ce e + h1 q_-1 + cz z + cz2 z2  on the VP latent.  prediction "v": e is the model's v output."""
    lib = load_library()
    k = _ksampler_struct(kind, schedule, **kw)
    a = np.ascontiguousarray(alphas_cumprod, dtype=np.float32)
    out = np.empty((2 * (a.size + 1), 12), dtype=np.float64)
    count = C.c_int32()
    check(lib.sdmi_ksampler_plan_ex(C.byref(k), _fp(a), a.size, int(n_steps), float(strength), _prediction(prediction), out.ctypes.data_as(C.POINTER(C.c_double)),
                                    out.shape[0], C.byref(count)))
    return out[:count.value].copy()


RESIZE_MODES = ("nearest", "bilinear", "bicubic")   # sdmi_resize_weights / sdmi_hires.mode 0, 1, 2 ("nearest" = torch's "nearest-exact")


def _resize_mode(mode) -> int:
    if isinstance(mode, str):
        if mode not in RESIZE_MODES:
            raise ValueError(f"resize mode must be one of {RESIZE_MODES}, got {mode!r}")
        return RESIZE_MODES.index(mode)
    return int(mode)


def resize_weights(in_size: int, out_size: int, mode="bicubic", antialias: bool = False):
    """The resampling table of one axis (sdmi_resize_weights, host only, no GPU): (first [out] int32, count [out] int32, taps [out, max_taps]
    float64) with y[o] = sum_j taps[o, j] x[first[o] + j], j < count[o] -- torch.nn.functional.interpolate's rule (align_corners=False)."""
    lib = load_library()
    m, aa = _resize_mode(mode), 1 if antialias else 0
    T, need = C.c_int32(), C.c_int32()
    check(lib.sdmi_resize_weights(int(in_size), int(out_size), m, aa, None, None, None, 0, C.byref(T), C.byref(need)))
    first = np.empty(int(out_size), dtype=np.int32)
    count = np.empty(int(out_size), dtype=np.int32)
    taps = np.empty((int(out_size), T.value), dtype=np.float64)
    i32 = C.POINTER(C.c_int32)
    check(lib.sdmi_resize_weights(int(in_size), int(out_size), m, aa, first.ctypes.data_as(i32), count.ctypes.data_as(i32),
                                  taps.ctypes.data_as(C.POINTER(C.c_double)), need.value, None, None))
    return first, count, taps


def load_lora_npz(path) -> dict:
    """{target: (down, up, alpha)} from an .npz holding "<target>::down", "<target>::up" and "<target>::alpha" per target (dump-tree
    names of conv / Linear weights; Linear [in,out]: down [rank,in], up [out,rank]; conv [cout,cin,k,k]: down [rank,cin,k,k], up [cout,rank]) --
    what StableDiffusion.lora_attach takes.  save_lora_npz writes it."""
    out = {}
    with np.load(str(path)) as z:
        keys = set(z.files)
        for key in sorted(keys):
            target, sep, part = key.rpartition("::")
            if not sep or part not in ("down", "up", "alpha"):
                raise ValueError(f"{path}: unexpected entry '{key}' (expected '<target>::down|up|alpha')")
            if part != "down":
                continue
            missing = [q for q in ("up", "alpha") if f"{target}::{q}" not in keys]
            if missing:
                raise ValueError(f"{path}: '{target}' lacks {missing}")
            alpha = np.asarray(z[f"{target}::alpha"], dtype=np.float64)
            if alpha.size != 1:
                raise ValueError(f"{path}: '{target}::alpha' must be one number")
            out[target] = (np.asarray(z[key], dtype=np.float32), np.asarray(z[f"{target}::up"], dtype=np.float32), float(alpha.reshape(())))
        for key in keys:
            if key.rpartition("::")[0] not in out:
                raise ValueError(f"{path}: '{key}' has no '::down' partner")
    return out


def save_lora_npz(path, tensors: dict) -> None:
    """The inverse of load_lora_npz."""
    flat = {}
    for target, (down, up, alpha) in tensors.items():
        flat[f"{target}::down"] = np.asarray(down, dtype=np.float32)
        flat[f"{target}::up"] = np.asarray(up, dtype=np.float32)
        flat[f"{target}::alpha"] = np.float32(alpha)
    np.savez(str(path), **flat)


LORA_MAX_RANK = 256


def check_lora_tensors(tensors, shapes: dict) -> list:
    """The argument checks of lora_attach (before anything reaches the library): [(target, down, up, rank, alpha)] as contiguous float32.
    `shapes` = dict(weight_specs())."""
    if not isinstance(tensors, dict) or not tensors:
        raise ValueError("lora tensors must be a non-empty dict {target: (down, up, alpha)}")
    out = []
    for target, item in tensors.items():
        if target not in shapes:
            raise ValueError(f"lora target '{target}' is not a tensor of this model")
        shape = tuple(shapes[target])
        if not target.endswith("/weight") or len(shape) not in (2, 4) or "embedding" in target:
            raise ValueError(f"lora target '{target}' is not a conv or Linear weight")
        try:
            down, up, alpha = item
        except (TypeError, ValueError):
            raise ValueError(f"lora target '{target}': expected (down, up, alpha)") from None
        down, up, alpha = _f32(down, name=f"{target} down"), _f32(up, name=f"{target} up"), float(alpha)
        if not np.isfinite(alpha):
            raise ValueError(f"lora target '{target}': alpha must be finite, got {alpha}")
        rank = down.shape[0] if down.ndim else 0
        if not 1 <= rank <= LORA_MAX_RANK:
            raise ValueError(f"lora target '{target}': rank must be 1..{LORA_MAX_RANK}, got {rank}")
        if len(shape) == 4:
            if shape[1] == 3:
                raise ValueError(f"lora target '{target}': the 3-channel conv_in is not supported")
            want_down, want_up = (rank,) + shape[1:], (shape[0], rank)
        else:
            want_down, want_up = (rank, shape[0]), (shape[1], rank)
        if down.shape != want_down:
            raise ValueError(f"lora target '{target}' {shape}: down must be {want_down}, got {down.shape}")
        if up.shape != want_up:
            raise ValueError(f"lora target '{target}' {shape}: up must be {want_up}, got {up.shape}")
        out.append((target, down, up, rank, alpha))
    return out


LORA_UNET, LORA_TE = 1, 2          # sdmi_lora_load_safetensors `which`
LORA_SKIP_UNKNOWN = 1               # ... and its flag


def lora_module_name(name: str) -> str:
    """The kohya-ss module name of the conv / Linear weight `name` of the UNet or the text encoder ("unet/.../weight", "clip/.../weight"):
    "lora_unet_" / "lora_te_" + its diffusers module path with "_" for "." (sdmi_lora_module_name, host only, no GPU).  SdmiError for any other name."""
    buf = C.create_string_buffer(256)
    check(load_library().sdmi_lora_module_name(name.encode(), buf, 256))
    return buf.value.decode()


def lora_check_safetensors(path, specs, which: int = LORA_UNET | LORA_TE, skip_unknown: bool = False) -> tuple:
    """The checks of lora_load_safetensors that need no device (sdmi_lora_check_safetensors, host only): the kohya file `path` against
    specs = [(dump name, shape)] (weight_specs()).  Returns (n_targets, n_skipped); SdmiError as the loader raises it."""
    specs = [(n, tuple(int(d) for d in shp)) for n, shp in specs if len(shp) in (2, 4)]
    names = (C.c_char_p * len(specs))(*[n.encode() for n, _ in specs])
    ndims = (C.c_int32 * len(specs))(*[len(shp) for _, shp in specs])
    dims = (C.c_int64 * (4 * len(specs)))(*[(shp + (1, 1))[k] for _, shp in specs for k in range(4)])
    nt, ns = C.c_int32(), C.c_int32()
    check(load_library().sdmi_lora_check_safetensors(str(path).encode(), names, ndims, dims, len(specs), int(which), LORA_SKIP_UNKNOWN if skip_unknown else 0,
                                                     C.byref(nt), C.byref(ns)))
    return nt.value, ns.value


class LoraAdapter:
    """One adapter attached to a StableDiffusion (sdmi_lora): .set_scale(s) re-merges its targets on the device, .scale reads it back,
    .detach() restores the targets and frees it.  Owned by the context: closing the StableDiffusion invalidates it."""

    def __init__(self, sd: "StableDiffusion", handle, n_skipped: int = 0):
        self._sd, self._a = sd, handle
        self.n_skipped = n_skipped   # modules of a file that were passed over (lora_load_safetensors(skip_unknown=True))

    def _handle(self):
        if self._a is None or not self._sd._ctx.value:
            raise ValueError("this adapter is detached (or its context is closed)")
        return self._a

    def set_scale(self, scale: float) -> None:
        s = float(scale)
        if not np.isfinite(s):
            raise ValueError(f"lora scale must be finite, got {scale}")
        check(self._sd._lib.sdmi_lora_set_scale(self._handle(), s))

    @property
    def scale(self) -> float:
        s, n = C.c_double(), C.c_int32()
        check(self._sd._lib.sdmi_lora_get_scale(self._handle(), C.byref(s), C.byref(n)))
        return s.value

    @property
    def n_targets(self) -> int:
        s, n = C.c_double(), C.c_int32()
        check(self._sd._lib.sdmi_lora_get_scale(self._handle(), C.byref(s), C.byref(n)))
        return n.value

    @property
    def factor_bytes(self) -> int:
        """device bytes held by the raw factors of a file-loaded adapter (0 for lora_attach's)"""
        b = C.c_size_t()
        check(self._sd._lib.sdmi_lora_factor_bytes(self._handle(), C.byref(b)))
        return b.value

    def detach(self) -> None:
        if self._a is not None and self._sd._ctx.value:
            a, self._a = self._a, None
            check(self._sd._lib.sdmi_lora_destroy(a))
        self._a = None


class LoraFileAdapter:
    """The two halves of one kohya file as two adapters (lora_load_safetensors(te_scale=...)): the "<lora:name:unet:te>" of the front-ends.
    .set_scale(unet, te) re-merges each half at its own scale, .scale reads (unet, te) back, .detach() frees both."""

    def __init__(self, unet: LoraAdapter, te: LoraAdapter):
        self.unet, self.te = unet, te
        self._sd = unet._sd

    def set_scale(self, unet: float, te: float = None) -> None:
        self.unet.set_scale(unet)
        self.te.set_scale(unet if te is None else te)

    @property
    def scale(self) -> tuple:
        return self.unet.scale, self.te.scale

    @property
    def n_targets(self) -> int:
        return self.unet.n_targets + self.te.n_targets

    @property
    def n_skipped(self) -> int:
        return self.unet.n_skipped + self.te.n_skipped

    @property
    def factor_bytes(self) -> int:
        return self.unet.factor_bytes + self.te.factor_bytes

    def detach(self) -> None:
        self.te.detach()
        self.unet.detach()


class MultiLoraAdapter:
    """The same adapter on every device of a MultiStableDiffusion."""

    def __init__(self, parts, owner=None):
        self._parts = list(parts)
        self._owner = owner

    def set_scale(self, *scale) -> None:
        for p in self._parts:
            p.set_scale(*scale)

    @property
    def scale(self) -> float:
        return self._parts[0].scale

    def detach(self) -> None:
        for p in self._parts:
            p.detach()
        if self._owner is not None:      # the owner no longer has to invalidate these device views when it closes
            views = {id(p._sd) for p in self._parts}
            self._owner._lora_views = [v for v in self._owner._lora_views if id(v) not in views]
            self._owner = None


__all__ = ["ModelConfig", "StableDiffusion", "MultiStableDiffusion", "mpk_list", "safetensors_list", "safetensors_model_family", "checkpoint_key", "default_alphas_cumprod", "control_step_on", "control_residual_shapes", "img2img_timesteps", "sampler_coefs", "ksampler_sigmas", "sigma_to_t", "ksampler_plan", "KSAMPLER_KINDS", "KSAMPLER_SCHEDULES", "KSAMPLER_PLAN_COLUMNS", "resize_weights", "load_lora_npz", "save_lora_npz", "lora_module_name", "lora_check_safetensors", "LoraAdapter", "LoraFileAdapter", "LORA_UNET", "LORA_TE", "LORA_SKIP_UNKNOWN", "UNet", "Autoencoder", "CLIP", "SimpleTokenizer", "qkv_attention", "SdmiError"]


@dataclass(frozen=True)
class ModelConfig:
    """Hyper-parameters hard-coded in the reference's *Config::init
    (unet/mod.rs:36-92, autoencoder/mod.rs:30-36, stablediffusion/mod.rs:116)."""
    model_channels: int = 320
    n_head: int = 8
    ctx_dim: int = 768
    latent_h: int = 64
    latent_w: int = 64
    vae_ch: int = 128
    precision: int = 0   # 0 = fp32 (BASELINE configs[0..1]); 1 = bf16 storage + fp32 accumulate (configs[2..3]); 2 = 1 + MXFP8 ResBlock convs (configs[4])
    # CLIP text encoder, CLIPConfig::new(49408, 768, 12, 77, 12) (stablediffusion/mod.rs:29); width = ctx_dim.
    # 0 layers (the default here: the sampling path takes embeddings) builds the context without it.
    clip_layers: int = 0
    clip_heads: int = 12
    clip_vocab: int = 49408
    clip_ctx: int = 77
    # input channels of the UNet: 4 = the latent alone; 5..12 = the latent + conditioning channels (9: the SD v1 inpainting checkpoints)
    unet_in_ch: int = 4
    # channels of a ControlNet's hint picture: 0 = no ControlNet, 3 = an RGB hint (the model gets the weight group controlnet/...)
    control_hint_ch: int = 0
    # 0 = SD v1; 1 = SD 2.x: model_channels-level width / 64 UNet heads of width 64 (n_head is ignored), exact GELU in the text encoder, encode_prompt pads with token 0
    variant: int = 0

    @classmethod
    def sd_v1_4(cls, precision: int = 0, clip: bool = True) -> "ModelConfig":
        """The reference's full StableDiffusionConfig::init (stablediffusion/mod.rs:22-39), text encoder included."""
        return cls(precision=precision, clip_layers=12 if clip else 0)

    @classmethod
    def sd_v2(cls, precision: int = 0, clip: bool = True) -> "ModelConfig":
        """SD 2.x (512-base, 768-v, 2.1): sd_v1_4 with 64-wide UNet heads and the OpenCLIP ViT-H text tower -- width 1024, 16 heads, 23 blocks + the final
        LayerNorm (its "penultimate" output, so clip_skip = 1 is SD 2's standard conditioning)."""
        return cls(precision=precision, ctx_dim=1024, clip_layers=23 if clip else 0, clip_heads=16, variant=1)


def _f32(a, shape=None, name="array") -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=np.float32)
    if shape is not None and tuple(a.shape) != tuple(shape):
        raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(a.shape)}")
    return a


def _fp(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_float))


class StableDiffusion:
    """`StableDiffusion<B>` (src/model/stablediffusion/mod.rs:41-48) on one MI355X."""

    def __init__(self, config: ModelConfig = ModelConfig(), device: int = 0, _borrowed_ctx=None):
        self._lib = load_library()
        self.config = config
        self._owned = _borrowed_ctx is None
        if _borrowed_ctx is not None:      # a per-device view of a MultiStableDiffusion (sdmi_multi_ctx): not ours to destroy
            self._ctx = C.c_void_p(_borrowed_ctx)
            self.unet = UNet(self)
            self.autoencoder = Autoencoder(self)
            self.clip = CLIP(self)
            return
        cfg = SdmiConfig()
        check(self._lib.sdmi_default_config(C.byref(cfg)))
        cfg.device = device
        cfg.model_channels = config.model_channels
        cfg.n_head = config.n_head
        cfg.ctx_dim = config.ctx_dim
        cfg.latent_h = config.latent_h
        cfg.latent_w = config.latent_w
        cfg.vae_ch = config.vae_ch
        cfg.precision = config.precision
        cfg.clip_layers = config.clip_layers
        cfg.clip_heads = config.clip_heads
        cfg.clip_vocab = config.clip_vocab
        cfg.clip_ctx = config.clip_ctx
        cfg.unet_in_ch = config.unet_in_ch
        cfg.control_hint_ch = config.control_hint_ch
        cfg.variant = config.variant
        self._ctx = C.c_void_p()
        check(self._lib.sdmi_create(C.byref(self._ctx), C.byref(cfg)))
        # every option this context was given, in order (bench.py prints the non-default ones next to its figures: `applied_options`)
        self.applied_options: list[tuple[str, str]] = []
        # SDMI_OPTS="key=value key=value": engine options applied to every context of the process (A/B runs of the test suite under another kernel setting).
        # A malformed entry is an error, not a silent no-op: a stale variable must not change a published figure unnoticed.
        for kv in os.environ.get("SDMI_OPTS", "").split():
            k, eq, v = kv.partition("=")
            if not k or not eq:
                raise ValueError(f"SDMI_OPTS: '{kv}' is not key=value")
            self.set_option(k, v)
        self.options_from_env = list(self.applied_options)
        self.unet = UNet(self)
        self.autoencoder = Autoencoder(self)
        self.clip = CLIP(self)

    # ---- lifecycle -----------------------------------------------------------
    def close(self):
        if getattr(self, "_ctx", None) is not None and self._ctx.value:
            if getattr(self, "_owned", True):
                self._lib.sdmi_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ---- weights ---------------------------------------------------------------
    def weight_specs(self):
        """[(name, shape)] of every tensor the hot path needs (reference dump names)."""
        n = self._lib.sdmi_weight_count(self._ctx)
        if n < 0:
            check(n)
        out = []
        name = C.c_char_p()
        ndim = C.c_int32()
        dims = (C.c_int64 * 4)()
        for i in range(n):
            check(self._lib.sdmi_weight_info(self._ctx, i, C.byref(name), C.byref(ndim), dims))
            out.append((name.value.decode(), tuple(int(dims[k]) for k in range(ndim.value))))
        return out

    def set_weight(self, name: str, array) -> None:
        a = np.ascontiguousarray(array, dtype=np.float32)
        dims = (C.c_int64 * max(1, a.ndim))(*a.shape)
        check(self._lib.sdmi_set_weight(self._ctx, name.encode(), _fp(a), a.ndim, dims))

    GROUP_HOT, GROUP_CLIP, GROUP_ENCODER = 1, 2, 4
    GROUP_CONTROL = 8   # never part of a packed image: sdmi_load_weights_packed keeps its groups 1..7

    @staticmethod
    def _group_of(name: str) -> int:
        if name.startswith("controlnet/"):
            return StableDiffusion.GROUP_CONTROL
        if name.startswith("clip/"):
            return StableDiffusion.GROUP_CLIP
        if name.startswith("autoencoder/encoder/") or name.startswith("autoencoder/quant_conv/"):
            return StableDiffusion.GROUP_ENCODER
        return StableDiffusion.GROUP_HOT

    def pack_weights(self, provider, groups: int = 1) -> np.ndarray:
        """The flat image sdmi_load_weights_packed expects: every tensor of the selected groups in weight_specs()
        order, fp32, reference layouts, back to back (SURVEY.md 8b "flat pack")."""
        from .synthetic import alphas_cumprod, named_tensor
        specs = self.weight_specs()
        shapes = dict(specs)
        n = self._lib.sdmi_packed_size(self._ctx, groups)
        if n < 0:
            check(int(n))
        flat = np.empty(int(n), dtype=np.float32)
        off = 0
        for name, shape in specs:
            if not (self._group_of(name) & groups):
                continue
            cnt = int(np.prod(shape))
            src = alphas_cumprod(shape[0]) if name == "alphas_cumprod" else named_tensor(provider, name, shape, shapes)
            flat[off:off + cnt] = np.asarray(src, dtype=np.float32).reshape(-1)
            off += cnt
        assert off == flat.size
        return flat

    def load_weights_packed(self, flat: np.ndarray, groups: int = 1) -> None:
        """One staged upload of the whole model (sdmi_load_weights_packed) + finalize."""
        flat = np.ascontiguousarray(flat, dtype=np.float32)
        check(self._lib.sdmi_load_weights_packed(self._ctx, _fp(flat), flat.size, groups))
        check(self._lib.sdmi_finalize_weights(self._ctx))

    def load_weights_mpk(self, path) -> None:
        """The reference's `burn` model type: a NamedMpkFileRecorder<FullPrecisionSettings> record (sample/main.rs:27-34)."""
        check(self._lib.sdmi_load_weights_mpk(self._ctx, str(path).encode()))
        check(self._lib.sdmi_finalize_weights(self._ctx))

    def load_weights_safetensors(self, path) -> None:
        """An SD v1.x checkpoint in the CompVis layout -- on a variant = 1 context an SD 2.x checkpoint in Stability's layout --, one
        .safetensors file (F32 / F16 / BF16), converted on the device + finalize.  A file of the other family is refused (safetensors_model_family)."""
        check(self._lib.sdmi_load_weights_safetensors(self._ctx, str(path).encode()))
        check(self._lib.sdmi_finalize_weights(self._ctx))

    # ---- ControlNet (include/sdmi.h "ControlNet") ------------------
    def load_control_safetensors(self, path) -> None:
        """A ControlNet in the cldm layout ("control_model.…"), one .safetensors file (F32 / F16 / BF16) -> the weight group controlnet/...
        (sdmi_load_control_safetensors).  The base model is not touched; a set control stays set."""
        check(self._lib.sdmi_load_control_safetensors(self._ctx, str(path).encode()))

    @property
    def control_ready(self) -> bool:
        r = self._lib.sdmi_control_ready(self._ctx)
        if r < 0:
            check(r)
        return bool(r)

    def set_control(self, hint, strength: float = 1.0, start: float = 0.0, end: float = 1.0) -> None:
        """The control of every later forward / sampling call of this context (sdmi_set_control; sticky): hint uint8 [n_hint, 8h, 8w, 3] (or [8h, 8w, 3]:
        one hint for every image), its values / 255; strength multiplies the 13 residuals; step i of the S steps a call runs is controlled iff
        start * S <= i < end * S.  None clears."""
        if hint is None:
            check(self._lib.sdmi_set_control(self._ctx, None))
            return
        hint = np.ascontiguousarray(hint)
        if hint.dtype != np.uint8:
            raise ValueError(f"hint must be uint8, got {hint.dtype}")
        if hint.ndim == 3:
            hint = hint[None]
        if hint.ndim != 4 or hint.shape[3] != 3:
            raise ValueError(f"hint must be [n, H, W, 3], got {hint.shape}")
        c = SdmiControl()
        c.hint_rgb = hint.ctypes.data_as(C.POINTER(C.c_uint8))
        c.n_hint, c.hint_h, c.hint_w = int(hint.shape[0]), int(hint.shape[1]), int(hint.shape[2])
        c.strength, c.start, c.end = float(strength), float(start), float(end)
        check(self._lib.sdmi_set_control(self._ctx, C.byref(c)))

    # ---- IP-Adapter (include/sdmi.h "IP-Adapter") -------------------
    def load_ip_adapter_safetensors(self, path) -> None:
        """An IP-Adapter in h94's ip-adapter_sd15.safetensors layout (F32 / F16 / BF16): image_proj.* and ip_adapter.<j>.to_k_ip / to_v_ip
        (sdmi_ip_adapter_load_safetensors).  The "plus" Resampler files and pickles are refused; the base model is not touched."""
        check(self._lib.sdmi_ip_adapter_load_safetensors(self._ctx, str(path).encode()))

    def set_ip_adapter_weights(self, proj_w, proj_b, norm_g, norm_b, wk, wv) -> None:
        """The adapter's tensors as arrays in the file's layouts (sdmi_ip_adapter_set_weights): proj_w [T ctx_dim, D], proj_b [T ctx_dim], norm_g / norm_b [ctx_dim],
        wk / wv: 16 matrices [C_i, ctx_dim] in the engine's order (ip_adapter_key's ctx_index)."""
        cd = self.config.ctx_dim
        proj_w = _f32(proj_w)
        if proj_w.ndim != 2 or proj_w.shape[0] % cd:
            raise ValueError(f"proj_w must be [T * {cd}, D], got {proj_w.shape}")
        T, D = proj_w.shape[0] // cd, proj_w.shape[1]
        proj_b, norm_g, norm_b = _f32(proj_b, (T * cd,), "proj_b"), _f32(norm_g, (cd,), "norm_g"), _f32(norm_b, (cd,), "norm_b")
        if len(wk) != 16 or len(wv) != 16:
            raise ValueError("wk / wv must hold 16 matrices")
        ks, vs = [], []
        for i in range(16):
            _, _, c = ip_adapter_key(self.config, i, "k", with_shape=True)
            ks.append(_f32(wk[i], (c, cd), f"wk[{i}]"))
            vs.append(_f32(wv[i], (c, cd), f"wv[{i}]"))
        pk, pv = (_capi._F * 16)(*[_fp(a) for a in ks]), (_capi._F * 16)(*[_fp(a) for a in vs])
        check(self._lib.sdmi_ip_adapter_set_weights(self._ctx, _fp(proj_w), _fp(proj_b), _fp(norm_g), _fp(norm_b), int(D), int(T), pk, pv))

    @property
    def ip_adapter_ready(self) -> bool:
        r = self._lib.sdmi_ip_adapter_ready(self._ctx)
        if r < 0:
            check(r)
        return bool(r)

    def clear_ip_adapter_weights(self) -> None:
        """Frees the adapter's weights and clears the setting (sdmi_ip_adapter_clear)."""
        check(self._lib.sdmi_ip_adapter_clear(self._ctx))

    def ip_image_tokens(self, embeds) -> np.ndarray:
        """image_proj alone (sdmi_ip_image_tokens): embeds [n, D] -> LayerNorm(reshape(Linear(embeds))) [n, T, ctx_dim]."""
        e = _f32(embeds)
        if e.ndim != 2:
            raise ValueError(f"embeds must be [n, D], got {e.shape}")
        n, D = e.shape
        T = self.ip_adapter_dims()[1]
        out = np.empty((n, T, self.config.ctx_dim), np.float32)
        check(self._lib.sdmi_ip_image_tokens(self._ctx, _fp(e), n, D, _fp(out)))
        return out

    def ip_adapter_dims(self) -> tuple:
        """(D, T) of the loaded adapter (sdmi_ip_adapter_dims): the image embedding's width and the tokens one picture becomes."""
        d, t = C.c_int32(), C.c_int32()
        check(self._lib.sdmi_ip_adapter_dims(self._ctx, C.byref(d), C.byref(t)))
        return int(d.value), int(t.value)

    def set_ip_adapter(self, embeds=None, tokens=None, negative_tokens=None, scale: float = 1.0, start: float = 0.0, end: float = 1.0) -> None:
        """The image prompt of every later forward / sampling call (sdmi_set_ip_adapter; sticky).  embeds [n_img, D] (or [n_sets, n_img, D]): the caller's CLIP
        image embeddings, projected by image_proj, the pictures of a set concatenated along the token axis; or tokens [T_ip, ctx_dim] (or [n_sets, T_ip, ctx_dim])
        projected outside.  negative_tokens: what the unconditional half of a CFG batch reads (default image_proj(0)).  Image i of a call reads set i mod n_sets.
        scale multiplies the image attention (0: the plain forward); step i of S is adapted iff start * S <= i < end * S.  set_ip_adapter(None) clears."""
        if embeds is None and tokens is None:
            check(self._lib.sdmi_set_ip_adapter(self._ctx, None))
            return
        keep = []
        a = _ip_adapter_struct(keep, embeds, tokens, negative_tokens, scale, start, end)
        if a.T_ip < 0:
            a.T_ip = -a.T_ip * self.ip_adapter_dims()[1]
        check(self._lib.sdmi_set_ip_adapter(self._ctx, C.byref(a)))

    def set_ip_adapter_file(self, embeds_path, scale: float = 1.0, start: float = 0.0, end: float = 1.0) -> None:
        """set_ip_adapter with embeds read from the tensor "image_embeds" [n, D] of a .safetensors file (sdmi_set_ip_adapter_file): one set of n pictures."""
        check(self._lib.sdmi_set_ip_adapter_file(self._ctx, str(embeds_path).encode(), float(scale), float(start), float(end)))

    def get_ip_adapter(self):
        """The setting in force (sdmi_get_ip_adapter): None, or {"n_sets", "T_ip", "scale", "start", "end"}."""
        a = SdmiIpAdapter()
        r = self._lib.sdmi_get_ip_adapter(self._ctx, C.byref(a))
        if r < 0:
            check(r)
        if not r:
            return None
        return {"n_sets": int(a.n_sets), "T_ip": int(a.T_ip), "scale": float(a.scale), "start": float(a.start), "end": float(a.end)}

    def op_ip_attention(self, q, k_ip, v_ip, o_text, scale, n_head: int, planes: bool = False) -> np.ndarray:
        """tests (sdmi_op_ip_attention): O_text + scale_b softmax(q K_ip^T d^-1/2) V_ip through the launch the model runs, in the context's storage type.
        q, o_text [n, nq, C]; k_ip, v_ip [n, T_ip, C]; scale [n].  planes (precision 0): O_text as bf16 planes, read-modify-write, joined."""
        q, k_ip, v_ip, o_text, scale = _f32(q), _f32(k_ip), _f32(v_ip), _f32(o_text), _f32(scale)
        if q.ndim != 3 or k_ip.ndim != 3:
            raise ValueError("op_ip_attention: q must be [n, nq, C] and k_ip [n, T_ip, C]")
        n, nq, c = q.shape
        T = k_ip.shape[1]
        _f32(k_ip, (n, T, c), "k_ip"); _f32(v_ip, (n, T, c), "v_ip"); _f32(o_text, (n, nq, c), "o_text"); _f32(scale, (n,), "scale")
        out = np.empty_like(q)
        check(self._lib.sdmi_op_ip_attention(self._ctx, _fp(q), _fp(k_ip), _fp(v_ip), _fp(o_text), _fp(scale), n, nq, T, c, int(n_head), 1 if planes else 0, _fp(out)))
        return out

    def ip_kv(self, n: int, cfg_pair: bool = False) -> list:
        """tests (sdmi_ip_kv): the K_ip / V_ip a call with n images would hoist -- [(K_i, V_i)] for the 16 cross attentions, each [nb, T_ip, C_i]."""
        size = self._lib.sdmi_ip_kv_size(self._ctx, int(n), 1 if cfg_pair else 0)
        if size < 0:
            check(int(size))
        flat = np.empty(int(size), np.float32)
        check(self._lib.sdmi_ip_kv(self._ctx, int(n), 1 if cfg_pair else 0, _fp(flat)))
        nb, T = (2 * n if cfg_pair else n), self.get_ip_adapter()["T_ip"]
        out, off = [], 0
        for i in range(16):
            _, _, c = ip_adapter_key(self.config, i, "k", with_shape=True)
            e = nb * T * c
            out.append((flat[off:off + e].reshape(nb, T, c), flat[off + e:off + 2 * e].reshape(nb, T, c)))
            off += 2 * e
        return out

    def control_hint_embed(self, hint) -> np.ndarray:
        """The hint embedding [n, model_channels, H / 8, W / 8] of hint uint8 [n, H, W, 3] (sdmi_control_hint_embed)."""
        hint = np.ascontiguousarray(hint, dtype=np.uint8)
        if hint.ndim != 4 or hint.shape[3] != 3:
            raise ValueError(f"hint must be [n, H, W, 3], got {hint.shape}")
        n, H, Wd = hint.shape[:3]
        out = np.empty((n, self.config.model_channels, H // 8, Wd // 8), np.float32)
        check(self._lib.sdmi_control_hint_embed(self._ctx, hint.ctypes.data_as(C.POINTER(C.c_uint8)), n, H, Wd, _fp(out)))
        return out

    def control_residuals(self, x, t: int, context) -> list:
        """The 13 residuals of the set control for x [n,4,h,w], timestep t and context [n,T,ctx_dim] (sdmi_control_residuals; strength and step window ignored):
        a list of NCHW arrays, zero_convs 0 .. 11 then middle_block_out."""
        h, w = self.latent_size
        x = _f32(x, name="x")
        if x.ndim != 4 or x.shape[1:] != (4, h, w):
            raise ValueError(f"x must be [n,4,{h},{w}], got {x.shape}")
        n = x.shape[0]
        context = _f32(context, name="context")
        if context.ndim != 3 or context.shape[0] != n or context.shape[2] != self.config.ctx_dim:
            raise ValueError(f"context must be [{n}, T, {self.config.ctx_dim}], got {context.shape}")
        total = self._lib.sdmi_control_residuals_size(self._ctx, n)
        if total < 0:
            check(int(total))
        flat = np.empty(int(total), np.float32)
        check(self._lib.sdmi_control_residuals(self._ctx, _fp(x), int(t), _fp(context), n, context.shape[1], _fp(flat)))
        mc = self.config.model_channels
        out, off = [], 0
        for c, s in control_residual_shapes(mc):
            shape = (n, c, h >> s, w >> s)
            cnt = int(np.prod(shape))
            out.append(flat[off:off + cnt].reshape(shape))
            off += cnt
        assert off == flat.size
        return out

    def set_stream(self, hip_stream, enable: bool = True) -> None:
        """Name the HIP stream (integer handle, e.g. torch.cuda.current_stream().cuda_stream) the caller's device
        buffers of the *_dev calls are produced / consumed on (sdmi_set_stream)."""
        check(self._lib.sdmi_set_stream(self._ctx, C.c_void_p(int(hip_stream) if hip_stream else 0), 1 if enable else 0))

    def set_latent_size(self, h: int, w: int) -> None:
        """The latent size [h, w] of every later call of this context (sdmi_set_latent_size; sticky): positive multiples of 8, pictures are 8x.
        config.latent_h / latent_w are the initial value; the weights do not depend on the size."""
        check(self._lib.sdmi_set_latent_size(self._ctx, int(h), int(w)))

    @property
    def latent_size(self) -> tuple:
        """the current (h, w) of the context (sdmi_get_latent_size); without a live context, the configured size"""
        if not self._ctx.value:
            return self.config.latent_h, self.config.latent_w
        h, w = C.c_int32(), C.c_int32()
        check(self._lib.sdmi_get_latent_size(self._ctx, C.byref(h), C.byref(w)))
        return h.value, w.value

    def set_sampler(self, kind="ddim", eta: float = 0.0, noise_seed: int = 0, image_base: int = 0) -> None:
        """Choose the sampler of every later sampling call of this context (sdmi_set_sampler; sticky): "ddim" with 0 <= eta <= 1
        (eta = 0, the default: the reference's deterministic DDIM = plain Euler; eta = 1 = Euler-ancestral), "dpmpp_2m"
        (DPM-Solver++(2M)) or "plms".  None restores the default.  noise_seed keys the step noise of eta > 0; image_base is the global
        index of the call's first image, so that a batch split into smaller calls draws the same noise per image."""
        if kind is None:
            check(self._lib.sdmi_set_sampler(self._ctx, None))
            return
        s = _sampler_struct(kind, eta, noise_seed, image_base)
        check(self._lib.sdmi_set_sampler(self._ctx, C.byref(s)))

    def get_sampler(self) -> dict:
        s = SdmiSampler()
        check(self._lib.sdmi_get_sampler(self._ctx, C.byref(s)))
        return {"kind": SAMPLER_KINDS[s.kind], "eta": s.eta, "noise_seed": s.noise_seed, "image_base": s.image_base}

    def set_ksampler(self, kind="dpmpp_2m", schedule="karras", eta: float = 0.0, rho: float = 7.0, sigma_min=None, sigma_max=None, noise_seed: int = 0,
                     image_base: int = 0) -> None:
        """Choose a sigma-schedule sampler for every later sampling call of this context (sdmi_set_ksampler; sticky): kind one of KSAMPLER_KINDS, schedule one of
        KSAMPLER_SCHEDULES, eta 0 .. 1 for the kinds that take noise ("euler" at eta 1 is Euler-ancestral), rho of the Karras spacing, sigma_min / sigma_max (None: the
        model's).  None clears it.  Setting it resets set_sampler's choice to the default, and any set_sampler call clears it."""
        if kind is None:
            check(self._lib.sdmi_set_ksampler(self._ctx, None))
            return
        k = _ksampler_struct(kind, schedule, eta, rho, sigma_min, sigma_max, noise_seed, image_base)
        check(self._lib.sdmi_set_ksampler(self._ctx, C.byref(k)))

    def get_ksampler(self):
        """The k-sampler in force as a dict, or None."""
        k, is_set = SdmiKSampler(), C.c_int32()
        check(self._lib.sdmi_get_ksampler(self._ctx, C.byref(k), C.byref(is_set)))
        if not is_set.value:
            return None
        return {"kind": KSAMPLER_KINDS[k.kind], "schedule": KSAMPLER_SCHEDULES[k.schedule], "eta": k.eta, "rho": k.rho, "sigma_min": k.sigma_min,
                "sigma_max": k.sigma_max, "noise_seed": k.noise_seed, "image_base": k.image_base}

    # ---- LoRA adapters (include/sdmi.h "LoRA adapters") ----------------
    def lora_attach(self, tensors, scale: float = 1.0) -> LoraAdapter:
        """Attach a LoRA adapter and merge it at `scale`: tensors = {target: (down, up, alpha)} (load_lora_npz), the effective weight of each
        target becomes W0 + scale * alpha / rank * up @ down, merged and re-packed on the device.  The context must have been given
        set_option("keep_masters", 1) before its weights were loaded.  Returns the adapter (.set_scale(s), .scale, .detach())."""
        items = check_lora_tensors(tensors, dict(self.weight_specs()))
        s = float(scale)
        if not np.isfinite(s):
            raise ValueError(f"lora scale must be finite, got {scale}")
        h = C.c_void_p()
        check(self._lib.sdmi_lora_create(self._ctx, C.byref(h)))
        adapter = LoraAdapter(self, h)
        try:
            for target, down, up, rank, alpha in items:
                check(self._lib.sdmi_lora_add(h, target.encode(), _fp(down), _fp(up), rank, alpha))
            adapter.set_scale(s)
        except Exception:
            adapter.detach()
            raise
        return adapter

    def _lora_load(self, path, which: int, skip_unknown: bool, scale: float) -> LoraAdapter:
        h, nt, ns = C.c_void_p(), C.c_int32(), C.c_int32()
        check(self._lib.sdmi_lora_load_safetensors(self._ctx, str(path).encode(), which, LORA_SKIP_UNKNOWN if skip_unknown else 0, C.byref(h), C.byref(nt), C.byref(ns)))
        adapter = LoraAdapter(self, h, ns.value)
        try:
            adapter.set_scale(scale)
        except Exception:
            adapter.detach()
            raise
        return adapter

    def lora_load_safetensors(self, path, scale: float = 1.0, te_scale: float = None, skip_unknown: bool = False):
        """Attach a kohya-ss / LyCORIS LoRA file (.safetensors: LoRA, LoCon and LoHa modules in F32 / F16 / BF16, named after diffusers modules) and merge it
        at `scale` (sdmi_lora_load_safetensors): the factors go to the device as the file holds them and are widened by the merge kernel.  te_scale=None: one
        LoraAdapter over the UNet and the text encoder.  Otherwise a LoraFileAdapter whose two halves carry their own scales (.set_scale(unet, te)).
        skip_unknown: modules this model has no tensor for (a text-encoder layer it lacks, a weight group that is not loaded) are passed over and counted in
        .n_skipped instead of refusing the file.  Needs set_option("keep_masters", 1) before the weights were loaded."""
        s = float(scale)
        t = s if te_scale is None else float(te_scale)
        if not (np.isfinite(s) and np.isfinite(t)):
            raise ValueError(f"lora scales must be finite, got {scale}, {te_scale}")
        if te_scale is None:
            return self._lora_load(path, LORA_UNET | LORA_TE, skip_unknown, s)
        unet = self._lora_load(path, LORA_UNET, skip_unknown, s)
        try:
            te = self._lora_load(path, LORA_TE, skip_unknown, t)
        except Exception:
            unet.detach()
            raise
        return LoraFileAdapter(unet, te)

    def effective_weight(self, name: str) -> np.ndarray:
        """The fp32 tensor (reference layout) currently packed for the conv / Linear weight `name`: the loaded one, or the merge of the
        adapters active on it (sdmi_lora_effective_weight; needs keep_masters)."""
        shapes = dict(self.weight_specs())
        if name not in shapes:
            raise ValueError(f"'{name}' is not a tensor of this model")
        out = np.empty(shapes[name], dtype=np.float32)
        check(self._lib.sdmi_lora_effective_weight(self._ctx, name.encode(), _fp(out), out.size))
        return out

    def load_weights(self, provider, clip: bool = True, vae_encoder: bool = True, control: bool = True) -> None:
        """Pull every tensor from `provider.get(name, shape, kind, fan_in)`
        (synthetic.SyntheticWeights) -- the counterpart of load_stable_diffusion
        (stablediffusion/load.rs:16-33) for seeded synthetic parameters.  `clip=False` leaves the
        optional clip/... group unset (context()/clip.forward then raise)."""
        specs = self.weight_specs()
        shapes = dict(specs)
        for name, shape in specs:
            if name.startswith("clip/") and not clip:
                continue
            if (name.startswith("autoencoder/encoder/") or name.startswith("autoencoder/quant_conv/")) and not vae_encoder:
                continue
            if name.startswith("controlnet/") and not control:
                continue
            if name == "alphas_cumprod":
                from .synthetic import alphas_cumprod
                self.set_weight(name, alphas_cumprod(shape[0]))
                continue
            from .synthetic import named_tensor
            arr = named_tensor(provider, name, shape, shapes)
            self.set_weight(name, arr)
        check(self._lib.sdmi_finalize_weights(self._ctx))

    # ---- prompt -> context (stablediffusion/mod.rs:194-210) ----------------------
    def context(self, tokenizer: "SimpleTokenizer", text: str) -> np.ndarray:
        """StableDiffusion::context: CLIP embedding [1, T, ctx_dim] of "<|startoftext|>{text}<|endoftext|>", T = tokens + 2."""
        cap = self.config.clip_ctx
        out = np.empty((cap, self.config.ctx_dim), dtype=np.float32)
        T = C.c_int32()
        check(self._lib.sdmi_context(self._ctx, tokenizer._tok, text.encode("utf-8"), _fp(out), cap, C.byref(T)))
        return out[None, :T.value].copy()

    def unconditional_context(self, tokenizer: "SimpleTokenizer") -> np.ndarray:
        """StableDiffusion::unconditional_context (:194-196): context("") squeezed to [2, ctx_dim]."""
        return self.context(tokenizer, "")[0]

    # ---- web-UI prompt encoding (no reference counterpart) ----
    def encode_prompt(self, tokenizer: "SimpleTokenizer", text: str, emphasis: bool = True, clip_skip: int = 1, min_chunks: int = 1) -> np.ndarray:
        """The prompt as the SD v1 front-ends encode it: [1, k * clip_ctx, ctx_dim] -- k chunks padded to clip_ctx tokens, with emphasis weights, the
        context's textual-inversion embeddings and CLIP skip applied.  encode_prompt(...)[0] is a valid unconditional_context."""
        opts = SdmiPromptOpts(int(bool(emphasis)), int(clip_skip), int(min_chunks))
        T = C.c_int32()
        cap = self.config.clip_ctx * max(1, int(min_chunks), len(text.encode("utf-8")) // 8 + 2)
        while True:
            out = np.empty((cap, self.config.ctx_dim), dtype=np.float32)
            st = self._lib.sdmi_encode_prompt(self._ctx, tokenizer._tok, text.encode("utf-8"), C.byref(opts), _fp(out), cap, C.byref(T))
            if st != 0 and T.value > cap:   # *T is always set: the one retry has the room
                cap = T.value
                continue
            check(st)
            return out[None, :T.value].copy()

    def add_embedding(self, tokenizer: "SimpleTokenizer", name: str, vectors) -> None:
        """A textual-inversion embedding: vectors [v, ctx_dim] (or [ctx_dim]) that stand for `name` wherever encode_prompt meets its tokens."""
        v = np.ascontiguousarray(vectors, dtype=np.float32)
        if v.ndim == 1:
            v = v[None]
        if v.ndim != 2 or v.shape[1] != self.config.ctx_dim:
            raise ValueError(f"vectors must be [v, {self.config.ctx_dim}], got {v.shape}")
        check(self._lib.sdmi_embedding_add(self._ctx, tokenizer._tok, name.encode("utf-8"), _fp(v), v.shape[0]))

    def load_embedding(self, tokenizer: "SimpleTokenizer", name: str, path) -> None:
        """add_embedding from a .safetensors file (tensor "emb_params" or the only tensor; F32 / F16 / BF16), converted on the device"""
        check(self._lib.sdmi_embedding_load_safetensors(self._ctx, tokenizer._tok, name.encode("utf-8"), str(path).encode()))

    def remove_embedding(self, name: str) -> None:
        check(self._lib.sdmi_embedding_remove(self._ctx, name.encode("utf-8")))

    def embeddings(self) -> list:
        """[(name, n_vectors)] in bank order"""
        out = []
        for line in _text_query(self._lib.sdmi_embedding_list, self._ctx).split("\n")[:-1]:
            name, v = line.rsplit("\t", 1)
            out.append((_listing_unescape(name), int(v)))
        return out

    def load_weights_dir(self, dump_dir: str) -> None:
        """npy-dump tree written by the reference's python/ exporters
        (load_stable_diffusion, stablediffusion/load.rs:16-33)."""
        check(self._lib.sdmi_load_weights_dir(self._ctx, str(dump_dir).encode()))
        check(self._lib.sdmi_finalize_weights(self._ctx))

    # ---- reference surface -------------------------------------------------------
    def _check_ctx(self, context, unconditional_context):
        cd = self.config.ctx_dim
        context = _f32(context, name="context")
        if context.ndim != 3 or context.shape[2] != cd:
            raise ValueError(f"context must be [n, T, {cd}], got {context.shape}")
        uncond = _f32(unconditional_context, name="unconditional_context")
        if uncond.ndim != 2 or uncond.shape[1] != cd:
            raise ValueError(f"unconditional_context must be [Tu, {cd}], got {uncond.shape}")
        return context, uncond

    def sample_latent(self, context, unconditional_context, unconditional_guidance_scale: float, n_steps: int,
                      init_latent=None, seed: int = 0) -> np.ndarray:
        """stablediffusion/mod.rs:102-160 -> latent [n,4,h,w].  `init_latent`
        is x_T (the reference draws it from an unseeded RNG)."""
        context, uncond = self._check_ctx(context, unconditional_context)
        n, T, _ = context.shape
        h, w = self.latent_size
        out = np.empty((n, 4, h, w), dtype=np.float32)
        x0 = None if init_latent is None else _f32(init_latent, (n, 4, h, w), "init_latent")
        check(self._lib.sdmi_sample_latent(self._ctx, _fp(context), n, T, _fp(uncond), uncond.shape[0],
                                           float(unconditional_guidance_scale), int(n_steps),
                                           None if x0 is None else _fp(x0), int(seed), _fp(out)))
        return out

    def latent_to_image(self, latent) -> np.ndarray:
        """stablediffusion/mod.rs:69-100 -> uint8 [n, 8h, 8w, 3] (the reference's Vec<Vec<u8>>)."""
        h, w = self.latent_size
        latent = _f32(latent, name="latent")
        if latent.ndim != 4 or latent.shape[1:] != (4, h, w):
            raise ValueError(f"latent must be [n,4,{h},{w}], got {latent.shape}")
        n = latent.shape[0]
        out = np.empty((n, 8 * h, 8 * w, 3), dtype=np.uint8)
        check(self._lib.sdmi_latent_to_image(self._ctx, _fp(latent), n, out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    def sample_image(self, context, unconditional_context, unconditional_guidance_scale: float, n_steps: int,
                     init_latent=None, seed: int = 0) -> np.ndarray:
        """stablediffusion/mod.rs:51-67 -> uint8 [n, 8h, 8w, 3]."""
        context, uncond = self._check_ctx(context, unconditional_context)
        n, T, _ = context.shape
        h, w = self.latent_size
        out = np.empty((n, 8 * h, 8 * w, 3), dtype=np.uint8)
        x0 = None if init_latent is None else _f32(init_latent, (n, 4, h, w), "init_latent")
        check(self._lib.sdmi_sample_image(self._ctx, _fp(context), n, T, _fp(uncond), uncond.shape[0],
                                          float(unconditional_guidance_scale), int(n_steps),
                                          None if x0 is None else _fp(x0), int(seed),
                                          out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    # ---- img2img (include/sdmi.h "img2img"; DESIGN.md section "img2img") ----------------------
    def _check_img2img(self, n, strength, mask, noise):
        h, w = self.latent_size
        s = float(strength)
        if not 0.0 < s <= 1.0:   # NaN fails too
            raise ValueError(f"strength must satisfy 0 < strength <= 1, got {strength}")
        if mask is not None:
            mask = _f32(mask, name="mask")
            if mask.shape not in ((n, h, w), (n, 1, h, w)):
                raise ValueError(f"mask must be [n,{h},{w}] or [n,1,{h},{w}] with n = {n}, got {mask.shape}")
            if not (np.isfinite(mask).all() and (mask >= 0).all() and (mask <= 1).all()):
                raise ValueError("mask values must lie in [0, 1]")
            mask = mask.reshape(n, 1, h, w)
        if noise is not None:
            noise = _f32(noise, (n, 4, h, w), "noise")
        return s, mask, noise

    def sample_latent_from(self, context, unconditional_context, unconditional_guidance_scale: float, n_steps: int, strength: float,
                           z0, mask=None, noise=None, seed: int = 0, cond=None) -> np.ndarray:
        """img2img in latent space -> latent [n,4,h,w].  cond [n, unet_in_ch - 4, h, w]: the conditioning channels of a UNet built with unet_in_ch > 4
        (sdmi_img2img_latent_cond; only the UNet sees them).  z0 [n,4,h,w] is the start latent in the sampler's space
        (0.18215 x the VAE posterior mean); the loop runs the last int(strength * L) of sample_latent's L timesteps.
        mask [n,h,w] / [n,1,h,w] (1 = regenerate, 0 = keep); noise [n,4,h,w], or None: image i draws from stream seed + i."""
        context, uncond = self._check_ctx(context, unconditional_context)
        n, T, _ = context.shape
        h, w = self.latent_size
        z0 = _f32(z0, (n, 4, h, w), "z0")
        s, mask, noise = self._check_img2img(n, strength, mask, noise)
        out = np.empty((n, 4, h, w), dtype=np.float32)
        if cond is not None:
            cond = self._check_cond(cond, n)
            check(self._lib.sdmi_img2img_latent_cond(self._ctx, _fp(context), n, T, _fp(uncond), uncond.shape[0], float(unconditional_guidance_scale),
                                                     int(n_steps), s, _fp(z0), None if mask is None else _fp(mask),
                                                     None if noise is None else _fp(noise), int(seed), _fp(cond), _fp(out)))
            return out
        check(self._lib.sdmi_img2img_latent(self._ctx, _fp(context), n, T, _fp(uncond), uncond.shape[0], float(unconditional_guidance_scale),
                                            int(n_steps), s, _fp(z0), None if mask is None else _fp(mask),
                                            None if noise is None else _fp(noise), int(seed), _fp(out)))
        return out

    def sample_image_from(self, context, unconditional_context, unconditional_guidance_scale: float, n_steps: int, strength: float,
                          init_image, mask=None, noise=None, seed: int = 0) -> np.ndarray:
        """img2img from a picture -> uint8 [n, 8h, 8w, 3].  init_image uint8 [n, 8h, 8w, 3] (sample_image's layout).
        mask at latent resolution ([n,h,w] / [n,1,h,w]) or at pixel resolution ([n,8h,8w], bool / u8 0..255 / float; reduced
        by an 8x8 max, so a touched pixel regenerates its latent cell).  Kept pixels go through one VAE round trip;
        they are not pasted back.  Needs the VAE encoder weights."""
        context, uncond = self._check_ctx(context, unconditional_context)
        n, T, _ = context.shape
        h, w = self.latent_size
        img = np.asarray(init_image)
        if img.dtype != np.uint8 or img.shape != (n, 8 * h, 8 * w, 3):
            raise ValueError(f"init_image must be uint8 [{n},{8 * h},{8 * w},3], got {img.dtype} {img.shape}")
        img = np.ascontiguousarray(img)
        if mask is not None:
            m = np.asarray(mask)
            if m.dtype == np.uint8:   # 0 / 255 image masks
                m = m.astype(np.float32) / np.float32(255.0)
            if m.shape == (n, 8 * h, 8 * w):
                m = m.astype(np.float32).reshape(n, h, 8, w, 8).max(axis=(2, 4))
            mask = m
        s, mask, noise = self._check_img2img(n, strength, mask, noise)
        out = np.empty((n, 8 * h, 8 * w, 3), dtype=np.uint8)
        check(self._lib.sdmi_img2img_image(self._ctx, _fp(context), n, T, _fp(uncond), uncond.shape[0], float(unconditional_guidance_scale),
                                           int(n_steps), s, img.ctypes.data_as(C.POINTER(C.c_uint8)), None if mask is None else _fp(mask),
                                           None if noise is None else _fp(noise), int(seed), out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    # ---- conditioned UNet and inpainting checkpoints (include/sdmi.h "conditioning channels") ------------------------------
    def _check_cond(self, cond, n) -> np.ndarray:
        h, w = self.latent_size
        return _f32(cond, (n, self.config.unet_in_ch - 4, h, w), "cond")

    def _check_inpaint_inputs(self, init_image, mask, n):
        h, w = self.latent_size
        img = np.asarray(init_image)
        if img.dtype != np.uint8 or img.shape != (n, 8 * h, 8 * w, 3):
            raise ValueError(f"init_image must be uint8 [{n},{8 * h},{8 * w},3], got {img.dtype} {img.shape}")
        m = np.asarray(mask)
        if m.dtype == np.bool_:
            m = m.astype(np.uint8) * np.uint8(255)
        if m.dtype != np.uint8 or m.shape != (n, 8 * h, 8 * w):
            raise ValueError(f"mask must be uint8 (>= 128: regenerate) or bool [{n},{8 * h},{8 * w}], got {m.dtype} {m.shape}")
        return np.ascontiguousarray(img), np.ascontiguousarray(m)

    def inpaint_cond(self, init_image, mask) -> np.ndarray:
        """The conditioning of an inpainting checkpoint (unet_in_ch = 9; sdmi_inpaint_cond): init_image uint8 [n,8h,8w,3], mask uint8 [n,8h,8w] (>= 128:
        regenerate) -> cond [n,5,h,w] = [latent mask | 0.18215 * encode(masked picture)].  Needs the VAE encoder weights."""
        n = int(np.asarray(init_image).shape[0])
        h, w = self.latent_size
        img, m = self._check_inpaint_inputs(init_image, mask, n)
        out = np.empty((n, 5, h, w), dtype=np.float32)
        check(self._lib.sdmi_inpaint_cond(self._ctx, img.ctypes.data_as(C.POINTER(C.c_uint8)), m.ctypes.data_as(C.POINTER(C.c_uint8)), n, _fp(out)))
        return out

    def inpaint_image(self, context, unconditional_context, unconditional_guidance_scale: float, n_steps: int, strength: float, init_image, mask,
                      latent_blend: bool = False, paste_back: bool = False, noise=None, seed: int = 0) -> np.ndarray:
        """Inpainting with an inpainting checkpoint (unet_in_ch = 9; sdmi_inpaint_image) -> uint8 [n,8h,8w,3].  mask uint8 [n,8h,8w], >= 128: regenerate.
        latent_blend: also blend the kept region toward the init latent after every step; paste_back: copy the kept pixels from init_image."""
        context, uncond = self._check_ctx(context, unconditional_context)
        n, T, _ = context.shape
        h, w = self.latent_size
        img, m = self._check_inpaint_inputs(init_image, mask, n)
        s, _, noise = self._check_img2img(n, strength, None, noise)
        opt = SdmiInpaint(latent_blend=1 if latent_blend else 0, paste_back=1 if paste_back else 0)
        out = np.empty((n, 8 * h, 8 * w, 3), dtype=np.uint8)
        check(self._lib.sdmi_inpaint_image(self._ctx, _fp(context), n, T, _fp(uncond), uncond.shape[0], float(unconditional_guidance_scale), int(n_steps), s,
                                           img.ctypes.data_as(C.POINTER(C.c_uint8)), m.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(opt),
                                           None if noise is None else _fp(noise), int(seed), out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    # ---- hires fix (include/sdmi.h "hires fix") ------------------------------
    def _hires_args(self, n, base_size, mode, antialias, hires_steps, strength, hires_seed, init_latent, hires_noise):
        h, w = self.latent_size
        hr = self._hires_struct(base_size, mode, antialias, hires_steps, strength, hires_seed)
        if hr.base_h <= 0 or hr.base_w <= 0 or hr.base_h % 8 or hr.base_w % 8:
            raise ValueError(f"base_size must be positive multiples of 8, got {base_size}")
        if not 0.0 < hr.strength <= 1.0:   # NaN fails too
            raise ValueError(f"strength must satisfy 0 < strength <= 1, got {strength}")
        x0 = None if init_latent is None else _f32(init_latent, (n, 4, hr.base_h, hr.base_w), "init_latent")
        noise = None if hires_noise is None else _f32(hires_noise, (n, 4, h, w), "hires_noise")
        return hr, x0, noise

    def sample_latent_hires(self, context, unconditional_context, unconditional_guidance_scale: float, n_steps: int, base_size, strength: float,
                            mode="bicubic", antialias: bool = False, hires_steps: int = 0, init_latent=None, seed: int = 0, hires_noise=None,
                            hires_seed: int = 0) -> np.ndarray:
        """Hires fix -> latent [n,4,h,w] at the context's current size: sample_latent at base_size = (base_h, base_w) (init_latent
        [n,4,base_h,base_w], or image i's stream seed + i), the latent resampled on the device (mode "nearest" / "bilinear" / "bicubic", torch's
        F.interpolate rule), then sample_latent_from over the last int(strength * L) of the hires_steps (0: n_steps) schedule with noise
        hires_noise [n,4,h,w] or image i's stream hires_seed + i."""
        context, uncond = self._check_ctx(context, unconditional_context)
        n, T, _ = context.shape
        h, w = self.latent_size
        hr, x0, noise = self._hires_args(n, base_size, mode, antialias, hires_steps, strength, hires_seed, init_latent, hires_noise)
        out = np.empty((n, 4, h, w), dtype=np.float32)
        check(self._lib.sdmi_hires_latent(self._ctx, _fp(context), n, T, _fp(uncond), uncond.shape[0], float(unconditional_guidance_scale), int(n_steps),
                                          None if x0 is None else _fp(x0), int(seed), C.byref(hr), None if noise is None else _fp(noise), _fp(out)))
        return out

    def sample_image_hires(self, context, unconditional_context, unconditional_guidance_scale: float, n_steps: int, base_size, strength: float,
                           mode="bicubic", antialias: bool = False, hires_steps: int = 0, init_latent=None, seed: int = 0, hires_noise=None,
                           hires_seed: int = 0) -> np.ndarray:
        """latent_to_image of sample_latent_hires -> uint8 [n, 8h, 8w, 3]."""
        context, uncond = self._check_ctx(context, unconditional_context)
        n, T, _ = context.shape
        h, w = self.latent_size
        hr, x0, noise = self._hires_args(n, base_size, mode, antialias, hires_steps, strength, hires_seed, init_latent, hires_noise)
        out = np.empty((n, 8 * h, 8 * w, 3), dtype=np.uint8)
        check(self._lib.sdmi_hires_image(self._ctx, _fp(context), n, T, _fp(uncond), uncond.shape[0], float(unconditional_guidance_scale), int(n_steps),
                                         None if x0 is None else _fp(x0), int(seed), C.byref(hr), None if noise is None else _fp(noise),
                                         out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    @staticmethod
    def _hires_struct(base_size, mode, antialias, hires_steps, strength, hires_seed) -> SdmiHires:
        hr = SdmiHires()
        hr.base_h, hr.base_w = int(base_size[0]), int(base_size[1])
        hr.mode = _resize_mode(mode)
        hr.antialias, hr.hires_steps, hr.strength, hr.hires_seed = (1 if antialias else 0), int(hires_steps or 0), float(strength), int(hires_seed)
        return hr

    def sample_latent_hires_dev(self, context_ptr: int, n: int, T: int, uncond_ptr: int, Tu: int, scale: float, n_steps: int, base_size,
                                strength: float, init_latent_ptr: int, hires_noise_ptr, latent_out_ptr: int, mode="bicubic", antialias: bool = False,
                                hires_steps: int = 0, hires_seed: int = 0) -> None:
        hr = self._hires_struct(base_size, mode, antialias, hires_steps, strength, hires_seed)
        check(self._lib.sdmi_hires_latent_dev(self._ctx, context_ptr, n, T, uncond_ptr, Tu, float(scale), int(n_steps), init_latent_ptr, C.byref(hr),
                                              hires_noise_ptr, latent_out_ptr))

    def sample_image_hires_dev(self, context_ptr: int, n: int, T: int, uncond_ptr: int, Tu: int, scale: float, n_steps: int, base_size,
                               strength: float, init_latent_ptr: int, hires_noise_ptr, rgb_out_ptr: int, mode="bicubic", antialias: bool = False,
                               hires_steps: int = 0, hires_seed: int = 0) -> None:
        hr = self._hires_struct(base_size, mode, antialias, hires_steps, strength, hires_seed)
        check(self._lib.sdmi_hires_image_dev(self._ctx, context_ptr, n, T, uncond_ptr, Tu, float(scale), int(n_steps), init_latent_ptr, C.byref(hr),
                                             hires_noise_ptr, rgb_out_ptr))

    def sample_latent_from_dev(self, context_ptr: int, n: int, T: int, uncond_ptr: int, Tu: int, scale: float, n_steps: int,
                               strength: float, z0_ptr: int, mask_ptr, noise_ptr, seed: int, latent_out_ptr: int) -> None:
        check(self._lib.sdmi_img2img_latent_dev(self._ctx, context_ptr, n, T, uncond_ptr, Tu, float(scale), int(n_steps), float(strength),
                                                z0_ptr, mask_ptr, noise_ptr, int(seed), latent_out_ptr))

    def sample_image_from_dev(self, context_ptr: int, n: int, T: int, uncond_ptr: int, Tu: int, scale: float, n_steps: int,
                              strength: float, init_rgb_ptr: int, mask_ptr, noise_ptr, seed: int, rgb_out_ptr: int) -> None:
        check(self._lib.sdmi_img2img_image_dev(self._ctx, context_ptr, n, T, uncond_ptr, Tu, float(scale), int(n_steps), float(strength),
                                               init_rgb_ptr, mask_ptr, noise_ptr, int(seed), rgb_out_ptr))

    # ---- device-pointer variants (zero copy; pointers are ints, e.g. torch .data_ptr()) ----
    def sample_image_dev(self, context_ptr: int, n: int, T: int, uncond_ptr: int, Tu: int, scale: float,
                         n_steps: int, init_latent_ptr: int, rgb_out_ptr: int) -> None:
        check(self._lib.sdmi_sample_image_dev(self._ctx, context_ptr, n, T, uncond_ptr, Tu, float(scale),
                                              int(n_steps), init_latent_ptr, rgb_out_ptr))

    def sample_latent_dev(self, context_ptr: int, n: int, T: int, uncond_ptr: int, Tu: int, scale: float,
                          n_steps: int, init_latent_ptr: int, latent_out_ptr: int) -> None:
        check(self._lib.sdmi_sample_latent_dev(self._ctx, context_ptr, n, T, uncond_ptr, Tu, float(scale),
                                               int(n_steps), init_latent_ptr, latent_out_ptr))

    def latent_to_image_dev(self, latent_ptr: int, n: int, rgb_out_ptr: int) -> None:
        check(self._lib.sdmi_latent_to_image_dev(self._ctx, latent_ptr, n, rgb_out_ptr))

    # ---- introspection ------------------------------------------------------------------
    def synchronize(self):
        check(self._lib.sdmi_synchronize(self._ctx))

    # options that change no kernel choice (measurement / dump switches): not listed as non-default settings
    _PASSIVE_OPTIONS = ("profile", "profile_reset", "record_shapes", "dump_shapes", "dump_choices", "dump_profile_tags", "dump_pool_fills", "roctx")

    def set_option(self, key: str, value) -> None:
        check(self._lib.sdmi_set_option(self._ctx, key.encode(), str(value).encode()))
        if hasattr(self, "applied_options") and key not in self._PASSIVE_OPTIONS:
            self.applied_options.append((key, str(value)))

    def last_call_stats(self) -> dict:
        ms, nk, fl = C.c_double(), C.c_int64(), C.c_double()
        check(self._lib.sdmi_last_call_stats(self._ctx, C.byref(ms), C.byref(nk), C.byref(fl)))
        return {"gpu_ms": ms.value, "kernels": nk.value, "flops": fl.value}

    PROFILE_CLASSES = ("conv_gemm", "splitk_reduce", "attention", "group_norm", "layer_norm", "conv_gemm_fp8", "conv_gemm_split", "split_rows", "other", "geglu")

    def profile_overhead_us(self) -> float:
        """what an empty HIP-event pair reads on the engine's stream (calibrated when profiling was switched on; subtracted from every sample)"""
        v = C.c_double()
        check(self._lib.sdmi_profile_overhead(self._ctx, C.byref(v)))
        return v.value * 1e3

    def profile_stats(self) -> dict:
        """Per-kernel-class HIP-event timings gathered while set_option("profile", 1)."""
        out = {}
        for i, name in enumerate(self.PROFILE_CLASSES):
            ms, n, fl, by = C.c_double(), C.c_int64(), C.c_double(), C.c_double()
            check(self._lib.sdmi_profile_stats(self._ctx, i, C.byref(ms), C.byref(n), C.byref(fl), C.byref(by)))
            out[name] = {"ms": ms.value, "launches": n.value, "flops": fl.value, "bytes": by.value}
        return out

    def bench_conv(self, n, cin, h, w, cout, k=3, stride=1, upsample2x=0, tile_cfg=-1, splitk=0, iters=10) -> float:
        ms = C.c_double()
        check(self._lib.sdmi_bench_conv(self._ctx, n, cin, h, w, cout, k, stride, upsample2x, tile_cfg, splitk, iters,
                                        C.byref(ms)))
        return ms.value

    def set_prediction(self, kind: str = "eps") -> None:
        """What the loaded UNet predicts: "eps" (the default; SD v1, SD 2.x 512-base) or "v" (SD 2.x 768-v, 2.1-768).  Sticky; applies to every sampling entry
        point and sampler (sdmi_set_prediction).  The checkpoint does not say which: the caller chooses."""
        check(self._lib.sdmi_set_prediction(self._ctx, _prediction(kind)))

    def set_guidance_rescale(self, phi: float = 0.0) -> None:
        """CFG rescale (sdmi_set_guidance_rescale): the guided model output of every evaluation is multiplied per image by
        phi * std(cond) / std(guided) + (1 - phi).  phi in [0, 1]; 0 (the default) is off and runs what ran before; sticky.  0.7 is the value v-prediction
        models trained with zero terminal SNR are usually sampled at."""
        check(self._lib.sdmi_set_guidance_rescale(self._ctx, float(phi)))

    def set_freeu(self, b1=1.0, b2=1.0, s1=1.0, s2=1.0, version: int = 1, start: float = 0.0, end: float = 1.0) -> None:
        """FreeU (sdmi_set_freeu), sticky: in front of the output blocks whose backbone input has 4 x model_channels channels (blocks 0..6)
        its first half is scaled by b1 and the low frequencies of the skip by s1; b2 / s2 where it has 2 x model_channels (blocks 7..9).  version 2 is ComfyUI's
        FreeU_V2 (the backbone factor follows the normalised channel mean).  start / end: the step window of a sampling call, as a control's.  set_freeu(None)
        clears; all four parameters at 1 run what ran before.  The paper's values: SD 1.4 (1.2, 1.4, 0.9, 0.2), SD 2.1 (1.1, 1.2, 0.9, 0.2)."""
        if b1 is None:
            check(self._lib.sdmi_set_freeu(self._ctx, 0, 1.0, 1.0, 1.0, 1.0, 0.0, 1.0))
            return
        check(self._lib.sdmi_set_freeu(self._ctx, int(version), float(b1), float(b2), float(s1), float(s2), float(start), float(end)))

    def get_freeu(self):
        """The FreeU state in force (sdmi_get_freeu): None when off, else {"version", "b1", "b2", "s1", "s2", "start", "end"}."""
        v = C.c_int32()
        p = [C.c_float() for _ in range(4)]
        st, en = C.c_double(), C.c_double()
        check(self._lib.sdmi_get_freeu(self._ctx, C.byref(v), *(C.byref(q) for q in p), C.byref(st), C.byref(en)))
        if not v.value:
            return None
        return {"version": int(v.value), "b1": p[0].value, "b2": p[1].value, "s1": p[2].value, "s2": p[3].value, "start": st.value, "end": en.value}

    def op_freeu(self, x, cx: int, version: int, b: float, s: float, planes: bool = False):
        """tests (sdmi_op_freeu): x [n, c, h, w] = cat([h, hs]) with cx backbone channels, through the model's FreeU launches in the engine's own layout -> y.
        planes = True: (y, what the bf16 planes of the buffer hold, or None where the buffer had none)."""
        x = _f32(x)
        if x.ndim != 4:
            raise ValueError(f"op_freeu: x must be [n, c, h, w], got {x.shape}")
        n, c, h, w = x.shape
        y = np.empty_like(x)
        y3 = np.empty_like(x) if planes else None
        r = self._lib.sdmi_op_freeu(self._ctx, _fp(x), n, c, h, w, int(cx), int(version), float(b), float(s), _fp(y), None if y3 is None else _fp(y3))
        if r < 0:
            check(r)
        return (y, y3 if r == 1 else None) if planes else y

    def set_zero_snr(self, on: bool = True) -> None:
        """Sample on the loaded schedule rescaled to zero terminal SNR (sdmi_set_zero_snr; rescale_zero_snr); False restores the loaded table bit for bit.
        Sticky, before or after the weights.  Needs set_prediction("v"); sigma-schedule samplers are refused on such a table."""
        check(self._lib.sdmi_set_zero_snr(self._ctx, 1 if on else 0))

    def schedule(self) -> np.ndarray:
        """The alphas_cumprod table in force (sdmi_schedule): the loaded one, or its zero-terminal-SNR rescale."""
        count = C.c_int32()
        check(self._lib.sdmi_schedule(self._ctx, None, 0, C.byref(count)))
        out = np.empty(count.value, dtype=np.float32)
        if count.value:
            check(self._lib.sdmi_schedule(self._ctx, _fp(out), out.size, C.byref(count)))
        return out

    ATTN_KERNELS = ("unfused", "flash", "split", "bf16")   # sdmi_attn_plan.kernel: GEMM path, k_attn.hip, k_attn_split.hip, k_attn_bf16.hip

    def attention_plan(self, n, n_head, nq, nk, d_head, has_mask=False) -> dict:
        """What this context would run for qkv_attention of the shape under its current options (sdmi_attention_plan; host only, no launch):
        {"kernel": one of ATTN_KERNELS, "waves", "q_rows", "kv_tile", "kv_splits"}."""
        p = SdmiAttnPlan()
        check(self._lib.sdmi_attention_plan(self._ctx, int(n), int(n_head), int(nq), int(nk), int(d_head), int(bool(has_mask)), C.byref(p)))
        return {"kernel": self.ATTN_KERNELS[p.kernel], "waves": int(p.waves), "q_rows": int(p.q_rows), "kv_tile": int(p.kv_tile), "kv_splits": int(p.kv_splits)}

    def bench_attention(self, n, nq, nk, n_state, n_head, iters=10) -> float:
        ms = C.c_double()
        check(self._lib.sdmi_bench_attention(self._ctx, n, nq, nk, n_state, n_head, iters, C.byref(ms)))
        return ms.value

    # ---- operator-level entry points (parity tests) ----------------------------------------
    def op_unpack_tensor(self, raw, dtype: str, transform: int = 0) -> np.ndarray:
        """The checkpoint conversion kernel on its own (sdmi_op_unpack_tensor): raw = float32, float16, or uint16 holding bf16 bits;
        dtype "F32" | "F16" | "BF16"; transform 0 copy, 1 2-D transpose, 2 [cout,cin,kh,kw] (cin < 32) padded to the next multiple of 4 input channels."""
        code = {"F32": 0, "F16": 1, "BF16": 2}[dtype]
        raw = np.ascontiguousarray(raw, dtype={0: np.float32, 1: np.float16, 2: np.uint16}[code])
        shape = raw.shape
        if transform == 1:
            out_shape = shape[::-1]
        elif transform == 2:
            out_shape = (shape[0], (shape[1] + 3) // 4 * 4) + tuple(shape[2:])
        else:
            out_shape = shape
        out = np.empty(out_shape, np.float32)
        dims = (C.c_int64 * raw.ndim)(*shape)
        check(self._lib.sdmi_op_unpack_tensor(self._ctx, raw.ctypes.data_as(C.c_void_p), code, raw.ndim, dims, int(transform), _fp(out)))
        return out

    def op_sampler_step(self, eps, latent, scale: float, row, rescale: float = 0.0, depth: int = 0, q_hist=None, noise_key: int = 0, noise_key2: int = 0,
                        mask=None, z0=None, e0=None, blend_prev: float = 0.0, blend_dir: float = 0.0):
        """One update launch of the sampler choice on its own (sdmi_op_sampler_step): eps [2n,4,h,w] (unconditional half first), latent [n,4,h,w],
        row = (cx, ce, h1, h2, h3, cz, cz2, qx, qe), q_hist [n_hist,n,4,h,w] (newest first).  Returns (latent_out, q_out); q_out is None at depth 0.
        rescale = 0 launches the elementwise kernels, otherwise the CFG-rescale kernel."""
        latent = _f32(latent)
        if latent.ndim != 4 or latent.shape[1] != 4:
            raise ValueError(f"op_sampler_step: latent must be [n,4,h,w], got {latent.shape}")
        n, _, h, w = latent.shape
        eps = _f32(eps, (2 * n, 4, h, w), "eps")
        row = np.ascontiguousarray(row, dtype=np.float64)
        if row.shape != (9,):
            raise ValueError(f"op_sampler_step: row must hold 9 coefficients, got {row.shape}")
        n_hist = 0
        if q_hist is not None:
            q_hist = _f32(q_hist)
            n_hist = q_hist.shape[0]
            q_hist = _f32(q_hist, (n_hist, n, 4, h, w), "q_hist")
        if mask is not None:
            mask, z0, e0 = _f32(mask, (n, h, w), "mask"), _f32(z0, (n, 4, h, w), "z0"), _f32(e0, (n, 4, h, w), "e0")
        out = np.empty_like(latent)
        q_out = np.empty_like(latent) if depth else None
        opt = lambda a: None if a is None else _fp(a)
        check(self._lib.sdmi_op_sampler_step(self._ctx, _fp(eps), _fp(latent), n, h, w, float(scale), float(rescale), row.ctypes.data_as(C.POINTER(C.c_double)),
                                             int(depth), n_hist, opt(q_hist) if n_hist else None, int(noise_key) & 0xFFFFFFFFFFFFFFFF,
                                             int(noise_key2) & 0xFFFFFFFFFFFFFFFF, opt(mask), opt(z0), opt(e0), float(blend_prev), float(blend_dir), _fp(out), opt(q_out)))
        return out, q_out

    def op_resize(self, x, out_size, mode="bicubic", antialias: bool = False):
        """The resampler of the hires fix on its own (sdmi_op_resize): x [n,4,h,w] -> [n,4,out_h,out_w]."""
        x = _f32(x)
        if x.ndim != 4 or x.shape[1] != 4:
            raise ValueError(f"op_resize: x must be [n,4,h,w], got {x.shape}")
        n, _, h, w = x.shape
        oh, ow = (int(v) for v in out_size)
        if oh <= 0 or ow <= 0:
            raise ValueError(f"op_resize: out_size must be positive, got {out_size}")
        m = _resize_mode(mode)
        out = np.empty((n, 4, oh, ow), dtype=np.float32)
        check(self._lib.sdmi_op_resize(self._ctx, _fp(x), n, h, w, oh, ow, m, 1 if antialias else 0, _fp(out)))
        return out

    def op_group_norm(self, x, gamma, beta, n_group=32, eps=1e-5, silu=False):
        x = _f32(x)
        n, c, h, w = x.shape
        out = np.empty_like(x)
        check(self._lib.sdmi_op_group_norm(self._ctx, _fp(x), _fp(_f32(gamma, (c,))), _fp(_f32(beta, (c,))), n, c, h, w,
                                           n_group, eps, int(silu), _fp(out)))
        return out

    def op_group_norm_fp8(self, x, gamma, beta, n_group=32, eps=1e-5, silu=False):
        """GroupNorm(+SiLU) with MXFP8 output (precision = 2), returned dequantised."""
        x = _f32(x)
        n, c, h, w = x.shape
        out = np.empty_like(x)
        check(self._lib.sdmi_op_group_norm_fp8(self._ctx, _fp(x), _fp(_f32(gamma, (c,))), _fp(_f32(beta, (c,))), n, c, h, w,
                                               n_group, eps, int(silu), _fp(out)))
        return out

    def op_layer_norm(self, x, gamma, beta, eps=1e-5):
        x = _f32(x)
        c = x.shape[-1]
        rows = x.size // c
        out = np.empty_like(x)
        check(self._lib.sdmi_op_layer_norm(self._ctx, _fp(x), _fp(_f32(gamma, (c,))), _fp(_f32(beta, (c,))), rows, c,
                                           eps, _fp(out)))
        return out

    def op_conv2d(self, x, weight, bias=None, stride=1, pad=None, upsample2x=False):
        x = _f32(x)
        weight = _f32(weight)
        n, cin, h, w = x.shape
        cout, cin2, k, k2 = weight.shape
        if cin2 != cin or k != k2:
            raise ValueError("conv2d: weight shape does not match input")
        if pad is None:
            pad = 1 if k == 3 else 0
        ups = 1 if upsample2x else 0
        ho = ((h << ups) + 2 * pad - k) // stride + 1
        wo = ((w << ups) + 2 * pad - k) // stride + 1
        out = np.empty((n, cout, ho, wo), dtype=np.float32)
        b = None if bias is None else _f32(bias, (cout,))
        check(self._lib.sdmi_op_conv2d(self._ctx, _fp(x), _fp(weight), None if b is None else _fp(b), n, cin, h, w, cout,
                                       k, stride, pad, ups, _fp(out)))
        return out

    def op_linear(self, x, weight, bias=None):
        x = _f32(x)
        weight = _f32(weight)
        cin, cout = weight.shape
        rows = x.size // cin
        out = np.empty(x.shape[:-1] + (cout,), dtype=np.float32)
        b = None if bias is None else _f32(bias, (cout,))
        check(self._lib.sdmi_op_linear(self._ctx, _fp(x), _fp(weight), None if b is None else _fp(b), rows, cin, cout,
                                       _fp(out)))
        return out

    def op_conv2d_epilogue(self, x, weight, bias=None, temb=None, resid=None, stride=1, upsample2x=False, temb_stride=None, resid_ld=0):
        """op_conv2d + temb[sample] + resid through the GEMM epilogue (tests).  temb: [cout] (one row for the batch) or [n, cout]; resid: the
        output's shape.  temb_stride (default: 0 for one row, cout per sample) and resid_ld (0: cout) are the strides the engine keeps them at."""
        x = _f32(x)
        weight = _f32(weight)
        n, cin, h, w = x.shape
        cout, cin2, k, k2 = weight.shape
        if cin2 != cin or k != k2:
            raise ValueError("conv2d: weight shape does not match input")
        pad = 1 if k == 3 else 0
        ups = 1 if upsample2x else 0
        ho = ((h << ups) + 2 * pad - k) // stride + 1
        wo = ((w << ups) + 2 * pad - k) // stride + 1
        out = np.empty((n, cout, ho, wo), dtype=np.float32)
        b = None if bias is None else _f32(bias, (cout,))
        t = None if temb is None else _f32(temb)
        if t is not None:
            if t.shape not in ((cout,), (n, cout)):
                raise ValueError("conv2d_epilogue: temb must be [cout] or [n, cout]")
            if temb_stride is None:
                temb_stride = 0 if t.ndim == 1 else cout
            if (temb_stride == 0) != (t.ndim == 1):
                raise ValueError("conv2d_epilogue: temb_stride 0 means one row for the batch")
        r = None if resid is None else _f32(resid, (n, cout, ho, wo))
        check(self._lib.sdmi_op_conv2d_epilogue(self._ctx, _fp(x), _fp(weight), None if b is None else _fp(b), None if t is None else _fp(t),
                                                temb_stride or 0, None if r is None else _fp(r), resid_ld, n, cin, h, w, cout, k, stride, pad, ups,
                                                _fp(out)))
        return out

    def op_conv2d_pair(self, x, h, w_skip, b_skip, w_out, b_out, planes=False):
        """conv3x3(h, w_out) + b_out + conv1x1(x, w_skip) + b_skip, the tail of a ResBlock with a shortcut (tests; precision 0).  Option skip_slices=1: one
        split-K launch carrying the shortcut on extra K slices; 0: two launches.  planes=True also returns the result the launch wrote as bf16 planes, joined."""
        x = _f32(x)
        h = _f32(h)
        n, cin_x, hh, ww = x.shape
        cout = h.shape[1]
        if h.shape != (n, cout, hh, ww):
            raise ValueError("conv2d_pair: x and h must cover the same pixels")
        ws = _f32(w_skip, (cout, cin_x, 1, 1))
        wo = _f32(w_out, (cout, cout, 3, 3))
        bs = None if b_skip is None else _f32(b_skip, (cout,))
        bo = None if b_out is None else _f32(b_out, (cout,))
        out = np.empty((n, cout, hh, ww), dtype=np.float32)
        out3 = np.empty_like(out) if planes else None
        check(self._lib.sdmi_op_conv2d_pair(self._ctx, _fp(x), _fp(h), _fp(ws), None if bs is None else _fp(bs), _fp(wo), None if bo is None else _fp(bo),
                                            n, cin_x, cout, hh, ww, _fp(out), None if out3 is None else _fp(out3)))
        return (out, out3) if planes else out

    def op_linear_pair(self, u, h, w_main, b_main, w_aux, b_aux, resid=None, resid_ld=0, out_ld=0, out="f32"):
        """u @ w_main + b_main + h @ w_aux + b_aux + resid, the tail of a transformer block with proj_out folded into the MLP's output Linear (tests; precision 0).
        Option proj_out_fold=1: one split-K launch carrying h @ w_aux on extra K slices; 0: two launches.  resid_ld / out_ld (0: cout): the row strides the engine
        keeps the residual and the result at.  out: "f32", "planes" (the bf16-plane output, joined) or "both" (a pair)."""
        u = _f32(u)
        h = _f32(h)
        rows, k_main = u.shape
        k_aux = h.shape[1]
        if h.shape[0] != rows:
            raise ValueError("linear_pair: u and h must have the same rows")
        wm = _f32(w_main)
        cout = wm.shape[1]
        wm = _f32(wm, (k_main, cout))
        wa = _f32(w_aux, (k_aux, cout))
        bm = None if b_main is None else _f32(b_main, (cout,))
        ba = None if b_aux is None else _f32(b_aux, (cout,))
        r = None if resid is None else _f32(resid, (rows, cout))
        if out not in ("f32", "planes", "both"):
            raise ValueError("linear_pair: out is 'f32', 'planes' or 'both'")
        o = np.empty((rows, cout), dtype=np.float32) if out != "planes" else None
        o3 = np.empty((rows, cout), dtype=np.float32) if out != "f32" else None
        check(self._lib.sdmi_op_linear_pair(self._ctx, _fp(u), _fp(h), _fp(wm), None if bm is None else _fp(bm), _fp(wa), None if ba is None else _fp(ba),
                                            None if r is None else _fp(r), resid_ld, rows, k_main, k_aux, cout, out_ld, None if o is None else _fp(o),
                                            None if o3 is None else _fp(o3)))
        return o if out == "f32" else o3 if out == "planes" else (o, o3)

    def op_linear_fold(self, w_lin, b_lin, w_proj):
        """(wf [cout, k_main], bf [cout]) = (w_proj @ w_lin.T, w_proj @ b_lin) through the loader's fold kernel (tests): w_lin [k_main, cmid] a Linear weight in the
        reference layout, b_lin [cmid] or None, w_proj [cout, cmid] a 1x1 convolution."""
        wl = _f32(w_lin)
        k_main, cmid = wl.shape
        wp = _f32(w_proj)
        cout = wp.shape[0]
        wp = _f32(wp, (cout, cmid))
        bl = None if b_lin is None else _f32(b_lin, (cmid,))
        wf = np.empty((cout, k_main), dtype=np.float32)
        bf = np.empty((cout,), dtype=np.float32)
        check(self._lib.sdmi_op_linear_fold(self._ctx, _fp(wl), None if bl is None else _fp(bl), _fp(wp), k_main, cmid, cout, _fp(wf), _fp(bf)))
        return wf, bf

    def op_linear_epilogue(self, x, weight, bias=None, resid=None, resid_ld=0):
        """op_linear + resid [rows, cout] through the GEMM epilogue (tests); resid_ld (0: cout) is the row stride the engine keeps it at."""
        x = _f32(x)
        weight = _f32(weight)
        cin, cout = weight.shape
        rows = x.size // cin
        out = np.empty(x.shape[:-1] + (cout,), dtype=np.float32)
        b = None if bias is None else _f32(bias, (cout,))
        r = None if resid is None else _f32(resid, out.shape)
        check(self._lib.sdmi_op_linear_epilogue(self._ctx, _fp(x), _fp(weight), None if b is None else _fp(b), None if r is None else _fp(r),
                                                resid_ld, rows, cin, cout, _fp(out)))
        return out

    # ---- the same operators on channel-slice views of wider buffers, as the UNet realises Tensor::cat (tests) ----
    def _view_call(self, parent, fn):
        """fn(); a refused call raises SdmiError carrying what the device left of the parent (.parent)"""
        try:
            fn()
        except SdmiError as e:
            e.parent = parent
            raise

    def op_conv2d_view(self, x, weight, bias=None, temb=None, resid=None, stride=1, upsample2x=False, temb_stride=None, resid_ld=0, *, parent, out_off,
                       in_ld=None, in_off=0, in_fill=float("nan"), in_planes=0, out_planes=0):
        """op_conv2d_epilogue with x read from columns [in_off, in_off + cin) of a buffer in_ld wide (the rest in_fill) and the result written to columns
        [out_off, out_off + cout) of `parent` [n*ho*wo, out_ld] (NHWC rows, prefilled by the caller; not modified).  Returns the whole parent as the
        engine left it; with out_planes = 3 (precision 0: fp32 and bf16-plane copies) the pair (fp32 copy, joined planes)."""
        x = _f32(x)
        weight = _f32(weight)
        n, cin, h, w = x.shape
        cout, cin2, k, k2 = weight.shape
        if cin2 != cin or k != k2:
            raise ValueError("conv2d: weight shape does not match input")
        pad = 1 if k == 3 else 0
        ups = 1 if upsample2x else 0
        ho = ((h << ups) + 2 * pad - k) // stride + 1
        wo = ((w << ups) + 2 * pad - k) // stride + 1
        out = np.array(parent, dtype=np.float32, order="C", copy=True)
        if out.ndim != 2 or out.shape[0] != n * ho * wo:
            raise ValueError(f"conv2d_view: parent must be [{n * ho * wo}, out_ld], got {out.shape}")
        b = None if bias is None else _f32(bias, (cout,))
        t = None if temb is None else _f32(temb)
        if t is not None:
            if t.shape not in ((cout,), (n, cout)):
                raise ValueError("conv2d_view: temb must be [cout] or [n, cout]")
            if temb_stride is None:
                temb_stride = 0 if t.ndim == 1 else cout
        r = None if resid is None else _f32(resid, (n, cout, ho, wo))
        v = SdmiOpView(cin if in_ld is None else in_ld, in_off, out.shape[1], out_off, in_fill, in_planes, out_planes)
        out3 = np.empty_like(out) if out_planes == 3 else None
        self._view_call(out, lambda: check(self._lib.sdmi_op_conv2d_view(
            self._ctx, _fp(x), _fp(weight), None if b is None else _fp(b), None if t is None else _fp(t), temb_stride or 0,
            None if r is None else _fp(r), resid_ld, n, cin, h, w, cout, k, stride, pad, ups, C.byref(v), _fp(out), None if out3 is None else _fp(out3))))
        return out if out3 is None else (out, out3)

    def op_linear_view(self, x, weight, bias=None, resid=None, resid_ld=0, *, parent, out_off):
        """op_linear_epilogue writing columns [out_off, out_off + cout) of `parent` [rows, out_ld]; returns the whole parent."""
        x = _f32(x)
        weight = _f32(weight)
        cin, cout = weight.shape
        rows = x.size // cin
        out = np.array(parent, dtype=np.float32, order="C", copy=True)
        if out.ndim != 2 or out.shape[0] != rows:
            raise ValueError(f"linear_view: parent must be [{rows}, out_ld], got {out.shape}")
        b = None if bias is None else _f32(bias, (cout,))
        r = None if resid is None else _f32(resid, (rows, cout))
        v = SdmiOpView(cin, 0, out.shape[1], out_off, float("nan"), 0, 0)
        self._view_call(out, lambda: check(self._lib.sdmi_op_linear_view(self._ctx, _fp(x), _fp(weight), None if b is None else _fp(b), None if r is None else _fp(r),
                                                                         resid_ld, rows, cin, cout, C.byref(v), _fp(out))))
        return out

    def op_group_norm_view(self, x, gamma, beta, eps=1e-5, silu=False, *, in_ld, in_off, in_fill=float("nan"), in_planes=0, form=0):
        """op_group_norm (32 groups) with x read from columns [in_off, in_off + c) of a buffer in_ld wide whose other columns hold in_fill.
        form 0: the context's GroupNorm, 1: the plane-writing form (precision 0), 2: MXFP8 output, dequantised (precision 2)."""
        x = _f32(x)
        n, c, h, w = x.shape
        out = np.empty_like(x)
        v = SdmiOpView(in_ld, in_off, c, 0, in_fill, in_planes, 0)
        check(self._lib.sdmi_op_group_norm_view(self._ctx, _fp(x), _fp(_f32(gamma, (c,))), _fp(_f32(beta, (c,))), n, c, h, w, 32, eps, int(silu), C.byref(v),
                                                form, _fp(out)))
        return out

    def op_cat_chain(self, x, w_x, b_x, w_skip, b_skip, gamma, beta, eps=1e-5, silu=True, dense=False):
        """GroupNorm(cat(conv3x3(x, w_x), conv3x3(x, w_skip))): the convolutions write the two channel slices of one buffer (dense=False, the UNet's
        way) or dense tensors joined by a copy (dense=True)."""
        x = _f32(x)
        n, cin, h, w = x.shape
        w_x, w_skip = _f32(w_x), _f32(w_skip)
        cx, cskip = w_x.shape[0], w_skip.shape[0]
        if w_x.shape != (cx, cin, 3, 3) or w_skip.shape != (cskip, cin, 3, 3):
            raise ValueError("cat_chain: weights must be [cout, cin, 3, 3]")
        out = np.empty((n, cx + cskip, h, w), dtype=np.float32)
        check(self._lib.sdmi_op_cat_chain(self._ctx, _fp(x), _fp(w_x), _fp(_f32(b_x, (cx,))), _fp(w_skip), _fp(_f32(b_skip, (cskip,))),
                                          _fp(_f32(gamma, (cx + cskip,))), _fp(_f32(beta, (cx + cskip,))), n, cin, h, w, cx, cskip, eps, int(silu), int(dense),
                                          _fp(out)))
        return out

    def op_geglu_forward(self, x, weight_in_out, bias, hidden):
        """GEGLU::forward (unet/mod.rs:579-591): x [rows, cin] -> [rows, hidden]."""
        x = _f32(x)
        rows, cin = x.shape
        w = _f32(weight_in_out, (cin, 2 * hidden))
        out = np.empty((rows, hidden), dtype=np.float32)
        b = None if bias is None else _f32(bias, (2 * hidden,))
        check(self._lib.sdmi_op_geglu_forward(self._ctx, _fp(x), _fp(w), None if b is None else _fp(b), rows, cin, hidden, _fp(out)))
        return out

    def op_geglu(self, proj):
        proj = _f32(proj)
        hidden = proj.shape[-1] // 2
        rows = proj.size // (2 * hidden)
        out = np.empty(proj.shape[:-1] + (hidden,), dtype=np.float32)
        check(self._lib.sdmi_op_geglu(self._ctx, _fp(proj), rows, hidden, _fp(out)))
        return out

    def op_timestep_embedding(self, t: int, dim: int):
        out = np.empty((1, dim), dtype=np.float32)
        check(self._lib.sdmi_op_timestep_embedding(self._ctx, int(t), dim, _fp(out)))
        return out

    def op_timestep_embedding_f(self, t: float, dim: int):
        """timestep_embedding at a fractional t (the k-samplers' evaluation times); an integer t gives op_timestep_embedding's bits"""
        out = np.empty((1, dim), dtype=np.float32)
        check(self._lib.sdmi_op_timestep_embedding_f(self._ctx, float(t), dim, _fp(out)))
        return out

    def qkv_attention(self, q, k, v, mask, n_head: int):
        """attention.rs:5-45: q [n,nq,c], k,v [n,nk,c], mask [>=nq, >=nk] or None.

        The mask is additive, in natural-log units (added to the scores before the softmax), and shared by every sample and head; its row
        stride goes down as mask_ld, so an over-sized mask is passed as it is.  -inf is allowed; a row without a live key comes back NaN,
        as in the reference.  The library reads nq rows of mask_ld floats and cannot see where the array ends, so a mask that is not
        two-dimensional or has fewer than nq rows is refused here (SdmiError, SDMI_ERR_INVALID); one narrower than nk is refused by the library."""
        q, k, v = _f32(q), _f32(k), _f32(v)
        n, nq, c = q.shape
        nk = k.shape[1]
        if k.shape != (n, nk, c) or v.shape != (n, nk, c):
            raise ValueError("qkv_attention: q/k/v shapes disagree")
        out = np.empty_like(q)
        m = None if mask is None else _f32(mask)
        if m is not None and (m.ndim != 2 or m.shape[0] < nq):
            raise SdmiError(-1, f"qkv_attention: mask must be [>= nq = {nq}, >= nk = {nk}], got {m.shape}")
        check(self._lib.sdmi_qkv_attention(self._ctx, _fp(q), _fp(k), _fp(v), None if m is None else _fp(m),
                                           0 if m is None else m.shape[1], n, nq, nk, c, n_head, _fp(out)))
        return out

    def qkv_attention_ragged(self, q, k, v, kv_len, n_head: int):
        """qkv_attention without a mask where row b of the batch attends to its first kv_len[b] keys only (the CFG batch's cross
        attention; tests): q [n,nq,c], k,v [n,nk,c], kv_len [n] or None (refused by the library, as are entries outside 1 .. nk)."""
        q, k, v = _f32(q), _f32(k), _f32(v)
        n, nq, c = q.shape
        nk = k.shape[1]
        if k.shape != (n, nk, c) or v.shape != (n, nk, c):
            raise ValueError("qkv_attention_ragged: q/k/v shapes disagree")
        kl = None
        if kv_len is not None:
            kl = np.ascontiguousarray(kv_len, dtype=np.int32)
            if kl.shape != (n,):
                raise ValueError(f"qkv_attention_ragged: kv_len must have shape ({n},), got {kl.shape}")
        out = np.empty_like(q)
        check(self._lib.sdmi_op_qkv_attention_ragged(self._ctx, _fp(q), _fp(k), _fp(v), None if kl is None else kl.ctypes.data_as(C.POINTER(C.c_int32)),
                                                     n, nq, nk, c, n_head, _fp(out)))
        return out

    def op_qkv_attention_view(self, q, k, v, mask, n_head: int, kv_len=None, *, q_view, k_view, v_view, packed, parent, out_off, out_planes=0, in_fill=float("nan")):
        """qkv_attention (with kv_len: qkv_attention_ragged) the way the model calls it (sdmi_op_qkv_attention_view; tests): q [n,nq,c], k,v [n,nk,c] are
        scattered into parents [n][rows][ld] full of in_fill at columns [off, off + c) -- q_view / k_view / v_view = (ld, off, rows); packed: the three are
        slices of one parent -- and the result is written to rows [0, nq), columns [out_off, out_off + c) of every sample of `parent` [n, out_rows, out_ld]
        (prefilled by the caller; not modified).  Returns the whole parent as the engine left it.  out_planes = 1 (a dense parent): through the kernels'
        plane-writing epilogue."""
        q, k, v = _f32(q), _f32(k), _f32(v)
        n, nq, c = q.shape
        nk = k.shape[1]
        if k.shape != (n, nk, c) or v.shape != (n, nk, c):
            raise ValueError("qkv_attention_view: q/k/v shapes disagree")
        m = None if mask is None else _f32(mask)
        if m is not None and (m.ndim != 2 or m.shape[0] < nq):
            raise SdmiError(-1, f"qkv_attention_view: mask must be [>= nq = {nq}, >= nk = {nk}], got {m.shape}")
        kl = None
        if kv_len is not None:
            kl = np.ascontiguousarray(kv_len, dtype=np.int32)
            if kl.shape != (n,):
                raise ValueError(f"qkv_attention_view: kv_len must have shape ({n},), got {kl.shape}")
        out = np.array(parent, dtype=np.float32, order="C", copy=True)
        if out.ndim != 3 or out.shape[0] != n:
            raise ValueError(f"qkv_attention_view: parent must be [{n}, out_rows, out_ld], got {out.shape}")
        view = SdmiAttnView(*q_view, *k_view, *v_view, int(bool(packed)), in_fill, out.shape[2], out_off, out.shape[1], out_planes)
        self._view_call(out, lambda: check(self._lib.sdmi_op_qkv_attention_view(
            self._ctx, _fp(q), _fp(k), _fp(v), None if m is None else _fp(m), 0 if m is None else m.shape[1],
            None if kl is None else kl.ctypes.data_as(C.POINTER(C.c_int32)), n, nq, nk, c, n_head, view, _fp(out))))
        return out


def _make_cfg(lib, config: ModelConfig, device: int = 0) -> SdmiConfig:
    cfg = SdmiConfig()
    check(lib.sdmi_default_config(C.byref(cfg)))
    cfg.device = device
    for f in ("model_channels", "n_head", "ctx_dim", "latent_h", "latent_w", "vae_ch", "precision", "clip_layers", "clip_heads",
              "clip_vocab", "clip_ctx", "unet_in_ch", "control_hint_ch", "variant"):
        setattr(cfg, f, getattr(config, f))
    return cfg


class MultiStableDiffusion:
    """`StableDiffusion::sample_image` for n images of one prompt, sharded over the GPUs of one node behind the C ABI
    (sdmi_create_multi / sdmi_sample_image_sharded): one process, one engine + host thread per device,
    ONE RCCL broadcast of the packed prompt embedding per call, contiguous image ranges, noise keyed by the global
    image index."""

    def __init__(self, config: ModelConfig = ModelConfig(), devices=(0,)):
        self._lib = load_library()
        self.config = config
        cfg = _make_cfg(self._lib, config)
        devs = (C.c_int32 * len(devices))(*devices)
        self._m = C.c_void_p()
        check(self._lib.sdmi_create_multi(C.byref(self._m), C.byref(cfg), devs, len(devices)))
        self.devices = tuple(devices)
        self._lora_views = []      # device views that carry a live adapter (lora_attach): invalidated by close()

    def close(self):
        if getattr(self, "_m", None) is not None and self._m.value:
            for v in self._lora_views:   # their adapters die with the device contexts
                v._ctx = C.c_void_p()
            self._lib.sdmi_destroy_multi(self._m)
            self._m = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def device_view(self, index: int) -> StableDiffusion:
        """The single-device surface of device `index` (weights, options); owned by this object."""
        ctx = self._lib.sdmi_multi_ctx(self._m, index)
        if not ctx:
            check(-1)
        return StableDiffusion(self.config, _borrowed_ctx=ctx)

    def load_weights(self, provider, clip: bool = False, vae_encoder: bool = False) -> None:
        for i in range(len(self.devices)):
            self.device_view(i).load_weights(provider, clip=clip, vae_encoder=vae_encoder)

    def load_weights_path(self, kind: str, path) -> None:
        """kind = "dump" (npy tree) | "burn" (.mpk record) | "safetensors" (CompVis checkpoint), on every device in parallel."""
        check(self._lib.sdmi_multi_load_weights(self._m, kind.encode(), str(path).encode()))

    def sample_image(self, context, unconditional_context, unconditional_guidance_scale: float, n_steps: int, n_images: int,
                     init_latents=None, seed: int = 0) -> np.ndarray:
        cd = self.config.ctx_dim
        h, w = self.latent_size
        context = _f32(context, name="context")
        if context.ndim == 3 and context.shape[0] == 1:
            context = context[0]
        if context.ndim != 2 or context.shape[1] != cd:
            raise ValueError(f"context must be [T, {cd}] (one prompt), got {context.shape}")
        uncond = _f32(unconditional_context, name="unconditional_context")
        if uncond.ndim != 2 or uncond.shape[1] != cd:
            raise ValueError(f"unconditional_context must be [Tu, {cd}], got {uncond.shape}")
        x0 = None if init_latents is None else _f32(init_latents, (n_images, 4, h, w), "init_latents")
        out = np.empty((n_images, 8 * h, 8 * w, 3), dtype=np.uint8)
        check(self._lib.sdmi_sample_image_sharded(self._m, _fp(context), context.shape[0], _fp(uncond), uncond.shape[0],
                                                  float(unconditional_guidance_scale), int(n_steps), int(n_images),
                                                  None if x0 is None else _fp(x0), int(seed),
                                                  out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    def set_sampler(self, kind="ddim", eta: float = 0.0, noise_seed: int = 0) -> None:
        """StableDiffusion.set_sampler on every device (sdmi_multi_set_sampler); each shard's image_base is the global index of its
        first image, so the step noise does not depend on the device count.  None restores the default."""
        if kind is None:
            check(self._lib.sdmi_multi_set_sampler(self._m, None))
            return
        s = _sampler_struct(kind, eta, noise_seed, 0)
        check(self._lib.sdmi_multi_set_sampler(self._m, C.byref(s)))

    def set_prediction(self, kind: str = "eps") -> None:
        """StableDiffusion.set_prediction on every device."""
        for i in range(len(self.devices)):
            self.device_view(i).set_prediction(kind)

    def set_guidance_rescale(self, phi: float = 0.0) -> None:
        """StableDiffusion.set_guidance_rescale on every device (sdmi_multi_set_guidance_rescale): the statistic is per image, sharding changes nothing."""
        check(self._lib.sdmi_multi_set_guidance_rescale(self._m, float(phi)))

    def set_zero_snr(self, on: bool = True) -> None:
        """StableDiffusion.set_zero_snr on every device (sdmi_multi_set_zero_snr)."""
        check(self._lib.sdmi_multi_set_zero_snr(self._m, 1 if on else 0))

    def set_freeu(self, b1=1.0, b2=1.0, s1=1.0, s2=1.0, version: int = 1, start: float = 0.0, end: float = 1.0) -> None:
        """StableDiffusion.set_freeu on every device (sdmi_multi_set_freeu): the edits are per sample, sharding changes nothing.  set_freeu(None) clears."""
        if b1 is None:
            check(self._lib.sdmi_multi_set_freeu(self._m, 0, 1.0, 1.0, 1.0, 1.0, 0.0, 1.0))
            return
        check(self._lib.sdmi_multi_set_freeu(self._m, int(version), float(b1), float(b2), float(s1), float(s2), float(start), float(end)))

    def set_ip_adapter(self, embeds=None, tokens=None, negative_tokens=None, scale: float = 1.0, start: float = 0.0, end: float = 1.0) -> None:
        """StableDiffusion.set_ip_adapter on every device (sdmi_multi_set_ip_adapter); each device holds its own copy of the adapter's weights
        (device_view(i).load_ip_adapter_safetensors).  set_ip_adapter(None) clears."""
        if embeds is None and tokens is None:
            check(self._lib.sdmi_multi_set_ip_adapter(self._m, None))
            return
        keep = []
        a = _ip_adapter_struct(keep, embeds, tokens, negative_tokens, scale, start, end)
        if a.T_ip < 0:
            a.T_ip = -a.T_ip * self.device_view(0).ip_adapter_dims()[1]
        check(self._lib.sdmi_multi_set_ip_adapter(self._m, C.byref(a)))

    def schedule(self) -> np.ndarray:
        """StableDiffusion.schedule of device 0 (every device holds the same table)."""
        return self.device_view(0).schedule()

    def set_ksampler(self, kind="dpmpp_2m", schedule="karras", eta: float = 0.0, rho: float = 7.0, sigma_min=None, sigma_max=None, noise_seed: int = 0) -> None:
        """StableDiffusion.set_ksampler on every device (sdmi_multi_set_ksampler); image_base per shard, as set_sampler."""
        if kind is None:
            check(self._lib.sdmi_multi_set_ksampler(self._m, None))
            return
        k = _ksampler_struct(kind, schedule, eta, rho, sigma_min, sigma_max, noise_seed, 0)
        check(self._lib.sdmi_multi_set_ksampler(self._m, C.byref(k)))

    def set_latent_size(self, h: int, w: int) -> None:
        """StableDiffusion.set_latent_size on every device context; if one refuses, every context keeps the size it had."""
        views = [self.device_view(i) for i in range(len(self.devices))]
        before = [v.latent_size for v in views]
        try:
            for v in views:
                v.set_latent_size(h, w)
        except Exception:
            for v, size in zip(views, before):
                v.set_latent_size(*size)
            raise

    @property
    def latent_size(self) -> tuple:
        """the current (h, w) of the first device context (sample_image refuses contexts that disagree)"""
        return self.device_view(0).latent_size

    def lora_attach(self, tensors, scale: float = 1.0) -> MultiLoraAdapter:
        """StableDiffusion.lora_attach on every device (adapters are per device context; each needs keep_masters before its weights are loaded)."""
        parts = []
        try:
            for i in range(len(self.devices)):
                parts.append(self.device_view(i).lora_attach(tensors, scale))
        except Exception:
            for p in parts:
                p.detach()
            raise
        self._lora_views.extend(p._sd for p in parts)
        return MultiLoraAdapter(parts, self)

    def lora_load_safetensors(self, path, scale: float = 1.0, te_scale: float = None, skip_unknown: bool = False) -> MultiLoraAdapter:
        """StableDiffusion.lora_load_safetensors on every device."""
        parts = []
        try:
            for i in range(len(self.devices)):
                parts.append(self.device_view(i).lora_load_safetensors(path, scale, te_scale, skip_unknown))
        except Exception:
            for p in parts:
                p.detach()
            raise
        self._lora_views.extend(p._sd for p in parts)
        return MultiLoraAdapter(parts, self)

    def broadcast_count(self) -> int:
        return int(self._lib.sdmi_multi_broadcast_count(self._m))


class UNet:
    """`UNet<B>` (src/model/unet/mod.rs:96-143): forward(x, timesteps, context)."""

    def __init__(self, sd: StableDiffusion):
        self._sd = sd

    def forward(self, x, timesteps, context, cond=None) -> np.ndarray:
        """cond [n, unet_in_ch - 4, h, w]: the conditioning channels of a UNet built with unet_in_ch > 4 (sdmi_unet_forward_cond)."""
        sd = self._sd
        h, w = sd.latent_size
        x = _f32(x, name="x")
        if x.ndim != 4 or x.shape[1:] != (4, h, w):
            raise ValueError(f"x must be [n,4,{h},{w}], got {x.shape}")
        ts = np.atleast_1d(np.asarray(timesteps)).astype(np.int64)
        if ts.size != 1:
            raise ValueError("the reference passes a single shared timestep (unet/mod.rs:112, Tensor<B,1,Int> of len 1)")
        context = _f32(context, name="context")
        n = x.shape[0]
        if context.ndim != 3 or context.shape[0] != n or context.shape[2] != sd.config.ctx_dim:
            raise ValueError(f"context must be [{n}, T, {sd.config.ctx_dim}], got {context.shape}")
        out = np.empty_like(x)
        if cond is not None:
            cond = sd._check_cond(cond, n)
            check(sd._lib.sdmi_unet_forward_cond(sd._ctx, _fp(x), int(ts[0]), _fp(context), _fp(cond), n, context.shape[1], _fp(out)))
            return out
        check(sd._lib.sdmi_unet_forward(sd._ctx, _fp(x), int(ts[0]), _fp(context), n, context.shape[1], _fp(out)))
        return out


class CLIP:
    """`CLIP<B>` (src/model/clip/mod.rs:48-75): forward(tokens [n, T] int) -> [n, T, ctx_dim]."""

    def __init__(self, sd: StableDiffusion):
        self._sd = sd

    def forward(self, tokens, emb_row=None, weights=None, clip_skip: int = 1) -> np.ndarray:
        """emb_row / weights [n, T] and clip_skip: the extended forward of the web-UI prompt encoding (sdmi_clip_forward_ex)"""
        sd = self._sd
        t = np.ascontiguousarray(tokens, dtype=np.int32)
        if t.ndim != 2:
            raise ValueError(f"tokens must be [n, seq_len], got {t.shape}")
        out = np.empty(t.shape + (sd.config.ctx_dim,), dtype=np.float32)
        if emb_row is None and weights is None and clip_skip == 1:
            check(sd._lib.sdmi_clip_forward(sd._ctx, t.ctypes.data_as(C.POINTER(C.c_int32)), t.shape[0], t.shape[1], _fp(out)))
            return out
        r = None if emb_row is None else np.ascontiguousarray(emb_row, dtype=np.int32)
        w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float32)
        for a, what in ((r, "emb_row"), (w, "weights")):
            if a is not None and a.shape != t.shape:
                raise ValueError(f"{what} must have the shape of tokens {t.shape}, got {a.shape}")
        check(sd._lib.sdmi_clip_forward_ex(sd._ctx, t.ctypes.data_as(C.POINTER(C.c_int32)), None if r is None else r.ctypes.data_as(C.POINTER(C.c_int32)),
                                           None if w is None else _fp(w), t.shape[0], t.shape[1], int(clip_skip), _fp(out)))
        return out


class SimpleTokenizer:
    """`SimpleTokenizer` (src/tokenizer.rs:74-196) -- the C++ tokenizer inside libsdmi (no GPU needed).

    The reference reads "bpe_simple_vocab_16e6.txt" from the working directory; here the merges file is an argument."""

    def __init__(self, merges_path):
        self._lib = load_library()
        self._tok = C.c_void_p()
        check(self._lib.sdmi_tokenizer_create(C.byref(self._tok), str(merges_path).encode()))

    def close(self):
        if getattr(self, "_tok", None) is not None and self._tok.value:
            self._lib.sdmi_tokenizer_destroy(self._tok)
            self._tok = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def vocab_size(self) -> int:
        return int(self._lib.sdmi_tokenizer_vocab_size(self._tok))

    def encode(self, text: str):
        data = text.encode("utf-8")
        n = C.c_int32()
        cap = 4 * len(data) + 8   # at most one token per byte
        ids = (C.c_int32 * cap)()
        check(self._lib.sdmi_tokenizer_encode(self._tok, data, ids, cap, C.byref(n)))
        return [int(ids[i]) for i in range(n.value)]

    def prompt_chunks(self, text: str, clip_ctx: int, emphasis: bool = True, min_chunks: int = 1, embeddings=()):
        """(ids, weights, emb_row), each [k, clip_ctx]: the padded chunks of a prompt (sdmi_prompt_chunks, host only).
        embeddings: [(name, n_vectors)]; emb_row numbers their vectors over the list in order, -1 elsewhere."""
        embeddings = list(embeddings)
        names = (C.c_char_p * max(1, len(embeddings)))(*[n.encode("utf-8") for n, _ in embeddings])
        counts = (C.c_int32 * max(1, len(embeddings)))(*[int(v) for _, v in embeddings])
        data = text.encode("utf-8")
        k, cap = C.c_int32(), max(1, int(min_chunks))
        while True:
            ids = np.empty((cap, clip_ctx), np.int32)
            w = np.empty((cap, clip_ctx), np.float32)
            rows = np.empty((cap, clip_ctx), np.int32)
            st = self._lib.sdmi_prompt_chunks(self._tok, data, int(clip_ctx), int(bool(emphasis)), int(min_chunks), names, counts, len(embeddings),
                                              ids.ctypes.data_as(C.POINTER(C.c_int32)), _fp(w), rows.ctypes.data_as(C.POINTER(C.c_int32)), cap, C.byref(k))
            if st != 0 and k.value > cap:   # *n_chunks is always set: the one retry has the room
                cap = k.value
                continue
            check(st)
            return ids[:k.value].copy(), w[:k.value].copy(), rows[:k.value].copy()

    def decode(self, tokens) -> str:
        t = np.ascontiguousarray(tokens, dtype=np.int32)
        n = C.c_int32()
        cap = 64 * max(1, t.size)
        buf = C.create_string_buffer(cap)
        check(self._lib.sdmi_tokenizer_decode(self._tok, t.ctypes.data_as(C.POINTER(C.c_int32)), t.size, buf, cap, C.byref(n)))
        return buf.raw[:n.value].decode("utf-8", "replace")


class Autoencoder:
    """`Autoencoder<B>` (src/model/autoencoder/mod.rs:47-71): decode_latent on the hot path; encode_image / forward
    with the optional encoder weights."""

    def __init__(self, sd: StableDiffusion):
        self._sd = sd

    def encode_image(self, x) -> np.ndarray:
        """autoencoder/mod.rs:60-66: image [n,3,8h,8w] -> latent [n,4,h,w] (first 4 quant_conv channels)."""
        sd = self._sd
        h, w = sd.latent_size
        x = _f32(x, name="x")
        if x.ndim != 4 or x.shape[1:] != (3, 8 * h, 8 * w):
            raise ValueError(f"x must be [n,3,{8 * h},{8 * w}], got {x.shape}")
        out = np.empty((x.shape[0], 4, h, w), dtype=np.float32)
        check(sd._lib.sdmi_encode_image(sd._ctx, _fp(x), x.shape[0], _fp(out)))
        return out

    def forward(self, x) -> np.ndarray:
        """autoencoder/mod.rs:56-58: decode_latent(encode_image(x))."""
        return self.decode_latent(self.encode_image(x))

    def decode_latent(self, latent) -> np.ndarray:
        sd = self._sd
        h, w = sd.latent_size
        latent = _f32(latent, name="latent")
        if latent.ndim != 4 or latent.shape[1:] != (4, h, w):
            raise ValueError(f"latent must be [n,4,{h},{w}], got {latent.shape}")
        n = latent.shape[0]
        out = np.empty((n, 3, 8 * h, 8 * w), dtype=np.float32)
        check(sd._lib.sdmi_decode_latent(sd._ctx, _fp(latent), n, _fp(out)))
        return out


def qkv_attention(sd: StableDiffusion, q, k, v, mask, n_head: int):
    """Free-function form, as in the reference (attention.rs:5)."""
    return sd.qkv_attention(q, k, v, mask, n_head)
