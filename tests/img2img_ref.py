"""CPU restatement of img2img (include/sdmi.h "img2img", DESIGN.md section "img2img"), composed from the oracle's
EncoderOracle.encode_image, StableDiffusionOracle.forward_diffuser and ddim_timesteps, plus a numpy restatement of the
library's N(0,1) stream (splitmix64 -> Box-Muller, uint64 wraparound, float32 arithmetic)."""
import math

import numpy as np
import torch

from oracle import sd_oracle as O

VAE_SCALE = np.float32(0.18215)


def timesteps(n_steps: int, strength: float, total: int = 1000):
    """rule 1: the last k = min(L, int(strength * L)) of sample_latent's L timesteps, and the schedule's step"""
    ts, step = O.ddim_timesteps(n_steps, total)
    L = len(ts)
    k = min(L, int(strength * L))
    if not (0.0 < strength <= 1.0) or k < 1:
        raise ValueError("strength")
    return ts[L - k:], step


def _splitmix64(x):
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def normal_stream(seed: int, count: int) -> np.ndarray:
    """elements 0..count-1 of stream `seed` (launch_fill_normal: image i of a seeded call uses seed + i, NCHW order)"""
    i = np.arange(count, dtype=np.uint64)
    with np.errstate(over="ignore"):
        r = _splitmix64(np.uint64(seed) * np.uint64(0xD1342543DE82EF95) + i)
    f = np.float32
    u1 = ((r >> np.uint64(40)).astype(np.uint32).astype(f) + f(1.0)) * (f(1.0) / f(16777217.0))
    u2 = ((r >> np.uint64(8)) & np.uint64(0xFFFFFF)).astype(np.uint32).astype(f) * (f(1.0) / f(16777216.0))
    return np.sqrt(f(-2.0) * np.log(u1)) * np.cos(f(6.283185307179586) * u2)


def seeded_noise(seed: int, n: int, h: int, w: int) -> np.ndarray:
    return np.stack([normal_stream(seed + i, 4 * h * w).reshape(4, h, w) for i in range(n)])


def rgb_to_model_input(rgb_u8: np.ndarray) -> np.ndarray:
    """n x [8h,8w,3] u8 -> the encoder's input [n,3,8h,8w] fp32, x = v / 127.5 - 1 (rule 2)"""
    x = rgb_u8.astype(np.float32) / np.float32(127.5) - np.float32(1.0)
    return np.ascontiguousarray(x.transpose(0, 3, 1, 2))


def encode_z0(encoder: "O.EncoderOracle", rgb_u8: np.ndarray) -> torch.Tensor:
    """rule 2, image API: z0 = 0.18215 * encode_image(x)"""
    return encoder.encode_image(torch.from_numpy(rgb_to_model_input(rgb_u8))) * 0.18215


@torch.no_grad()
def sample_latent_from(ora: "O.StableDiffusionOracle", context, uncond, scale: float, n_steps: int, strength: float, z0, eps, mask=None):
    """rules 1 and 3-6 in the oracle's dtype: x_t0 = sqrt(a_t0) z0 + sqrt(1 - a_t0) eps, then sample_latent's update per step,
    each followed by the mask blend toward sqrt(a_prev) z0 + sqrt(1 - a_prev) eps"""
    dt = ora.dtype
    ts, step = timesteps(n_steps, strength, ora.n_steps)
    z0 = torch.as_tensor(z0).to(dt)
    eps = torch.as_tensor(eps).to(dt)
    context = torch.as_tensor(context).to(dt)
    uncond = torch.as_tensor(uncond).to(dt)
    m = None if mask is None else torch.as_tensor(mask).to(dt).reshape(z0.shape[0], 1, z0.shape[2], z0.shape[3])
    a0 = float(ora.alphas[ts[0]])
    latent = math.sqrt(a0) * z0 + math.sqrt(1.0 - a0) * eps
    for t in ts:
        cur = float(ora.alphas[t])
        prev = float(ora.alphas[t - step]) if t >= step else 1.0
        sqrt_noise = math.sqrt(1.0 - cur)
        e = ora.forward_diffuser(latent, t, context, uncond, scale)
        predx0 = (latent - e * sqrt_noise) / math.sqrt(cur)
        dir_latent = e * math.sqrt(1.0 - prev - 0.0)
        latent = predx0 * math.sqrt(prev) + dir_latent
        if m is not None:
            latent = m * latent + (1.0 - m) * (math.sqrt(prev) * z0 + math.sqrt(1.0 - prev) * eps)
    return latent
