"""CPU restatement of the conditioned UNet input and of the inpainting conditioning (include/sdmi.h "a UNet with conditioning channels"),
built on the oracle without editing it: a UNetOracle whose first block reads unet_in_ch channels, the cond rule of the CompVis inpainting script with
EncoderOracle (posterior mean for its posterior sample), and img2img_ref's sampler with torch.cat([x, cond], 1) in front of every forward."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import img2img_ref as R
from oracle import sd_oracle as O


class CondUNetOracle(O.UNetOracle):
    """UNetOracle whose conv_in takes unet_in_ch inputs (forward already accepts any channel count); zero_cond: the conv_in weight is zeroed on the
    channels 4 and up (the reference file's own check)"""

    def __init__(self, provider, dims, dtype=torch.float32, unet_in_ch=9, zero_cond=False):
        super().__init__(provider, dims, dtype)
        self.unet_in_ch = unet_in_ch
        self.zero_cond = zero_cond

    def plan(self):
        inp, out = super().plan()
        kind, name, _, cout = inp[0]
        return [(kind, name, self.unet_in_ch, cout)] + inp[1:], out

    def _block(self, kind, path, x, emb, ctx, cin, cout):
        if kind == "conv" and self.zero_cond:
            w, b = self.P.conv(path, cin, cout, 3)
            w = w.clone()
            w[:, 4:] = 0
            return O.conv2d(x, (w, b), padding=1)
        return super()._block(kind, path, x, emb, ctx, cin, cout)


class CondProvider:
    """a weight provider that answers the 4-channel conv_in with the first 4 input channels of the unet_in_ch one: the plain oracle on it is what the
    conditioned oracle with a conv_in zeroed on channels 4.. computes"""

    def __init__(self, provider, unet_in_ch):
        self.p, self.c = provider, unet_in_ch

    def get(self, name, shape, kind, fan_in=0):
        if name == "unet/input_blocks/conv/weight" and tuple(shape)[1] == 4:
            return np.ascontiguousarray(self.p.get(name, (shape[0], self.c, 3, 3), kind, self.c * 9)[:, :4])
        if name == "unet/input_blocks/conv/bias":
            return self.p.get(name, shape, kind, self.c * 9)
        return self.p.get(name, shape, kind, fan_in)


def latent_mask(mask_u8: np.ndarray, h: int, w: int) -> np.ndarray:
    """pixel mask n x [8h,8w] u8 (>= 128: regenerate) -> [n,h,w] of 0 / 1: torch's legacy `nearest` at the exact scale 8"""
    m = torch.from_numpy((np.asarray(mask_u8) >= 128).astype(np.float32))[:, None]
    return F.interpolate(m, size=(h, w)).numpy()[:, 0]


def masked_input(rgb_u8: np.ndarray, mask_u8: np.ndarray) -> np.ndarray:
    """(v / 127.5 - 1) * (mask < 128) as the encoder's [n,3,8h,8w] input"""
    x = R.rgb_to_model_input(rgb_u8)
    return x * (np.asarray(mask_u8) < 128).astype(np.float32)[:, None]


def inpaint_cond(encoder: "O.EncoderOracle", rgb_u8: np.ndarray, mask_u8: np.ndarray) -> torch.Tensor:
    """cond [n,5,h,w] = [m, 0.18215 * encode_image(masked picture)[:, :4]]"""
    z = encoder.encode_image(torch.from_numpy(masked_input(rgb_u8, mask_u8))) * 0.18215
    m = torch.from_numpy(latent_mask(mask_u8, z.shape[2], z.shape[3]))[:, None].to(z.dtype)
    return torch.cat([m, z], 1)


@torch.no_grad()
def forward_diffuser(unet, latent, t, context, uncond, scale, cond):
    n = latent.shape[0]
    x = torch.cat([latent, cond], 1)
    u = unet.forward(x, t, uncond.unsqueeze(0).repeat(n, 1, 1))
    c = unet.forward(x, t, context)
    return u + (c - u) * scale


@torch.no_grad()
def sample_latent_from(unet, alphas, context, uncond, scale, n_steps, strength, z0, eps, cond, mask=None):
    """img2img_ref.sample_latent_from with torch.cat([x, cond], 1) in front of each forward"""
    dt = unet.dtype
    alphas = np.asarray(alphas, np.float32)
    ts, step = R.timesteps(n_steps, strength, len(alphas))
    z0, eps, context, uncond, cond = (torch.as_tensor(a).to(dt) for a in (z0, eps, context, uncond, cond))
    m = None if mask is None else torch.as_tensor(mask).to(dt).reshape(z0.shape[0], 1, z0.shape[2], z0.shape[3])
    a0 = float(alphas[ts[0]])
    latent = math.sqrt(a0) * z0 + math.sqrt(1.0 - a0) * eps
    for t in ts:
        cur = float(alphas[t])
        prev = float(alphas[t - step]) if t >= step else 1.0
        e = forward_diffuser(unet, latent, t, context, uncond, scale, cond)
        predx0 = (latent - e * math.sqrt(1.0 - cur)) / math.sqrt(cur)
        latent = predx0 * math.sqrt(prev) + e * math.sqrt(1.0 - prev - 0.0)
        if m is not None:
            latent = m * latent + (1.0 - m) * (math.sqrt(prev) * z0 + math.sqrt(1.0 - prev) * eps)
    return latent
