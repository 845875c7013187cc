"""CPU restatement of CFG rescale (include/sdmi.h "CFG rescale and zero-terminal-SNR schedules"; diffusers' rescale_noise_cfg): the per-image
factor and one sampler step with it in numpy float64, the same step restated in float32 the way the kernel sums (two-pass statistics, a float32 partial per thread
over its pixels, float64 merges), and the oracle with the rescale hook that the textbook loops of sampler_ref / ksampler_ref / zero_snr_ref drive."""
import math

import numpy as np
import torch

from img2img_ref import normal_stream
from oracle import sd_oracle as O

M64 = (1 << 64) - 1


def factor(ec, g, phi):
    """f_b = phi std(ec_b) / std(g_b) + (1 - phi) over each image's elements ([n, ...] numpy float64); 1 where std(g_b) = 0 or a statistic is not finite"""
    n = ec.shape[0]
    sc, sg = ec.reshape(n, -1).std(axis=1), g.reshape(n, -1).std(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = phi * sc / sg + (1.0 - phi)
    return np.where((sg > 0.0) & np.isfinite(f), f, 1.0)


def _sum_as_kernel(v, threads):
    """sum of v [pixels, 4] float32: thread t adds (x + y) + (z + w) of pixels t, t + threads, ... in float32, the partials merge in float64"""
    p = v.shape[0]
    per = ((v[:, 0] + v[:, 1]) + (v[:, 2] + v[:, 3])).astype(np.float32)
    rounds = -(-p // threads)
    per = np.concatenate([per, np.zeros(rounds * threads - p, np.float32)]).reshape(rounds, threads)
    part = np.zeros(threads, np.float32)
    for r in range(rounds):
        part = (part + per[r]).astype(np.float32)
    return float(part.astype(np.float64).sum())


def factor_f32(ec, g, phi):
    """the same in float32 as the kernel forms it; ec, g [n,4,h,w] float32"""
    n, _, h, w = ec.shape
    hw = h * w
    threads = min(1024, (hw + 63) // 64 * 64)
    out = np.ones(n, np.float32)
    for b in range(n):
        sq = []
        for a in (ec[b], g[b]):
            px = np.ascontiguousarray(a.reshape(4, hw).T)
            mean = np.float32(_sum_as_kernel(px, threads) / (4.0 * hw))
            d = (px - mean).astype(np.float32)
            sq.append(_sum_as_kernel((d * d).astype(np.float32), threads))
        with np.errstate(divide="ignore", invalid="ignore"):
            f = float(np.float32(phi)) * np.sqrt(np.float64(sq[0]) / np.float64(sq[1])) + (1.0 - float(np.float32(phi)))
        out[b] = np.float32(f) if (sq[1] > 0.0 and np.isfinite(f)) else np.float32(1.0)
    return out


def step_noise(key: int, n: int, h: int, w: int) -> np.ndarray:
    return np.stack([normal_stream((key + b) & M64, 4 * h * w).reshape(4, h, w) for b in range(n)])


def step(dtype, eps, latent, scale, phi, row, q_hist=(), noise_key=0, noise_key2=0, mask=None, z0=None, e0=None, blend_prev=0.0, blend_dir=0.0):
    """One launch of sdmi_op_sampler_step in `dtype` (np.float64: the reference; np.float32: the formula as the kernel rounds it, without its contractions).
    The coefficients are what the kernel receives: float32.  Returns (latent_out, q, f)."""
    f32 = np.float32
    n = latent.shape[0]
    cx, ce, h1, h2, h3, cz, cz2, qx, qe = (dtype(f32(v)) for v in row)
    sc, bp, bd = dtype(f32(scale)), dtype(f32(blend_prev)), dtype(f32(blend_dir))
    eu, ec, x = eps[:n].astype(dtype), eps[n:].astype(dtype), latent.astype(dtype)
    g = eu + (ec - eu) * sc
    if phi == 0.0:
        f = np.ones(n, dtype)
    elif dtype == np.float64:
        f = factor(ec, g, float(f32(phi)))
    else:
        f = factor_f32(ec, g, phi)
    e = f.astype(dtype).reshape(n, 1, 1, 1) * g
    q = qx * x + qe * e
    nx = cx * x + ce * e
    for hk, qk in zip((h1, h2, h3), q_hist):
        nx = nx + hk * np.asarray(qk).astype(dtype)
    _, _, h, w = latent.shape
    if cz != 0:
        nx = nx + cz * step_noise(noise_key, n, h, w).astype(dtype)
    if cz2 != 0:
        nx = nx + cz2 * step_noise(noise_key2, n, h, w).astype(dtype)
    if mask is not None:
        m = np.asarray(mask).astype(dtype).reshape(n, 1, h, w)
        nx = m * nx + (dtype(1.0) - m) * (bp * np.asarray(z0).astype(dtype) + bd * np.asarray(e0).astype(dtype))
    return nx, q, f


# ---- the oracle with the rescale hook (GPU parity tests) ---------------------------------------------------------------------------------
class GuidanceOracle(O.StableDiffusionOracle):
    """StableDiffusionOracle whose guided model output is rescaled per image (phi) before anything else sees it.  prediction "v": the UNet's output is v;
    forward_diffuser returns the eps the rescaled guided v stands for (as sd2_ref.SD2Oracle), guided() the rescaled guided output itself.  max_f: the largest
    factor applied so far."""

    def __init__(self, provider, alphas_cumprod, dims, dtype=torch.float32, prediction="eps", phi=0.0, unet=None, cond=None):
        super().__init__(provider, alphas_cumprod, dims, dtype)
        self.prediction, self.phi, self.max_f = prediction, float(phi), 1.0
        if unet is not None:   # a conditioned UNet (inpaint_ref.CondUNetOracle): cond [n, unet_in_ch - 4, h, w] goes behind the latent of every forward
            self.unet = unet
        self.cond = None if cond is None else torch.as_tensor(cond).to(dtype)

    def alpha_at(self, t) -> float:
        import ksampler_ref as K
        if float(t) == int(t):
            return float(self.alphas[int(t)])
        ls = np.log(K.model_sigmas(self.alphas))
        lo = int(math.floor(t))
        wgt = float(t) - lo
        s = math.exp((1.0 - wgt) * ls[lo] + wgt * ls[lo + 1])
        return 1.0 / (1.0 + s * s)

    @torch.no_grad()
    def guided(self, latent, t, context, uncond, scale):
        n = latent.shape[0]
        x = latent if self.cond is None else torch.cat([latent, self.cond], 1)
        u = self.unet.forward(x, t, uncond.unsqueeze(0).repeat(n, 1, 1))
        c = self.unet.forward(x, t, context)
        g = u + (c - u) * scale
        if self.phi != 0.0:
            sc, sg = c.reshape(n, -1).std(dim=1), g.reshape(n, -1).std(dim=1)
            f = self.phi * sc / sg + (1.0 - self.phi)
            f = torch.where((sg > 0) & torch.isfinite(f), f, torch.ones_like(f))
            self.max_f = max(self.max_f, float(f.max()))
            g = f.reshape(n, 1, 1, 1) * g
        return g

    @torch.no_grad()
    def forward_diffuser(self, latent, t, context, uncond, scale):
        out = self.guided(latent, t, context, uncond, scale)
        if self.prediction == "eps":
            return out
        a = self.alpha_at(t)
        return math.sqrt(a) * out + math.sqrt(1.0 - a) * latent
