"""CPU references for the SD 2.x variant (sdmi_config.variant = 1) -- TEST INFRASTRUCTURE ONLY.

Three restatements on top of the oracle, none of them pinned by the reference (which has no SD 2 side):
  * the UNet with C / 64 heads of width 64 at every level (UNetOracle.mha with another head count, nothing else);
  * the OpenCLIP text tower: the CLIP oracle's block with the exact (erf) GELU in its MLP, and the chunker's padding with token id 0 behind a
    chunk's first <|endoftext|>;
  * v-prediction: the model output is v = sqrt(a) eps - sqrt(1 - a) x0, so eps = sqrt(a) v + sqrt(1 - a) x at the evaluation's timestep.  The
    loops are the TEXTBOOK eps loops of sampler_ref / ksampler_ref run on that eps -- independent of the rewritten coefficient tables.
"""
import math

import numpy as np
import torch

import ksampler_ref as K
import prompt_ref as R
import sampler_ref as SR
from oracle import clip_oracle as CO
from oracle import sd_oracle as O

HEAD = 64


class UNetOracleV2(O.UNetOracle):
    """SD 2.x: every attention has c // 64 heads of width 64; Dims.n_head is ignored"""

    def mha(self, path, x, context, c, c_ctx):
        P = self.P
        xa = x if context is None else context
        q = O.linear(x, *P.linear(f"{path}/query", c, c, bias=False))
        k = O.linear(xa, *P.linear(f"{path}/key", c_ctx, c, bias=False))
        v = O.linear(xa, *P.linear(f"{path}/value", c_ctx, c, bias=False))
        wv = O.qkv_attention(q, k, v, None, c // HEAD)
        return O.linear(wv, *P.linear(f"{path}/out", c, c))


class OpenClipOracle(CO.CLIPOracle):
    """the same pre-LN causal transformer with the exact GELU"""

    def block(self, path, x, mask):
        c = self.d.n_state
        h = O.layer_norm(x, *self.P.norm(f"{path}/attn_ln", c))
        q = O.linear(h, *self.P.linear(f"{path}/attn/query", c, c))
        k = O.linear(h, *self.P.linear(f"{path}/attn/key", c, c))
        v = O.linear(h, *self.P.linear(f"{path}/attn/value", c, c))
        x = x + O.linear(O.qkv_attention(q, k, v, mask, self.d.n_head), *self.P.linear(f"{path}/attn/out", c, c))
        h = O.layer_norm(x, *self.P.norm(f"{path}/mlp_ln", c))
        h = O.gelu_erf(O.linear(h, *self.P.linear(f"{path}/mlp/fc1", c, 4 * c)))
        return x + O.linear(h, *self.P.linear(f"{path}/mlp/fc2", 4 * c, c))


def prompt_chunks(encode, start_token, end_token, text, clip_ctx, pad_id=0, **kw):
    """prompt_ref.prompt_chunks with everything BEHIND a chunk's first <|endoftext|> set to pad_id (an embedding's positions carry <|endoftext|> ids
    as content: they stay)"""
    ids, w, rows = R.prompt_chunks(encode, start_token, end_token, text, clip_ctx, **kw)
    ids = ids.copy()
    for c in range(len(ids)):
        free = np.flatnonzero((ids[c] == end_token) & (rows[c] < 0))
        first = int(free[0])               # the chunk's <|endoftext|>: the first one that is no embedding vector
        assert (ids[c, first:] == end_token).all() and (rows[c, first:] < 0).all()
        ids[c, first + 1:] = pad_id
    return ids, w, rows


class SD2Oracle(O.StableDiffusionOracle):
    """StableDiffusionOracle on the 64-wide-head UNet.  prediction "v": forward_diffuser returns the eps the guided v output stands for,
    eps = sqrt(a_t) v + sqrt(1 - a_t) x -- CFG is applied to v, as the engine does; a_t at a fractional t is 1 / (1 + sigma(t)^2) with ln sigma interpolated
    between the table's neighbours (k-diffusion's t_to_sigma, the inverse of ksampler_ref.sigma_to_t)."""

    def __init__(self, provider, alphas_cumprod, dims, dtype=torch.float32, prediction="eps"):
        super().__init__(provider, alphas_cumprod, dims, dtype)
        self.unet = UNetOracleV2(provider, dims, dtype)
        self.prediction = prediction

    def alpha_at(self, t) -> float:
        if float(t) == int(t):
            return float(self.alphas[int(t)])
        ls = np.log(K.model_sigmas(self.alphas))
        lo = int(math.floor(t))
        w = float(t) - lo
        s = math.exp((1.0 - w) * ls[lo] + w * ls[lo + 1])
        return 1.0 / (1.0 + s * s)

    @torch.no_grad()
    def forward_diffuser(self, latent, t, context, uncond, scale):
        out = super().forward_diffuser(latent, t, context, uncond, scale)
        if self.prediction == "eps":
            return out
        a = self.alpha_at(t)
        return math.sqrt(a) * out + math.sqrt(1.0 - a) * latent


def sample_latent_default(ora, ctx, unc, scale, n_steps, x_T):
    """the default path: DDIM(eta = 0) over sample_latent's timesteps"""
    ts, step = O.ddim_timesteps(n_steps, len(ora.alphas))
    return SR.sample_latent(ora, ctx, unc, scale, ts, step, x_T, "ddim")


def sample_latent_k(ora, ctx, unc, scale, n_steps, x_T, kind, schedule):
    sg = K.sigmas(schedule, ora.alphas, n_steps)
    return K.sample_latent(ora, ctx, unc, scale, sg, 0, x_T, kind)


def sample_latent_from(ora, ctx, unc, scale, n_steps, strength, z0, eps, mask):
    """img2img on the default path: the last steps of the schedule from the re-noised z0, the mask blend after every update"""
    import img2img_ref as IR
    ts, step = IR.timesteps(n_steps, strength, len(ora.alphas))
    a0 = float(ora.alphas[ts[0]])
    z0_, eps_ = torch.as_tensor(z0).to(ora.dtype), torch.as_tensor(eps).to(ora.dtype)
    x = math.sqrt(a0) * z0_ + math.sqrt(1.0 - a0) * eps_
    return SR.sample_latent(ora, ctx, unc, scale, ts, step, x, "ddim", mask=mask, z0=z0_, eps=eps_)


def v_of(x, e, a, b):
    """the v a model would output at (x, t) when its eps is e: v = a e - b x0, x0 = (x - b e) / a"""
    return a * e - b * (x - b * e) / a
