"""CPU restatement of IP-Adapter (include/sdmi.h "IP-Adapter"): Ye et al., "IP-Adapter", as diffusers' IPAdapterAttnProcessor runs it.
image_proj and the decoupled attention operator in float64 numpy; IpUNetOracle is oracle.sd_oracle.UNetOracle whose mha adds the image term on every attn2, so that
UNetOracle.forward, controlnet_ref.controlled_forward and freeu_ref.freeu_forward all run it unchanged.  Nothing under oracle/ is touched."""
import numpy as np
import torch

import controlnet_ref as CR
from oracle import sd_oracle as O
from stable_diffusion_burn_amd import synthetic as syn

# the 16 cross attentions in the engine's order (sdmi_ip_adapter_key's ctx_index)
LAYER_PATHS = ([f"input_blocks/rt{i}" for i in range(1, 7)] + ["middle_block"] +
               [f"output_blocks/{n}" for n in ("rt1", "rt2", "rtu1", "rt3", "rt4", "rtu2", "rt5", "rt6", "rt7")])


def image_proj(ad: dict, embeds, ctx_dim: int, dtype=np.float64):
    """tokens = LayerNorm(reshape(Linear(embeds), [T, ctx_dim])), eps 1e-5: embeds [n, D] -> [n, T, ctx_dim]"""
    e = np.asarray(embeds, dtype)
    w, b = np.asarray(ad["image_proj.proj.weight"], dtype), np.asarray(ad["image_proj.proj.bias"], dtype)
    y = (e @ w.T + b).reshape(e.shape[0], -1, ctx_dim)
    mu = y.mean(axis=-1, keepdims=True)
    var = ((y - mu) ** 2).mean(axis=-1, keepdims=True)
    y = (y - mu) / np.sqrt(var + dtype(1e-5))
    return (y * np.asarray(ad["image_proj.norm.weight"], dtype) + np.asarray(ad["image_proj.norm.bias"], dtype)).astype(dtype)


def tokens_of(ad: dict, embeds, ctx_dim: int, dtype=np.float64):
    """embeds [n_img, D]: the pictures of one set concatenated along the token axis -> [T n_img, ctx_dim]"""
    return image_proj(ad, embeds, ctx_dim, dtype).reshape(-1, ctx_dim)


def zero_tokens(ad: dict, ctx_dim: int, n_img: int, dtype=np.float64):
    """the default negative: image_proj(0) per picture"""
    d = np.asarray(ad["image_proj.proj.weight"]).shape[1]
    return tokens_of(ad, np.zeros((n_img, d)), ctx_dim, dtype)


def attention(q, k, v, n_head):
    """softmax(q k^T d^-1/2) v per head, float64: q [n, nq, C], k / v [n, T, C]"""
    q, k, v = (np.asarray(a, np.float64) for a in (q, k, v))
    n, nq, c = q.shape
    d = c // n_head
    qh = q.reshape(n, nq, n_head, d).transpose(0, 2, 1, 3)
    kh = k.reshape(n, -1, n_head, d).transpose(0, 2, 1, 3)
    vh = v.reshape(n, -1, n_head, d).transpose(0, 2, 1, 3)
    s = qh @ kh.transpose(0, 1, 3, 2) / np.sqrt(d)
    s = s - s.max(axis=-1, keepdims=True)
    p = np.exp(s)
    p = p / p.sum(axis=-1, keepdims=True)
    return (p @ vh).transpose(0, 2, 1, 3).reshape(n, nq, c)


def op(q, k_ip, v_ip, o_text, scale, n_head):
    """what sdmi_op_ip_attention computes: O_text + scale_b Attn(q, K_ip, V_ip), float64; scale [n]"""
    s = np.asarray(scale, np.float64).reshape(-1, 1, 1)
    return np.asarray(o_text, np.float64) + s * attention(q, k_ip, v_ip, n_head)


def layer_kv(ad: dict, model_channels: int, tokens, dtype=np.float64):
    """[(K_i, V_i)] of the 16 cross attentions for tokens [nb, T_ip, ctx_dim]"""
    t = np.asarray(tokens, dtype)
    return [(t @ np.asarray(ad[kk], dtype).T, t @ np.asarray(ad[kv], dtype).T) for kk, kv, _ in syn.ip_adapter_layers(model_channels)]


class IpUNetOracle(O.UNetOracle):
    """UNetOracle with the decoupled cross attention: ip = None (the plain model) or (adapter dict, tokens [n, T_ip, ctx_dim], scale)"""

    def __init__(self, provider, dims, dtype=torch.float32, root="unet"):
        super().__init__(provider, dims, dtype, root)
        self.ip = None
        self._index = {f"{root}/{p}/transformer/transformer/attn2": i for i, p in enumerate(LAYER_PATHS)}

    def mha(self, path, x, context, c, c_ctx):
        if self.ip is None or not path.endswith("/attn2"):
            return super().mha(path, x, context, c, c_ctx)
        ad, tokens, scale = self.ip
        P = self.P
        kk, kv, cc = syn.ip_adapter_layers(self.d.model_channels)[self._index[path]]
        assert cc == c, (path, cc, c)
        tok = torch.as_tensor(tokens).to(self.dtype)
        q = O.linear(x, *P.linear(f"{path}/query", c, c, bias=False))
        k = O.linear(context, *P.linear(f"{path}/key", c_ctx, c, bias=False))
        v = O.linear(context, *P.linear(f"{path}/value", c_ctx, c, bias=False))
        k_ip = tok @ torch.from_numpy(np.ascontiguousarray(ad[kk])).to(self.dtype).T
        v_ip = tok @ torch.from_numpy(np.ascontiguousarray(ad[kv])).to(self.dtype).T
        a = O.qkv_attention(q, k, v, None, self.d.n_head) + scale * O.qkv_attention(q, k_ip, v_ip, None, self.d.n_head)
        return O.linear(a, *P.linear(f"{path}/out", c, c))


@torch.no_grad()
def ip_forward(unet: IpUNetOracle, x, t, context, ip, residuals=None, strength=0.0):
    """one forward with the adapter state ip (None: off); residuals / strength: a ControlNet's (controlnet_ref)"""
    unet.ip = ip
    try:
        return CR.controlled_forward(unet, x, t, context, residuals, strength)
    finally:
        unet.ip = None


class IpPredictor:
    """forward_diffuser with an adapter: the conditional half reads tokens [n, T_ip, ctx_dim], the unconditional half neg [n, T_ip, ctx_dim]; step index i of the call
    decides whether the adapter is on (the control's window rule).  control: (ControlNetOracle, hint01, strength) or None."""

    def __init__(self, provider, dims, dtype, ad, tokens, neg, scale, start=0.0, end=1.0, n_steps=1, control=None):
        self.unet = IpUNetOracle(provider, dims, dtype)
        self.dtype = dtype
        self.ad, self.tokens, self.neg, self.scale = ad, tokens, neg, scale
        self.on = set(CR.window(start, end, n_steps))
        self.control = control

    @torch.no_grad()
    def forward(self, x, t, context, tokens, step=0):
        r, st = None, 0.0
        if self.control is not None:
            ctl, hint, st = self.control
            r = ctl.forward(x, t, context, hint)
        ip = (self.ad, tokens, self.scale) if (step in self.on and self.scale != 0) else None
        return ip_forward(self.unet, x, t, context, ip, r, st)

    @torch.no_grad()
    def forward_diffuser(self, latent, t, context, uncond, scale, step):
        n = latent.shape[0]
        u = self.forward(latent, t, uncond.unsqueeze(0).repeat(n, 1, 1), self.neg, step)
        c = self.forward(latent, t, context, self.tokens, step)
        return u + (c - u) * scale
