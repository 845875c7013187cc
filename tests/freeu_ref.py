"""CPU restatement of FreeU (include/sdmi.h "FreeU"): Si et al., "FreeU: Free Lunch in Diffusion U-Net", as ComfyUI's FreeU / FreeU_V2 nodes
ship it -- the rule keyed on the channel count of the backbone tensor entering an output block.  fourier_filter follows the published code literally with numpy.fft;
closed_form is the four-coefficient formula the engine evaluates; freeu_forward is UNetOracle.forward with the two edits in front of every torch.cat, built the way
controlnet_ref.controlled_forward is.  Nothing under oracle/ is touched."""
from dataclasses import dataclass

import numpy as np
import torch

from oracle import sd_oracle as O


@dataclass(frozen=True)
class Params:
    b1: float = 1.0
    b2: float = 1.0
    s1: float = 1.0
    s2: float = 1.0
    version: int = 1


def fourier_filter(x, s, threshold=1):
    """Fourier_filter(x, threshold, scale) of the published code, float64: x [..., H, W]"""
    x = np.asarray(x, np.float64)
    H, W = x.shape[-2:]
    f = np.fft.fftshift(np.fft.fftn(x, axes=(-2, -1)), axes=(-2, -1))
    mask = np.ones(x.shape, np.float64)
    cr, cc = H // 2, W // 2
    mask[..., cr - threshold:cr + threshold, cc - threshold:cc + threshold] = s
    f = f * mask
    return np.fft.ifftn(np.fft.ifftshift(f, axes=(-2, -1)), axes=(-2, -1)).real


def _freqs(n):
    return (-1, 0) if n >= 2 else (0,)


def closed_form(x, s):
    """v' = v + (s - 1) / (H W) sum_{f in F(H) x F(W)} (A_f cos phi_f + B_f sin phi_f), float64: at most seven real sums per (sample, channel)"""
    x = np.asarray(x, np.float64)
    H, W = x.shape[-2:]
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    out = x.copy()
    for fy in _freqs(H):
        for fx in _freqs(W):
            phi = 2.0 * np.pi * (fy * yy / H + fx * xx / W)
            c, sn = np.cos(phi), np.sin(phi)
            A = (x * c).sum(axis=(-2, -1), keepdims=True)
            B = (x * sn).sum(axis=(-2, -1), keepdims=True)
            out += (s - 1.0) / (H * W) * (A * c + B * sn)
    return out


def backbone(h, b, version):
    """h [n, cx, H, W] float64 -> the scaled copy.  Version 2's published code divides by max - min; where that is zero this takes m_hat = 0 (the one deviation)."""
    h = np.array(h, np.float64)
    half = h.shape[1] // 2
    if version == 1:
        h[:, :half] *= b
        return h
    m = h.mean(axis=1, keepdims=True)
    n = m.shape[0]
    lo = m.reshape(n, -1).min(axis=1).reshape(n, 1, 1, 1)
    hi = m.reshape(n, -1).max(axis=1).reshape(n, 1, 1, 1)
    span = hi - lo
    mh = np.where(span > 0, (m - lo) / np.where(span > 0, span, 1.0), 0.0)
    h[:, :half] *= (b - 1.0) * mh + 1.0
    return h


def op(x, cx, version, b, s):
    """what sdmi_op_freeu computes: x [n, c, H, W] = cat([h, hs]), float64"""
    x = np.asarray(x, np.float64)
    h = backbone(x[:, :cx], b, version) if b != 1 else x[:, :cx]
    hs = closed_form(x[:, cx:], s) if s != 1 else x[:, cx:]
    return np.concatenate([h, hs], axis=1)


def group_of(cx, mc):
    return 1 if cx == 4 * mc else 2 if cx == 2 * mc else 0


def plan(unet: O.UNetOracle, latent_h, latent_w):
    """the block rule applied to the oracle's own topology: [(group, cx, cskip, h, w)] per output block"""
    inp, out = unet.plan()
    mc = unet.d.model_channels
    sizes, h, w = [], latent_h, latent_w
    for kind, _, _, cout in inp:
        if kind == "down":
            h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1     # 3 x 3, stride 2, pad 1
        sizes.append((cout, h, w))
    rows = []
    for _, _, cin, _ in out:
        cskip, h, w = sizes.pop()
        cx = cin - cskip
        rows.append((group_of(cx, mc), cx, cskip, h, w))
    return rows


def _edit(x, saved, params, mc):
    g = group_of(x.shape[1], mc)
    if not g:
        return x, saved
    b, s = (params.b1, params.s1) if g == 1 else (params.b2, params.s2)
    if b != 1:
        x = torch.from_numpy(backbone(x.double().numpy(), b, params.version)).to(x.dtype)
    if s != 1:
        saved = torch.from_numpy(fourier_filter(saved.double().numpy(), s)).to(saved.dtype)
    return x, saved


@torch.no_grad()
def freeu_forward(unet: O.UNetOracle, x, t: int, context, params, residuals=None, strength=0):
    """UNetOracle.forward with FreeU in front of every torch.cat; params None = the plain forward.  residuals / strength: a ControlNet's (controlnet_ref), added to the
    saved skips and the middle block's output BEFORE FreeU sees them.  The two edits are evaluated in float64 and cast back to the oracle's dtype."""
    x = x.to(unet.dtype)
    context = context.to(unet.dtype)
    emb = unet.time_embed(t)
    inp, out = unet.plan()
    mc = unet.d.model_channels
    saved = []
    for kind, name, cin, cout in inp:
        x = unet._block(kind, f"{unet.root}/input_blocks/{name}", x, emb, context, cin, cout)
        saved.append(x)
    mp = f"{unet.root}/middle_block"
    x = unet.res_block(f"{mp}/res1", x, emb, 4 * mc, 4 * mc)
    x = unet.spatial_transformer(f"{mp}/transformer", x, context, 4 * mc)
    x = unet.res_block(f"{mp}/res2", x, emb, 4 * mc, 4 * mc)
    if residuals is not None:
        r = [v.to(unet.dtype) for v in residuals]
        saved = [sv + strength * r[j] for j, sv in enumerate(saved)]
        x = x + strength * r[12]
    for kind, name, cin, cout in out:
        hs = saved.pop()
        if params is not None:
            x, hs = _edit(x, hs, params, mc)
        x = torch.cat([x, hs], dim=1)
        x = unet._block(kind, f"{unet.root}/output_blocks/{name}", x, emb, context, cin, cout)
    x = O.group_norm(x, *unet.P.norm(f"{unet.root}/norm_out", mc))
    x = O.silu(x)
    return O.conv2d(x, unet.P.conv(f"{unet.root}/conv_out", mc, 4, 3), padding=1)


class FreeUPredictor:
    """forward_diffuser with FreeU (and optionally a ControlNet: `control` = a controlnet_ref.ControlledPredictor-like (ctl, hint, strength) triple): step index i of the
    call decides whether FreeU is on -- the control's window rule -- and both CFG halves are treated alike."""

    def __init__(self, provider, dims, dtype, params, start=0.0, end=1.0, n_steps=1, control=None):
        import controlnet_ref as CR
        self.unet = O.UNetOracle(provider, dims, dtype)
        self.params, self.dtype = params, dtype
        self.on = set(CR.window(start, end, n_steps))
        self.control = control     # (ControlNetOracle, hint01, strength) or None: controlled on every step

    @torch.no_grad()
    def forward(self, x, t, context, step=0):
        r, st = None, 0
        if self.control is not None:
            ctl, hint, st = self.control
            r = ctl.forward(x, t, context, hint)
        return freeu_forward(self.unet, x, t, context, self.params if step in self.on else None, r, st)

    @torch.no_grad()
    def forward_diffuser(self, latent, t, context, uncond, scale, step):
        n = latent.shape[0]
        u = self.forward(latent, t, uncond.unsqueeze(0).repeat(n, 1, 1), step)
        c = self.forward(latent, t, context, step)
        return u + (c - u) * scale
