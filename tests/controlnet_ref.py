"""CPU restatement of ControlNet for SD v1 (include/sdmi.h "ControlNet"), composed from the oracle's UNetOracle: a ControlNet is the
UNet's time MLP, encoder and middle block under another root, plus the hint convolutions, one zero convolution per input block and middle_block_out
(ControlNet's cldm.py: ControlNet.forward and ControlledUnetModel.forward).  Nothing under oracle/ is touched."""
import math

import numpy as np
import torch

from oracle import sd_oracle as O

HINT_WIDTHS = (16, 16, 32, 32, 96, 96, 256)   # cldm.py input_hint_block: constants, not multiples of model_channels
HINT_STRIDES = (1, 1, 2, 1, 2, 1, 2, 1)


def hint01(hint_u8: np.ndarray) -> torch.Tensor:
    """n x [H, W, 3] u8 -> [n, 3, H, W] in [0, 1] (fp64: the division is the engine's fp32 one up to its last bit)"""
    return torch.from_numpy(np.ascontiguousarray(hint_u8.transpose(0, 3, 1, 2)).astype(np.float32) / np.float32(255.0))


class ControlNetOracle(O.UNetOracle):
    def __init__(self, provider, dims: O.Dims = O.Dims(), dtype=torch.float32):
        super().__init__(provider, dims, dtype, root="controlnet")

    @torch.no_grad()
    def hint_embed(self, hint):
        """input_hint_block: eight 3x3 pad-1 convolutions, SiLU after all but the last; hint [n, 3, 8h, 8w] in [0, 1] -> [n, mc, h, w]"""
        widths = (hint.shape[1],) + HINT_WIDTHS + (self.d.model_channels,)
        x = hint.to(self.dtype)
        for i in range(8):
            x = O.conv2d(x, self.P.conv(f"{self.root}/hint/c{i}", widths[i], widths[i + 1], 3), stride=HINT_STRIDES[i], padding=1)
            if i != 7:
                x = O.silu(x)
        return x

    @torch.no_grad()
    def forward(self, x, t: int, context, hint):
        """ControlNet.forward: the 13 residuals.  hint [n or 1, 3, 8h, 8w] in [0, 1]."""
        x = x.to(self.dtype)
        context = context.to(self.dtype)
        emb = self.time_embed(t)
        guided = self.hint_embed(hint)
        if guided.shape[0] != x.shape[0]:
            guided = guided.repeat(x.shape[0] // guided.shape[0], 1, 1, 1)
        inp, _ = self.plan()
        mc = self.d.model_channels
        outs = []
        for j, (kind, name, cin, cout) in enumerate(inp):
            x = self._block(kind, f"{self.root}/input_blocks/{name}", x, emb, context, cin, cout)
            if j == 0:
                x = x + guided
            outs.append(O.conv2d(x, self.P.conv(f"{self.root}/zero_convs/{j}", cout, cout, 1)))
        mp = f"{self.root}/middle_block"
        x = self.res_block(f"{mp}/res1", x, emb, 4 * mc, 4 * mc)
        x = self.spatial_transformer(f"{mp}/transformer", x, context, 4 * mc)
        x = self.res_block(f"{mp}/res2", x, emb, 4 * mc, 4 * mc)
        outs.append(O.conv2d(x, self.P.conv(f"{self.root}/middle_block_out", 4 * mc, 4 * mc, 1)))
        return outs


@torch.no_grad()
def controlled_forward(unet: O.UNetOracle, x, t: int, context, residuals, strength: float):
    """ControlledUnetModel.forward: UNetOracle.forward with saved.pop() + s r[j] and mid + s r[12].  The encoder runs on the unmodified activations."""
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
        saved = [s + strength * r[j] for j, s in enumerate(saved)]
        x = x + strength * r[12]
    for kind, name, cin, cout in out:
        x = torch.cat([x, saved.pop()], dim=1)
        x = unet._block(kind, f"{unet.root}/output_blocks/{name}", x, emb, context, cin, cout)
    x = O.group_norm(x, *unet.P.norm(f"{unet.root}/norm_out", mc))
    x = O.silu(x)
    return O.conv2d(x, unet.P.conv(f"{unet.root}/conv_out", mc, 4, 3), padding=1)


def window(start: float, end: float, n_steps: int) -> list:
    """the controlled step indices of a call of n_steps steps: start * S <= i < end * S in f64 (python floats are f64)"""
    return [i for i in range(n_steps) if start * n_steps <= i < end * n_steps]


class ControlledPredictor:
    """forward_diffuser with a ControlNet: both CFG halves are controlled (no guess mode); step index i of the call decides whether the control is on."""

    def __init__(self, provider, dims, dtype, hint, strength, start=0.0, end=1.0, n_steps=1):
        self.unet = O.UNetOracle(provider, dims, dtype)
        self.ctl = ControlNetOracle(provider, dims, dtype)
        self.hint, self.strength = hint, strength
        self.on = set(window(start, end, n_steps))
        self.dtype = dtype

    @torch.no_grad()
    def forward(self, x, t, context, step=0):
        r = self.ctl.forward(x, t, context, self.hint) if (step in self.on and self.strength != 0.0) else None
        return controlled_forward(self.unet, x, t, context, r, self.strength)

    @torch.no_grad()
    def forward_diffuser(self, latent, t, context, uncond, scale, step):
        n = latent.shape[0]
        u = self.forward(latent, t, uncond.unsqueeze(0).repeat(n, 1, 1), step)
        c = self.forward(latent, t, context, step)
        return u + (c - u) * scale


@torch.no_grad()
def sample(pred: ControlledPredictor, alphas, context, uncond, scale, ts, step_size, x_start):
    """sample_latent's DDIM loop (eta = 0) over the timesteps ts -- the full schedule or an img2img tail -- the control window counting ts's own steps"""
    dt = pred.dtype
    latent = torch.as_tensor(x_start).to(dt)
    context = torch.as_tensor(context).to(dt)
    uncond = torch.as_tensor(uncond).to(dt)
    for i, t in enumerate(ts):
        cur = float(alphas[t])
        prev = float(alphas[t - step_size]) if t >= step_size else 1.0
        e = pred.forward_diffuser(latent, t, context, uncond, scale, i)
        predx0 = (latent - e * math.sqrt(1.0 - cur)) / math.sqrt(cur)
        latent = predx0 * math.sqrt(prev) + e * math.sqrt(1.0 - prev)
    return latent
