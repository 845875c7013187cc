"""Reference side of the LoRA tests: seeded adapter factors, the merge W = W0 + sum_a c_a (up_a . down_a) in float64, the
rounding bound of the device merge, and a weight provider that hands the oracle the merged tensors -- so the oracle runs the adapted model.

Layouts (include/sdmi.h "LoRA adapters"): Linear weight [in, out]: down [rank, in], up [out, rank], delta[i][o] = sum_j up[o][j] down[j][i].
Conv weight [cout, cin, k, k]: down [rank, cin, k, k], up [cout, rank], delta = up @ down.reshape(rank, -1).
"""
import zlib

import numpy as np

U = 2.0 ** -24   # unit roundoff of fp32


def coef(scale, alpha, rank) -> np.float32:
    """c = (float)(scale * alpha / rank), formed in f64 from the f32 alpha the C ABI receives"""
    return np.float32(float(scale) * float(np.float32(alpha)) / float(rank))


def delta_f64(shape, down, up) -> np.ndarray:
    """up . down in the target's layout, float64"""
    down, up = np.asarray(down, np.float64), np.asarray(up, np.float64)
    r = down.shape[0]
    if len(shape) == 4:
        return (up @ down.reshape(r, -1)).reshape(shape)
    return down.T @ up.T          # [in, rank] @ [rank, out]


def abs_delta_f64(shape, down, up) -> np.ndarray:
    """sum_j |P||Q|: what the rounding bound weighs"""
    return delta_f64(shape, np.abs(down), np.abs(up))


def merge_f64(w0, terms) -> np.ndarray:
    """W0 + sum c (up . down) in float64; terms = [(down, up, c)] with c the f32 coefficient, zero coefficients skipped"""
    w = np.asarray(w0, np.float64).copy()
    for down, up, c in terms:
        if float(c) != 0.0:
            w += float(c) * delta_f64(w0.shape, down, up)
    return w


def merge_bound(w0, terms) -> np.ndarray:
    """Elementwise bound on |fp32 merge - merge_f64|: (r_sum + A + 2) u (|W0| + sum_a |c_a| sum_j |P_a||Q_a|), r_sum the summed ranks and A the
    number of active adapters -- the gamma_n bound of an fp32 sum of r_sum + 1 terms in any order, each product rounded once more by its
    coefficient (gamma_n ~ n u; the + 2 covers the coefficient multiply and the second-order terms at these n)."""
    active = [(d, u, c) for d, u, c in terms if float(c) != 0.0]
    mag = np.abs(np.asarray(w0, np.float64))
    for down, up, c in active:
        mag = mag + abs(float(c)) * abs_delta_f64(w0.shape, down, up)
    r_sum = sum(int(np.asarray(d).shape[0]) for d, _, _ in active)
    return (r_sum + len(active) + 2) * U * mag


def make_adapter(targets, seed: int, rel: float = 0.1) -> dict:
    """{target: (down, up, alpha)} for targets = {name: (shape, rank)}: seeded normals scaled so that at scale 1 the delta's RMS is `rel` x the RMS of
    the synthetic W0 (U(-b, b), b = fan_in^-1/2: RMS b / sqrt(3)).  alpha = rank / 2 (a power-of-two-free ratio would do as well; the point is
    alpha != rank, so the coefficient is not 1)."""
    out = {}
    for name, (shape, rank) in targets.items():
        shape = tuple(int(v) for v in shape)
        fan_in = shape[1] * shape[2] * shape[3] if len(shape) == 4 else shape[0]
        n_out = shape[0] if len(shape) == 4 else shape[1]
        alpha = rank / 2.0
        w_rms = 1.0 / np.sqrt(3.0 * fan_in)
        sigma = np.sqrt(rel * w_rms / (np.sqrt(rank) * alpha / rank))   # RMS(up . down) = sigma^2 sqrt(rank)
        g = np.random.default_rng([int(seed), zlib.crc32(name.encode("utf-8"))])
        down = (sigma * g.standard_normal((rank,) + (shape[1:] if len(shape) == 4 else (fan_in,)))).astype(np.float32)
        up = (sigma * g.standard_normal((n_out, rank))).astype(np.float32)
        out[name] = (down, up, float(alpha))
    return out


class LoraProvider:
    """SyntheticWeights with adapters merged in: get() returns float32(merge_f64(W0, ...)) for the targets of `adapters` = [(tensors, scale)],
    the base tensor otherwise.  The effective weight of the engine is an fp32 tensor too, equal to this one within merge_bound."""

    def __init__(self, base, adapters):
        self.base = base
        self.adapters = list(adapters)

    def terms(self, name):
        return [(t[name][0], t[name][1], coef(s, t[name][2], t[name][0].shape[0])) for t, s in self.adapters if name in t]

    def get(self, name, shape, kind, fan_in=0):
        w0 = self.base.get(name, shape, kind, fan_in)
        terms = self.terms(name)
        if not terms:
            return w0
        return merge_f64(w0, terms).astype(np.float32)


ST = "unet/input_blocks/rt1/transformer"        # the first SpatialTransformer
TB = ST + "/transformer"


def arithmetic_targets(d) -> dict:
    """test 1: every target kind and the edge shapes of the merge kernel (Cc = 36; R = 4; ranks 1, 3, 4, 16, 33 -- 33 crosses the 16-column rank chunk twice)"""
    c, cd = d.model_channels, d.ctx_dim
    return {
        "unet/input_blocks/conv/weight": ((c, 4, 3, 3), 3),
        "unet/input_blocks/rt1/res/conv_in/weight": ((c, c, 3, 3), 16),
        ST + "/proj_in/weight": ((c, c, 1, 1), 4),
        TB + "/attn1/query/weight": ((c, c), 33),
        TB + "/attn1/key/weight": ((c, c), 1),
        TB + "/attn1/value/weight": ((c, c), 4),
        TB + "/attn2/key/weight": ((cd, c), 16),
        TB + "/mlp/geglu/proj/weight": ((c, 8 * c), 33),
        "unet/lin1_time_embed/weight": ((c, 4 * c), 3),
        "unet/conv_out/weight": ((4, c, 3, 3), 4),               # R = 4: a row count below (and no multiple of) the kernel's 32-row tile
    }


def repack_targets(d) -> dict:
    """test 2: attn1 query (pre_scale at precision >= 1) and value (packed q | k | v), attn2 key, a ResBlock 3x3 convolution (MXFP8 copy at precision 2), proj_out, and the 4-row conv_out"""
    c, cd = d.model_channels, d.ctx_dim
    return {
        TB + "/attn1/query/weight": ((c, c), 8),
        TB + "/attn1/value/weight": ((c, c), 3),
        TB + "/attn2/key/weight": ((cd, c), 4),
        "unet/input_blocks/rt1/res/conv_out/weight": ((c, c, 3, 3), 5),
        ST + "/proj_out/weight": ((c, c, 1, 1), 16),
        "unet/conv_out/weight": ((4, c, 3, 3), 3),                # R = 4: the merge kernel's row tail, seen through a forward pass
    }


def parity_targets(d) -> dict:
    """test 4: the attention projections, a ResBlock convolution and the 1x1 projections of the transformers at every resolution the data passes on the way down,
    the middle block, and the first and last output blocks -- enough of the model that a 10 % delta moves the output by far more than the parity bars"""
    c, cd = d.model_channels, d.ctx_dim
    out = {}
    for path, ch in (("unet/input_blocks/rt1", c), ("unet/input_blocks/rt3", 2 * c), ("unet/input_blocks/rt5", 4 * c), ("unet/output_blocks/rt1", 4 * c),
                     ("unet/output_blocks/rt7", c)):
        tb = path + "/transformer/transformer"
        out[tb + "/attn1/query/weight"] = ((ch, ch), 8)
        out[tb + "/attn1/key/weight"] = ((ch, ch), 8)
        out[tb + "/attn1/value/weight"] = ((ch, ch), 8)
        out[tb + "/attn1/out/weight"] = ((ch, ch), 8)
        out[tb + "/attn2/query/weight"] = ((ch, ch), 4)
        out[tb + "/attn2/key/weight"] = ((cd, ch), 4)
        out[tb + "/attn2/value/weight"] = ((cd, ch), 4)
        out[tb + "/mlp/lin/weight"] = ((4 * ch, ch), 4)
        out[path + "/transformer/proj_out/weight"] = ((ch, ch, 1, 1), 8)
        out[path + "/res/conv_out/weight"] = ((ch, ch, 3, 3), 4)
    tb = "unet/middle_block/transformer/transformer"
    out[tb + "/attn1/value/weight"] = ((4 * c, 4 * c), 8)
    out[tb + "/attn2/value/weight"] = ((cd, 4 * c), 8)
    out["unet/middle_block/res1/conv_in/weight"] = ((4 * c, 4 * c, 3, 3), 4)
    return out


PARITY_SEED, PARITY_SCALE = 11, 1.0
