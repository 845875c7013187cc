"""Reference side of the LoRA-file tests (DESIGN.md section 9c "files"): the kohya-ss module name of a CompVis key, restated in Python from the renaming table
of the diffusers conversion (never by calling the library); the LoHa delta in float64; the rounding bound of the device's LoHa merge; seeded kohya files.

Layouts as lora_ref: Linear weight [in, out], conv weight [cout, cin, k, k].  A LoHa module holds w1_a, w2_a [out, r] and w1_b, w2_b [r, in] (a conv's
[r, cin k k]); its delta is (w1_a . w1_b) o (w2_a . w2_b) in torch's [out, in] layout, so each pair is an (up, down) pair of lora_ref.delta_f64.
"""
import re

import numpy as np

import lora_ref as L

U = L.U

UNET_ROOT, TE_ROOT = "model.diffusion_model.", "cond_stage_model.transformer."
_RES = {"in_layers.2": "conv1", "emb_layers.1": "time_emb_proj", "out_layers.3": "conv2", "skip_connection": "conv_shortcut"}
_ATTN = re.compile(r"^(proj_in|proj_out|transformer_blocks\.0\.(attn[12]\.(to_[qkv]|to_out\.0)|ff\.net\.0\.proj|ff\.net\.2))$")
_TE = re.compile(r"^text_model\.encoder\.layers\.\d+\.(self_attn\.(q|k|v|out)_proj|mlp\.fc[12])$")


def diffusers_path(compvis: str):
    """CompVis module path of the SD v1 UNet (no root, no ".weight") -> diffusers module path; None for a module that is no conv / Linear layer.
    The table: 4 levels, 2 ResBlocks per level, input block 3 i + j + 1 = down_blocks.i.{resnets,attentions}.j, input block 3 i + 3 = the downsampler of
    level i, output block 3 i + j = up_blocks.i.{resnets,attentions}.j, the upsampler the last element of output block 3 i + 2."""
    fixed = {"input_blocks.0.0": "conv_in", "out.2": "conv_out", "time_embed.0": "time_embedding.linear_1", "time_embed.2": "time_embedding.linear_2"}
    if compvis in fixed:
        return fixed[compvis]
    m = re.match(r"^(input_blocks|output_blocks)\.(\d+)\.(\d+)\.(.+)$", compvis)
    if m:
        down, n, e, rest = m.group(1) == "input_blocks", int(m.group(2)), int(m.group(3)), m.group(4)
        if down:
            if not 1 <= n <= 11:
                return None
            i, j = divmod(n - 1, 3)
            if j == 2:
                return f"down_blocks.{i}.downsamplers.0.conv" if (e, rest) == (0, "op") else None
            level = f"down_blocks.{i}"
        else:
            if n > 11:
                return None
            i, j = divmod(n, 3)
            if rest == "conv":
                return f"up_blocks.{i}.upsamplers.0.conv" if j == 2 and i < 3 and e == (1 if i == 0 else 2) else None
            level = f"up_blocks.{i}"
        if e == 0 and rest in _RES:
            return f"{level}.resnets.{j}.{_RES[rest]}"
        has_attn = i < 3 if down else i > 0
        if e == 1 and has_attn and _ATTN.match(rest):
            return f"{level}.attentions.{j}.{rest}"
        return None
    m = re.match(r"^middle_block\.([012])\.(.+)$", compvis)
    if m:
        e, rest = int(m.group(1)), m.group(2)
        if e == 1:
            return f"mid_block.attentions.0.{rest}" if _ATTN.match(rest) else None
        return f"mid_block.resnets.{e // 2}.{_RES[rest]}" if rest in _RES else None
    return None


def module_names(checkpoint_key: str):
    """(kohya module name, CompVis-style module name) of the checkpoint key of a weight; None when it is no LoRA target"""
    if not checkpoint_key.endswith(".weight"):
        return None
    key = checkpoint_key[:-len(".weight")]
    if key.startswith(UNET_ROOT):
        path = key[len(UNET_ROOT):]
        d = diffusers_path(path)
        return None if d is None else ("lora_unet_" + d.replace(".", "_"), "lora_unet_" + path.replace(".", "_"))
    if key.startswith(TE_ROOT):
        path = key[len(TE_ROOT):]
        if not _TE.match(path):
            return None
        return ("lora_te_" + path.replace(".", "_"),) * 2
    return None


# names found in real files (the issue's anchors): kohya module name -> CompVis key
ANCHORS = {
    "lora_unet_down_blocks_0_attentions_0_transformer_blocks_0_attn1_to_q": "model.diffusion_model.input_blocks.1.1.transformer_blocks.0.attn1.to_q",
    "lora_unet_up_blocks_3_attentions_2_transformer_blocks_0_ff_net_0_proj": "model.diffusion_model.output_blocks.11.1.transformer_blocks.0.ff.net.0.proj",
    "lora_unet_up_blocks_1_attentions_0_transformer_blocks_0_attn2_to_out_0": "model.diffusion_model.output_blocks.3.1.transformer_blocks.0.attn2.to_out.0",
    "lora_unet_mid_block_attentions_0_proj_out": "model.diffusion_model.middle_block.1.proj_out",
    "lora_unet_down_blocks_1_resnets_0_conv_shortcut": "model.diffusion_model.input_blocks.4.0.skip_connection",
    "lora_unet_down_blocks_0_downsamplers_0_conv": "model.diffusion_model.input_blocks.3.0.op",
    "lora_unet_up_blocks_0_upsamplers_0_conv": "model.diffusion_model.output_blocks.2.1.conv",
    "lora_unet_up_blocks_2_upsamplers_0_conv": "model.diffusion_model.output_blocks.8.2.conv",
    "lora_unet_mid_block_resnets_1_conv2": "model.diffusion_model.middle_block.2.out_layers.3",
    "lora_unet_down_blocks_3_resnets_1_time_emb_proj": "model.diffusion_model.input_blocks.11.0.emb_layers.1",
    "lora_unet_time_embedding_linear_2": "model.diffusion_model.time_embed.2",
    "lora_te_text_model_encoder_layers_11_mlp_fc2": "cond_stage_model.transformer.text_model.encoder.layers.11.mlp.fc2",
}


def sd14_targets(golden_keys_path):
    """[(dump name, checkpoint key, dump shape)] of every conv / Linear weight of the full-size SD v1 model, from tests/golden/sd14_ckpt_keys.txt (which pins the
    dump name -> checkpoint key map against the reference's own Python side): 4-D weights, and 2-D ones the dump holds transposed (a Linear; an embedding is not)."""
    out = []
    for line in open(golden_keys_path).read().splitlines():
        name, key, shape, tr = line.split("\t")
        shape = tuple(int(v) for v in shape.split(","))
        if not name.endswith("/weight") or not (len(shape) == 4 or (len(shape) == 2 and tr == "T")):
            continue
        out.append((name, key, shape[::-1] if tr == "T" else shape))
    return out


# ---- LoHa ------------------------------------------------------------------------------------------------------------------------------------------
def loha_delta_f64(shape, w1_a, w1_b, w2_a, w2_b) -> np.ndarray:
    """(w1_a . w1_b) o (w2_a . w2_b) in the target's layout, float64"""
    r = np.asarray(w1_b).shape[0]
    return L.delta_f64(shape, np.asarray(w1_b).reshape(r, -1), w1_a) * L.delta_f64(shape, np.asarray(w2_b).reshape(r, -1), w2_a)


def _abs_products(shape, item):
    """per term: (rank, sum |.||.| weight of the bound) -- a plain term (down, up) or a LoHa term (w1_a, w1_b, w2_a, w2_b)"""
    if len(item) == 2:
        down, up = item
        return int(np.asarray(down).shape[0]), L.abs_delta_f64(shape, down, up), False
    w1_a, w1_b, w2_a, w2_b = (np.abs(np.asarray(w, np.float64)) for w in item)
    return int(w1_b.shape[0]), loha_delta_f64(shape, w1_a, w1_b, w2_a, w2_b), True


def merge_f64(w0, terms) -> np.ndarray:
    """W0 + sum c delta in float64; terms = [(factors, c)], factors = (down, up) or (w1_a, w1_b, w2_a, w2_b), c the f32 coefficient; zero coefficients skipped"""
    w = np.asarray(w0, np.float64).copy()
    for item, c in terms:
        if float(c) == 0.0:
            continue
        w += float(c) * (L.delta_f64(w0.shape, *item) if len(item) == 2 else loha_delta_f64(w0.shape, *item))
    return w


def merge_bound(w0, terms) -> np.ndarray:
    """Elementwise bound on |fp32 merge - merge_f64| for a list of plain and LoHa terms, derived from the kernel's order of operations (csrc/k_lora.hip), never measured.

    One element, T active terms, u = 2^-24, gamma_n ~ n u.  A rank-r product is an FMA chain of r roundings from 0: |d - D| <= gamma_r A with A = sum_j |p_j||q_j|, and
    |d| <= (1 + gamma_r) A.  A LoHa term multiplies two such chains and rounds once, h = d1 d2 (1 + delta):
        |h - D1 D2| <= |d1 - D1||d2| + |D1||d2 - D2| + u |d1 d2| <= (2 gamma_r + u) A1 A2 + O(u^2) = (2 r + 1) u A1 A2 + O(u^2).
    The T updates w = fma(c, x, w) round once each, so the sum over W0 and the T products carries gamma_T of its absolute terms on top:
        |w - W| <= gamma_T (|W0| + sum_t |c_t| |x_t|) + sum_t |c_t| |x_t - X_t|
                <= u [ (T + 2) |W0| + sum_plain (T + r_t + 2) |c_t| A_t + sum_loha (T + 2 r_t + 3) |c_t| A1_t A2_t ],
    the + 2 per term covering the second-order terms at these r and T (r <= 256, T <= 16: below 1e-4 of a first-order term each), as in lora_ref.merge_bound --
    to which this reduces, term by term not larger, when every term is plain.  For a single LoHa term of rank r: (2 r + 4) u |c| A1 A2 + 3 u |W0|."""
    active = [(item, c) for item, c in terms if float(c) != 0.0]
    T = len(active)
    bound = (T + 2) * np.abs(np.asarray(w0, np.float64))
    for item, c in active:
        r, mag, hada = _abs_products(w0.shape, item)
        bound = bound + (T + (2 * r + 3 if hada else r + 2)) * abs(float(c)) * mag
    return U * bound


def make_loha(targets, seed: int, rel: float = 0.1) -> dict:
    """{target: (w1_a, w1_b, w2_a, w2_b, alpha)} for targets = {name: (shape, rank)}: seeded normals of one sigma, chosen so that at scale 1 the delta's RMS is `rel` x
    the RMS of the synthetic W0 (RMS of a product of two independent rank-r products of sigma-normals: sigma^4 r); alpha = rank / 2.  w_b is 2-D: [r, in] / [r, cin k k]."""
    import zlib
    out = {}
    for name, (shape, rank) in targets.items():
        shape = tuple(int(v) for v in shape)
        fan_in = shape[1] * shape[2] * shape[3] if len(shape) == 4 else shape[0]
        n_out = shape[0] if len(shape) == 4 else shape[1]
        alpha = rank / 2.0
        sigma = (rel / np.sqrt(3.0 * fan_in) / (rank * alpha / rank)) ** 0.25
        g = np.random.default_rng([int(seed), zlib.crc32(name.encode("utf-8")), 7])
        w = [(sigma * g.standard_normal(s)).astype(np.float32) for s in ((n_out, rank), (rank, fan_in), (n_out, rank), (rank, fan_in))]
        out[name] = (w[0], w[1], w[2], w[3], float(alpha))
    return out


# ---- what a file of dtype F16 / BF16 holds: the factors rounded once, then widened exactly ------------------------------------------------------------
def stored(a, dtype: str) -> np.ndarray:
    from stable_diffusion_burn_amd import weights as W
    a = np.asarray(a, np.float32)
    if dtype == "F32":
        return a
    if dtype == "F16":
        return a.astype(np.float16).astype(np.float32)
    return W.bf16_to_f32(W.bf16_bits(a)).reshape(a.shape)


def stored_adapter(adapter: dict, dtype: str, alpha_dtype=None) -> dict:
    """the adapter a file of `dtype` written from `adapter` holds, host-widened: every factor and alpha rounded to dtype (alpha None stays None)"""
    alpha_dtype = alpha_dtype or dtype
    out = {}
    for name, item in adapter.items():
        alpha = item[-1]
        out[name] = tuple(stored(f, dtype) for f in item[:-1]) + (None if alpha is None else float(stored(np.float32(alpha), alpha_dtype)),)
    return out


def loha_terms(item, scale):
    """((w1_a, w1_b, w2_a, w2_b), c) of a LoHa item at `scale`"""
    return (tuple(item[:4]), L.coef(scale, item[4], np.asarray(item[1]).shape[0]))


def plain_terms(item, scale):
    down, up, alpha = item
    r = np.asarray(down).shape[0]
    return ((down, up), L.coef(scale, r if alpha is None else alpha, r))


class FileLoraProvider:
    """lora_ref.LoraProvider for adapters that mix plain and LoHa items: get() returns float32(merge_f64(W0, ...)) for their targets"""

    def __init__(self, base, adapters):
        self.base, self.adapters = base, list(adapters)   # [(tensors, scale)]

    def get(self, name, shape, kind, fan_in=0):
        w0 = self.base.get(name, shape, kind, fan_in)
        terms = [loha_terms(t[name], s) if len(t[name]) == 5 else plain_terms(t[name], s) for t, s in self.adapters if name in t]
        return merge_f64(w0, terms).astype(np.float32) if terms else w0
