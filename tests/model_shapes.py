"""The operator shapes one UNet forward and one VAE decode launch, as a function of the model's dimensions, the latent size and the batch -- TEST
INFRASTRUCTURE ONLY.  Written from the architecture in oracle/sd_oracle.py (Dims, UNetOracle.plan / forward, DecoderOracle.decode_latent); the engine
is not consulted.  tests/test_model_shapes_gpu.py pins the GEMM shapes below against the engine's own record (options record_shapes / dump_shapes) on
the half-width model at two latent sizes; the rule is parametric in Dims, so what matches there is the engine's rule at full width.

How the engine groups the reference's layers into launches, as far as the shapes show it (the same in all three precisions):
  * the self-attention's query / key / value projections are one Linear with 3 c outputs; the cross-attention's are three;
  * a GEGLU projection is one launch with `hidden` gated outputs (2 hidden weight rows);
  * the time-embedding Linears see one row (one timestep for the batch);
  * a ResBlock's 1x1 shortcut may ride on its second convolution's launch (conv_pairs), proj_out on the MLP's output Linear (linear_pairs); both are
    also listed as launches of their own, which is what runs where the pair is declined;
  * the VAE's single-head attention at precision 0 is two GEMMs per sample (scores, then probabilities x values) around a row softmax.
"""
from collections import namedtuple

Conv = namedtuple("Conv", "n cin h w cout k stride ups epi")          # epi: "" | "temb" (bias + time-embedding row) | "resid" (bias + residual)
Linear = namedtuple("Linear", "rows cin cout bias resid")
Geglu = namedtuple("Geglu", "rows cin hidden")
Attention = namedtuple("Attention", "n nq nk c heads")
GroupNorm = namedtuple("GroupNorm", "n c h w silu")
LayerNorm = namedtuple("LayerNorm", "rows c")
ConvPair = namedtuple("ConvPair", "n cin_x cout h w")                 # conv3x3(h [cout]) + conv1x1(x [cin_x]): a ResBlock's tail with a shortcut
LinearPair = namedtuple("LinearPair", "rows k_main k_aux cout")       # u [k_main] @ w + h [k_aux] @ w_aux + resid: the MLP's output Linear carrying proj_out


class Shapes:
    """the distinct items of each operator, in the order the model first meets them"""
    FIELDS = ("convs", "linears", "geglus", "attentions", "group_norms", "layer_norms", "conv_pairs", "linear_pairs")

    def __init__(self):
        for f in self.FIELDS:
            setattr(self, f, [])

    def add(self, item):
        lst = getattr(self, {Conv: "convs", Linear: "linears", Geglu: "geglus", Attention: "attentions", GroupNorm: "group_norms", LayerNorm: "layer_norms",
                             ConvPair: "conv_pairs", LinearPair: "linear_pairs"}[type(item)])
        if item not in lst:
            lst.append(item)

    def merge(self, other):
        for f in self.FIELDS:
            for item in getattr(other, f):
                self.add(item)
        return self

    def shortcut_keys(self):
        """The GEMM keys a paired launch removes from the engine's record.  conv_pairs: the 1x1 shortcut (it rides on the second convolution's launch, whose
        own key stays).  linear_pairs: the MLP's output Linear (rows, 4 c, c) -- the folded launch is recorded by the pair planner, not by launch_gemm, while
        proj_out's key equals proj_in's and is therefore always seen.  A key listed here may be absent; every other key of the rule must be present."""
        keys = {gemm_key(Conv(p.n, p.cin_x, p.h, p.w, p.cout, 1, 1, 0, "")) for p in self.conv_pairs}
        return keys | {gemm_key(Linear(p.rows, p.k_main, p.cout, True, True)) for p in self.linear_pairs}

    def gemm_keys(self, unfused_attention=True):
        """the engine's dump_shapes keys NB,Cin,Hs,Ws,N,KH,stride,ups of every GEMM; unfused_attention: the two GEMMs of single-head attention too"""
        keys = {gemm_key(i) for f in ("convs", "linears", "geglus") for i in getattr(self, f)}
        if unfused_attention:
            for a in self.attentions:
                if a.heads == 1:
                    keys |= {f"1,{a.c},1,{a.nq},{a.nk},1,1,0", f"1,{a.nk},1,{a.nq},{a.c},1,1,0"}
        return keys


def against_record(rule, seen):
    """(extra, missing): the engine's recorded GEMM keys (option dump_shapes) the rule does not name, and the GEMMs the rule names that were not launched.
    Exactly two kinds of launch are excused, so the pin is "equal up to these": (1) the keys of shortcut_keys(), absent where the engine took the pair;
    (2) a GEGLU projection the engine ran unfused (few rows), which it records with N = 2 hidden instead of N = hidden -- either key is accepted, one of the
    two must be there."""
    keys = rule.gemm_keys()
    unfused = {gemm_key(g): gemm_key(g._replace(hidden=2 * g.hidden)) for g in rule.geglus}
    extra = set(seen) - keys - set(unfused.values())
    missing = {k for k in keys - set(seen) if k not in rule.shortcut_keys() and unfused.get(k) not in seen}
    return extra, missing


def arrives_as_planes(item, dims):
    """Does the fp32 model hand this GEMM its activations as three bf16 planes (so that the planner chooses among the plane tiles, cfg 300 ...)?  The engine's rule
    is Engine::plane_gemm -- in_features a multiple of 32, at least 32 outputs -- wherever the producer of the tensor writes planes.  The producers that do not:
    the time embedding (one row), the prompt context (attn2's key / value Linears) and the VAE attention block's GroupNorm (its q / k / v / proj_out 1x1
    convolutions at 4 vae_ch channels).  tests/test_model_shapes_gpu.py pins this against the tile families the half-width model's launches took."""
    if isinstance(item, Conv):
        if item.cin % 32 or item.cout < 32:
            return False
        return not (item.n == 1 and item.k == 1 and item.cin == item.cout == 4 * dims.vae_ch)
    if isinstance(item, Linear):
        return item.cin % 32 == 0 and item.cout >= 32 and item.rows > 1 and item.cin != dims.ctx_dim
    if isinstance(item, Geglu):
        return item.cin % 32 == 0
    raise TypeError(item)


def choice_key(item):
    """the 'M,N,K k<KH> s<stride> u<ups> W<width>' head of the engine's dump_choices line of a GEMM"""
    if isinstance(item, Conv):
        pad = 1 if item.k == 3 else 0
        ho = ((item.h << item.ups) + 2 * pad - item.k) // item.stride + 1
        wo = ((item.w << item.ups) + 2 * pad - item.k) // item.stride + 1
        return f"{item.n * ho * wo},{item.cout},{item.cin * item.k * item.k} k{item.k} s{item.stride} u{item.ups} W{item.w}"
    if isinstance(item, Linear):
        return f"{item.rows},{item.cout},{item.cin} k1 s1 u0 W{item.rows}"
    if isinstance(item, Geglu):
        return f"{item.rows},{item.hidden},{item.cin} k1 s1 u0 W{item.rows}"
    raise TypeError(item)


def gemm_key(item):
    if isinstance(item, Conv):
        return f"{item.n},{item.cin},{item.h},{item.w},{item.cout},{item.k},{item.stride},{item.ups}"
    if isinstance(item, Linear):
        return f"1,{item.cin},1,{item.rows},{item.cout},1,1,0"
    if isinstance(item, Geglu):
        return f"1,{item.cin},1,{item.rows},{item.hidden},1,1,0"
    raise TypeError(item)


def level_sizes(h, w, levels=4):
    """the (h, w) of the UNet's levels: each Downsample is a 3x3 convolution of stride 2 and padding 1"""
    out = [(h, w)]
    for _ in range(levels - 1):
        h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        out.append((h, w))
    return out


# ---- UNet (unet/mod.rs:36-143) --------------------------------------------------------------------------------------------------------------------------
def _res_block(s, dims, n, cin, cout, h, w):
    """ResBlock::forward unet/mod.rs:713-733"""
    s.add(GroupNorm(n, cin, h, w, True))
    s.add(Conv(n, cin, h, w, cout, 3, 1, 0, "temb"))
    s.add(Linear(1, dims.emb_dim, cout, True, False))         # lin_embed on silu(emb)
    s.add(GroupNorm(n, cout, h, w, True))
    s.add(Conv(n, cout, h, w, cout, 3, 1, 0, "resid"))
    if cin != cout:
        s.add(Conv(n, cin, h, w, cout, 1, 1, 0, ""))            # skip_connection
        s.add(ConvPair(n, cin, cout, h, w))


def _transformer(s, dims, n, c, h, w, ctx_rows, ctx_len):
    """SpatialTransformer::forward unet/mod.rs:462-480 around TransformerBlock (:522-526), MultiHeadAttention (:642-652) and the GEGLU MLP (:552-591)"""
    rows = n * h * w
    s.add(GroupNorm(n, c, h, w, False))
    s.add(Conv(n, c, h, w, c, 1, 1, 0, ""))                     # proj_in
    s.add(LayerNorm(rows, c))
    s.add(Linear(rows, c, 3 * c, False, False))                 # attn1: query | key | value
    s.add(Attention(n, h * w, h * w, c, dims.n_head))
    s.add(Linear(rows, c, c, True, True))                       # attn1 / attn2 out, + x
    s.add(Linear(rows, c, c, False, False))                     # attn2 query
    s.add(Linear(ctx_rows, dims.ctx_dim, c, False, False))      # attn2 key, value
    s.add(Attention(n, h * w, ctx_len, c, dims.n_head))
    s.add(Geglu(rows, c, 4 * c))
    s.add(Linear(rows, 4 * c, c, True, True))                   # mlp lin, + x
    s.add(Conv(n, c, h, w, c, 1, 1, 0, "resid"))                # proj_out, + x_in
    s.add(LinearPair(rows, 4 * c, c, c))


def unet_shapes(dims, h, w, n, ctx_len=77, ctx_rows=None, levels=None):
    """One UNet::forward on n latents of h x w.  ctx_len: the longest context's token count; ctx_rows: the context rows of the whole batch (default
    n ctx_len).  levels: the subset of level indices (0 = the latent's size ... 3) to return, default all; the items that belong to no level (the
    time embedding) come with level 0."""
    mc = dims.model_channels
    c = [mc, 2 * mc, 4 * mc, 4 * mc]
    ctx_rows = n * ctx_len if ctx_rows is None else ctx_rows
    size = level_sizes(h, w)
    per = [Shapes() for _ in range(4)]

    def block(kind, lv, cin, cout):
        s = per[lv]
        hh, ww = size[lv]
        if kind == "conv":
            s.add(Conv(n, cin, hh, ww, cout, 3, 1, 0, ""))
            return lv
        if kind == "down":
            s.add(Conv(n, cin, hh, ww, cin, 3, 2, 0, ""))
            return lv + 1
        _res_block(s, dims, n, cin, cout, hh, ww)
        if kind in ("rt", "rtu"):
            _transformer(s, dims, n, cout, hh, ww, ctx_rows, ctx_len)
        if kind in ("ru", "rtu"):
            s.add(Conv(n, cout, hh, ww, cout, 3, 1, 1, ""))     # Upsample: nearest-2x in front of the convolution (h, w: the source's)
            return lv - 1
        return lv

    per[0].add(Linear(1, mc, dims.emb_dim, True, False))
    per[0].add(Linear(1, dims.emb_dim, dims.emb_dim, True, False))
    # input blocks, unet/mod.rs:36-92 (UNetOracle.plan)
    lv = 0
    skips = []
    for kind, cin, cout in [("conv", 4, c[0]), ("rt", c[0], c[0]), ("rt", c[0], c[0]), ("down", c[0], c[0]), ("rt", c[0], c[1]), ("rt", c[1], c[1]), ("down", c[1], c[1]),
                            ("rt", c[1], c[2]), ("rt", c[2], c[2]), ("down", c[2], c[2]), ("r", c[2], c[2]), ("r", c[2], c[2])]:
        lv = block(kind, lv, cin, cout)
        skips.append(cin if kind == "down" else cout)
    block("r", 3, c[3], c[3])                                    # middle: ResTransformerRes
    _transformer(per[3], dims, n, c[3], *size[3], ctx_rows, ctx_len)
    cur = c[3]
    for kind, cout in [("r", c[2]), ("r", c[2]), ("ru", c[2]), ("rt", c[2]), ("rt", c[2]), ("rtu", c[2]), ("rt", c[1]), ("rt", c[1]), ("rtu", c[1]), ("rt", c[0]), ("rt", c[0]),
                       ("rt", c[0])]:
        lv = block(kind, lv, cur + skips.pop(), cout)
        cur = cout
    assert lv == 0 and not skips
    per[0].add(GroupNorm(n, mc, h, w, True))
    per[0].add(Conv(n, mc, h, w, 4, 3, 1, 0, ""))
    out = Shapes()
    for i in (range(4) if levels is None else levels):
        out.merge(per[i])
    return out


# ---- VAE decoder (autoencoder/mod.rs:205-217) -----------------------------------------------------------------------------------------------------------------
def _resnet_block(s, n, cin, cout, h, w):
    """ResnetBlock::forward autoencoder/mod.rs:514-527"""
    s.add(GroupNorm(n, cin, h, w, True))
    s.add(Conv(n, cin, h, w, cout, 3, 1, 0, ""))
    s.add(GroupNorm(n, cout, h, w, True))
    s.add(Conv(n, cout, h, w, cout, 3, 1, 0, "resid"))
    if cin != cout:
        s.add(Conv(n, cin, h, w, cout, 1, 1, 0, ""))            # nin_shortcut
        s.add(ConvPair(n, cin, cout, h, w))


def decoder_shapes(dims, h, w, n=1, levels=None):
    """Decoder::forward on n latents of h x w (the engine decodes one sample per launch: n = 1).  levels: 0 = the latent's size (with the middle block and
    the heads in front of it) ... 3 = eight times that (with norm_out / conv_out)."""
    c = dims.vae_ch
    chans = [(4 * c, 4 * c), (4 * c, 4 * c), (4 * c, 2 * c), (2 * c, c)]
    per = [Shapes() for _ in range(4)]
    s = per[0]
    c0 = chans[0][0]
    s.add(Conv(n, 4, h, w, 4, 1, 1, 0, ""))                     # post_quant_conv
    s.add(Conv(n, 4, h, w, c0, 3, 1, 0, ""))                    # conv_in
    _resnet_block(s, n, c0, c0, h, w)
    s.add(GroupNorm(n, c0, h, w, False))                        # ConvSelfAttentionBlock :563-607
    s.add(Conv(n, c0, h, w, c0, 1, 1, 0, ""))                   # q, k, v
    s.add(Attention(n, h * w, h * w, c0, 1))
    s.add(Conv(n, c0, h, w, c0, 1, 1, 0, "resid"))              # proj_out, + x
    _resnet_block(s, n, c0, c0, h, w)
    for i, (cin, cout) in enumerate(chans):
        hh, ww = h << i, w << i
        for j in range(3):
            _resnet_block(per[i], n, cin if j == 0 else cout, cout, hh, ww)
        if i != len(chans) - 1:
            per[i].add(Conv(n, cout, hh, ww, cout, 3, 1, 1, ""))     # upsampler
    per[3].add(GroupNorm(n, c, h << 3, w << 3, True))
    per[3].add(Conv(n, c, h << 3, w << 3, 3, 3, 1, 0, ""))
    out = Shapes()
    for i in (range(4) if levels is None else levels):
        out.merge(per[i])
    return out
