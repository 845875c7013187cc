"""Operator parity at the full-width shapes of picture sizes other than 512 x 512, with the plan left to the engine.

set_latent_size and the hires pass make every latent size that is a multiple of 8 a workload, and the GEMM tile tables are tuned for 64 x 64 only:
other sizes run on the planner's fallbacks (the cost-model tile, the split-K count, the kernel-row upgrade, the resid_acc gates, the MXFP8 split, paired
launches without a row in the pairs table) and on attention grids of other sizes.  Here every distinct operator shape of the full-width model
(Dims(320, 8, 768, ...)) is run through the operator entry points of one operator-only context per precision, with gemm_tile, splitk and
attn_kv_splits automatic -- and, at precision 0, with the activations handed over as the model hands them: as three bf16 planes wherever its producers
write planes (M.arrives_as_planes; op_conv2d_view with in_planes = 3, geglu_fuse = 8), so that the planner takes the branch it takes in the model
(plane_choice: the plane tiles, cfg 300 ...) and not the fp32-input branch of op_conv2d / op_linear:

  * a 72 x 88 latent at batch 2 (one CFG step of one image: M = 6336 n, 1584 n, 396 n, 99 n -- no level a multiple of a 256-row tile): every UNet
    level and every level of the VAE decoder (which the engine runs one sample per launch: n = 1);
  * a 128 x 128 latent at batch 2: the two largest UNet levels (M = 32768, 8192) and the decoder's two largest (512 x 512, 1024 x 1024).

The shapes come from tests/model_shapes.py, pinned below against the engine's own record on the half-width model at two sizes.  For each shape:
 (a) the result against the fp64 reference at the sampled outputs of tests/sampled_ref.py, at the operator bars of the neighbouring modules:
     2e-5 max(1, |ref|) at precision 0, 2^-8 max(1, |ref|) for bf16 / MXFP8 outputs, 2e-4 for the fp32 heads of the bf16 engine, 2^-7 for bf16
     attention and 2^-6 on its single-head path; inputs as those modules draw them (unit-scale x, weights / sqrt(K), rounded to bf16 or put on
     the MX grid on the host);
 (b) the same call with the plainest kernel forced (GEMM: the 128 x 128 four-wave tile without split-K, no plane / split / large-tile family at
     precision 0; attention: no key slices, attn_split = 0, attn_bf16 = 0): the two results at EVERY element within twice the bar -- both are
     within one bar of the truth, and this reaches the outputs the sample leaves out -- and the forced one through (a) as well; where the automatic
     launch took a kernel-row tile (104 / 105), the plain tile it replaces (100 / 101) must give the same bits;
 (c) the plan the automatic call took (option dump_choices; attention: the profile tag's slice count), printed with the test id and gathered in
     profiles/model_shapes_plan.txt (written when SDMI_MODEL_SHAPES_PLAN names a file).

Large activations are a seeded block of 4099 pixels repeated along the pixel axis (each sample from its own offset): drawing 10^8 normals per test
would cost more than everything else here.  4099 is prime, so no tile, row or image stride is a multiple of the period, and a read from a wrong pixel,
row, sample or channel sees a different value.  Tensors up to 2 M elements are drawn in full.

The last section places operands around the 32-bit lines: 2 GiB is the smallest tensor at which a signed 32-bit byte offset wraps, 4 GiB is the
engine's stated limit for a GEMM operand.
"""
import functools
import math
import os
import time
import zlib

import numpy as np
import pytest
import torch

import model_shapes as M
import sampled_ref as S
from oracle import mx_oracle as MX
from oracle import sd_oracle as O

pytestmark = pytest.mark.gpu

FP32_BAR, BF16_BAR, HEAD_BAR, ATTN16_BAR, ATTN16_1HEAD_BAR = 2e-5, 2 ** -8, 2e-4, 2 ** -7, 2 ** -6
DIMS = O.Dims(320, 8, 768, 64, 64, 128)
SIZE_A, SIZE_B = (72, 88), (128, 128)
PERIOD = 4099            # pixels / rows of the repeated block (prime)
FULL_DRAW = 2 << 20      # tensors up to this many elements are drawn in full

_DEFAULTS = {"gemm_tile": "auto", "splitk": 0, "gemm_planes": "default", "gemm_f32s": 1, "gemm_x32": 1, "fp8_tile": "auto", "attn_kv_splits": 0, "attn_split": 1,
             "attn_bf16": 1, "skip_slices": 1, "proj_out_fold": 2}
# the plainest kernel of each route
PLAIN_GEMM = {0: {"gemm_tile": 0, "splitk": 1, "gemm_planes": 0, "gemm_f32s": 0, "gemm_x32": 0}, 1: {"gemm_tile": 0, "splitk": 1}, 2: {"gemm_tile": 0, "splitk": 1}}
PLAIN_FP8 = {"fp8_tile": 0, "splitk": 1}
PLAIN_ATTN = {"attn_kv_splits": 1, "attn_split": 0, "attn_bf16": 0}       # (attn_kv_splits: 0 is the automatic rule, 1 is "never")
FAMILY = {0: "4-wave", 1: "large", 2: "split", 3: "planes"}


# ---- the shapes ---------------------------------------------------------------------------------------------------------------------------------------------
def _model_shapes():
    s = M.Shapes()
    s.merge(M.unet_shapes(DIMS, *SIZE_A, 2)).merge(M.decoder_shapes(DIMS, *SIZE_A, 1))
    s.merge(M.unet_shapes(DIMS, *SIZE_B, 2, levels=(0, 1))).merge(M.decoder_shapes(DIMS, *SIZE_B, 1, levels=(2, 3)))
    return s


SHAPES = _model_shapes()


def _is_fp8_conv(c):
    """the ResBlock / ResnetBlock 3x3 convolutions: what precision 2 runs on MXFP8 operands"""
    return c.k == 3 and c.stride == 1 and c.ups == 0 and c.cin % 32 == 0 and c.cout % 32 == 0


def _is_head(c):
    return c.cin < 32 or c.cout <= 4


def _by_weight(items, key):
    return sorted(items, key=key)        # neighbours share their cached weight


CONV_PARAMS = [(p, c) for p in (0, 1, 2) for c in _by_weight(SHAPES.convs, lambda c: (c.cin, c.cout, c.k)) if p < 2 or _is_fp8_conv(c) or _is_head(c)]
LINEAR_PARAMS = [(p, li) for p in (0, 1) for li in _by_weight(SHAPES.linears, lambda li: (li.cin, li.cout))]
GEGLU_PARAMS = [(p, g) for p in (0, 1) for g in SHAPES.geglus]
# beyond the two sizes: cross-attention over a two-chunk prompt, the VAE's single-head path at 16384 tokens (self-attention 16384 x 16384 at d = 40
# and cross-attention from 16384 queries are the 128 x 128 latent's own, the single-head path at 6336 tokens the 72 x 88 decoder's)
ATTENTIONS = SHAPES.attentions + [M.Attention(2, 6336, 154, 320, 8), M.Attention(1, 16384, 16384, 512, 1)]
SELF_16384 = M.Attention(2, 16384, 16384, 320, 8)
# (precision 0's 16384 x 16384 case last: the test behind it shares its operands and reference)
ATTN_PARAMS = [(1, a) for a in ATTENTIONS] + [(0, a) for a in ATTENTIONS if a != SELF_16384] + [(0, SELF_16384)]
assert SELF_16384 in ATTENTIONS
GROUP_NORMS = list(SHAPES.group_norms)
for _gn in (M.GroupNorm(1, 128, 1024, 1024, False), M.GroupNorm(1, 128, 1024, 1024, True), M.GroupNorm(1, 256, 512, 512, False), M.GroupNorm(1, 256, 512, 512, True)):
    if _gn not in GROUP_NORMS:
        GROUP_NORMS.append(_gn)
GN_PARAMS = [(p, g) for p in (0, 1) for g in GROUP_NORMS]
LN_PARAMS = [(p, ln) for p in (0, 1) for ln in SHAPES.layer_norms]


def _id(v):
    if isinstance(v, tuple) and isinstance(v[0], int) and hasattr(v[1], "_fields"):
        return f"p{v[0]}-{type(v[1]).__name__}-" + "-".join(str(x) if x != "" else "plain" for x in v[1])
    return None


# ---- contexts ---------------------------------------------------------------------------------------------------------------------------------------------------
class _Engines:
    def __init__(self):
        self._sd = {}

    def __call__(self, precision):
        if precision not in self._sd:
            from stable_diffusion_burn_amd import ModelConfig, StableDiffusion
            self._sd[precision] = StableDiffusion(ModelConfig(64, 1, 64, 8, 8, 64, precision=precision))
        return self._sd[precision]

    def close(self):
        for sd in self._sd.values():
            sd.close()
        self._sd.clear()


@pytest.fixture(scope="module")
def engines():
    """one operator-only context per precision, made at first use and closed with the module"""
    e = _Engines()
    yield e
    e.close()


# ---- operands ------------------------------------------------------------------------------------------------------------------------------------------------------
def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double()


def bf16_round(a):
    """round to nearest even onto bf16, kept as fp32 (finite inputs); 32-bit arithmetic so that a 10^9-element tensor needs no 64-bit temporary"""
    u = np.array(a, dtype=np.float32, order="C", copy=True).view(np.uint32)
    u += np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))
    u &= np.uint32(0xFFFF0000)
    return u.view(np.float32)


def _seed(*what):
    return zlib.crc32(repr(what).encode())


def _grid(a, fmt, axis):
    """a on the grid of its storage type: 'f32' as it is, 'bf16' rounded, 'mx' MXFP8 blocks of 32 along `axis` (as tests/test_fp8_gpu.py prepares them)"""
    if fmt == "bf16":
        return bf16_round(a)
    if fmt == "mx":
        return MX.mx_quantize(_t(a), axis).numpy().astype(np.float32)
    return np.ascontiguousarray(a, dtype=np.float32)


def _repeat_cols(block, length, offset):
    """[c, length]: the columns offset, offset + 1, ... of `block` [c, period] repeated for ever"""
    c, period = block.shape
    out = np.empty((c, length), dtype=np.float32)
    pos, src = 0, offset % period
    while pos < length:
        take = min(period - src, length - pos)
        out[:, pos:pos + take] = block[:, src:src + take]
        pos, src = pos + take, 0
    return out


def _acts(n, c, h, w, fmt, seed, scale=1.0, zeros=False):
    """[n, c, h, w] unit-scale activations on the grid of fmt (MX blocks: 32 channels of a pixel)"""
    if zeros:
        return np.zeros((n, c, h, w), dtype=np.float32)
    g = np.random.default_rng(seed)
    hw = h * w
    if n * c * hw <= FULL_DRAW or n * hw <= 2 * PERIOD:
        return _grid(g.standard_normal((n, c, h, w), dtype=np.float32) * np.float32(scale), fmt, 1)
    block = _grid(g.standard_normal((c, PERIOD), dtype=np.float32) * np.float32(scale), fmt, 0)
    return np.stack([_repeat_cols(block, hw, 1237 * s) for s in range(n)]).reshape(n, c, h, w)


def _rows(rows, c, fmt, seed, zeros=False):
    """[rows, c] unit-scale activations (MX blocks: 32 channels of a row)"""
    if zeros:
        return np.zeros((rows, c), dtype=np.float32)
    g = np.random.default_rng(seed)
    if rows * c <= FULL_DRAW or rows <= 2 * PERIOD:
        return _grid(g.standard_normal((rows, c), dtype=np.float32), fmt, 1)
    block = _grid(g.standard_normal((PERIOD, c), dtype=np.float32), fmt, 1)
    return np.ascontiguousarray(np.resize(block, (rows, c)))      # whole rows of the block, repeated


W_PERIOD = 32 * 31253     # elements of the repeated weight block: whole MX groups of 32 times a prime, so no two output channels share a row


def _weights(shape, fan_in, fmt, seed):
    """unit-scale weights / sqrt(fan_in) of `shape` whose LAST axis is the input channels (MX groups: 32 of them), on the grid of fmt.  Large tensors repeat
    a seeded block of W_PERIOD elements: every group of 32 input channels is a whole group of the block, and rows that are a period apart do not exist
    (9 cin d = 32 x 31253 t has no solution with d below 31253 rows)."""
    g = np.random.default_rng(seed)
    size = int(np.prod(shape))
    scale = np.float32(1.0 / math.sqrt(fan_in))
    if size <= 2 * W_PERIOD or shape[-1] % 32:
        return _grid(g.standard_normal(shape, dtype=np.float32) * scale, fmt, len(shape) - 1)
    block = _grid((g.standard_normal(W_PERIOD, dtype=np.float32) * scale).reshape(-1, 32), fmt, 1).reshape(-1)
    return np.resize(block, size).reshape(shape)


@functools.lru_cache(maxsize=3)
def _conv_weight(cout, cin, k, fmt):
    """[cout, cin, k, k] and its bias"""
    w = _weights((cout, k, k, cin), cin * k * k, fmt, _seed("conv weight", cout, cin, k))
    b = np.random.default_rng(_seed("conv bias", cout, cin, k)).standard_normal(cout).astype(np.float32)
    return np.ascontiguousarray(w.transpose(0, 3, 1, 2)), b


@functools.lru_cache(maxsize=3)
def _linear_weight(cin, cout, fmt):
    """[cin, cout] (the reference's layout) and its bias"""
    w = _weights((cout, cin), cin, fmt, _seed("linear weight", cin, cout))
    b = np.random.default_rng(_seed("linear bias", cin, cout)).standard_normal(cout).astype(np.float32)
    return np.ascontiguousarray(w.T), b


# ---- running, reading the plan back, checking -------------------------------------------------------------------------------------------------------------------------
PLAN = {}        # (precision, item) -> the automatic plan's lines, for the table


def _run(sd, tmp_path, fn, attention=False, **opts):
    """fn() under the given engine options (restored afterwards) -> (result, the launches it made: dump_choices lines, and for attention the profile tags
    'attention n.. nq.. nk.. h.. d.. slices=S')"""
    path, tags = tmp_path / "choices.txt", tmp_path / "tags.txt"
    try:
        for k, v in opts.items():
            sd.set_option(k, v)
        sd.set_option("record_shapes", 1)
        if attention:
            sd.set_option("profile", 2)
        out = fn()
        sd.set_option("dump_choices", str(path))
        lines = path.read_text().splitlines()
        if attention:
            sd.set_option("dump_profile_tags", str(tags))
            lines += [ln.split("\t", 1)[1] for ln in tags.read_text().splitlines() if "\tattention " in ln]
    finally:
        sd.set_option("record_shapes", 0)
        if attention:
            sd.set_option("profile", 0)
            sd.set_option("profile_reset", 1)
        for k in opts:
            sd.set_option(k, _DEFAULTS[k])
    return out, lines


def _field(line, name):
    for tok in line.split():
        if tok.startswith(name + "="):
            return int(tok.split("=")[1])
    return None


def _family(line):
    if line.startswith("attention "):
        return "attention"
    if " fp8 " in line:
        return "fp8"
    return FAMILY[min(_field(line, "cfg") // 100, 3)]


def _note_plan(request, precision, item, lines):
    PLAN[(precision, item)] = list(lines)
    print(f"\n{request.node.name}: " + " | ".join(lines))


def _check(got, ref, what, rel, scale=None):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, f"{what}: shape {got.shape} vs {ref.shape}"
    assert np.isfinite(got).all(), f"{what}: non-finite output"
    err = np.abs(got - ref)
    bound = rel * max(1.0, float(np.abs(ref).max()) if scale is None else scale)
    idx = np.unravel_index(int(err.argmax()), err.shape)
    assert err.max() <= bound, f"{what}: max|d|={err.max():.3e} > {bound:.3e} at sampled position {idx} (got {got[idx]:.6f}, ref {ref[idx]:.6f})"


def _max_diff(a, b):
    """max |a - b| over every element, in pieces (no temporary of the tensors' size)"""
    a, b = a.reshape(-1), b.reshape(-1)
    worst, step = 0.0, 1 << 25
    for i in range(0, a.size, step):
        d = float(np.abs(a[i:i + step] - b[i:i + step]).max())      # (a NaN or an infinity anywhere comes out of max)
        assert math.isfinite(d), "non-finite output"
        worst = max(worst, d)
    return worst


def _check_everywhere(auto, plain, ref, what, rel):
    """both results are within one bar of the truth, so within two of each other -- at every element, not only the sampled ones"""
    bound = 2 * rel * max(1.0, float(np.abs(ref).max()))
    d = _max_diff(auto, plain)
    assert d <= bound, f"{what}: automatic and plain kernel differ by {d:.3e} > {bound:.3e} somewhere"


def _fmt(precision, fp8=False):
    return "f32" if precision == 0 else "mx" if fp8 else "bf16"


# ---- 1. the shape rule is the engine's ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(16, 16), (8, 24)])
def test_shape_rule_matches_the_engine(sd_tiny, tiny_dims, tmp_path, size):
    """tests/model_shapes.py against what the half-width model launches (options record_shapes / dump_shapes: keys NB,Cin,Hs,Ws,N,KH,stride,ups): one UNet
    forward at batch 2 and one decode, at the model's own 16 x 16 latent and at 8 x 24 after set_latent_size.  Every launch must be one the rule names; every GEMM
    the rule names must be launched, except a shortcut / proj_out that rode on its neighbour's launch (conv_pairs / linear_pairs: absent from the record where the
    pair was taken) and a GEGLU projection that ran unfused (then recorded with its 2 hidden weight rows)."""
    from stable_diffusion_burn_amd import synthetic as syn
    h, w = size
    sd = sd_tiny
    lat = np.stack([syn.initial_latent(i, h, w) for i in range(2)])
    ctx = np.stack([syn.cond_context(i, 77, tiny_dims.ctx_dim) for i in range(2)])
    try:
        sd.set_latent_size(h, w)
        seen, choices = {}, {}
        for part, fn in (("unet", lambda: sd.unet.forward(lat, [999], ctx)), ("vae", lambda: sd.latent_to_image(lat))):
            sd.set_option("record_shapes", 1)
            fn()
            sd.set_option("dump_shapes", str(tmp_path / f"{part}.txt"))
            sd.set_option("dump_choices", str(tmp_path / f"{part}.choices.txt"))
            sd.set_option("record_shapes", 0)
            seen[part] = {ln.split()[0] for ln in (tmp_path / f"{part}.txt").read_text().splitlines()}
            choices[part] = (tmp_path / f"{part}.choices.txt").read_text().splitlines()
    finally:
        sd.set_option("record_shapes", 0)
        sd.set_latent_size(tiny_dims.latent_h, tiny_dims.latent_w)
    for part, rule in (("unet", M.unet_shapes(tiny_dims, h, w, 2)), ("vae", M.decoder_shapes(tiny_dims, h, w, 1))):
        extra, missing = M.against_record(rule, seen[part])
        assert not extra, f"{part} at {size}: the engine launched GEMMs the rule does not name: {sorted(extra)}"
        assert not missing, f"{part} at {size}: the rule names GEMMs the engine did not launch: {sorted(missing)}"
        assert len(seen[part]) > 10
        # which launches get their activations as planes (M.arrives_as_planes): a plane tile (cfg 300 ...) there, and nowhere else
        want = {}
        for item in rule.convs + rule.linears + rule.geglus:
            want.setdefault(M.choice_key(item), set()).add(M.arrives_as_planes(item, tiny_dims))
        checked = 0
        for ln in choices[part]:
            head = " ".join(ln.split()[:5])
            if head in want and "(no planes)" not in ln:
                assert want[head] == {_field(ln, "cfg") >= 300}, f"{part} at {size}: planes expected {want[head]}: {ln}"
                checked += 1
        assert checked > 10


# ---- 2. convolutions ---------------------------------------------------------------------------------------------------------------------------------------------------
def _conv_operands(precision, c, zeros=False):
    fp8 = precision == 2 and _is_fp8_conv(c)
    fmt = _fmt(precision, fp8)
    x = _acts(c.n, c.cin, c.h, c.w, fmt, _seed("conv x", c, precision), 1.5 if fp8 else 1.0, zeros)
    wt, b = _conv_weight(c.cout, c.cin, c.k, fmt)
    ho, wo = S.out_hw(c.h, c.w, c.k, c.stride, c.ups)
    g = np.random.default_rng(_seed("conv epilogue", c))
    temb = g.standard_normal(c.cout).astype(np.float32) if c.epi == "temb" else None       # one row for the batch: one timestep
    resid = _acts(c.n, c.cout, ho, wo, "f32" if precision == 0 else "bf16", _seed("conv resid", c), 1.0, zeros) if c.epi == "resid" else None
    return x, wt, b, temb, resid


def _conv_call(sd, c, ops):
    x, wt, b, temb, resid = ops
    if temb is None and resid is None:
        return sd.op_conv2d(x, wt, b, stride=c.stride, upsample2x=bool(c.ups))
    return sd.op_conv2d_epilogue(x, wt, b, temb, resid, stride=c.stride, upsample2x=bool(c.ups))


def _nchw(rows, n, ho, wo):
    """[n ho wo, c] NHWC rows -> [n, c, ho, wo]"""
    t = torch.from_numpy(rows).view(n, ho, wo, rows.shape[1]).permute(0, 3, 1, 2).contiguous()
    return t.numpy()


def _conv_auto(sd, precision, c, ops):
    """The call whose plan is the model's.  At precision 0 the model hands a plane-eligible layer its activations as three bf16 planes (M.arrives_as_planes), and the
    planner then chooses among the plane tiles only; op_conv2d would hand it fp32 and get a plan the model never runs.  op_conv2d_view with in_planes = 3 builds the
    input as the UNet does (fp32 + planes) and writes a dense parent."""
    if precision == 0 and M.arrives_as_planes(c, DIMS):
        x, wt, b, temb, resid = ops
        ho, wo = S.out_hw(c.h, c.w, c.k, c.stride, c.ups)
        parent = np.zeros((c.n * ho * wo, c.cout), dtype=np.float32)
        rows = sd.op_conv2d_view(x, wt, b, temb, resid, stride=c.stride, upsample2x=bool(c.ups), parent=parent, out_off=0, in_planes=3)
        return _nchw(rows, c.n, ho, wo)
    return _conv_call(sd, c, ops)


def _conv_bar(precision, c):
    return FP32_BAR if precision == 0 else HEAD_BAR if c.cout <= 4 else BF16_BAR


@pytest.mark.parametrize("case", CONV_PARAMS, ids=_id)
def test_conv2d_model_shape(engines, tmp_path, request, case):
    precision, c = case
    sd = engines(precision)
    fp8 = precision == 2 and _is_fp8_conv(c)
    ops = _conv_operands(precision, c)
    x, wt, b, temb, resid = ops
    ho, wo = S.out_hw(c.h, c.w, c.k, c.stride, c.ups)
    pix = S.sample_pixels(c.n, ho, wo, seed=_seed("pixels", c))
    ref = S.conv_at(x, wt, b, pix, c.stride, c.ups, temb, resid)
    bar = _conv_bar(precision, c)
    what = f"precision {precision} conv {tuple(c)}"
    auto, lines = _run(sd, tmp_path, lambda: _conv_auto(sd, precision, c, ops))
    _note_plan(request, precision, c, lines)
    assert len(lines) == 1 and (" fp8 " in lines[0]) == fp8, f"{what}: {lines}"
    if precision == 0:
        assert (_field(lines[0], "cfg") >= 300) == M.arrives_as_planes(c, DIMS), f"{what}: planes in, plane tile out (and only then): {lines}"
    _check(S.at_pixels(auto, pix), ref, f"{what}, automatic plan [{lines[0]}]", bar)
    plain, plines = _run(sd, tmp_path, lambda: _conv_call(sd, c, ops), **(PLAIN_FP8 if fp8 else PLAIN_GEMM[precision]))
    assert len(plines) == 1 and _field(plines[0], "cfg") == 0 and _field(plines[0], "splits") == 1, f"{what}: the plain kernel was not taken: {plines}"
    _check(S.at_pixels(plain, pix), ref, f"{what}, plain kernel", bar)
    _check_everywhere(auto, plain, ref, what, bar)
    cfg = _field(lines[0], "cfg")
    if not fp8 and cfg in (104, 105):        # the kernel-row tile and the plain tile it replaces: the same sums in the same order
        twin, tlines = _run(sd, tmp_path, lambda: _conv_call(sd, c, ops), gemm_tile=cfg - 4, splitk=_field(lines[0], "splits"))
        assert _field(tlines[0], "cfg") == cfg - 4, tlines
        assert np.array_equal(auto, twin), f"{what}: kernel-row tile {cfg} differs from tile {cfg - 4}"


@pytest.mark.parametrize("pair", SHAPES.conv_pairs, ids=lambda p: "-".join(map(str, p)))
def test_conv2d_pair_model_shape(engines, tmp_path, request, pair):
    """a ResBlock's tail with a shortcut, as the fp32 engine launches it: conv3x3(h) + conv1x1(x) in one split-K launch where the pair planner takes it (a row of the
    pairs table, or its fallback rule), else -- the entry point says so -- as two launches.  Both against the reference and against each other everywhere."""
    sd = engines(0)
    n, cin_x, cout, h, w = pair
    x = _acts(n, cin_x, h, w, "f32", _seed("pair x", pair))
    hh = _acts(n, cout, h, w, "f32", _seed("pair h", pair))
    w_out, b_out = _conv_weight(cout, cout, 3, "f32")
    w_skip, b_skip = _conv_weight(cout, cin_x, 1, "f32")
    pix = S.sample_pixels(n, h, w, seed=_seed("pixels", pair))
    ref = S.conv_at(hh, w_out, b_out, pix) + S.conv_at(x, w_skip, b_skip, pix)
    what = f"conv pair {tuple(pair)}"
    from stable_diffusion_burn_amd import SdmiError
    try:
        paired, lines = _run(sd, tmp_path, lambda: sd.op_conv2d_pair(x, hh, w_skip, b_skip, w_out, b_out), skip_slices=1)
    except SdmiError as e:
        assert e.status == -5 and "do not pair" in str(e), e        # SDMI_ERR_UNSUPPORTED: the planner declined, nothing ran
        paired, lines = None, ["pair declined"]
    two, lines2 = _run(sd, tmp_path, lambda: sd.op_conv2d_pair(x, hh, w_skip, b_skip, w_out, b_out), skip_slices=0)
    _note_plan(request, 0, pair, lines + lines2)
    assert len(lines2) == 2, lines2
    _check(S.at_pixels(two, pix), ref, f"{what}, two launches", FP32_BAR)
    if paired is not None:
        assert len(lines) == 1 and " pair " in lines[0], lines
        _check(S.at_pixels(paired, pix), ref, f"{what} [{lines[0]}]", FP32_BAR)
        _check_everywhere(paired, two, ref, what, FP32_BAR)


# ---- 3. Linear, GEGLU ----------------------------------------------------------------------------------------------------------------------------------------------------
def _linear_operands(precision, li, zeros=False):
    fmt = _fmt(precision)
    x = _rows(li.rows, li.cin, fmt, _seed("linear x", li, precision), zeros)
    wt, b = _linear_weight(li.cin, li.cout, fmt)
    resid = _rows(li.rows, li.cout, fmt, _seed("linear resid", li), zeros) if li.resid else None
    return x, wt, (b if li.bias else None), resid


def _linear_call(sd, li, ops):
    x, wt, b, resid = ops
    return sd.op_linear(x, wt, b) if resid is None else sd.op_linear_epilogue(x, wt, b, resid)


def _linear_auto(sd, precision, li, ops):
    """As _conv_auto: at precision 0 a plane-eligible Linear gets its rows as planes.  No Linear entry point takes planes, but a Linear IS the 1x1 convolution over
    a 1 x rows image -- Engine::gemm and Engine::conv fill the same ConvGemm (NB = 1, Hs = 1, Ws = rows, KH = 1), which is all the planner and the kernel see."""
    if precision == 0 and M.arrives_as_planes(li, DIMS):
        x, wt, b, resid = ops
        x4 = np.ascontiguousarray(x.T).reshape(1, li.cin, 1, li.rows)
        w4 = np.ascontiguousarray(wt.T).reshape(li.cout, li.cin, 1, 1)
        r4 = None if resid is None else np.ascontiguousarray(resid.T).reshape(1, li.cout, 1, li.rows)
        return sd.op_conv2d_view(x4, w4, b, None, r4, parent=np.zeros((li.rows, li.cout), dtype=np.float32), out_off=0, in_planes=3)
    return _linear_call(sd, li, ops)


@pytest.mark.parametrize("case", LINEAR_PARAMS, ids=_id)
def test_linear_model_shape(engines, tmp_path, request, case):
    precision, li = case
    sd = engines(precision)
    ops = _linear_operands(precision, li)
    rs = S.sample_rows(1, li.rows, seed=_seed("rows", li))
    ref = S.linear_at(ops[0], ops[1], ops[2], rs, ops[3])
    bar = FP32_BAR if precision == 0 else BF16_BAR
    what = f"precision {precision} linear {tuple(li)}"
    auto, lines = _run(sd, tmp_path, lambda: _linear_auto(sd, precision, li, ops))
    _note_plan(request, precision, li, lines)
    assert len(lines) == 1, lines
    if precision == 0:
        assert (_field(lines[0], "cfg") >= 300) == M.arrives_as_planes(li, DIMS), f"{what}: {lines}"
    _check(auto[rs], ref, f"{what}, automatic plan [{lines[0]}]", bar)
    plain, plines = _run(sd, tmp_path, lambda: _linear_call(sd, li, ops), **PLAIN_GEMM[precision])
    assert len(plines) == 1 and _field(plines[0], "cfg") == 0 and _field(plines[0], "splits") == 1, plines
    _check(plain[rs], ref, f"{what}, plain kernel", bar)
    _check_everywhere(auto, plain, ref, what, bar)


@pytest.mark.parametrize("pair", SHAPES.linear_pairs, ids=lambda p: "-".join(map(str, p)))
def test_linear_pair_model_shape(engines, tmp_path, request, pair):
    """a transformer block's tail as the fp32 engine launches it: the MLP's output Linear (folded with proj_out at load) carrying proj_out of the hidden state on extra
    K slices, plus the residual -- one launch where the planner takes it, else two"""
    sd = engines(0)
    rows, k_main, k_aux, cout = pair
    u = _rows(rows, k_main, "f32", _seed("lpair u", pair))
    hh = _rows(rows, k_aux, "f32", _seed("lpair h", pair))
    resid = _rows(rows, cout, "f32", _seed("lpair resid", pair))
    w_main, b_main = _linear_weight(k_main, cout, "f32")
    w_aux, b_aux = _linear_weight(k_aux, cout, "f32")
    rs = S.sample_rows(1, rows, seed=_seed("rows", pair))
    ref = S.linear_at(u, w_main, b_main, rs, resid) + S.linear_at(hh, w_aux, b_aux, rs)
    what = f"linear pair {tuple(pair)}"
    from stable_diffusion_burn_amd import SdmiError
    try:
        paired, lines = _run(sd, tmp_path, lambda: sd.op_linear_pair(u, hh, w_main, b_main, w_aux, b_aux, resid), proj_out_fold=1)
    except SdmiError as e:
        assert e.status == -5 and "do not pair" in str(e), e
        paired, lines = None, ["fold declined"]
    two, lines2 = _run(sd, tmp_path, lambda: sd.op_linear_pair(u, hh, w_main, b_main, w_aux, b_aux, resid), proj_out_fold=0)
    _note_plan(request, 0, pair, lines + lines2)
    assert len(lines2) == 2, lines2
    _check(two[rs], ref, f"{what}, two launches", FP32_BAR)
    if paired is not None:
        assert len(lines) == 1 and " fold " in lines[0], lines
        _check(paired[rs], ref, f"{what} [{lines[0]}]", FP32_BAR)
        _check_everywhere(paired, two, ref, what, FP32_BAR)


def _geglu_auto(sd, tmp_path, precision, gg, x, wt, b):
    """precision 0: the model's form -- x as planes, the gate in the plane GEMM's epilogue (geglu_fuse = 8: the entry point splits x into planes and returns the
    launch's fp32 output), the tile from the plane table or the cost model"""
    if precision:
        return _run(sd, tmp_path, lambda: sd.op_geglu_forward(x, wt, b, gg.hidden))
    try:
        sd.set_option("geglu_fuse", 8)
        got, lines = _run(sd, tmp_path, lambda: sd.op_geglu_forward(x, wt, b, gg.hidden))
        # the same launch's plane output (geglu_fuse = 7: the model's form), joined back, IS the fp32 result split -- also where the planner declines the fused
        # tile (few rows: a split-K projection + the gate kernel), where the fp32 copy was once left unwritten
        sd.set_option("geglu_fuse", 7)
        planes = sd.op_geglu_forward(x, wt, b, gg.hidden)
        if int(lines[0].split(",")[1]) == gg.hidden:      # one fused launch wrote both: the same bits
            np.testing.assert_array_equal(planes, got, err_msg=f"geglu {tuple(gg)}: plane output differs from the fp32 output")
        else:                                               # two gate kernels (fp32 / planes) behind one projection: each within the bar, so within two of each other
            d = _max_diff(planes, got)
            assert d <= 2 * FP32_BAR * max(1.0, float(np.abs(got).max())), f"geglu {tuple(gg)}: plane and fp32 output differ by {d:.3e}"
        return got, lines
    finally:
        sd.set_option("geglu_fuse", 1)


@pytest.mark.parametrize("case", GEGLU_PARAMS, ids=_id)
def test_geglu_forward_model_shape(engines, tmp_path, request, case):
    """GEGLU::forward (unet/mod.rs:579-591) with the engine's own fusion choice, and unfused (geglu_fuse = 0: the plain projection GEMM + the gate kernel)"""
    precision, gg = case
    sd = engines(precision)
    fmt = _fmt(precision)
    x = _rows(gg.rows, gg.cin, fmt, _seed("geglu x", gg, precision))
    wt, b = _linear_weight(gg.cin, 2 * gg.hidden, fmt)
    rs = S.sample_rows(1, gg.rows, seed=_seed("rows", gg))
    proj = _t(S.linear_at(x, wt, b, rs))
    ref = (proj[:, :gg.hidden] * O.gelu_erf(proj[:, gg.hidden:])).numpy()
    bar = FP32_BAR if precision == 0 else BF16_BAR
    what = f"precision {precision} geglu {tuple(gg)}"
    auto, lines = _geglu_auto(sd, tmp_path, precision, gg, x, wt, b)
    _note_plan(request, precision, gg, lines)
    assert len(lines) == 1, lines
    if precision == 0:
        assert _field(lines[0], "cfg") >= 300, f"{what}: x arrives as planes: {lines}"
    fused = int(lines[0].split(",")[1]) == gg.hidden        # (unfused: the projection's 2 hidden columns are the GEMM's N)
    # unfused at bf16, the projection is rounded to bf16 before the gate: tests/test_bf16_gpu.py's bar for that form is 2^-7
    abar = bar if precision == 0 or fused else 2 ** -7
    _check(auto[rs], ref, f"{what}, automatic plan {lines}", abar)
    try:
        sd.set_option("geglu_fuse", 0)
        plain, plines = _run(sd, tmp_path, lambda: sd.op_geglu_forward(x, wt, b, gg.hidden), **PLAIN_GEMM[precision])
    finally:
        sd.set_option("geglu_fuse", 1)
    assert len(plines) == 1 and _field(plines[0], "cfg") == 0 and _field(plines[0], "splits") == 1, plines
    pbar = bar if precision == 0 else 2 ** -7
    _check(plain[rs], ref, f"{what}, unfused", pbar)
    bound = (abar + pbar) * max(1.0, float(np.abs(ref).max()))
    d = _max_diff(auto, plain)
    assert d <= bound, f"{what}: fused and unfused differ by {d:.3e} > {bound:.3e} somewhere"


# ---- 4. attention ------------------------------------------------------------------------------------------------------------------------------------------------------------
def _attn_operands(precision, a):
    g = np.random.default_rng(_seed("attention", a))
    fmt = _fmt(precision)
    return tuple(_grid(g.standard_normal((a.n, s, a.c)), fmt, 2) for s in (a.nq, a.nk, a.nk))


def _attn_bar(precision, a):
    return FP32_BAR if precision == 0 else ATTN16_BAR if a.heads > 1 else ATTN16_1HEAD_BAR


@functools.lru_cache(maxsize=2)
def _attn_case(precision, a):
    """operands, sampled query rows and their fp64 reference, shared by the tests of one shape"""
    q, k, v = _attn_operands(precision, a)
    rs = S.sample_rows(a.n, a.nq, seed=_seed("rows", a))
    return q, k, v, rs, S.attention_at(q, k, v, rs, a.heads)


@pytest.mark.parametrize("case", ATTN_PARAMS, ids=_id)
def test_attention_model_shape(engines, tmp_path, request, case):
    """qkv_attention (attention.rs:5-45) at the model's sequence lengths -- up to 16384 x 16384 at d = 40, 16384 queries against a 77-token context, and the VAE's
    single-head path (two GEMMs around a row softmax of up to 16384 columns: a 1 GiB fp32 score matrix, a K = 16384 product) -- with the engine's own kernel and
    key-slice choice, and with the plainest kernel (fp32 matrix instruction / widened bf16, no key slices; single head: plain GEMM tiles)."""
    precision, a = case
    sd = engines(precision)
    q, k, v, rs, ref = _attn_case(precision, a)
    bar = _attn_bar(precision, a)
    what = f"precision {precision} attention {tuple(a)}"
    auto, lines = _run(sd, tmp_path, lambda: sd.qkv_attention(q, k, v, None, a.heads), attention=True)
    _note_plan(request, precision, a, lines)
    flat = lambda o: o.reshape(a.n * a.nq, a.c)
    _check(flat(auto)[rs], ref, f"{what}, automatic plan {lines}", bar)
    opts = dict(PLAIN_ATTN)
    if a.heads == 1:
        opts.update(PLAIN_GEMM[precision])
    plain, plines = _run(sd, tmp_path, lambda: sd.qkv_attention(q, k, v, None, a.heads), attention=True, **opts)
    assert all(_field(ln, "slices") == 1 for ln in plines if ln.startswith("attention ")), plines
    if a.heads == 1:
        gl = [ln for ln in plines if not ln.startswith("attention ")]
        assert len(gl) == 2 and all(_field(ln, "cfg") == 0 and _field(ln, "splits") == 1 for ln in gl), f"{what}: the plain GEMM tile was not taken: {plines}"
    # bf16 storage widened onto the fp32 kernel rounds q d^-0.5 log2 e once more like the bf16 kernel does (tests/test_bf16_gpu.py): the same bar
    _check(flat(plain)[rs], ref, f"{what}, plain kernel", bar)
    _check_everywhere(auto, plain, ref, what, bar)


def test_self_attention_16384_fp32_kernels_and_key_slices(engines, tmp_path, request):
    """16384 x 16384 at d = 40, n = 2, precision 0: k_attn_split.hip (attn_split = 1, the automatic choice above), k_attn.hip (attn_split = 0), and both with the keys
    cut into 8 slices merged by the second launch -- the automatic rule never slices a grid this large, so the merge launch at this length is forced here"""
    a = SELF_16384
    sd = engines(0)
    q, k, v, rs, ref = _attn_case(0, a)
    outs = {}
    for split in (1, 0):
        for slices in (1, 8):
            got, lines = _run(sd, tmp_path, lambda: sd.qkv_attention(q, k, v, None, 8), attention=True, attn_split=split, attn_kv_splits=slices)
            print(f"attn_split={split} attn_kv_splits={slices}: {lines}")
            assert [_field(ln, "slices") for ln in lines if ln.startswith("attention ")] == [slices], lines
            _check(got.reshape(-1, a.c)[rs], ref, f"attention {tuple(a)} attn_split={split} slices={slices}", FP32_BAR)
            outs[(split, slices)] = got
    for key, got in outs.items():
        _check_everywhere(got, outs[(1, 1)], ref, f"attention {tuple(a)} {key} against (1, 1)", FP32_BAR)


# ---- 5. GroupNorm, LayerNorm ---------------------------------------------------------------------------------------------------------------------------------------------
def _gn_input(n, c, h, w, fmt, seed):
    """unit-scale noise (a repeated block where large) + 0.9 + a ramp from -1 to 1 along each sample's pixels: on a repeated block alone, statistics taken over a
    PART of the pixels would equal those over all of them; with the ramp they do not"""
    x = _acts(n, c, h, w, "f32", seed, 1.7).reshape(n, c, h * w)
    x += (np.linspace(-1.0, 1.0, h * w, dtype=np.float32) + np.float32(0.9))[None, None, :]
    x = x.reshape(n, c, h, w)
    return bf16_round(x) if fmt == "bf16" else x


@pytest.mark.parametrize("case", GN_PARAMS, ids=_id)
def test_group_norm_model_shape(engines, case):
    """GroupNorm (+ SiLU) up to a megapixel: (1, 128, 1024, 1024) is 4 M elements per group.  Statistics in fp64 over the whole tensor, values at the sampled pixels."""
    precision, gn = case
    sd = engines(precision)
    x = _gn_input(gn.n, gn.c, gn.h, gn.w, _fmt(precision), _seed("gn", gn[:4]))
    g = np.random.default_rng(_seed("gn affine", gn.c))
    gamma = (1 + 0.1 * g.standard_normal(gn.c)).astype(np.float32)
    beta = (0.1 * g.standard_normal(gn.c)).astype(np.float32)
    pix = S.sample_pixels(gn.n, gn.h, gn.w, seed=_seed("pixels", gn))
    ref = S.group_norm_at(x, gamma, beta, 32, 1e-5, gn.silu, pix)
    got = sd.op_group_norm(x, gamma, beta, 32, 1e-5, gn.silu)
    _check(S.at_pixels(got, pix), ref, f"precision {precision} group_norm {tuple(gn)}", FP32_BAR if precision == 0 else BF16_BAR)
    assert np.isfinite(got).all()


@pytest.mark.parametrize("case", LN_PARAMS, ids=_id)
def test_layer_norm_model_shape(engines, case):
    precision, ln = case
    sd = engines(precision)
    x = _rows(ln.rows, ln.c, "f32", _seed("ln", ln)) * 2 - 0.5
    x = bf16_round(x) if precision else x
    g = np.random.default_rng(_seed("ln affine", ln.c))
    gamma = (1 + 0.1 * g.standard_normal(ln.c)).astype(np.float32)
    beta = (0.1 * g.standard_normal(ln.c)).astype(np.float32)
    rs = S.sample_rows(1, ln.rows, seed=_seed("rows", ln))
    got = sd.op_layer_norm(x, gamma, beta, 1e-5)
    ref = O.layer_norm(_t(x[rs]), _t(gamma), _t(beta), 1e-5).numpy()
    _check(got[rs], ref, f"precision {precision} layer_norm {tuple(ln)}", FP32_BAR if precision == 0 else BF16_BAR)
    assert np.isfinite(got).all()


# ---- 6. the plan table ---------------------------------------------------------------------------------------------------------------------------------------------------
def _plan_lines_of(sd, tmp_path, precision, item):
    """the automatic plan of an item no test above has run in this session: the same call on zero operands (the plan depends on shapes and strides only)"""
    if isinstance(item, M.Conv):
        ops = _conv_operands(precision, item, zeros=True)
        return _run(sd, tmp_path, lambda: _conv_auto(sd, precision, item, ops))[1]
    if isinstance(item, M.Linear):
        ops = _linear_operands(precision, item, zeros=True)
        return _run(sd, tmp_path, lambda: _linear_auto(sd, precision, item, ops))[1]
    if isinstance(item, M.Geglu):
        wt, b = _linear_weight(item.cin, 2 * item.hidden, _fmt(precision))
        return _geglu_auto(sd, tmp_path, precision, item, np.zeros((item.rows, item.cin), np.float32), wt, b)[1]
    q, k = np.zeros((item.n, item.nq, item.c), np.float32), np.zeros((item.n, item.nk, item.c), np.float32)
    return _run(sd, tmp_path, lambda: sd.qkv_attention(q, k, k, None, item.heads), attention=True)[1]


def test_plan_table_is_not_trivial(engines, tmp_path):
    """What the automatic plan chose for every shape above, by precision: more than one kernel family, at least one split-K launch, at least one key-sliced
    attention.  Nothing else is asserted of the plan -- the table is for reading (profiles/model_shapes_plan.txt; written where SDMI_MODEL_SHAPES_PLAN names a file)."""
    rows = []
    for params in (CONV_PARAMS, LINEAR_PARAMS, GEGLU_PARAMS, ATTN_PARAMS):
        for precision, item in params:
            if (precision, item) not in PLAN:
                PLAN[(precision, item)] = _plan_lines_of(engines(precision), tmp_path, precision, item)
            rows.append((precision, item, PLAN[(precision, item)]))
    rows += [(0, p, PLAN[(0, p)]) for p in SHAPES.conv_pairs + SHAPES.linear_pairs if (0, p) in PLAN]
    text = ["# precision | operator and shape | what the automatic plan launched: M,N,K k<KH> s<stride> u<ups> W<width> [pair|fold|fp8] cfg=<tile> splits=<K slices> acc=<resid_acc>;",
            "# attention: slices=<key slices>.  Written by tests/test_model_shapes_gpu.py on an MI355X; 72 x 88 and 128 x 128 latents, batch 2."]
    for precision, item, lines in rows:
        fams = ",".join(sorted({_family(ln) for ln in lines if "=" in ln}))
        text.append(f"{precision} | {type(item).__name__}{tuple(item)} | {fams} | " + " ; ".join(lines))
    out = os.environ.get("SDMI_MODEL_SHAPES_PLAN")
    if out:
        with open(out, "w") as f:
            f.write("\n".join(text) + "\n")
    for precision in (0, 1, 2):
        lines = [ln for p, _, ls in rows if p == precision for ln in ls if "=" in ln]
        fams = {_family(ln) for ln in lines if not ln.startswith("attention ")}
        assert len(fams) > 1, f"precision {precision}: one kernel family only: {fams}"
    assert any((_field(ln, "splits") or 1) > 1 for _, _, ls in rows for ln in ls), "no split-K launch"
    assert any((_field(ln, "slices") or 1) > 1 for p, _, ls in rows if p == 0 for ln in ls), "no key-sliced attention"


# ---- 7. operands around the 32-bit lines -------------------------------------------------------------------------------------------------------------------------------
BIG_ROWS, BIG_C, BIG_PERIOD = 2944 * 2944, 64, 100003       # 8 667 136 rows of 64 channels: 2.22 GB of fp32 (> 2^31 bytes), 3.33 GB as three bf16 planes


def _big_rows(rows, c, seed):
    """[rows, c]: a seeded block of BIG_PERIOD rows (prime) repeated -- rows r and r + BIG_PERIOD hold the same values, and no tile height divides the period"""
    block = np.random.default_rng(seed).standard_normal((BIG_PERIOD, c)).astype(np.float32)
    return np.tile(block, ((rows + BIG_PERIOD - 1) // BIG_PERIOD, 1))[:rows]


def _line_rows(rows, row_bytes, lines=(1 << 31, 1 << 32)):
    """the first and last rows, and those within +-2 of the row whose byte offset crosses each 32-bit line"""
    picks = [0, 1, 2, rows - 3, rows - 2, rows - 1]
    for line in lines:
        r = line // row_bytes
        picks += [r + d for d in (-2, -1, 0, 1, 2)]
    return np.unique([p for p in picks if 0 <= p < rows])


def _periodic_everywhere(got, rows_axis0, ref, what, rel):
    """rows r and r + BIG_PERIOD see the same inputs, so their outputs are two results of the same sum, each within one bar of the truth: every row of the output is
    tied to the sampled fp64 reference this way, without a second launch"""
    a, b = got[:rows_axis0 - BIG_PERIOD], got[BIG_PERIOD:rows_axis0]
    bound = 2 * rel * max(1.0, float(np.abs(ref).max()))
    d = _max_diff(a, b)
    assert d <= bound, f"{what}: rows one period apart differ by {d:.3e} > {bound:.3e}"


def test_linear_input_and_output_above_2_gib(engines, tmp_path):
    """A Linear layer whose fp32 input [8 667 136, 64] and fp32 output (Cout = 64) are 2.22 GB each: byte offsets above 2^31 on both sides of the kernel and in the
    host-layout conversions around it."""
    t0 = time.time()
    sd = engines(0)
    x = _big_rows(BIG_ROWS, BIG_C, 71)
    g = np.random.default_rng(72)
    wt = (g.standard_normal((BIG_C, 64)) / math.sqrt(BIG_C)).astype(np.float32)
    b = g.standard_normal(64).astype(np.float32)
    assert x.nbytes > 1 << 31
    got, lines = _run(sd, tmp_path, lambda: sd.op_linear(x, wt, b))
    assert got.nbytes > 1 << 31
    rs = np.union1d(_line_rows(BIG_ROWS, BIG_C * 4), S.sample_rows(1, BIG_ROWS, seed=73))
    ref = S.linear_at(x, wt, b, rs)
    _check(got[rs], ref, f"linear 2.2 GB in / out {lines}", FP32_BAR)
    _periodic_everywhere(got, BIG_ROWS, ref, "linear 2.2 GB in / out", FP32_BAR)
    print(f"\nlinear above 2 GiB: {lines}; {time.time() - t0:.1f} s")


def _big_image(h, w, seed):
    """[1, 64, h, w]: a seeded block of BIG_PERIOD pixels repeated along the pixel axis"""
    block = np.random.default_rng(seed).standard_normal((BIG_C, BIG_PERIOD)).astype(np.float32)
    return _repeat_cols(block, h * w, 0).reshape(1, BIG_C, h, w)


def _conv_line_pixels(h, w, row_bytes):
    """_line_rows for a 3x3 convolution: also the pixels one image row above and below a line (their taps straddle it)"""
    base = _line_rows(h * w, row_bytes)
    return np.unique(np.clip(np.concatenate([base, base - w, base + w]), 0, h * w - 1))


def test_conv3x3_plane_path_above_2_gib(engines, tmp_path):
    """The same 2.22 GB input through a 3x3 convolution with Cout = 8 on a plane tile (k_gemm3p.hip): its activation planes are 3.33 GB, so 32-bit piece offsets above
    2^31 are in use.  An fp32 tensor handed to op_conv2d reaches a plane tile by option gemm_tile (the model's producers write planes themselves; here
    launch_gemm splits the tensor in front of the launch); dump_choices must show that the plane tile ran."""
    t0 = time.time()
    sd = engines(0)
    x = _big_image(2944, 2944, 81)
    g = np.random.default_rng(82)
    wt = (g.standard_normal((8, BIG_C, 3, 3)) / math.sqrt(BIG_C * 9)).astype(np.float32)
    b = g.standard_normal(8).astype(np.float32)
    got, lines = _run(sd, tmp_path, lambda: sd.op_conv2d(x, wt, b), gemm_tile=305)
    assert len(lines) == 1 and _field(lines[0], "cfg") == 305, f"not the plane tile: {lines}"
    # byte offsets of pixel p: 256 p in the fp32 tensor, 384 p in the planes
    pix = np.unique(np.concatenate([_conv_line_pixels(2944, 2944, 256), _conv_line_pixels(2944, 2944, 384), S.sample_pixels(1, 2944, 2944, seed=83)]))
    ref = S.conv_at(x, wt, b, pix)
    _check(S.at_pixels(got, pix), ref, f"conv3x3 on planes above 2 GiB {lines}", FP32_BAR)
    print(f"\nconv3x3 planes above 2 GiB: {lines}; {time.time() - t0:.1f} s")


def test_conv3x3_planes_past_their_limit_fall_back_to_fp32_activations(engines, tmp_path):
    """900 M input elements (3.6 GB of fp32, below the 4 GiB operand limit) whose planes would be 5.4 GB, past the 0xFFFFFF00-byte reach of the plane kernel's 32-bit
    piece offsets: gemm_plan_in clears p_ok, so the plane tile asked for by option gemm_tile (the previous test's) must NOT be taken -- the launch goes to a family
    that reads fp32 activations -- and the result must hold the bar."""
    t0 = time.time()
    sd = engines(0)
    h, w = 3750, 3750                                  # 14 062 500 pixels x 64 channels = 900 M elements
    x = _big_image(h, w, 91)
    assert x.nbytes < 0xFFFFFFE0 and x.size * 6 >= 0xFFFFFF00
    g = np.random.default_rng(92)
    wt = (g.standard_normal((8, BIG_C, 3, 3)) / math.sqrt(BIG_C * 9)).astype(np.float32)
    b = g.standard_normal(8).astype(np.float32)
    got, lines = _run(sd, tmp_path, lambda: sd.op_conv2d(x, wt, b), gemm_tile=305)
    assert len(lines) == 1 and _field(lines[0], "cfg") < 300, f"a plane tile past the planes' limit: {lines}"
    pix = np.unique(np.concatenate([_conv_line_pixels(h, w, 256), S.sample_pixels(1, h, w, seed=93)]))
    ref = S.conv_at(x, wt, b, pix)
    _check(S.at_pixels(got, pix), ref, f"conv3x3 with planes past their limit {lines}", FP32_BAR)
    print(f"\nconv3x3 planes past their limit: {lines}; {time.time() - t0:.1f} s")


def test_operand_of_4_gib_is_refused(engines, tmp_path):
    """An activation operand of 4 GiB is refused with SDMI_ERR_UNSUPPORTED naming the limit, before anything is launched, and the context goes on working."""
    from stable_diffusion_burn_amd import SdmiError
    t0 = time.time()
    sd = engines(0)
    rows = (1 << 32) // (BIG_C * 4)                    # 16 777 216 rows x 64 channels x 4 bytes = 2^32
    x = np.zeros((rows, BIG_C), dtype=np.float32)
    wt = np.zeros((BIG_C, 8), dtype=np.float32)
    sd.op_linear(x[:256], wt, None)
    before = sd.last_call_stats()
    path = tmp_path / "choices.txt"
    try:
        sd.set_option("record_shapes", 1)
        with pytest.raises(SdmiError) as e:
            sd.op_linear(x, wt, None)
        sd.set_option("dump_choices", str(path))
    finally:
        sd.set_option("record_shapes", 0)
    assert e.value.status == -5 and "4 GiB" in str(e.value), e.value       # SDMI_ERR_UNSUPPORTED
    del x
    # no GEMM was planned or launched by the refused call, and it did not complete as a call: the context still reports the small call in front of it
    assert path.read_text() == "", path.read_text()
    assert sd.last_call_stats() == before
    # ... and the next small call on the same context is correct
    g = np.random.default_rng(95)
    xs = g.standard_normal((300, BIG_C)).astype(np.float32)
    ws = (g.standard_normal((BIG_C, 8)) / 8).astype(np.float32)
    _check(sd.op_linear(xs, ws, None), O.linear(_t(xs), _t(ws), None).numpy(), "linear after a refused call", FP32_BAR)
    print(f"4 GiB refusal: {time.time() - t0:.1f} s")


def test_group_norm_one_sample_above_2_gib(engines):
    """GroupNorm on one sample of 2.22 GB, (1, 64, 2944, 2944): 17 M elements per group; statistics over the whole tensor, values at sampled pixels and around the
    2^31-byte line, the last pixel included"""
    t0 = time.time()
    sd = engines(0)
    h = w = 2944
    x = _big_image(h, w, 101).reshape(1, BIG_C, h * w)
    x *= np.float32(1.7)
    x += (np.linspace(-1.0, 1.0, h * w, dtype=np.float32) + np.float32(0.9))[None, None, :]      # (see _gn_input)
    x = x.reshape(1, BIG_C, h, w)
    g = np.random.default_rng(102)
    gamma = (1 + 0.1 * g.standard_normal(BIG_C)).astype(np.float32)
    beta = (0.1 * g.standard_normal(BIG_C)).astype(np.float32)
    pix = np.unique(np.concatenate([_line_rows(h * w, BIG_C * 4), S.sample_pixels(1, h, w, seed=103)]))
    assert pix[-1] == h * w - 1
    ref = S.group_norm_at(x, gamma, beta, 32, 1e-5, True, pix)
    got = sd.op_group_norm(x, gamma, beta, 32, 1e-5, True)
    _check(S.at_pixels(got, pix), ref, "group_norm (1, 64, 2944, 2944)", FP32_BAR)
    print(f"\ngroup_norm above 2 GiB: {time.time() - t0:.1f} s")
