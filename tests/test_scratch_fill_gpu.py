"""No result may depend on device memory nobody wrote.

DevPool hands out blocks of 1-GiB slabs at deterministic addresses: a fresh slab usually reads as zeros and a reused block holds the same leftover on every
run, so a kernel that reads an unwritten pad column, scale byte, split-K slab row, history slot or merge buffer gives plausible results, and the same bits
twice.  Option pool_fill (tests) overwrites every block the pool hands out -- and, set before the weights are loaded, every persistent allocation -- with
one byte.  The rule under test: for the same inputs the output of every public call is finite and BIT-IDENTICAL with the fill off and with the bytes

    0x00  the control: if it differs, the engine depends on leftovers that are not zero.  Runs first in every case.
    0xFF  NaN in fp32, in bf16, in e4m3 and as an E8M0 scale: "garbage x 0" (a zero-padded weight against an unwritten activation pad, p = 0
          against an unwritten V row).
    0x5A  finite in all four (1.5e16 in fp32 and bf16, 20 in e4m3, 2^-37 as a scale): the reads NaN hides -- fmaxf / fminf drop a NaN operand, so NaN
          vanishes in running maxima, clamps and saturating conversions.

These are patterns, not tolerances: nothing here is measured, every comparison is np.array_equal on the raw bits.  Every case also reads the engine's
own count of filled blocks (option dump_pool_fills): > 0 with the fill on, 0 with it off -- the proof that the switch is live -- and the number of kernel
launches (last_call_stats), which the fill must not change.

Section A: whole calls on three contexts per precision, created one after the other -- plain, and with pool_fill = 0xFF / 0x5A set BEFORE load_weights, so
that weight arenas, planes, masters and MXFP8 copies start from that byte; all three run the per-call patterns, and the filled contexts' outputs must equal
the plain context's (kept in _PLAIN: pytest runs the plain context's cases first, a module-scoped fixture's parameters in their order).  Precision 0 runs the
half-width model of conftest.tiny_dims (with test_clip_gpu.py's tiny text encoder); precision 1 / 2 refuse it (bf16 needs channel counts that are multiples
of 64) and run test_hires_gpu.py's BF16_DIMS.
Section B: the operator entries on one context per precision, at the smallest shapes the neighbouring modules use for each path; one case per family
also holds its 0xFF result against the fp64 oracle at that family's bar, so that both sides cannot be equally wrong.
"""
import math

import numpy as np
import pytest
import torch

import lora_ref as L
import resize_ref as RR
from oracle import mx_oracle as MX
from oracle import sd_oracle as O
from stable_diffusion_burn_amd import synthetic as syn
from test_clip_gpu import MINI_VOCAB
from test_views_gpu import BF16_BAR, FP32_BAR, _check, _conv_case, _gn_check, _prefill, _ref, _t, bf16_round

pytestmark = pytest.mark.gpu

PATTERNS = (0x00, 0xFF, 0x5A)     # the control first


# ---- the sweep ------------------------------------------------------------------------------------------------------------------------------------------------
def _raw(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 2: np.uint16, 1: np.uint8}[a.dtype.itemsize])


def _fills(sd, tmp_path):
    """(blocks, bytes) the engine filled since this was last read"""
    path = tmp_path / "pool_fills.txt"
    sd.set_option("dump_pool_fills", str(path))
    blocks, nbytes = (int(v) for v in path.read_text().split())
    return blocks, nbytes


def _sweep(sd, tmp_path, fn, what, ref=None, oracle=None):
    """fn() -> array or tuple of arrays, with the fill off and under each pattern: finite, bit-identical, the same number of launches, blocks filled only
    while the switch is on.  ref: what another context gave for the same call.  oracle(outputs): run on the 0xFF result.  Returns (outputs with the fill
    off, bytes filled by one call)."""
    def run():
        out = fn()
        out = tuple(out) if isinstance(out, (tuple, list)) else (out,)
        for i, a in enumerate(out):
            if a.dtype.kind == "f":
                assert np.isfinite(a).all(), f"{what}: output {i} is not finite"
        return out, sd.last_call_stats()["kernels"]

    nbytes = 0
    try:
        sd.set_option("pool_fill", -1)
        _fills(sd, tmp_path)
        off, k_off = run()
        assert _fills(sd, tmp_path) == (0, 0), f"{what}: blocks filled while pool_fill is off"
        if ref is not None:
            assert len(ref) == len(off)
            for i, (a, b) in enumerate(zip(off, ref)):
                assert np.array_equal(_raw(a), _raw(b)), f"{what}: output {i} differs from the plain context's (fill off): a persistent buffer is read where nobody wrote it"
        for byte in PATTERNS:
            sd.set_option("pool_fill", byte)
            got, k = run()
            blocks, nbytes = _fills(sd, tmp_path)
            assert blocks > 0, f"{what}: pool_fill={byte:#04x} filled no block"
            assert k == k_off, f"{what}: {k} launches under pool_fill={byte:#04x}, {k_off} without"
            for i, (a, b) in enumerate(zip(got, off)):
                assert a.shape == b.shape and a.dtype == b.dtype
                same = _raw(a) == _raw(b)
                assert same.all(), (f"{what}: output {i} under pool_fill={byte:#04x} differs from the unfilled run in {int((~same).sum())} of {same.size} elements "
                                    f"(first at {tuple(int(v) for v in np.argwhere(~same)[0])}): uninitialised pool memory is read")
            if byte == 0xFF and oracle is not None:
                oracle(got)
    finally:
        sd.set_option("pool_fill", -1)
    return off, nbytes


def _options(sd, opts):
    for k, v in opts.items():
        sd.set_option(k, v)


_DEFAULTS = {"gemm_tile": "auto", "splitk": 0, "gemm_planes": "default", "gemm_f32s": 1, "attn_split": 1, "attn_kv_splits": 0, "conv3_reuse": 1, "geglu_fuse": 1,
             "fp8_tile": "auto", "resid_acc": 3, "fp8_ops": 0, "cfg_share": 1, "attn_bf16_variant": "default", "fp8_linear": 0}


def _with(sd, opts, fn):
    """fn under engine options, restored afterwards"""
    def call():
        try:
            _options(sd, opts)
            return fn()
        finally:
            _options(sd, {k: _DEFAULTS[k] for k in opts})
    return call


# =================================================================================================================================================================
# Section A: whole calls
# =================================================================================================================================================================
DIMS = {0: O.Dims(160, 4, 64, 16, 16, 32), 1: O.Dims(320, 8, 768, 16, 16, 64), 2: O.Dims(320, 8, 768, 16, 16, 64)}
KINDS = ("plain", 0xFF, 0x5A)
_PLAIN = {}     # (precision, case) -> the plain context's outputs


class _Ctx:
    def __init__(self, sd, precision, kind):
        self.sd, self.precision, self.kind, self.d = sd, precision, kind, DIMS[precision]

    def case(self, tmp_path, name, fn, nbytes_at_least=0):
        """one call of section A: the sweep on this context, against the plain context's result on the filled ones; precision 2 under fp8_linear 0 and 1"""
        for wide in ((0, 1) if self.precision == 2 else (None,)):
            key = (self.precision, name, wide)
            what = f"precision {self.precision}{'' if wide is None else f' fp8_linear={wide}'}, context {self.kind if self.kind == 'plain' else hex(self.kind)}: {name}"
            call = fn if wide is None else _with(self.sd, {"fp8_linear": wide}, fn)
            if self.kind == "plain":
                _PLAIN[key], nbytes = _sweep(self.sd, tmp_path, call, what)
            else:
                assert key in _PLAIN, f"{what}: the plain context's case did not run (it runs first and keeps its result for this comparison)"
                _, nbytes = _sweep(self.sd, tmp_path, call, what, ref=_PLAIN[key])
            assert nbytes >= nbytes_at_least, f"{what}: {nbytes} bytes filled, the output alone has {nbytes_at_least}"


@pytest.fixture(scope="module", params=[pytest.param((p, k), id=f"p{p}-{k if k == 'plain' else hex(k)}") for p in (0, 1, 2) for k in KINDS])
def ctx(request, synth, tmp_path_factory):
    from stable_diffusion_burn_amd import ModelConfig, StableDiffusion
    precision, kind = request.param
    d = DIMS[precision]
    # test_clip_gpu.py's tiny text encoder (always fp32): two layers of 64-wide heads over the mini vocabulary
    sd = StableDiffusion(ModelConfig(d.model_channels, d.n_head, d.ctx_dim, d.latent_h, d.latent_w, d.vae_ch, precision=precision,
                                     clip_layers=2, clip_heads=d.ctx_dim // 64, clip_vocab=MINI_VOCAB, clip_ctx=16))
    try:
        tmp = tmp_path_factory.mktemp("fills")
        sd.set_option("keep_masters", 1)          # the LoRA cases
        if kind != "plain":
            sd.set_option("pool_fill", kind)      # before the first weight: arenas, planes, masters, fused q | k | v buffers, MXFP8 copies
        sd.load_weights(synth)
        blocks, _ = _fills(sd, tmp)
        assert (blocks > 0) == (kind != "plain"), f"loading the weights filled {blocks} blocks on the {kind} context"
        sd.set_option("pool_fill", -1)
        if precision == 2:
            sd.set_option("fp8_min_rows", 1)      # the small latents have few rows per GEMM: the MXFP8 path anyway
        yield _Ctx(sd, precision, kind)
    finally:
        sd.close()


def _lat(n, h, w, first=0):
    return np.stack([syn.initial_latent(first + i, h, w) for i in range(n)])


def _prompts(d, n, T, Tu):
    return np.stack([syn.cond_context(i, T, d.ctx_dim) for i in range(n)]), syn.uncond_context(Tu, d.ctx_dim)


@pytest.mark.parametrize("T", [7, 77])
@pytest.mark.parametrize("t", [999, 49])
@pytest.mark.parametrize("n", [1, 3])
def test_unet_forward(ctx, tmp_path, n, t, T):
    d, sd = ctx.d, ctx.sd
    lat, (c, _) = _lat(n, d.latent_h, d.latent_w), _prompts(d, n, T, 2)
    ctx.case(tmp_path, f"unet.forward n={n} t={t} T={T}", lambda: sd.unet.forward(lat, [t], c), nbytes_at_least=lat.nbytes)


def test_fill_is_no_kernel_and_counts_only_while_on(ctx, tmp_path):
    """last_call_stats()["kernels"] of a UNet forward is the same number with the fill off and on; dump_pool_fills reads 0 0 while off, and with the fill on
    at least the output's size"""
    d, sd = ctx.d, ctx.sd
    lat, (c, _) = _lat(2, d.latent_h, d.latent_w), _prompts(d, 2, 7, 2)
    try:
        _fills(sd, tmp_path)
        base = sd.unet.forward(lat, [500], c)
        k_off = sd.last_call_stats()["kernels"]
        assert _fills(sd, tmp_path) == (0, 0)
        sd.set_option("pool_fill", 0xFF)
        got = sd.unet.forward(lat, [500], c)
        k_on = sd.last_call_stats()["kernels"]
        blocks, nbytes = _fills(sd, tmp_path)
        sd.set_option("pool_fill", -1)
        again = sd.unet.forward(lat, [500], c)
        assert _fills(sd, tmp_path) == (0, 0)
    finally:
        sd.set_option("pool_fill", -1)
    assert k_on == k_off > 0 and blocks > 0 and nbytes >= got.nbytes
    assert np.array_equal(_raw(got), _raw(base)) and np.array_equal(_raw(again), _raw(base))


@pytest.mark.parametrize("share", [0, 1])
@pytest.mark.parametrize("T,Tu", [(7, 2), (3, 6), (65, 129)])
def test_sample_latent_cfg(ctx, tmp_path, T, Tu, share):
    """unequal context lengths: the packed CFG context is zero-padded to the longer one"""
    d, sd = ctx.d, ctx.sd
    lat, (c, u) = _lat(1, d.latent_h, d.latent_w), _prompts(d, 1, T, Tu)
    ctx.case(tmp_path, f"sample_latent T={T} Tu={Tu} cfg_share={share}", _with(sd, {"cfg_share": share}, lambda: sd.sample_latent(c, u, 7.5, 3, init_latent=lat)))


def test_sample_image(ctx, tmp_path):
    d, sd = ctx.d, ctx.sd
    lat, (c, u) = _lat(1, d.latent_h, d.latent_w), _prompts(d, 1, 7, 2)
    ctx.case(tmp_path, "sample_image", lambda: sd.sample_image(c, u, 7.5, 2, init_latent=lat))


def test_encode_and_img2img(ctx, tmp_path):
    d, sd = ctx.d, ctx.sd
    h, w = d.latent_h, d.latent_w
    (c, u) = _prompts(d, 1, 7, 2)
    img = np.random.default_rng(3).integers(0, 256, (1, 8 * h, 8 * w, 3), dtype=np.uint8)
    x = np.ascontiguousarray((img.astype(np.float32) / np.float32(127.5) - np.float32(1.0)).transpose(0, 3, 1, 2))
    mask = np.zeros((1, h, w), np.float32)
    mask[:, 3:11, 2:9] = 1.0
    noise = _lat(1, h, w, first=40)
    ctx.case(tmp_path, "encode_image", lambda: sd.autoencoder.encode_image(x))
    ctx.case(tmp_path, "sample_image_from mask strength 0.5", lambda: sd.sample_image_from(c, u, 7.5, 4, 0.5, img, mask=mask, noise=noise))


@pytest.mark.parametrize("sampler", [("dpmpp_2m", 0.0), ("plms", 0.0), ("ddim", 1.0)])
def test_samplers(ctx, tmp_path, sampler):
    """the multistep samplers' history slots and the stochastic sampler's noise draw"""
    d, sd = ctx.d, ctx.sd
    lat, (c, u) = _lat(2, d.latent_h, d.latent_w), _prompts(d, 2, 7, 2)
    try:
        sd.set_sampler(sampler[0], eta=sampler[1], noise_seed=5)
        ctx.case(tmp_path, f"sample_latent sampler={sampler}", lambda: sd.sample_latent(c, u, 7.5, 4, init_latent=lat))
    finally:
        sd.set_sampler(None)


def test_size_changes_and_hires(ctx, tmp_path):
    """one context at several sizes: blocks are reused at another shape, with the pads in other places; the resampler's intermediate buffer and tap tables"""
    d, sd = ctx.d, ctx.sd
    (c, u) = _prompts(d, 1, 7, 2)
    try:
        sd.set_latent_size(8, 24)
        lat = _lat(1, 8, 24)
        ctx.case(tmp_path, "unet.forward at 8 x 24", lambda: sd.unet.forward(lat, [500], c))
        sd.set_latent_size(16, 16)
        lat = _lat(1, 16, 16)
        ctx.case(tmp_path, "unet.forward back at 16 x 16", lambda: sd.unet.forward(lat, [500], c))
        lat8, noise = _lat(1, 8, 8), _lat(1, 16, 16, first=40)
        ctx.case(tmp_path, "sample_image_hires (8, 8) -> (16, 16) bicubic",
                 lambda: sd.sample_image_hires(c, u, 7.5, 2, (8, 8), 0.5, mode="bicubic", init_latent=lat8, hires_noise=noise))
    finally:
        sd.set_latent_size(d.latent_h, d.latent_w)


# the cost model picks small tiles at these sizes: the other kernel families forced, as test_unet_forward_large_tiles_forced / test_unet_forward_bf16_large_tiles_forced do
FORCED = {0: [{"gemm_tile": t} for t in (100, 103, 200, 203, 204, 205)] + [{"gemm_planes": v} for v in (0, 1, 2)] + [{"gemm_f32s": 0}, {"attn_split": 0}, {"attn_kv_splits": 3}],
          1: [{"gemm_tile": t} for t in (100, 103)] + [{"conv3_reuse": v} for v in (0, 1)] + [{"geglu_fuse": v} for v in (0, 2, 3)]}


def test_unet_forward_forced_families(ctx, tmp_path):
    d, sd = ctx.d, ctx.sd
    lat, (c, _) = _lat(2, d.latent_h, d.latent_w), _prompts(d, 2, 7, 2)
    for opts in FORCED[min(ctx.precision, 1)]:
        ctx.case(tmp_path, f"unet.forward {opts}", _with(sd, opts, lambda: sd.unet.forward(lat, [500], c)))


def test_lora(ctx, tmp_path):
    """the factor buffer, the merge's staging buffer and the re-packed weights: a forward with one rank-4 adapter on a conv and on a Linear target, one after
    its detach, and effective_weight of both"""
    d, sd = ctx.d, ctx.sd
    mc = d.model_channels
    targets = {"unet/input_blocks/rt1/res/conv_in/weight": ((mc, mc, 3, 3), 4), L.TB + "/attn1/query/weight": ((mc, mc), 4)}
    ad = L.make_adapter(targets, 21)
    lat, (c, _) = _lat(2, d.latent_h, d.latent_w), _prompts(d, 2, 7, 2)

    def attached():
        a = sd.lora_attach(ad, scale=0.9)        # the factors are uploaded and merged under the pattern of the moment
        try:
            return [sd.unet.forward(lat, [500], c)] + [sd.effective_weight(n) for n in targets]
        finally:
            a.detach()

    ctx.case(tmp_path, "lora attached: unet.forward, effective_weight", attached)
    ctx.case(tmp_path, "lora detached: unet.forward, effective_weight", lambda: [sd.unet.forward(lat, [500], c)] + [sd.effective_weight(n) for n in targets])


@pytest.mark.parametrize("n,T", [(1, 1), (3, 16)])
def test_clip_forward(ctx, tmp_path, n, T):
    tokens = np.random.default_rng(n * 100 + T).integers(0, MINI_VOCAB, (n, T)).astype(np.int32)
    ctx.case(tmp_path, f"clip.forward n={n} T={T}", lambda: ctx.sd.clip.forward(tokens))


# =================================================================================================================================================================
# Section B: operator entries -- the scratch each path allocates: slabs, quantised copies, merge buffers, staged epilogue operands
# =================================================================================================================================================================
@pytest.fixture(scope="module")
def ops_of():
    """ops_of(precision): the module's operator context of that precision (no weights), made on first use"""
    from stable_diffusion_burn_amd import ModelConfig, StableDiffusion
    made = {}

    def get(precision):
        if precision not in made:
            made[precision] = StableDiffusion(ModelConfig(64, 1, 64, 8, 8, 64, precision=precision))
            made[precision].precision = precision
        return made[precision]
    yield get
    for sd in made.values():
        sd.close()


def _precisions(*ps):
    return pytest.mark.parametrize("precision", ps, ids=lambda p: f"p{p}")


def _bar(sd):
    return BF16_BAR if sd.precision else FP32_BAR


def _operands(sd, *arrays):
    """operands as the kernels of this precision see them (bf16 storage: rounded on the host first, so that the oracle comparison isolates the kernel)"""
    return tuple(bf16_round(a) if sd.precision else a for a in arrays)


# ---- convolutions ----------------------------------------------------------------------------------------------------------------------------------------------
def _conv_operands(sd, case, seed):
    n, cin, h, w, cout = case
    g = np.random.default_rng(seed)
    x = g.standard_normal((n, cin, h, w)).astype(np.float32)
    wt = (g.standard_normal((cout, cin, 3, 3)) / math.sqrt(cin * 9)).astype(np.float32)
    return _operands(sd, x, wt) + (g.standard_normal(cout).astype(np.float32),)


def _conv_oracle(sd, x, wt, b, what):
    ref = O.conv2d(_t(x), (_t(wt), _t(b)), padding=1).numpy()
    return lambda got: _check(got[0], ref, what, _bar(sd))


# every tile the precision has on one awkward shape (test_conv2d_all_tiles / test_conv2d_bf16_all_tiles: the bf16 kernels need Cin % 64 == 0, so 128 there)
ALL_TILES = {0: ((2, 96, 13, 11, 208), list(range(10)) + [100, 101, 102, 103] + list(range(200, 206)) + list(range(300, 309))),
             1: ((2, 128, 13, 11, 208), list(range(10)) + [100, 101, 102, 103])}


@pytest.mark.parametrize("splitk", [1, 3])
@pytest.mark.parametrize("precision,tile", [(p, t) for p in (0, 1) for t in ALL_TILES[p][1]])
def test_conv_all_tiles(ops_of, tmp_path, precision, tile, splitk):
    sd = ops_of(precision)
    case = ALL_TILES[precision][0]
    x, wt, b = _conv_operands(sd, case, 1000 + tile)
    what = f"conv {case} precision {precision} tile={tile} splitk={splitk}"
    oracle = _conv_oracle(sd, x, wt, b, what) if tile in (0, 100, 200, 300) and splitk == 3 else None
    _sweep(sd, tmp_path, _with(sd, {"gemm_tile": tile, "splitk": splitk}, lambda: sd.op_conv2d(x, wt, b)), what, oracle=oracle)


# the kernel-row tiles of k_gemm_bf16t.hip take 3x3 layers over widths 16 .. 128 with whole 256-row tiles only (TCASES of test_bf16_gpu.py)
@pytest.mark.parametrize("case,splitk", [((2, 128, 16, 16, 320), 1), ((1, 64, 32, 16, 48), 3)])
@pytest.mark.parametrize("tile", [104, 105])
def test_conv_kernel_row_tiles_bf16(ops_of, tmp_path, tile, case, splitk):
    sd = ops_of(1)
    x, wt, b = _conv_operands(sd, case, 3300 + tile)
    what = f"conv {case} bf16 tile={tile} splitk={splitk}"
    _sweep(sd, tmp_path, _with(sd, {"gemm_tile": tile, "splitk": splitk}, lambda: sd.op_conv2d(x, wt, b)), what,
           oracle=_conv_oracle(sd, x, wt, b, what) if tile == 104 else None)


@pytest.mark.parametrize("case,opts", [((2, 32, 8, 8, 128), {"splitk": 9}),        # one k tile per slice
                                       ((1, 2560, 8, 8, 1280), {})])               # K = 23040: the engine's own split-K
@_precisions(0, 1)
def test_conv_split_k_edges(ops_of, tmp_path, precision, case, opts):
    ops = ops_of(precision)
    if ops.precision and case[1] % 64:
        case = (case[0], 64) + case[2:]      # the bf16 kernels need Cin % 64 == 0: one 64-element k tile per slice
    x, wt, b = _conv_operands(ops, case, case[1])
    _sweep(ops, tmp_path, _with(ops, opts, lambda: ops.op_conv2d(x, wt, b)), f"conv {case} precision {ops.precision} {opts}")


# ---- MXFP8 -----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ra", [0, 3])
@pytest.mark.parametrize("splitk", [1, 3])
@pytest.mark.parametrize("tile", ["auto", 0, 1, 2])
@pytest.mark.parametrize("case", [(3, 64, 5, 7, 96), (2, 320, 16, 16, 320), (1, 1280, 16, 16, 1280)])
@_precisions(2)
def test_conv_mxfp8(ops_of, tmp_path, precision, case, tile, splitk, ra):
    """conv_gemm_fp8x_kernel with bias, a time-embedding row per sample and a residual (staged by the entry point), in the epilogue and as the accumulators' initial value"""
    ops = ops_of(precision)
    what = f"mxfp8 conv {case} fp8_tile={tile} splitk={splitk} resid_acc={ra}"
    oracle = None
    if case[1] == 64:      # operands on the MX grid and the fp64 convolution (cached per shape by test_views_gpu.py)
        x, wt, b, temb, resid, conv = _conv_case(case + (3, 1, 0), "mx")
        oracle = lambda got: _check(got[0], _ref(conv, b, temb, resid), what, BF16_BAR)      # noqa: E731
    else:                  # GPU against GPU: the operands need not be on the grid, and no fp64 convolution of this size is computed
        n, cin, h, w, cout = case
        g = np.random.default_rng(cin + cout)
        x, wt = bf16_round(g.standard_normal((n, cin, h, w)) * 1.5), (g.standard_normal((cout, cin, 3, 3)) / math.sqrt(cin * 9)).astype(np.float32)
        b, temb, resid = g.standard_normal(cout).astype(np.float32), g.standard_normal((n, cout)).astype(np.float32), bf16_round(g.standard_normal((n, cout, h, w)))
    _sweep(ops, tmp_path, _with(ops, {"fp8_tile": tile, "splitk": splitk, "resid_acc": ra}, lambda: ops.op_conv2d_epilogue(x, wt, b, temb, resid)), what, oracle=oracle)


@pytest.mark.parametrize("rows,cin,cout", [(1100, 32, 64), (77, 64, 160), (513, 640, 5120)])
@_precisions(2)
def test_linear_mxfp8(ops_of, tmp_path, precision, rows, cin, cout):
    """cin = 32: four threads per row write the twelve pad groups 32 .. 127 and their scale bytes -- the pad loop that left them unwritten before round 4"""
    ops = ops_of(precision)
    g = np.random.default_rng(rows + cin)
    x = MX.mx_quantize(_t(bf16_round(g.standard_normal((rows, cin)))), 1).numpy().astype(np.float32)
    w = MX.mx_quantize(_t(g.standard_normal((cin, cout)) / math.sqrt(cin)), 0).numpy().astype(np.float32)
    b = g.standard_normal(cout).astype(np.float32)
    ref = x.astype(np.float64) @ w.astype(np.float64) + b
    what = f"linear fp8 ({rows}, {cin}, {cout})"
    _sweep(ops, tmp_path, _with(ops, {"fp8_ops": 1}, lambda: ops.op_linear(x, w, b)), what, oracle=lambda got: _check(got[0], ref, what, BF16_BAR))


def _rel_rms(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.sqrt(np.mean((got - ref) ** 2)) / np.sqrt(np.mean(ref ** 2)))


def _quantiser_oracle(ref64, what):
    """the bar of test_quantising_layer_norm_and_geglu_match_the_oracle_quantiser"""
    want = MX.mx_quantize(ref64, 1).numpy()

    def check(got):
        same = float(np.mean(got[0] == want.astype(np.float32)))
        assert same > 0.99 and _rel_rms(got[0], want) < 6e-3, f"{what}: {100 * same:.2f} % identical to the oracle quantiser, rel-RMS {_rel_rms(got[0], want):.2e}"
    return check


@pytest.mark.parametrize("rows,c", [(33, 1280), (257, 320)])
@_precisions(2)
def test_layer_norm_mxfp8(ops_of, tmp_path, precision, rows, c):
    ops = ops_of(precision)
    g = np.random.default_rng(rows + c)
    x = bf16_round(g.standard_normal((rows, c)) * 2 + 0.5)
    gam, bet = g.standard_normal(c).astype(np.float32), g.standard_normal(c).astype(np.float32)
    what = f"layer_norm fp8 ({rows}, {c})"
    _sweep(ops, tmp_path, _with(ops, {"fp8_ops": 1}, lambda: ops.op_layer_norm(x, gam, bet)), what,
           oracle=_quantiser_oracle(O.layer_norm(_t(x), _t(gam), _t(bet)), what))


@_precisions(2)
def test_geglu_mxfp8(ops_of, tmp_path, precision):
    ops = ops_of(precision)
    proj = bf16_round(np.random.default_rng(99).standard_normal((200, 2 * 1280)))
    a, gate = _t(proj[:, :1280]), _t(proj[:, 1280:])
    _sweep(ops, tmp_path, _with(ops, {"fp8_ops": 1}, lambda: ops.op_geglu(proj)), "geglu fp8 (200, 2 x 1280)",
           oracle=_quantiser_oracle(_t(bf16_round((a * O.gelu_erf(gate)).numpy())), "geglu fp8"))


def _gn_operands(shape, seed, rounded):
    g = np.random.default_rng(seed)
    c = shape[1]
    x = (g.standard_normal(shape) * 1.7 + 0.9).astype(np.float32)
    return (bf16_round(x) if rounded else x), (1 + 0.1 * g.standard_normal(c)).astype(np.float32), (0.1 * g.standard_normal(c)).astype(np.float32)


def _gn_ref(x, gamma, beta, silu):
    ref = O.group_norm(_t(x), _t(gamma), _t(beta), 32, 1e-5)
    return (O.silu(ref) if silu else ref).numpy()


@pytest.mark.parametrize("silu", [True, False])
@pytest.mark.parametrize("shape", [(2, 320, 16, 16), (2, 640, 8, 8)])
@_precisions(2)
def test_group_norm_mxfp8(ops_of, tmp_path, precision, shape, silu):
    ops = ops_of(precision)
    x, gamma, beta = _gn_operands(shape, shape[1] + shape[2], True)
    what = f"group_norm fp8 {shape} silu={silu}"
    _sweep(ops, tmp_path, lambda: ops.op_group_norm_fp8(x, gamma, beta, 32, 1e-5, silu), what,
           oracle=lambda got: _gn_check("mxfp8", got[0], _gn_ref(x, gamma, beta, silu), what))


# ---- GroupNorm / LayerNorm at fp32 and bf16 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("silu", [True, False])
@pytest.mark.parametrize("shape", [(1, 32, 4, 4), (2, 640, 1, 1), (1, 1920, 8, 8)])
@_precisions(0, 1)
def test_group_norm(ops_of, tmp_path, precision, shape, silu):
    ops = ops_of(precision)
    x, gamma, beta = _gn_operands(shape, shape[1] * 7 + shape[2], bool(ops.precision))
    what = f"group_norm {shape} precision {ops.precision} silu={silu}"
    _sweep(ops, tmp_path, lambda: ops.op_group_norm(x, gamma, beta, 32, 1e-5, silu), what, oracle=lambda got: _check(got[0], _gn_ref(x, gamma, beta, silu), what, _bar(ops)))


@pytest.mark.parametrize("case", [(2, 320, 16, 16, 640, 960), (1, 32, 4, 4, 8, 48), (1, 160, 16, 16, 160, 320)])     # n, c, h, w, in_off, in_ld (GN_CASES of test_views_gpu.py)
@_precisions(0)
def test_group_norm_view_planes(ops_of, tmp_path, precision, case):
    """the plane-writing GroupNorm reading a channel slice, from planes where the slice allows it"""
    ops = ops_of(precision)
    n, c, h, w, off, ld = case
    x, gamma, beta = _gn_operands((n, c, h, w), c * 7 + h + off, False)
    what = f"group_norm planes {case}"
    inp = 3 if (off % 32 == 0 and ld % 32 == 0) else 0
    _sweep(ops, tmp_path, lambda: ops.op_group_norm_view(x, gamma, beta, 1e-5, True, in_ld=ld, in_off=off, in_planes=inp, form=1), what,
           oracle=lambda got: _gn_check("planes", got[0], _gn_ref(x, gamma, beta, True), what))


@pytest.mark.parametrize("rows,c", [(5, 2048), (257, 320)])
@_precisions(0, 1)
def test_layer_norm(ops_of, tmp_path, precision, rows, c):
    ops = ops_of(precision)
    g = np.random.default_rng(rows + c)
    (x,) = _operands(ops, (g.standard_normal((rows, c)) * 2 - 0.5).astype(np.float32))
    gamma, beta = (1 + 0.1 * g.standard_normal(c)).astype(np.float32), (0.1 * g.standard_normal(c)).astype(np.float32)
    what = f"layer_norm ({rows}, {c}) precision {ops.precision}"
    ref = O.layer_norm(_t(x), _t(gamma), _t(beta), 1e-5).numpy()
    _sweep(ops, tmp_path, lambda: ops.op_layer_norm(x, gamma, beta, 1e-5), what, oracle=lambda got: _check(got[0], ref, what, _bar(ops)))


# ---- attention -------------------------------------------------------------------------------------------------------------------------------------------------
def _qkv(sd, case, seed):
    n, nq, nk, c, heads = case
    g = np.random.default_rng(seed)
    return _operands(sd, *(g.standard_normal((n, s, c)).astype(np.float32) for s in (nq, nk, nk)))


def _attn_oracle(sd, q, k, v, mask, heads, what):
    ref = O.qkv_attention(_t(q), _t(k), _t(v), None if mask is None else _t(mask), heads).numpy()
    # test_qkv_attention / test_qkv_attention_bf16: 2^-7 for the fused bf16 kernels at this fp32 boundary (q is rounded once more), 2^-6 for the unfused bf16 path
    bar = FP32_BAR if not sd.precision else (2 ** -7 if heads > 1 else 2 ** -6)
    return lambda got: _check(got[0], ref, what, bar)


ATTN = [(1, 100, 37, 160, 4),      # ragged queries and keys
        (1, 64, 2, 40, 1),         # two keys
        (3, 2048, 77, 640, 8),     # the 8-wave instance
        (1, 64, 64, 128, 1)]       # the unfused path: softmax rows and a transposed operand through the pool


@pytest.mark.parametrize("case", ATTN)
@_precisions(0, 1)
def test_attention(ops_of, tmp_path, precision, case):
    ops = ops_of(precision)
    q, k, v = _qkv(ops, case, sum(case))
    what = f"qkv_attention {case} precision {ops.precision}"
    _sweep(ops, tmp_path, lambda: ops.qkv_attention(q, k, v, None, case[4]), what, oracle=_attn_oracle(ops, q, k, v, None, case[4], what))


@pytest.mark.parametrize("splits", [2, 3])
@_precisions(0)
def test_attention_key_slices(ops_of, tmp_path, precision, splits):
    """slices of the keys plus the merge launch: the partial outputs and their (maximum, sum) pairs go through the pool"""
    ops = ops_of(precision)
    case = (1, 517, 1000, 320, 8)
    q, k, v = _qkv(ops, case, 7000 + splits)
    what = f"qkv_attention {case} attn_kv_splits={splits}"
    _sweep(ops, tmp_path, _with(ops, {"attn_kv_splits": splits}, lambda: ops.qkv_attention(q, k, v, None, 8)), what, oracle=_attn_oracle(ops, q, k, v, None, 8, what))


@_precisions(0)
def test_attention_causal_mask(ops_of, tmp_path, precision):
    ops = ops_of(precision)
    case = (1, 77, 77, 320, 8)
    q, k, v = _qkv(ops, case, 77)
    mask = np.triu(np.full((77, 77), -np.inf, np.float32), 1)
    _sweep(ops, tmp_path, lambda: ops.qkv_attention(q, k, v, mask, 8), "qkv_attention causal T = 77", oracle=_attn_oracle(ops, q, k, v, mask, 8, "qkv_attention causal"))


@pytest.mark.parametrize("variant", [1, 2, 4])
@_precisions(1)
def test_attention_bf16_variants(ops_of, tmp_path, precision, variant):
    ops = ops_of(precision)
    case = (2, 50, 100, 320, 8)
    q, k, v = _qkv(ops, case, 50 + variant)
    what = f"qkv_attention bf16 {case} variant {variant}"
    _sweep(ops, tmp_path, _with(ops, {"attn_bf16_variant": 0x100 | variant}, lambda: ops.qkv_attention(q, k, v, None, 8)), what,
           oracle=_attn_oracle(ops, q, k, v, None, 8, what))


# ---- GEGLU::forward, the concat chain, the resampler, views ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision,fuse", [(0, f) for f in (0, 2, 3, 4, 5, 6)] + [(1, f) for f in (0, 2, 3)])
def test_geglu_forward(ops_of, tmp_path, precision, fuse):
    sd = ops_of(precision)
    rows, cin, hidden = 513, 128, 384
    g = np.random.default_rng(rows + hidden + fuse)
    x, w = _operands(sd, g.standard_normal((rows, cin)).astype(np.float32), (g.standard_normal((cin, 2 * hidden)) / math.sqrt(cin)).astype(np.float32))
    b = g.standard_normal(2 * hidden).astype(np.float32)
    proj = _t(x) @ _t(w) + _t(b)
    ref = (proj[:, :hidden] * O.gelu_erf(proj[:, hidden:])).numpy()
    what = f"geglu_forward ({rows}, {cin}, {hidden}) precision {precision} fuse={fuse}"
    # test_geglu_forward_bf16: unfused, the projection is rounded to bf16 before the gate -- one more rounding
    bar = FP32_BAR if not precision else (2 ** -8 if fuse else 2 ** -7)
    _sweep(sd, tmp_path, _with(sd, {"geglu_fuse": fuse}, lambda: sd.op_geglu_forward(x, w, b, hidden)), what, oracle=lambda got: _check(got[0], ref, what, bar))


@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("cut", [(160, 160), (320, 160)])      # the half-width model's own cuts
@_precisions(0, 1)
def test_cat_chain(ops_of, tmp_path, precision, cut, dense):
    """two convolutions write the channel slices of one buffer (or dense tensors joined by a copy), GroupNorm + SiLU reads the whole"""
    ops = ops_of(precision)
    cx, cskip = cut
    n, cin, h, w = 2, 64, 13, 11
    g = np.random.default_rng(cx * 3 + cskip)
    x, wx, ws = _operands(ops, g.standard_normal((n, cin, h, w)).astype(np.float32), (g.standard_normal((cx, cin, 3, 3)) / math.sqrt(cin * 9)).astype(np.float32),
                          (g.standard_normal((cskip, cin, 3, 3)) / math.sqrt(cin * 9)).astype(np.float32))
    bx, bs = g.standard_normal(cx).astype(np.float32), (g.standard_normal(cskip) + 2.0).astype(np.float32)
    gamma, beta = (1 + 0.1 * g.standard_normal(cx + cskip)).astype(np.float32), (0.1 * g.standard_normal(cx + cskip)).astype(np.float32)
    what = f"cat chain {cut} precision {ops.precision} dense={dense}"
    oracle = None
    if not ops.precision:      # (at bf16 the halves are stored rounded between the operators: test_views_gpu.py::test_cat_chain holds that form against the oracle)
        ya, yb = O.conv2d(_t(x), (_t(wx), _t(bx)), padding=1), O.conv2d(_t(x), (_t(ws), _t(bs)), padding=1)
        ref = O.silu(O.group_norm(torch.cat([ya, yb], dim=1), _t(gamma), _t(beta), 32, 1e-5)).numpy()
        oracle = lambda got: _check(got[0], ref, what, FP32_BAR)      # noqa: E731
    _sweep(ops, tmp_path, lambda: ops.op_cat_chain(x, wx, bx, ws, bs, gamma, beta, silu=True, dense=dense), what, oracle=oracle)


@pytest.mark.parametrize("mode", [0, 1, 2])
@_precisions(0)
def test_resize(ops_of, tmp_path, precision, mode):
    """both axes change: the intermediate [n h][ow] buffer and the two tap tables"""
    ops = ops_of(precision)
    x = np.random.default_rng(8 * 1000 + 24 * 10 + mode).standard_normal((2, 4, 8, 24)).astype(np.float32)
    ref, s, tx, ty = RR.resize(x, 20, 8, mode, 0)

    def oracle(got):      # test_hires_gpu.py::_check_resize
        if mode == 0:
            assert np.array_equal(got[0], ref.astype(np.float32)), "nearest is a gather"
        else:
            assert (np.abs(got[0].astype(np.float64) - ref) <= (tx + ty + 8) * 2.0 ** -24 * s).all()
    _sweep(ops, tmp_path, lambda: ops.op_resize(x, (20, 8), RR.MODES[mode]), f"resize (8, 24) -> (20, 8) {RR.MODES[mode]}", oracle=oracle)


@_precisions(0, 1, 2)
def test_conv_view_model_cut(ops_of, tmp_path, precision):
    """a convolution with bias, time-embedding row and residual writing the back slice of the cut (320, 160), the parent as the UNet allocates it (fp32: also as planes)"""
    ops = ops_of(precision)
    fmt = ("f32", "bf16", "mx")[ops.precision]
    case, off, ld = (2, 64, 13, 11, 160, 3, 1, 0), 320, 480
    x, wt, b, temb, resid, conv = _conv_case(case, fmt)
    pre = _prefill(2 * 13 * 11, ld)
    outp = 3 if ops.precision == 0 else 0
    what = f"conv view {case} {fmt} slice [{off}, {off + 160}) of {ld}"

    def oracle(got):
        for parent in got:
            y = np.ascontiguousarray(parent[:, off:off + 160].reshape(2, 13, 11, 160).transpose(0, 3, 1, 2))
            _check(y, _ref(conv, b, temb, resid), what, _bar(ops))
    _sweep(ops, tmp_path, lambda: ops.op_conv2d_view(x, wt, b, temb, resid, resid_ld=160 + 24, parent=pre, out_off=off, out_planes=outp), what, oracle=oracle)


@_precisions(0, 1, 2)
def test_linear_view_model_cut(ops_of, tmp_path, precision):
    ops = ops_of(precision)
    rows, cin, cout = 77, 64, 160
    g = np.random.default_rng(rows + cin + cout)
    x, wt = g.standard_normal((rows, cin)).astype(np.float32), (g.standard_normal((cin, cout)) / math.sqrt(cin)).astype(np.float32)
    b, resid = g.standard_normal(cout).astype(np.float32), g.standard_normal((rows, cout)).astype(np.float32)
    if ops.precision == 2:
        x, wt = MX.mx_quantize(_t(bf16_round(x)), 1).numpy().astype(np.float32), MX.mx_quantize(_t(wt), 0).numpy().astype(np.float32)
    elif ops.precision == 1:
        x, wt = bf16_round(x), bf16_round(wt)
    if ops.precision:
        resid = bf16_round(resid)
    off, ld = 320, 480
    pre = _prefill(rows, ld)
    ref = x.astype(np.float64) @ wt.astype(np.float64) + b + resid
    what = f"linear view ({rows}, {cin}, {cout}) precision {ops.precision} slice [{off}, {off + cout}) of {ld}"
    _sweep(ops, tmp_path, _with(ops, {"fp8_ops": 1} if ops.precision == 2 else {}, lambda: ops.op_linear_view(x, wt, b, resid, resid_ld=cout + 8, parent=pre, out_off=off)), what,
           oracle=lambda got: _check(got[0][:, off:off + cout], ref, what, _bar(ops)))
