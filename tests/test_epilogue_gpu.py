"""The GEMM epilogue terms beyond x W + bias -- the time-embedding row a ResBlock's first convolution adds (unet/mod.rs:713-733) and the residual of
its second one, of proj_out and of the attention / feed-forward output projections -- against the fp64 oracle, through sdmi_op_conv2d_epilogue /
sdmi_op_linear_epilogue, which take both from the caller and hand them to the kernels in the model's own ConvGemm fields.

Round 6 moved these terms into the accumulators' initial value on the large-tile bf16 and MXFP8 kernels (option resid_acc, k_gemm_bf16_epi.hpp
gemm_acc_init_bf16): a tile inside one sample folds the time-embedding row into its per-column terms, interior tiles load the residual in batches,
edge tiles take a general form, the kernel-row convolution a one-pass form; the split-K reduce has a 16-byte form.  Every path is held here to the
operator bars of its module -- 2^-8 max(1, |ref|) for bf16 outputs, 2e-5 max(1, |ref|) at precision 0 -- with the residual and the time-embedding
rows drawn at unit scale, per element and per sample, so a term that is dropped, doubled or taken from the wrong sample is an O(1) error.  Every
case also reads back (option dump_choices) which tile, split count and resid_acc bits its launch took.  Where the code claims bit-identity
(persistent tile loop and one-tile form, kernel-row and plain tile, lean and general fp32 epilogue, vector and scalar split-K reduce, the gates
that leave resid_acc unset) it is asserted; resid_acc changes the fp32 summation order, so against resid_acc = 0 only the bar holds.
"""
import functools
import math
import zlib

import numpy as np
import pytest
import torch

from oracle import mx_oracle as MX
from oracle import sd_oracle as O

pytestmark = pytest.mark.gpu

BF16_BAR, FP32_BAR = 2 ** -8, 2e-5


def bf16_round(a):
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(a))


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double()


def _check(got, ref, what, rel):
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    assert got.shape == ref.shape, what
    assert np.isfinite(got).all(), f"{what}: non-finite output (a padding column read?)"
    err = np.abs(got - ref).max()
    bound = rel * max(1.0, np.abs(ref).max())
    assert err <= bound, f"{what}: max|d|={err:.3e} > {bound:.3e}"


def _engine(precision):
    from stable_diffusion_burn_amd import ModelConfig, StableDiffusion
    return StableDiffusion(ModelConfig(64, 1, 64, 8, 8, 64, precision=precision))


@pytest.fixture(scope="module")
def ops32():
    sd = _engine(0)
    yield sd
    sd.close()


@pytest.fixture(scope="module")
def ops16():
    sd = _engine(1)
    yield sd
    sd.close()


@pytest.fixture(scope="module")
def ops8():
    sd = _engine(2)
    yield sd
    sd.close()


_DEFAULTS = {"gemm_tile": "auto", "splitk": 0, "resid_acc": 3, "fp8_tile": "auto", "fp8_ops": 0, "op_misalign": 0, "gemm_bf16x_variant": "default",
             "gemm3x_variant": "default", "gemm_planes": "default", "geglu_fuse": 1}


def _run(sd, tmp_path, fn, **opts):
    """fn() under the given engine options (restored afterwards) -> (result, the GEMM launches it made: dump_choices lines)"""
    path = tmp_path / "choices.txt"
    try:
        for k, v in opts.items():
            sd.set_option(k, v)
        sd.set_option("record_shapes", 1)
        out = fn()
        sd.set_option("dump_choices", str(path))
    finally:
        sd.set_option("record_shapes", 0)
        for k in opts:
            sd.set_option(k, _DEFAULTS[k])
    return out, path.read_text().splitlines()


def _launched(lines, what, cfg=None, splits=None, acc=None, fp8=False):
    """exactly one GEMM launch, and it took the given tile / split count / resid_acc bits"""
    assert len(lines) == 1, f"{what}: expected one GEMM launch, got {lines}"
    ln = lines[0]
    assert (" fp8 " in ln) == fp8, f"{what}: {ln}"
    if cfg is not None:
        assert f" cfg={cfg} " in ln, f"{what}: tile not taken: {ln}"
    if splits is not None:
        assert f" splits={splits} " in ln, f"{what}: split count not taken: {ln}"
    if acc is not None:
        assert f" acc={acc} " in ln, f"{what}: resid_acc bits {acc} expected: {ln}"


def _acc_bits(ra, splitk, bias, temb, resid, resid_ok=True):
    if splitk != 1:
        return 0
    return (ra & 1 if resid is not None and resid_ok else 0) | (ra & 2 if bias is not None or temb is not None else 0)


# ---- operands and fp64 references, cached per shape ---------------------------------------------------------------------------------------------------------------
def _out_hw(h, w, k, stride, ups):
    pad = 1 if k == 3 else 0
    return ((h << ups) + 2 * pad - k) // stride + 1, ((w << ups) + 2 * pad - k) // stride + 1


@functools.lru_cache(maxsize=None)
def _conv_case(case, fmt):
    """x, weight, bias, per-sample temb, shared temb, residual and the fp64 conv(x) (no bias) of one shape; fmt: 'f32', 'bf16' (inputs rounded to
    bf16) or 'mx' (inputs on the MX grid); the residual is bf16-rounded at bf16 / MX"""
    n, cin, h, w, cout, k, stride, ups = case
    g = np.random.default_rng(zlib.crc32(repr((case, fmt)).encode()))
    x = g.standard_normal((n, cin, h, w)).astype(np.float32)
    wt = (g.standard_normal((cout, cin, k, k)) / math.sqrt(cin * k * k)).astype(np.float32)
    if fmt == "bf16":
        x, wt = bf16_round(x), bf16_round(wt)
    elif fmt == "mx":
        x = MX.mx_quantize(_t(x) * 1.5, 1).numpy().astype(np.float32)
        wt = MX.mx_quantize(_t(wt), 1).numpy().astype(np.float32)
    ho, wo = _out_hw(h, w, k, stride, ups)
    b = g.standard_normal(cout).astype(np.float32)
    temb = g.standard_normal((n, cout)).astype(np.float32)
    temb1 = g.standard_normal(cout).astype(np.float32)
    resid = g.standard_normal((n, cout, ho, wo)).astype(np.float32)
    if fmt != "f32":
        resid = bf16_round(resid)
    xin = O.upsample2x(_t(x)) if ups else _t(x)
    conv = O.conv2d(xin, (_t(wt), None), stride=stride, padding=1 if k == 3 else 0).numpy()
    return x, wt, b, temb, temb1, resid, conv


def _ref(conv, bias=None, temb=None, resid=None):
    r = conv.copy()
    if bias is not None:
        r += np.asarray(bias, np.float64)[None, :, None, None]
    if temb is not None:
        t = np.asarray(temb, np.float64)
        r += (t[None] if t.ndim == 1 else t)[:, :, None, None]
    if resid is not None:
        r += resid
    return r


# operand sets: (bias, temb: None / "one" (shared by the batch) / "each" (per sample), resid)
OPSETS = [(True, "one", False), (True, None, True), (True, "each", True), (False, "each", False), (False, None, True)]


def _operands(c, opset):
    x, wt, b, temb, temb1, resid, conv = c
    ub, ut, ur = opset
    return (b if ub else None), (temb if ut == "each" else temb1 if ut == "one" else None), (resid if ur else None)


def _conv_epi(sd, tmp_path, case, c, bias, temb, resid, **opts):
    n, cin, h, w, cout, k, stride, ups = case
    tstride = opts.pop("temb_stride", None)
    rld = opts.pop("resid_ld", 0)
    return _run(sd, tmp_path, lambda: sd.op_conv2d_epilogue(c[0], c[1], bias, temb, resid, stride=stride, upsample2x=bool(ups), temb_stride=tstride,
                                                            resid_ld=rld), **opts)


# ---- 1. the bf16 large tiles 100 - 103: resid_acc x split-K x operand sets ---------------------------------------------------------------------------------------------
BF16_CASES = [
    # n, cin, h, w, cout, k, stride, ups
    (2, 64, 23, 19, 200, 3, 1, 0),    # 437 pixels per sample: tile boundaries inside a sample, ragged M, N tail
    (6, 64, 5, 7, 96, 3, 1, 0),       # M = 210: below one tile, 35 pixels per sample -- several samples per tile; N = 96
    (8, 128, 8, 8, 328, 3, 1, 0),     # the 8 x 8 level: four samples per 256-row tile; N tail 328
    (3, 64, 20, 18, 320, 3, 2, 0),    # stride 2
    (2, 128, 9, 11, 320, 3, 1, 1),    # nearest-2x upsampling in front
    (4, 192, 12, 13, 200, 1, 1, 0),   # 1 x 1
]


@pytest.mark.parametrize("case", BF16_CASES)
@pytest.mark.parametrize("splitk", [1, 3])
@pytest.mark.parametrize("ra", [0, 1, 2, 3])
@pytest.mark.parametrize("tile", [100, 101, 102, 103])
def test_conv2d_bf16_large_tile_epilogue(ops16, tmp_path, case, splitk, ra, tile):
    c = _conv_case(case, "bf16")
    for opset in OPSETS:
        bias, temb, resid = _operands(c, opset)
        what = f"bf16 conv {case} tile={tile} splitk={splitk} resid_acc={ra} operands={opset}"
        got, lines = _conv_epi(ops16, tmp_path, case, c, bias, temb, resid, gemm_tile=tile, splitk=splitk, resid_acc=ra)
        _launched(lines, what, cfg=tile, splits=splitk, acc=_acc_bits(ra, splitk, bias, temb, resid))
        _check(got, _ref(c[6], bias, temb, resid), what, BF16_BAR)


# ---- 2. the kernel-row convolution (k_gemm_bf16t.hip, tiles 104 / 105; its one-pass accumulator init) --------------------------------------------------------------------
KROW_CASES = [(2, 128, 16, 16, 320, 3, 1, 0), (4, 64, 16, 32, 200, 3, 1, 0), (1, 192, 32, 32, 328, 3, 1, 0)]


@pytest.mark.parametrize("case", KROW_CASES)
@pytest.mark.parametrize("ra", [0, 3])
@pytest.mark.parametrize("tile", [104, 105])
def test_conv2d_bf16_kernel_row_epilogue(ops16, tmp_path, case, ra, tile):
    """the oracle, and bit for bit the plain tile of the same shape (100 / 101) at the same resid_acc -- test_conv2d_bf16_kernel_row_tiles's identity with the
    time-embedding row (per sample) and the residual in the accumulators"""
    c = _conv_case(case, "bf16")
    _, _, b, temb, _, resid, conv = c
    what = f"bf16 conv {case} tile={tile} resid_acc={ra}"
    got, lines = _conv_epi(ops16, tmp_path, case, c, b, temb, resid, gemm_tile=tile, splitk=1, resid_acc=ra)
    _launched(lines, what, cfg=tile, splits=1, acc=ra)
    plain, lines = _conv_epi(ops16, tmp_path, case, c, b, temb, resid, gemm_tile=tile - 4, splitk=1, resid_acc=ra)
    _launched(lines, what, cfg=tile - 4, splits=1, acc=ra)
    _check(got, _ref(conv, b, temb, resid), what, BF16_BAR)
    np.testing.assert_array_equal(got, plain, err_msg=f"{what}: kernel-row tile differs from tile {tile - 4}")


# ---- 3. the persistent tile loop (gemm_bf16x_variant bit 0) with the residual and per-sample rows in the accumulators ----------------------------------------------------
def _variants(sd, fn, what, variants=(1, 4, 5, 8, 13)):
    """bit 0: persistent tile loop; bit 2: staggered DMA; bit 3: the general epilogue on interior tiles -- all bit-identical to variant 0 (one tile per workgroup)"""
    try:
        sd.set_option("gemm_bf16x_variant", 0)
        base = fn()
        for v in variants:
            sd.set_option("gemm_bf16x_variant", v)
            got = fn()
            assert np.isfinite(got).all(), f"{what} variant {v}"
            np.testing.assert_array_equal(got, base, err_msg=f"{what}: gemm_bf16x_variant={v} differs from 0")
    finally:
        sd.set_option("gemm_bf16x_variant", "default")
    return base


@pytest.mark.parametrize("tile", [100, 101, 102])
def test_conv2d_bf16_persistent_epilogue(ops16, tmp_path, tile):
    n, cin, h, w, cout = 4, 64, 136, 136, 320         # 289 .. 867 tiles of 256 rows: more than the chip has CUs
    g = np.random.default_rng(6100 + tile)
    x = bf16_round(g.standard_normal((n, cin, h, w)))
    wt = bf16_round(g.standard_normal((cout, cin, 1, 1)) / math.sqrt(cin))
    b = g.standard_normal(cout).astype(np.float32)
    temb = g.standard_normal((n, cout)).astype(np.float32)
    resid = bf16_round(g.standard_normal((n, cout, h, w)))
    what = f"bf16 1x1 conv persistent tile={tile}"
    _, lines = _run(ops16, tmp_path, lambda: ops16.op_conv2d_epilogue(x, wt, b, temb, resid), gemm_tile=tile, splitk=1)
    _launched(lines, what, cfg=tile, splits=1, acc=3)
    try:
        ops16.set_option("gemm_tile", tile)
        ops16.set_option("splitk", 1)
        got = _variants(ops16, lambda: ops16.op_conv2d_epilogue(x, wt, b, temb, resid), what)
    finally:
        ops16.set_option("gemm_tile", "auto")
        ops16.set_option("splitk", 0)
    hw = h * w
    for s in range(n):       # the oracle on the rows of a few fragment groups per sample: the first, two around the middle, the last
        rs = np.r_[0:48, hw // 2 - 40:hw // 2 + 40, hw - 48:hw]
        xs = x[s].reshape(cin, hw)[:, rs].T.astype(np.float64)
        ref = xs @ wt.reshape(cout, cin).T.astype(np.float64) + b + temb[s] + resid[s].reshape(cout, hw)[:, rs].T
        _check(got[s].reshape(cout, hw)[:, rs].T, ref, f"{what} sample {s}", BF16_BAR)


@pytest.mark.parametrize("tile", [100, 101, 102, 103])
def test_linear_bf16_persistent_epilogue(ops16, tmp_path, tile):
    rows, cin, cout = 70001, 128, 320
    g = np.random.default_rng(6200 + tile)
    x = bf16_round(g.standard_normal((rows, cin)))
    wt = bf16_round(g.standard_normal((cin, cout)) / math.sqrt(cin))
    b = g.standard_normal(cout).astype(np.float32)
    resid = bf16_round(g.standard_normal((rows, cout)))
    what = f"bf16 linear ({rows},{cin},{cout}) persistent tile={tile}"
    _, lines = _run(ops16, tmp_path, lambda: ops16.op_linear_epilogue(x, wt, b, resid), gemm_tile=tile, splitk=1)
    _launched(lines, what, cfg=tile, splits=1, acc=3)
    try:
        ops16.set_option("gemm_tile", tile)
        ops16.set_option("splitk", 1)
        got = _variants(ops16, lambda: ops16.op_linear_epilogue(x, wt, b, resid), what)
    finally:
        ops16.set_option("gemm_tile", "auto")
        ops16.set_option("splitk", 0)
    rs = np.r_[0:300, rows // 2:rows // 2 + 300, rows - 300:rows]
    _check(got[rs], O.linear(_t(x[rs]), _t(wt), _t(b)).numpy() + resid[rs], what, BF16_BAR)


# ---- 4. the bf16 one-tile kernels 0 - 9 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("splitk", [1, 3])
@pytest.mark.parametrize("tile", list(range(10)))
def test_conv2d_bf16_small_tile_epilogue(ops16, tmp_path, tile, splitk):
    case = (3, 128, 9, 7, 200, 3, 1, 0)
    c = _conv_case(case, "bf16")
    _, _, b, temb, _, resid, conv = c
    what = f"bf16 conv {case} tile={tile} splitk={splitk}"
    got, lines = _conv_epi(ops16, tmp_path, case, c, b, temb, resid, gemm_tile=tile, splitk=splitk)
    _launched(lines, what, cfg=tile, splits=splitk, acc=0)
    _check(got, _ref(conv, b, temb, resid), what, BF16_BAR)


# ---- 5. MXFP8 (precision 2: k_fp8.hip) ---------------------------------------------------------------------------------------------------------------------------------
FP8_CASES = [(2, 320, 16, 16, 320, 3, 1, 0), (1, 256, 24, 40, 512, 3, 1, 0), (3, 64, 5, 7, 96, 3, 1, 0), (6, 128, 8, 8, 256, 3, 1, 0)]


@pytest.mark.parametrize("case", FP8_CASES)
@pytest.mark.parametrize("splitk", [1, 3])
@pytest.mark.parametrize("ra", [0, 3])
@pytest.mark.parametrize("tile", ["auto", 0, 1, 2])
def test_conv3x3_mxfp8_epilogue(ops8, tmp_path, case, splitk, ra, tile):
    c = _conv_case(case, "mx")
    _, _, b, temb, _, resid, conv = c
    for bias, tm, rs in [(b, temb, None), (b, None, resid), (b, temb, resid)]:
        what = f"mxfp8 conv {case} fp8_tile={tile} splitk={splitk} resid_acc={ra} temb={tm is not None} resid={rs is not None}"
        got, lines = _conv_epi(ops8, tmp_path, case, c, bias, tm, rs, fp8_tile=tile, splitk=splitk, resid_acc=ra)
        _launched(lines, what, cfg=None if tile == "auto" else tile, splits=splitk, acc=_acc_bits(ra, splitk, bias, tm, rs), fp8=True)
        _check(got, _ref(conv, bias, tm, rs), what, BF16_BAR)


# ---- 6. Linear with a residual where cin != cout: the feed-forward down-projections ---------------------------------------------------------------------------------------
FF_DOWN = [(4173, 1280, 320), (4173, 2560, 640), (4173, 5120, 1280)]


@functools.lru_cache(maxsize=None)
def _linear_case(shape, fmt):
    rows, cin, cout = shape
    g = np.random.default_rng(zlib.crc32(repr((shape, fmt)).encode()))
    x = g.standard_normal((rows, cin)).astype(np.float32)
    wt = (g.standard_normal((cin, cout)) / math.sqrt(cin)).astype(np.float32)
    resid = g.standard_normal((rows, cout)).astype(np.float32)
    if fmt == "bf16":
        x, wt, resid = bf16_round(x), bf16_round(wt), bf16_round(resid)
    b = g.standard_normal(cout).astype(np.float32)
    rs = np.r_[0:512, rows // 2:rows // 2 + 512, rows - 512:rows]       # first, middle and last tiles (the ragged one)
    ref = O.linear(_t(x[rs]), _t(wt), _t(b)).numpy() + resid[rs]
    return x, wt, b, resid, rs, ref


@pytest.mark.parametrize("shape", FF_DOWN)
@pytest.mark.parametrize("ra", [0, 3])
@pytest.mark.parametrize("tile", [100, 101, 102, 103])
def test_linear_bf16_ff_down_residual(ops16, tmp_path, shape, ra, tile):
    x, wt, b, resid, rs, ref = _linear_case(shape, "bf16")
    what = f"bf16 linear {shape} tile={tile} resid_acc={ra}"
    got, lines = _run(ops16, tmp_path, lambda: ops16.op_linear_epilogue(x, wt, b, resid), gemm_tile=tile, splitk=1, resid_acc=ra)
    _launched(lines, what, cfg=tile, splits=1, acc=ra)
    _check(got[rs], ref, what, BF16_BAR)


@pytest.mark.parametrize("shape", FF_DOWN)
@pytest.mark.parametrize("splitk", [0, 1, 3])
def test_linear_fp32_ff_down_residual(ops32, tmp_path, shape, splitk):
    x, wt, b, resid, rs, ref = _linear_case(shape, "f32")
    what = f"fp32 linear {shape} splitk={splitk}"
    got, lines = _run(ops32, tmp_path, lambda: ops32.op_linear_epilogue(x, wt, b, resid), splitk=splitk)
    _launched(lines, what, splits=splitk or None, acc=0)
    _check(got[rs], ref, what, FP32_BAR)


# ---- 7. precision 0 convolutions: plane tiles (300 + x) and 2x tiles (100 + x); the lean epilogue against the general one -------------------------------------------------
FP32_CASES = [(2, 64, 32, 32, 320, 3, 1, 0), (5, 96, 8, 8, 160, 3, 1, 0)]


@pytest.mark.parametrize("splitk", [1, 3])
@pytest.mark.parametrize("tile", [100, 101, 102, 103] + list(range(300, 309)))
def test_conv2d_fp32_epilogue_lean_and_general(ops32, tmp_path, tile, splitk):
    """gemm3x_variant 2 (the lean epilogue on interior single-sample tiles) and 66 (bit 6: the general form everywhere) bit for bit -- now with a per-sample
    time-embedding row and a residual on top of the bias -- and both against the oracle"""
    for case in FP32_CASES:
        c = _conv_case(case, "f32")
        _, _, b, temb, _, resid, conv = c
        what = f"fp32 conv {case} tile={tile} splitk={splitk}"
        outs = {}
        for variant in (2, 66):
            outs[variant], lines = _conv_epi(ops32, tmp_path, case, c, b, temb, resid, gemm_tile=tile, splitk=splitk, gemm3x_variant=variant,
                                             gemm_planes=2)
            _launched(lines, what, cfg=tile, splits=splitk)
        _check(outs[2], _ref(conv, b, temb, resid), what, FP32_BAR)
        np.testing.assert_array_equal(outs[2], outs[66], err_msg=f"{what}: lean and general epilogue differ")


# ---- 8. GEGLU forward at precision 1: the bias's gate half N apart in the accumulator-init form ------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cin,hidden", [(1000, 320, 1280), (777, 64, 328)])
@pytest.mark.parametrize("ra", [0, 3])
@pytest.mark.parametrize("fuse", [2, 3])
def test_geglu_forward_bf16_resid_acc(ops16, tmp_path, rows, cin, hidden, ra, fuse):
    g = np.random.default_rng(6300 + rows + hidden)
    x = bf16_round(g.standard_normal((rows, cin)))
    w = bf16_round(g.standard_normal((cin, 2 * hidden)) / math.sqrt(cin))
    b = g.standard_normal(2 * hidden).astype(np.float32)
    what = f"geglu_forward bf16 ({rows},{cin},{hidden}) fuse={fuse} resid_acc={ra}"
    got, lines = _run(ops16, tmp_path, lambda: ops16.op_geglu_forward(x, w, b, hidden), geglu_fuse=fuse, resid_acc=ra)
    _launched(lines, what, cfg=104 - fuse, splits=1, acc=ra & 2)
    proj = _t(x) @ _t(w) + _t(b)
    _check(got, (proj[:, :hidden] * O.gelu_erf(proj[:, hidden:])).numpy(), what, BF16_BAR)


# ---- 9. the resid_acc gates: strides and base addresses the accumulator-init loads cannot take leave the bit unset -----------------------------------------------------
# (gate, its options, the operands it gates -- (bias, temb, resid) as in OPSETS -- and the resid_acc bits left when all three are present)
GATES = [("resid_ld % 4 == 2", {"resid_ld": 322}, (False, None, True), 2), ("temb_stride % 4 != 0", {"temb_stride": 321}, (True, "each", False), 1),
         ("op_misalign", {"op_misalign": 1}, (True, "each", True), 0)]


@pytest.mark.parametrize("gate,extra,gated,acc", GATES, ids=[g[0] for g in GATES])
@pytest.mark.parametrize("tile", [100, 101, 102, 103])
def test_resid_acc_gates_bf16(ops16, tmp_path, gate, extra, gated, acc, tile):
    """With all three terms the launch keeps only the bit the gate allows.  With the gated terms alone it keeps none: the result is bit-identical to
    resid_acc = 0 on the same operands.  Both match the oracle, and the NaN padding behind cout is never read (finite outputs)."""
    case = (2, 64, 23, 19, 320, 3, 1, 0)
    c = _conv_case(case, "bf16")
    _, _, b, temb, _, resid, conv = c
    what = f"bf16 conv {case} tile={tile} gate {gate}"
    got, lines = _conv_epi(ops16, tmp_path, case, c, b, temb, resid, gemm_tile=tile, splitk=1, **extra)
    _launched(lines, what, cfg=tile, splits=1, acc=acc)
    _check(got, _ref(conv, b, temb, resid), what, BF16_BAR)
    bias, tm, rs = _operands(c, gated)
    outs = {}
    for ra in (3, 0):
        outs[ra], lines = _conv_epi(ops16, tmp_path, case, c, bias, tm, rs, gemm_tile=tile, splitk=1, resid_acc=ra, **extra)
        _launched(lines, f"{what}, gated terms only, resid_acc={ra}", cfg=tile, splits=1, acc=0)
    _check(outs[3], _ref(conv, bias, tm, rs), f"{what}, gated terms only", BF16_BAR)
    np.testing.assert_array_equal(outs[3], outs[0], err_msg=f"{what}: gated terms only, differs from resid_acc = 0")


@pytest.mark.parametrize("gate,extra,gated,acc", [("temb_stride % 4 != 0", {"temb_stride": 258}, (True, "each", False), 1), ("op_misalign", {"op_misalign": 1}, (True, "each", True), 0)],
                         ids=["temb_stride", "op_misalign"])
def test_resid_acc_gates_mxfp8(ops8, tmp_path, gate, extra, gated, acc):
    case = FP8_CASES[3]
    c = _conv_case(case, "mx")
    _, _, b, temb, _, resid, conv = c
    what = f"mxfp8 conv {case} gate {gate}"
    got, lines = _conv_epi(ops8, tmp_path, case, c, b, temb, resid, fp8_tile=0, splitk=1, **extra)
    _launched(lines, what, cfg=0, splits=1, acc=acc, fp8=True)
    _check(got, _ref(conv, b, temb, resid), what, BF16_BAR)
    bias, tm, rs = _operands(c, gated)
    outs = {}
    for ra in (3, 0):
        outs[ra], lines = _conv_epi(ops8, tmp_path, case, c, bias, tm, rs, fp8_tile=0, splitk=1, resid_acc=ra, **extra)
        _launched(lines, f"{what}, gated terms only, resid_acc={ra}", cfg=0, splits=1, acc=0, fp8=True)
    _check(outs[3], _ref(conv, bias, tm, rs), f"{what}, gated terms only", BF16_BAR)
    np.testing.assert_array_equal(outs[3], outs[0], err_msg=f"{what}: gated terms only, differs from resid_acc = 0")


@pytest.mark.parametrize("case", [BF16_CASES[0], BF16_CASES[2], BF16_CASES[5]])
@pytest.mark.parametrize("tile", [100, 102])
def test_splitk_reduce_bf16_vector_and_scalar_forms(ops16, tmp_path, case, tile):
    """k_gemm_bf16.hip splitk_reduce_bf16_kernel: the 16-byte form (resid_ld % 4 == 0, aligned operands) and the scalar one (odd resid_ld, or the operands
    one element off their alignment) -- the same sums in the same order, bit for bit; the scalar ones must not read the NaN padding"""
    c = _conv_case(case, "bf16")
    _, _, b, temb, _, resid, conv = c
    cout = case[4]
    what = f"bf16 conv {case} tile={tile} splitk=3 reduce"
    outs = {}
    for name, extra in [("vector", {}), ("odd resid_ld", {"resid_ld": cout + 1}), ("odd temb_stride", {"temb_stride": cout + 3}), ("misaligned", {"op_misalign": 1})]:
        outs[name], lines = _conv_epi(ops16, tmp_path, case, c, b, temb, resid, gemm_tile=tile, splitk=3, **extra)
        _launched(lines, f"{what} {name}", cfg=tile, splits=3, acc=0)
    _check(outs["vector"], _ref(conv, b, temb, resid), what, BF16_BAR)
    for name in ("odd resid_ld", "odd temb_stride", "misaligned"):
        np.testing.assert_array_equal(outs[name], outs["vector"], err_msg=f"{what}: {name} (scalar form) differs from the vector form")


def test_epilogue_entries_reject_bad_strides(ops16):
    """temb_stride below cout is refused, not read past"""
    case = BF16_CASES[0]
    c = _conv_case(case, "bf16")
    with pytest.raises(Exception):
        ops16.op_conv2d_epilogue(c[0], c[1], c[2], c[3], None, temb_stride=case[4] - 4)
